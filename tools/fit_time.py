"""Times one training step (sample 30 sub-steps + E_loc + VJP + Adam + sampler update) on the host path (tree gradients,
pretrain.adam on NumPy trees, wf.invalidate = recompile + dqmc_set_weights) and on the device path (fit.fit_wf with
optimizer.AdamOptimizer) in the same process: 4096 float32 walkers, LiH / PauliNet and N2 / FermiNet, warm-up first, then
median and minimum of --reps steps (device-synchronised host clock).  Also the update alone: Engine.set_params of a tree
against Engine.adam_step.  Prints one JSON line per system; exits 1 if a device-path median exceeds the host path's."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepqmc_amd import MolecularHamiltonian, Molecule  # noqa: E402
from deepqmc_amd.fit import TrainState, fit_wf  # noqa: E402
from deepqmc_amd.loss import compute_energy_loss_and_grad  # noqa: E402
from deepqmc_amd.optimizer import AdamOptimizer  # noqa: E402
from deepqmc_amd.pretrain import adam, apply_updates  # noqa: E402
from deepqmc_amd.sampling import DecorrSampler, MoleculeIdxSampler, MultiElectronicStateSampler, MultiNuclearGeometrySampler  # noqa: E402
from deepqmc_amd.wf import NeuralNetworkWaveFunction  # noqa: E402

DEV = 'cuda:0'


def setup(h, name, walkers, length):
    wf = NeuralNetworkWaveFunction(h, name, dtype=torch.float32, device=DEV)
    params = [wf.init(7, perturb_envelopes=0.1)]
    sampler = MultiNuclearGeometrySampler(MultiElectronicStateSampler(DecorrSampler(h, wf, length=length), 1))
    R = torch.as_tensor(np.asarray(h.mol.coords)[None], dtype=torch.float32, device=DEV)
    return wf, params, sampler, sampler.init(5, params, walkers, R)


def host_steps(h, wf, params, sampler, st, n, lr):
    opt = adam(lr)
    opt_state = [opt.init(p) for p in params]
    mis = MoleculeIdxSampler(0, 1, 1)
    times = []
    for k in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st, pc, _ = sampler.sample(1000003 + k, st, params, mis.sample())
        _, grads, _ = compute_energy_loss_and_grad(k, h, wf, params, pc)
        for s, p in enumerate(params):
            upd, opt_state[s] = opt.update(grads[s], opt_state[s], p)
            apply_updates(p, upd)
            wf.invalidate(p)
        st = sampler.update(st, params)
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return times


def device_steps(h, wf, params, sampler, st, n, lr):
    times = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in fit_wf(1, h, wf, AdamOptimizer(lr), MoleculeIdxSampler(0, 1, 1), sampler, range(n), TrainState(st, params, None), None):
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
    return times


def update_alone(wf, params, reps):
    eng = wf.engine(params[0])
    tree = params[0]
    host, dev = [], []
    theta = eng.params_flat(tree)
    mu, nu, g = torch.zeros_like(theta), torch.zeros_like(theta), torch.randn_like(theta)
    eng.adam_step(theta, mu, nu, g, lr=1e-6, t=1)
    for k in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.set_params(tree)
        torch.cuda.synchronize()
        host.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        eng.adam_step(theta, mu, nu, g, lr=1e-6, t=k + 2)
        torch.cuda.synchronize()
        dev.append(1e3 * (time.perf_counter() - t0))
    return host, dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--walkers', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--length', type=int, default=30)
    a = ap.parse_args()
    ok = True
    for mol, name in (('LiH', 'paulinet'), ('N2', 'ferminet')):
        h = MolecularHamiltonian(mol=Molecule.from_name(mol))
        out = {'system': f'{mol}/{name}', 'walkers': a.walkers, 'dtype': 'float32', 'sub_steps': a.length, 'reps': a.reps}
        counters = {}
        for label, run in (('host', host_steps), ('device', device_steps)):
            wf, params, sampler, st = setup(h, name, a.walkers, a.length)
            t = run(h, wf, params, sampler, st, a.warmup + a.reps, 1e-4)[a.warmup:]
            out[f'{label}_step_ms'] = round(float(np.median(t)), 3)
            out[f'{label}_step_min_ms'] = round(min(t), 3)
            counters[label] = wf.engine(params[0]).graph_counters()
            if label == 'device':
                hu, du = update_alone(wf, params, a.reps)
                out['set_params_ms'], out['set_params_min_ms'] = round(float(np.median(hu)), 3), round(min(hu), 3)
                out['adam_step_ms'], out['adam_step_min_ms'] = round(float(np.median(du)), 3), round(min(du), 3)
            wf.release()
        out['host_over_device'] = round(out['host_step_ms'] / out['device_step_ms'], 3)
        out['graph_counters'] = counters
        print(json.dumps(out), flush=True)
        ok = ok and out['device_step_ms'] <= out['host_step_ms']
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
