"""Times training steps of several electronic states with the penalties of loss.create_loss_fn, and the loss assembly alone
(dqmc_clip_rows + dqmc_loss_cotangents against the same formulas in torch), in one process on one GPU.

Cases: LiH / PauliNet with S = 3 x 2048 float32 walkers and N2 / FermiNet with S = 2 x 2048.  Per case: median and minimum of
--reps steps of fit_wf after --warmup (device-synchronised host clock) with the energy loss only (AdamOptimizer without a loss
function), with alpha = 4 scaled by max_gap_std, and with alpha = 4 plus the squared spin penalty (lambda = 1); then the
assembly alone -- from the last value pass to the first VJP -- on the kernel path and on the torch path, alternated call by
call on the inputs of one evaluated batch.  --single adds the single-state comparison at 4096 walkers: AdamOptimizer without
a loss function against AdamOptimizer(loss_fn=create_loss_fn(h, wf)) (energy only), alternated run by run.  One JSON line per
case; exits 1 if the kernel-path assembly takes longer than the torch-path assembly.

--profile N --path kernel|torch: nothing is timed; N assembly calls of that path run on synthetic inputs of the LiH case's
shape -- the workload of a `rocprofv3 --kernel-trace --stats` run.  The launches of one call are the kernel count of such a
run minus that of a --profile 0 run, divided by N."""
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
from deepqmc_amd.loss import create_loss_fn  # noqa: E402
from deepqmc_amd.optimizer import AdamOptimizer  # noqa: E402
from deepqmc_amd.sampling import DecorrSampler, MoleculeIdxSampler, MultiElectronicStateSampler, MultiNuclearGeometrySampler  # noqa: E402
from deepqmc_amd.wf import NeuralNetworkWaveFunction  # noqa: E402

DEV = 'cuda:0'
CONFIGS = {'energy_only': None, 'alpha4_max_gap_std': dict(alpha=4.0, scale_overlap_by='max_gap_std'),
           'alpha4_spin1': dict(alpha=4.0, scale_overlap_by='max_gap_std', spin_penalty=1.0)}


def setup(h, name, n_states, walkers, length):
    wf = NeuralNetworkWaveFunction(h, name, dtype=torch.float32, device=DEV)
    params = [wf.init(7 + s, perturb_envelopes=0.1) for s in range(n_states)]
    sampler = MultiNuclearGeometrySampler(MultiElectronicStateSampler(DecorrSampler(h, wf, length=length), n_states))
    R = torch.as_tensor(np.asarray(h.mol.coords)[None], dtype=torch.float32, device=DEV)
    return wf, params, sampler, sampler.init(5, params, walkers, R)


def steps(h, wf, params, sampler, st, n, opt):
    times = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in fit_wf(1, h, wf, opt, MoleculeIdxSampler(0, 1, 1), sampler, range(n), TrainState(st, params, None), None):
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
    return times


def med_min(t):
    return round(float(np.median(t)), 3), round(min(t), 3)


def assembly_inputs(fn, h, wf, params, sampler, st):
    _, pc, _ = sampler.sample(99, st, params, MoleculeIdxSampler(0, 1, 1).sample())
    S = len(params)
    nan = torch.full((1, S), float('nan'), dtype=torch.float64, device=DEV)
    v = fn.evaluate(3, params, (pc, None, {}))
    args = (v['e64'][0].contiguous(), v['weight'][0].contiguous(), v['psi_ratio'][0].contiguous(), v['spin'],
            {'energy_ewm': nan, 'std_ewm': nan})
    return args, wf.engine(params[0])


def time_assembly(fn, args, eng, reps, warmup):
    t = {'kernel': [], 'torch': []}
    for k in range(warmup + reps):
        for path in ('kernel', 'torch'):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn.cotangents(*args, path=path, engine=eng)
            torch.cuda.synchronize()
            if k >= warmup:
                t[path].append(1e3 * (time.perf_counter() - t0))
    return t


def synthetic_inputs(S, B):
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64, device=DEV)
    nan = torch.full((1, S), float('nan'), dtype=torch.float64, device=DEV)
    return (rnd(S, B) - 8.0, torch.ones(S, B, dtype=torch.float64, device=DEV), 0.3 * rnd(S, S, B) + 0.2, 0.75 + rnd(S, B),
            {'energy_ewm': nan, 'std_ewm': nan})


def profile(n, path):
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    wf = NeuralNetworkWaveFunction(h, 'paulinet', dtype=torch.float32, device=DEV)
    eng = wf.engine(wf.init(7))
    fn = create_loss_fn(h, wf, **CONFIGS['alpha4_spin1'])
    args = synthetic_inputs(3, 2048)
    torch.cuda.synchronize()
    for _ in range(n):
        fn.cotangents(*args, path=path, engine=eng)
    torch.cuda.synchronize()
    print(json.dumps({'profile_calls': n, 'path': path, 'S': 3, 'B': 2048}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--walkers', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--length', type=int, default=30)
    ap.add_argument('--single', action='store_true')
    ap.add_argument('--profile', type=int, default=None)
    ap.add_argument('--path', choices=('kernel', 'torch'), default='kernel')
    a = ap.parse_args()
    if a.profile is not None:
        return profile(a.profile, a.path)
    ok = True
    for mol, name, S in (('LiH', 'paulinet', 3), ('N2', 'ferminet', 2)):
        h = MolecularHamiltonian(mol=Molecule.from_name(mol))
        out = {'system': f'{mol}/{name}', 'states': S, 'walkers': a.walkers, 'dtype': 'float32', 'sub_steps': a.length, 'reps': a.reps}
        for label, kw in CONFIGS.items():
            wf, params, sampler, st = setup(h, name, S, a.walkers, a.length)
            opt = AdamOptimizer(1e-4) if kw is None else AdamOptimizer(1e-4, loss_fn=create_loss_fn(h, wf, **kw))
            t = steps(h, wf, params, sampler, st, a.warmup + a.reps, opt)[a.warmup:]
            out[f'{label}_step_ms'], out[f'{label}_step_min_ms'] = med_min(t)
            if label == 'alpha4_spin1':
                args, eng = assembly_inputs(opt.loss_fn, h, wf, params, sampler, st)
                ta = time_assembly(opt.loss_fn, args, eng, a.reps, a.warmup)
                for path in ('kernel', 'torch'):
                    out[f'assembly_{path}_ms'], out[f'assembly_{path}_min_ms'] = med_min(ta[path])
                ok = ok and out['assembly_kernel_ms'] <= out['assembly_torch_ms']
            wf.release()
        print(json.dumps(out), flush=True)
        if a.single:
            one = {'system': f'{mol}/{name}', 'states': 1, 'walkers': 4096, 'dtype': 'float32', 'sub_steps': a.length, 'reps': a.reps}
            for rep in range(2):
                for label in ('no_loss_fn', 'loss_fn_energy_only'):
                    wf, params, sampler, st = setup(h, name, 1, 4096, a.length)
                    opt = AdamOptimizer(1e-4) if label == 'no_loss_fn' else AdamOptimizer(1e-4, loss_fn=create_loss_fn(h, wf))
                    t = steps(h, wf, params, sampler, st, a.warmup + a.reps, opt)[a.warmup:]
                    one[f'{label}_step_ms_run{rep}'], one[f'{label}_step_min_ms_run{rep}'] = med_min(t)
                    wf.release()
            print(json.dumps(one), flush=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
