"""Times one KFAC training step (sample 30 sub-steps + E_loc + dqmc_log_psi_kfac + direction + update + sampler update) at 4096
float32 walkers, LiH / PauliNet and N2 / FermiNet, on the device path (fit.fit_wf with optimizer.KFACOptimizer) and on the only
way to take the same step without it: the tree direction of loss.compute_energy_loss_and_kfac, the norm constraint and the
update on host trees, wf.invalidate (recompile + dqmc_set_weights).  The two loops advance ALTERNATELY in one process, one
step each, so that clock and thermal drift hit both alike; warm-up first, then median and minimum of --reps steps
(device-synchronised host clock).  Also: the direction alone -- Engine.kfac_direction against the tree code from the same
factors -- its share of the device step, and the graph counters of both paths.  One JSON line per system; exits 1 if a
device-path median is not below the host path's by more than the spread (max - min of the faster half) of either.
--profile N: only N device-path steps after the warm-up, the workload of a `rocprofv3 --kernel-trace --stats` run."""
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
from deepqmc_amd.loss import _kfac_directions_tree, compute_energy_loss_and_kfac  # noqa: E402
from deepqmc_amd.optimizer import InverseSchedule, KFACOptimizer  # noqa: E402
from deepqmc_amd.pretrain import apply_updates  # noqa: E402
from deepqmc_amd.sampling import DecorrSampler, MoleculeIdxSampler, MultiElectronicStateSampler, MultiNuclearGeometrySampler  # noqa: E402
from deepqmc_amd.wf import NeuralNetworkWaveFunction  # noqa: E402

DEV = 'cuda:0'
NORM_CONSTRAINT, DAMPING, EMA = 1e-3, 1e-3, 0.95
LR = InverseSchedule(0.05, 10000)


def setup(h, name, walkers, length):
    wf = NeuralNetworkWaveFunction(h, name, dtype=torch.float32, device=DEV)
    params = [wf.init(7, perturb_envelopes=0.1)]
    sampler = MultiNuclearGeometrySampler(MultiElectronicStateSampler(DecorrSampler(h, wf, length=length), 1))
    R = torch.as_tensor(np.asarray(h.mol.coords)[None], dtype=torch.float32, device=DEV)
    return wf, params, sampler, sampler.init(5, params, walkers, R)


def host_steps(h, wf, params, sampler, st, n):
    """Generator: one host-path step per next(), yielding its time in ms."""
    mis = MoleculeIdxSampler(0, 1, 1)
    state = None
    for k in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st, pc, _ = sampler.sample(1000003 + k, st, params, mis.sample())
        _, deltas, stats, state = compute_energy_loss_and_kfac(k, h, wf, params, pc, state, DAMPING, EMA)
        for s, p in enumerate(params):
            lr, dot = LR(k), float(stats['precon_grad_dot'][s])
            coeff = min(1.0, float(np.sqrt(NORM_CONSTRAINT / (lr * lr * dot)))) if dot > 0 else 1.0
            apply_updates(p, {m: {leaf: -lr * coeff * np.asarray(v) for leaf, v in leaves.items()} for m, leaves in deltas[s].items()})
            wf.invalidate(p)
        st = sampler.update(st, params)
        torch.cuda.synchronize()
        yield 1e3 * (time.perf_counter() - t0)


def device_steps(h, wf, params, sampler, st, n, box=None):
    opt = KFACOptimizer(LR, norm_constraint=NORM_CONSTRAINT, damping=DAMPING, ema=EMA)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _, state, _, _ in fit_wf(1, h, wf, opt, MoleculeIdxSampler(0, 1, 1), sampler, range(n), TrainState(st, params, None), None):
        torch.cuda.synchronize()
        if box is not None:
            box['sampler_state'] = state.sampler
        yield 1e3 * (time.perf_counter() - t0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()


def direction_alone(h, wf, params, sampler, smpl_state, walkers, reps, warmup):
    """Engine.kfac_direction against the tree code (torch Cholesky per module, host trees), both from the same factors: those of
    the training run's own walkers after its last step."""
    eng = wf.engine(params[0])
    _, pc, _ = sampler.sample(99, smpl_state, params, MoleculeIdxSampler(0, 1, 1).sample())
    r = (pc.r if hasattr(pc, 'r') else pc)[0, 0].contiguous()
    lay = eng.program.kfac_layout()
    fac = torch.empty(lay['n_factor_doubles'], dtype=torch.float64, device=DEV)
    rest = torch.empty(walkers, lay['n_rest'], dtype=torch.float32, device=DEV)
    cot = torch.randn(walkers, dtype=torch.float32, device=DEV) / walkers
    cached = eng.log_psi_kfac(r, cot, out=(fac, rest))
    sign, logpsi, g, _, _ = cached
    gt = eng.grad_to_params(g)
    state = eng.kfac_state()
    out = (torch.empty_like(gt), torch.empty(1, dtype=torch.float64, device=DEV))
    dev, tree = [], []
    real = eng.log_psi_kfac
    tstate = None
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.kfac_direction(gt, fac, rest, logpsi, sign, state, k == 0, EMA, DAMPING, out=out)
        torch.cuda.synchronize()
        dev.append(1e3 * (time.perf_counter() - t0))
        eng.log_psi_kfac = lambda *a, **kw: cached        # the tree code from the same factors, without the reverse pass
        try:
            t0 = time.perf_counter()
            _, _, _, tstate = _kfac_directions_tree(wf, params, r[None, None], [None], None, [cot], {}, tstate, DAMPING, EMA)
            torch.cuda.synchronize()
            tree.append(1e3 * (time.perf_counter() - t0))
        except RuntimeError as e:      # torch.linalg.cholesky raises on a factor that is not positive definite (the kernels give NaN)
            print(f'tree direction failed: {e}', file=sys.stderr)
            tree.append(float('nan'))
        finally:
            eng.log_psi_kfac = real
    return dev[warmup:], tree[warmup:]


def spread(t):
    fast = sorted(t)[:max(len(t) // 2, 1)]
    return max(fast) - min(fast)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--walkers', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--length', type=int, default=30)
    ap.add_argument('--profile', type=int, default=0, help='only this many device-path steps after the warm-up (for rocprofv3)')
    ap.add_argument('--systems', default='LiH/paulinet,N2/ferminet')
    a = ap.parse_args()
    ok = True
    for item in a.systems.split(','):
        mol, name = item.split('/')
        h = MolecularHamiltonian(mol=Molecule.from_name(mol))
        if a.profile:
            wf, params, sampler, st = setup(h, name, a.walkers, a.length)
            t = list(device_steps(h, wf, params, sampler, st, a.warmup + a.profile))[a.warmup:]
            print(json.dumps({'system': item, 'profile_steps': a.profile, 'device_step_ms': round(float(np.median(t)), 3)}), flush=True)
            wf.release()
            continue
        out = {'system': item, 'walkers': a.walkers, 'dtype': 'float32', 'sub_steps': a.length, 'reps': a.reps}
        n = a.warmup + a.reps
        box = {}
        wf_h, params_h, sampler_h, st_h = setup(h, name, a.walkers, a.length)
        wf_d, params_d, sampler_d, st_d = setup(h, name, a.walkers, a.length)
        gh, gd = host_steps(h, wf_h, params_h, sampler_h, st_h, n), device_steps(h, wf_d, params_d, sampler_d, st_d, n, box)
        th, td = [], []
        for _ in range(n):                   # alternate: one device-path step, one host-path step
            td.append(next(gd))
            th.append(next(gh))
        gd.close()
        th, td = th[a.warmup:], td[a.warmup:]
        for label, t in (('host', th), ('device', td)):
            out[f'{label}_step_ms'], out[f'{label}_step_min_ms'] = round(float(np.median(t)), 3), round(min(t), 3)
            out[f'{label}_step_spread_ms'] = round(spread(t), 3)
        out['graph_counters'] = {'host': wf_h.engine(params_h[0]).graph_counters(), 'device': wf_d.engine(params_d[0]).graph_counters()}
        wf_h.release()
        dd, dt = direction_alone(h, wf_d, params_d, sampler_d, box['sampler_state'], a.walkers, a.reps, a.warmup)
        out['kfac_direction_ms'], out['kfac_direction_min_ms'] = round(float(np.median(dd)), 3), round(min(dd), 3)
        out['tree_direction_ms'], out['tree_direction_min_ms'] = round(float(np.median(dt)), 3), round(min(dt), 3)
        out['direction_share_of_device_step'] = round(out['kfac_direction_ms'] / out['device_step_ms'], 3)
        out['host_over_device'] = round(out['host_step_ms'] / out['device_step_ms'], 3)
        blocks = wf_d.engine(params_d[0]).program.kfac_blocks()[0]
        out['factor_dims'] = sorted({d for b in blocks.values() for d in (b['n_in'] + int(b['has_bias']), b['n_out'])})
        wf_d.release()
        print(json.dumps(out), flush=True)
        ok = ok and out['host_step_ms'] - out['device_step_ms'] > max(out['host_step_spread_ms'], out['device_step_spread_ms'])
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
