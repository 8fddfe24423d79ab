"""Times the observable monitors on one GPU: LiH / PauliNet, S = 3 states x 2048 float32 walkers, AdamOptimizer with the
multi-state loss (alpha = 4, max_gap_std); the median (and minimum) of --reps runs after --warmup, host clock around work that
ends in a device synchronise.

Without --mode the tool only starts child processes, one per measurement, each with its own time limit, and stops at the first
that fails:
  step      one fit_wf step with observable_monitors=None, from this tree and -- with --parent-root DIR, a built checkout of the
            parent commit -- from that tree, alternated parent, this, parent, this: the parent's own run-to-run spread is the
            yardstick for the difference.
  monitors  the time of one call of every monitor on one sampled batch.
  os        Engine.oscillator_strength against the same formulas in torch, alternated call by call in one process.
It prints one JSON line per measurement and writes the summary to --out.  Exits 1 if the step of this tree is slower than the
parent's slower run by more than the spread between the parent's two runs, or if the kernels take longer than torch."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = 'cuda:0'
S, LOSS = 3, dict(alpha=4.0, scale_overlap_by='max_gap_std')


def setup(root, walkers, length):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from deepqmc_amd import MolecularHamiltonian, Molecule
    from deepqmc_amd.loss import create_loss_fn
    from deepqmc_amd.optimizer import AdamOptimizer
    from deepqmc_amd.sampling import DecorrSampler, MultiElectronicStateSampler, MultiNuclearGeometrySampler
    from deepqmc_amd.wf import NeuralNetworkWaveFunction
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    wf = NeuralNetworkWaveFunction(h, 'paulinet', dtype=torch.float32, device=DEV)
    params = [wf.init(7 + s, perturb_envelopes=0.1) for s in range(S)]
    sampler = MultiNuclearGeometrySampler(MultiElectronicStateSampler(DecorrSampler(h, wf, length=length), S))
    R = torch.as_tensor(np.asarray(h.mol.coords)[None], dtype=torch.float32, device=DEV)
    opt = AdamOptimizer(1e-4, loss_fn=create_loss_fn(h, wf, **LOSS))
    return h, wf, params, sampler, sampler.init(5, params, walkers, R), opt


def med_min(t):
    t = sorted(t)
    return round(t[len(t) // 2] if len(t) % 2 else 0.5 * (t[len(t) // 2 - 1] + t[len(t) // 2]), 3), round(t[0], 3)


def timed(fn, reps, warmup):
    import torch
    out = []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            out.append(1e3 * (time.perf_counter() - t0))
    return out


def mode_step(a):
    """A step of fit_wf as the parent commit knows it: no observable_monitors argument at all."""
    import torch
    h, wf, params, sampler, st, opt = setup(a.root, a.walkers, a.length)
    from deepqmc_amd.fit import TrainState, fit_wf
    from deepqmc_amd.sampling import MoleculeIdxSampler
    t = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in fit_wf(1, h, wf, opt, MoleculeIdxSampler(0, 1, 1), sampler, range(a.warmup + a.reps), TrainState(st, params, None), None):
        torch.cuda.synchronize()
        t.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
    med, mn = med_min(t[a.warmup:])
    print(json.dumps({'mode': 'step', 'root': a.root, 'step_ms': med, 'step_min_ms': mn}), flush=True)


def mode_monitors(a):
    import torch
    h, wf, params, sampler, st, opt = setup(a.root, a.walkers, a.length)
    from deepqmc_amd import observable as obs
    from deepqmc_amd.sampling import MoleculeIdxSampler
    from deepqmc_amd.types import Psi
    st, pc, _ = sampler.sample(99, st, params, MoleculeIdxSampler(0, 1, 1).sample())
    v = opt.loss_fn.evaluate(3, params, (pc, None, {}))
    psi = Psi(torch.stack([s['psi'].sign for s in st['elec'][0]])[None], torch.stack([s['psi'].log for s in st['elec'][0]])[None])
    out = {'mode': 'monitors'}
    names = ('r', 'R', 'psi', 'local_energy', 'psi_ratio', 'spin', 'hf_force_bare', 'hf_force_bare_anti', 'hf_force_ac_zvq',
             'hf_force_ac_zvq_anti', 'hf_force_ac_zvzbq', 'hf_force_ac_zb', 'hf_force_ac_zvqzb', 'finite_difference_force',
             'oscillator_strength')
    for name in names:
        m = obs.observable_monitor_from_name(name).finalize(h, wf)
        m.save_samples = False
        t = timed(lambda: m(0, 11, params, pc, psi, v['e_loc'], v['psi_ratio']), a.reps, a.warmup)
        out[f'{name}_ms'], out[f'{name}_min_ms'] = med_min(t)
    print(json.dumps(out), flush=True)


def torch_oscillator_strength(r, ratio, e):
    """observable.py:556-605 in torch float64: r [S, B, N, 3], ratio [S, S, B], e [S, B] -> (os_mean, os_err)."""
    B = e.shape[-1]
    e = e.double()
    E, err_E = e.mean(-1), e.std(-1, unbiased=False) / B ** 0.5
    ex = E[None, :] - E[:, None]
    ex_err = (err_E ** 2 + err_E[:, None] ** 2) ** 0.5
    cd = (-r.double()).sum(-2)[None] * ratio[..., None]
    cd_mean, cd_err = cd.mean(-2), cd.std(-2, unbiased=False) / B ** 0.5
    rel = cd_err / cd_mean
    ds_vec = cd_mean * cd_mean.transpose(0, 1)
    ds_err_vec = ds_vec.abs() * (rel ** 2 + rel.transpose(0, 1) ** 2) ** 0.5
    ds, ds_err = ds_vec.sum(-1), (ds_err_vec ** 2).sum(-1) ** 0.5
    os_mean = (2 / 3) * ex * ds
    return os_mean, (2 / 3) * os_mean.abs() * ((ex_err / ex) ** 2 + (ds_err / ds) ** 2) ** 0.5


def mode_os(a):
    import torch
    h, wf, params, sampler, st, opt = setup(a.root, a.walkers, a.length)
    from deepqmc_amd.sampling import MoleculeIdxSampler
    st, pc, _ = sampler.sample(99, st, params, MoleculeIdxSampler(0, 1, 1).sample())
    v = opt.loss_fn.evaluate(3, params, (pc, None, {}))
    eng = wf.engine(params[0])
    r, ratio, e = pc.r[0].contiguous(), v['psi_ratio'][0].contiguous(), v['e_loc'][0].contiguous()
    t = {'kernel': [], 'torch': []}
    for k in range(a.warmup + a.reps):
        for path, fn in (('kernel', lambda: eng.oscillator_strength(r, ratio, e)), ('torch', lambda: torch_oscillator_strength(r, ratio, e))):
            (dt,) = timed(fn, 1, 0)
            if k >= a.warmup:
                t[path].append(dt)
    got, want = eng.oscillator_strength(r, ratio, e)[0], torch_oscillator_strength(r, ratio, e)[0]
    off = ~torch.eye(S, dtype=torch.bool, device=got.device)
    out = {'mode': 'os', 'largest_relative_deviation': float(((got - want).abs() / want.abs())[off].max())}
    for path in t:
        out[f'{path}_ms'], out[f'{path}_min_ms'] = med_min(t[path])
    print(json.dumps(out), flush=True)


def child(mode, root, a, limit):
    cmd = [sys.executable, os.path.abspath(__file__), '--mode', mode, '--root', root, '--walkers', str(a.walkers), '--reps', str(a.reps),
           '--warmup', str(a.warmup), '--length', str(a.length)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f'{mode} ({root}) ended with status {p.returncode}: nothing more is started')
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=('step', 'monitors', 'os'), default=None)
    ap.add_argument('--root', default=os.path.dirname(HERE))
    ap.add_argument('--parent-root', default=None)
    ap.add_argument('--walkers', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--length', type=int, default=30)
    ap.add_argument('--limit', type=int, default=240, help='seconds per child process')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(HERE), 'profiles', 'observable_time.txt'))
    a = ap.parse_args()
    if a.mode is not None:
        return {'step': mode_step, 'monitors': mode_monitors, 'os': mode_os}[a.mode](a) or 0
    lines = [f'tools/observable_time.py: LiH / PauliNet, {S} states x {a.walkers} float32 walkers, {a.length} sub-steps, AdamOptimizer with '
             f'alpha = 4 (max_gap_std); median (minimum) of {a.reps} after {a.warmup} warm-up, ms, one MI355X', '']
    ok = True
    steps = {'parent': [], 'this': []}
    for rep in range(2):
        for label, root in (('parent', a.parent_root), ('this', a.root)):
            if root is not None:
                steps[label].append(child('step', root, a, a.limit))
    for label, runs in steps.items():
        for k, run in enumerate(runs):
            lines.append(f'step, observable_monitors=None, {label:6s} run {k}: {run["step_ms"]:9.3f} ({run["step_min_ms"]:.3f})')
    if steps['parent']:
        p = [run['step_ms'] for run in steps['parent']]
        spread = abs(p[0] - p[1])
        worst = max(run['step_ms'] for run in steps['this'])
        ok = worst <= max(p) + spread
        lines.append(f"parent's run-to-run spread {spread:.3f}; slowest run of this tree minus slowest run of the parent {worst - max(p):+.3f}"
                     f" -> {'within' if ok else 'BEYOND'} the spread")
    else:
        lines.append('parent: not measured (no --parent-root)')
    mon = child('monitors', a.root, a, 2 * a.limit)
    lines += ['', 'one call of a monitor (save_samples=False), all three states:']
    lines += [f'  {k[:-3]:26s} {mon[k]:9.3f} ({mon[k[:-3] + "_min_ms"]:.3f})' for k in mon if k.endswith('_ms') and not k.endswith('_min_ms')]
    o = child('os', a.root, a, a.limit)
    ok = ok and o['kernel_ms'] <= o['torch_ms']
    lines += ['', f"Engine.oscillator_strength (2 launches): {o['kernel_ms']:.3f} ({o['kernel_min_ms']:.3f}); the same formulas in torch: "
              f"{o['torch_ms']:.3f} ({o['torch_min_ms']:.3f}); largest relative deviation of os_mean {o['largest_relative_deviation']:.1e}"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
