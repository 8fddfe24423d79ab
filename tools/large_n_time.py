"""Times the local-energy call and the determinant kernels for the electron counts beyond the benchmark systems' (22, 36, 44,
49 and 64 electrons; production widths: FermiNet 256 x 4 interactions, Psiformer 256 x 4 heads x 64), 256 walkers, float32 at
library defaults and float64, all in one process (device-synchronised host clock, warm-up first; median and minimum of
--reps calls, the two loops of a comparison alternated).  Prints one JSON line per measurement and appends it to --out.

  eloc        E_loc call time per (ansatz, N, dtype), with the per-kernel-class device times of the library's own timers; float32
              also with option refine 0 (the float32 pass alone: at 256 walkers the default refines every walker in float64)
  slogdet     N = 64 (and 49): Laplacian mode, k_slogdet_mfma64 (option slogdet_mfma 1) against k_slogdet_dyn (0); value-only,
              k_slogdet_reg<64, 64> (1) against k_slogdet_lu (3) -- device time of the `slogdet` launches alone
  --profile K only K float32 E_loc calls of one system (--n, --ansatz), for a rocprofv3 --kernel-trace --stats run of its own"""
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
from deepqmc_amd.engine import Engine  # noqa: E402
from deepqmc_amd.params import init_params  # noqa: E402
from deepqmc_amd.sampling import synthetic_walkers  # noqa: E402
from deepqmc_amd.spec import ANSATZES  # noqa: E402

DEV = 'cuda:0'


def ring(z, n, bond=2.6):
    rad = bond / (2 * np.sin(np.pi / n))
    phi = 2 * np.pi * np.arange(n) / n
    return np.stack([rad * np.cos(phi), rad * np.sin(phi), np.zeros(n)], 1), [z] * n


def line(charges, bond):
    n = len(charges)
    return np.stack([np.zeros(n), np.zeros(n), bond * (np.arange(n) - (n - 1) / 2)], 1), list(charges)


SYSTEMS = {22: (line([8, 6, 8], 2.2), 0), 36: (ring(6, 6), 0), 42: (None, 0), 44: (line([15, 15, 14], 3.8), 0), 49: (ring(7, 7), 1),
           64: (ring(8, 8), 0)}


def make(name, n, dtype):
    if n == 42:
        mol = Molecule.from_name('benzene')
    else:
        (coords, charges), spin = SYSTEMS[n]
        mol = Molecule(coords=coords, charges=charges, charge=0, spin=spin)
    h = MolecularHamiltonian(mol=mol)
    spec = ANSATZES[name]()
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=7, perturb_envelopes=0.1)
    return h, Engine(spec, h, tree, dtype=dtype, device=DEV)


def emit(out, rec):
    line_ = json.dumps(rec)
    print(line_, flush=True)
    if out:
        with open(out, 'a') as f:
            f.write(line_ + '\n')


def clock(f):
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='eloc,slogdet')
    ap.add_argument('--n', default='22,36,44,49,64')
    ap.add_argument('--ansatz', default='ferminet,psiformer')
    ap.add_argument('--dtypes', default='float32,float64')
    ap.add_argument('--walkers', type=int, default=256)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--profile', type=int, default=0)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    ns = [int(x) for x in a.n.split(',')]
    names = a.ansatz.split(',')
    if a.profile:
        h, eng = make(names[0], ns[0], torch.float32)
        r = torch.as_tensor(synthetic_walkers(h, a.walkers, seed=1), dtype=torch.float32, device=DEV)
        for _ in range(a.profile):
            eng.local_energy(r)
        torch.cuda.synchronize()
        eng.close()
        return
    if 'slogdet' in a.what:
        for n in (64, 49, 42):
            for dtype in (torch.float32, torch.float64):
                h, eng = make('ferminet', n, dtype)
                r = torch.as_tensor(synthetic_walkers(h, a.walkers, seed=1), dtype=dtype, device=DEV)
                eng.set_option('pass_graph', 0)            # (an option switch drops the captured graphs: eager launches both ways)
                eng.set_option('refine', 0)                # the float32 pass alone
                for mode, call, opts in (('laplacian', lambda: eng.local_energy(r), (1, 0)), ('value', lambda: eng.wf_eval(r), (1, 3))):
                    t = {o: [] for o in opts}
                    for o in opts:
                        eng.set_option('slogdet_mfma', o)
                        call(); call()
                    torch.cuda.synchronize()
                    eng.timing(True)
                    for _ in range(a.reps):
                        for o in opts:
                            eng.set_option('slogdet_mfma', o)
                            eng.timing_reset()
                            call()
                            torch.cuda.synchronize()
                            t[o].append(eng.timing_report()['slogdet']['ms'])
                    eng.timing(False)
                    eng.set_option('slogdet_mfma', 1)
                    emit(a.out, {'what': 'slogdet', 'mode': mode, 'n_elec': n, 'dtype': str(dtype).split('.')[-1], 'walkers': a.walkers,
                                 'n_det': eng.spec.n_determinants, 'reps': a.reps,
                                 **{f'option_{o}_ms_median': round(float(np.median(v)), 4) for o, v in t.items()},
                                 **{f'option_{o}_ms_min': round(min(v), 4) for o, v in t.items()}})
                eng.close()
    if 'eloc' in a.what:
        for n in ns:
            for name in names:
                for dn in a.dtypes.split(','):
                    dtype = getattr(torch, dn)
                    h, eng = make(name, n, dtype)
                    r = torch.as_tensor(synthetic_walkers(h, a.walkers, seed=1), dtype=dtype, device=DEV)
                    f = lambda: eng.local_energy(r)
                    for _ in range(3):                       # eager, capture, replay; the float64 twin
                        f()
                    torch.cuda.synchronize()
                    t = [clock(f) for _ in range(a.reps)]
                    n_ref = eng.last_refined() if dtype == torch.float32 else 0
                    eng.timing(True); eng.timing_reset()
                    f(); torch.cuda.synchronize()
                    rep = {k: round(v['ms'], 3) for k, v in eng.timing_report().items() if v['ms'] > 0}
                    eng.timing(False)
                    off = {}
                    if dtype == torch.float32:              # the float32 pass alone: at this batch size the default refines every walker
                        eng.set_option('refine', 0)
                        for _ in range(3):
                            f()
                        torch.cuda.synchronize()
                        t0 = [clock(f) for _ in range(a.reps)]
                        eng.timing(True); eng.timing_reset()
                        f(); torch.cuda.synchronize()
                        off = {'refine_off_ms_median': round(float(np.median(t0)), 3), 'refine_off_ms_min': round(min(t0), 3),
                               'refine_off_device_ms_by_kernel_class': {k: round(v['ms'], 3) for k, v in eng.timing_report().items() if v['ms'] > 0}}
                        eng.timing(False)
                    emit(a.out, {'what': 'eloc', 'ansatz': name, 'n_elec': n, 'lanes': (3 * n + 2 + 15) // 16 * 16, 'dtype': dn, 'walkers': a.walkers,
                                 'reps': a.reps, 'ms_median': round(float(np.median(t)), 3), 'ms_min': round(min(t), 3), 'n_refined': int(n_ref),
                                 'device_ms_by_kernel_class': rep, **off})
                    eng.close()


if __name__ == '__main__':
    main()
