"""Times the reverse pass through attention (option "attention_reverse"): dqmc_log_psi_vjp and dqmc_log_psi_grad_coords of float32
Psiformers, alternated with dqmc_local_energy in one process (device-synchronised host clock, warm-up first, median and minimum
of --reps), and the per-record split of one VJP from dqmc_timing (attention_bwd against linear_bwd, slogdet_bwd, orbitals_bwd).
Systems: LiH at 4096 walkers, and benzene at the largest power-of-two walker count up to --max-walkers whose VJP runs as one
walker chunk under the default "ws_budget_mb".  Prints one JSON line per system.  --profile N: only N VJP calls per system
(for a rocprofv3 --kernel-trace --stats run of its own)."""
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

SPLIT = ('attention_bwd', 'linear_bwd', 'slogdet_bwd', 'orbitals_bwd')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--max-walkers', type=int, default=4096)
    ap.add_argument('--systems', default='LiH,benzene')
    ap.add_argument('--profile', type=int, default=0)
    a = ap.parse_args()
    for mol in a.systems.split(','):
        h = MolecularHamiltonian(mol=Molecule.from_name(mol))
        spec = ANSATZES['psiformer']()
        tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=7, perturb_envelopes=0.1)
        eng = Engine(spec, h, tree, dtype=torch.float32, device='cuda:0')
        eng.set_option('attention_reverse', 1)
        walkers = 4096 if mol == 'LiH' else a.max_walkers
        r = torch.as_tensor(synthetic_walkers(h, walkers, seed=1), dtype=torch.float32, device='cuda:0')
        while mol != 'LiH':          # the largest power of two that is one chunk
            eng.log_psi_vjp(r)
            if eng.last_chunks()['own'] == 1 or walkers <= 64:
                break
            walkers //= 2
            r = r[:walkers].contiguous()
        if a.profile:
            for _ in range(a.profile):
                eng.log_psi_vjp(r)
            torch.cuda.synchronize()
            continue
        calls = {'vjp': lambda: eng.log_psi_vjp(r), 'grad_coords': lambda: eng.log_psi_grad_coords(r),
                 'local_energy': lambda: eng.local_energy(r)}
        for f in calls.values():          # warm-up: code objects, workspaces, gather tables, the float64 twin
            f(); f()
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, f in calls.items():
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                t[k].append(1e3 * (time.perf_counter() - t0))
        chunks = {}
        for k in ('vjp', 'grad_coords'):
            calls[k]()
            chunks[k] = eng.last_chunks()['own']
        eng.timing(True)
        eng.timing_reset()
        eng.log_psi_vjp(r)
        torch.cuda.synchronize()
        rep = eng.timing_report()
        eng.timing(False)
        total = sum(v['ms'] for v in rep.values())
        out = {'system': f'{mol}/psiformer', 'electrons': h.n_elec, 'walkers': walkers, 'dtype': 'float32', 'reps': a.reps, 'chunks': chunks}
        for k, v in t.items():
            out[f'{k}_ms'] = round(float(np.median(v)), 3)
            out[f'{k}_min_ms'] = round(min(v), 3)
        out['vjp_records_ms'] = {k: round(rep[k]['ms'], 3) for k in sorted(rep, key=lambda k: -rep[k]['ms'])}
        out['vjp_records_total_ms'] = round(total, 3)
        out['split_share_of_vjp_records'] = {k: round(rep[k]['ms'] / total, 4) for k in SPLIT if k in rep}
        print(json.dumps(out), flush=True)
        eng.close()


if __name__ == '__main__':
    main()
