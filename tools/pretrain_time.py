"""Times dqmc_pretrain_loss_grad against dqmc_log_psi_vjp at 4096 float32 walkers, LiH / PauliNet and N2 / FermiNet,
alternating the two in one run (device-synchronised host clock, warm-up first).  Prints one JSON line per system, with the
share of the target and loss kernels in the call (per-launch HIP-event timing in a pass of its own).  --profile N: only N
pretraining calls per system (for a rocprofv3 --kernel-trace --stats run of its own)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepqmc_amd import MolecularHamiltonian, Molecule  # noqa: E402
from deepqmc_amd.engine import Engine  # noqa: E402
from deepqmc_amd.params import init_params  # noqa: E402
from deepqmc_amd.sampling import synthetic_walkers  # noqa: E402
from deepqmc_amd.spec import ANSATZES  # noqa: E402
from pretrain_util import synthetic_dataset, upload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--walkers', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--profile', type=int, default=0)
    a = ap.parse_args()
    for mol, name in (('LiH', 'paulinet'), ('N2', 'ferminet')):
        h = MolecularHamiltonian(mol=Molecule.from_name(mol))
        spec = ANSATZES[name]()
        tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=7, perturb_envelopes=0.1)
        eng = Engine(spec, h, tree, dtype=torch.float32, device='cuda:0')
        r = torch.as_tensor(synthetic_walkers(h, a.walkers, seed=1), dtype=torch.float32, device='cuda:0')
        upload(eng, synthetic_dataset(h, 'cas', seed=3))
        if a.profile:
            for _ in range(a.profile):
                eng.pretrain_loss_grad(r)
            torch.cuda.synchronize()
            continue
        calls = {'pretrain': lambda: eng.pretrain_loss_grad(r), 'vjp': lambda: eng.log_psi_vjp(r)}
        for f in calls.values():          # warm-up: code objects, workspaces, gather tables
            f(); f()
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, f in calls.items():
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                t[k].append(1e3 * (time.perf_counter() - t0))
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = {k: float(np.percentile(v, 75) - np.percentile(v, 25)) for k, v in t.items()}
        eng.timing(True)                  # per-launch events serialise the call: shares only, not the times above
        eng.timing_reset()
        for _ in range(5):
            eng.pretrain_loss_grad(r)
        rep = eng.timing_report()
        eng.timing(False)
        total = sum(v['ms'] for v in rep.values())
        share = {k: round(rep[k]['ms'] / total, 4) if k in rep else 0.0 for k in ('pretrain_target', 'pretrain_loss')}
        print(json.dumps({'system': f'{mol}/{name}', 'walkers': a.walkers, 'dtype': 'float32', 'reps': a.reps,
                          'pretrain_ms': round(med['pretrain'], 3), 'vjp_ms': round(med['vjp'], 3),
                          'pretrain_min_ms': round(min(t['pretrain']), 3), 'vjp_min_ms': round(min(t['vjp']), 3),
                          'pretrain_iqr_ms': round(spread['pretrain'], 3), 'vjp_iqr_ms': round(spread['vjp'], 3),
                          'pretrain_over_vjp': round(med['pretrain'] / med['vjp'], 3), 'timed_kernel_share': share}), flush=True)
        eng.close()


if __name__ == '__main__':
    main()
