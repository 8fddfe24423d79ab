"""Times Engine.ecp_force('bare') against Engine.local_energy (same ECP, same seed) at 4096 float32 walkers: LiH / PauliNet
with synthetic two-centre tables and N2 / FermiNet with synthetic tables on both atoms, alternating the two calls in one run
(device-synchronised host clock, warm-up first).  Prints one JSON line per system.  --profile N: only N force calls per
system (for a rocprofv3 --kernel-trace --stats run of its own)."""
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

# synthetic coefficient tables in pyscf's ECP format (deepqmc_amd/ecp.py); n_core, local r^-1 / r^0 / r^1 terms, s and p channels
LOC_LI = [-1, [[], [[5.4104, 1.0]], [[4.6015, -4.6015]], [[2.7052, 5.4104]]]]
LOC_H = [-1, [[], [[21.24, 1.0]], [[21.78, -10.85]], [[21.24, 21.24]]]]
LOC_N = [-1, [[], [[12.9, 5.0]], [[12.3, -9.2]], [[12.9, 64.5]]]]
TABLES = {
    'LiH': {'Li': [0, [LOC_LI, [0, [[], [], [[1.3302, 6.7529], [0.9, -0.8]]]], [1, [[], [], [[1.25, 0.45]]]]]],
            'H': [0, [LOC_H, [0, [[], [], [[0.7, 0.3]]]]]]},
    'N2': {'N': [2, [LOC_N, [0, [[], [], [[9.2, 43.7], [3.1, -1.9]]]], [1, [[], [], [[2.6, 0.8]]]]]]},
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--walkers', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--profile', type=int, default=0)
    a = ap.parse_args()
    for mol, name in (('LiH', 'paulinet'), ('N2', 'ferminet')):
        m = Molecule.from_name(mol)
        h = MolecularHamiltonian(mol=m, ecp_type='synthetic', ecp_mask=[True] * len(m.charges), ecp_tables=TABLES[mol])
        spec = ANSATZES[name]()
        tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=7, perturb_envelopes=0.1)
        eng = Engine(spec, h, tree, dtype=torch.float32, device='cuda:0')
        r = torch.as_tensor(synthetic_walkers(h, a.walkers, seed=1), dtype=torch.float32, device='cuda:0')
        if a.profile:
            for _ in range(a.profile):
                eng.ecp_force('bare', r, rng=5)
            torch.cuda.synchronize()
            eng.close()
            continue
        calls = {'ecp_force': lambda: eng.ecp_force('bare', r, rng=5), 'local_energy': lambda: eng.local_energy(r, rng=5)}
        for f in calls.values():          # warm-up: code objects, workspaces, gather tables, the float64 twin
            f(); f()
        calls['ecp_force']()
        chunks = eng.last_chunks()['own']
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, f in calls.items():
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                t[k].append(1e3 * (time.perf_counter() - t0))
        med = {k: float(np.median(v)) for k, v in t.items()}
        n_nl = len(h.pot.nuc_with_nl_pot)
        print(json.dumps({'system': f'{mol}/{name}', 'walkers': a.walkers, 'dtype': 'float32', 'reps': a.reps, 'n_elec': h.n_elec,
                          'n_nl': n_nl, 'configs_per_walker': 1 + 11 * n_nl * h.n_elec, 'chunks': chunks,
                          'ecp_force_ms': round(med['ecp_force'], 3), 'local_energy_ms': round(med['local_energy'], 3),
                          'ecp_force_min_ms': round(min(t['ecp_force']), 3), 'local_energy_min_ms': round(min(t['local_energy']), 3),
                          'ecp_force_over_local_energy': round(med['ecp_force'] / med['local_energy'], 2)}), flush=True)
        eng.close()


if __name__ == '__main__':
    main()
