"""Times the per-walker backward of the nuclear-token stream (option "nuclear_coords"): cyclobutadiene (C4H4) / TransPsiformer at
production widths, float32 walkers at defaults on the MI355X, one process, device-synchronised host clock, warm-up first, median
and minimum of --reps, the calls alternated round by round:
  grad_coords_R         log_psi_grad_coords with want_R=True (the stream's backward runs, batched over the walkers)
  grad_coords_r         log_psi_grad_coords with want_R=False (it never does): the difference is the new code
  log_psi_vjp           dqmc_log_psi_vjp of the same context
and, from device events (dqmc_debug_nuc_dx_time), the batched dX kernel k_nucb_dx against launch_linear_bwd<double> restricted
to dX (k_lin_dz + k_lin_dx) on the stream's largest token-row shape (walkers x n_nuc rows, D x D).
Prints one JSON line.  --tiny: narrow widths and few walkers (a rehearsal of the script, not a measurement)."""
import argparse
import ctypes
import dataclasses
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--walkers', type=int, default=512)
    ap.add_argument('--molecule', default='cyclobutadiene_square')
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--tiny', action='store_true')
    a = ap.parse_args()
    dev = torch.device(a.device)
    lib = None
    if dev.type != 'cuda':
        if not a.tiny:
            raise SystemExit('a measurement needs the GPU (--tiny on the CPU rehearses the script through the SIMT emulation)')
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        from simt_util import emu_lib
        lib = emu_lib()
    sync = torch.cuda.synchronize if dev.type == 'cuda' else (lambda: None)
    h = MolecularHamiltonian(mol=Molecule.from_name(a.molecule))
    spec = ANSATZES['transpsiformer'](h.mol.charges)
    if a.tiny:
        spec = dataclasses.replace(spec, embedding_dim=32, n_interactions=2, n_determinants=2)
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=7, perturb_envelopes=0.1)
    eng = Engine(spec, h, tree, dtype=torch.float32, device=dev, lib=lib, nuclear_coords=True)
    r = torch.as_tensor(synthetic_walkers(h, a.walkers, seed=1), dtype=torch.float32, device=dev)
    calls = {'grad_coords_R': lambda: eng.log_psi_grad_coords(r), 'grad_coords_r': lambda: eng.log_psi_grad_coords(r, want_R=False),
             'log_psi_vjp': lambda: eng.log_psi_vjp(r)}
    for f in calls.values():          # warm-up: code objects, workspaces, gather tables
        f(); f()
    sync()
    t = {k: [] for k in calls}
    chunks = {}
    for _ in range(a.reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            sync()
            t[k].append(1e3 * (time.perf_counter() - t0))
            chunks[k] = eng.last_chunks()['own']
    # the stream's share by device events
    eng.timing(True)
    eng.timing_reset()
    eng.log_psi_grad_coords(r)
    rep = eng.timing_report()
    eng.timing(False)
    ms2, shape3 = (ctypes.c_double * 2)(), (ctypes.c_int * 3)()
    eng._check(eng.lib.dqmc_debug_nuc_dx_time(eng._ctx, a.walkers, a.reps, ms2, shape3))
    out = {'system': f'{a.molecule}/transpsiformer', 'electrons': h.n_elec, 'nuclei': h.n_nuc, 'embedding_dim': spec.embedding_dim,
           'layers': spec.n_interactions, 'determinants': spec.n_determinants, 'walkers': a.walkers, 'dtype': 'float32', 'reps': a.reps,
           'chunks': chunks, 'n_derived': int(eng.program.nuclear_stream['n_derived']), 'tiny': bool(a.tiny)}
    for k, v in t.items():
        out[f'{k}_ms'] = round(float(np.median(v)), 4)
        out[f'{k}_min_ms'] = round(min(v), 4)
    out['stream_backward_ms'] = round(out['grad_coords_R_ms'] - out['grad_coords_r_ms'], 4)
    out['nuc_coords_event_ms'] = round(rep['nuc_coords']['ms'], 4)
    out['dx_shape'] = list(shape3)
    out['k_nucb_dx_ms'] = round(ms2[0], 4)
    out['linear_bwd_f64_dx_ms'] = round(ms2[1], 4)
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == '__main__':
    main()
