"""Times TransPsiformer training (option "nuclear_reverse"): cyclobutadiene (C4H4) / TransPsiformer at production widths, float32
walkers at defaults on the MI355X, one process, device-synchronised host clock, warm-up first, median and minimum of --reps:
  weights_from_params   dqmc_weights_from_params with the nuclear stream registered (fold + scatter + re-pack) against a context
                        of the same program without one (copy + re-pack), alternated call by call
  fold_vjp              dqmc_grad_to_params with the stream (gathers + nuc_fold_vjp) against the context without one (gather):
                        the differences are the fold and its VJP alone
  log_psi_vjp           dqmc_log_psi_vjp (attention backward with constant rows) alternated with dqmc_local_energy
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
    on = Engine(spec, h, tree, dtype=torch.float32, device=dev, lib=lib, nuclear_reverse=True)
    # the same ansatz compiled without the flag: the parameter map alone, no registered stream (what a device update and the
    # gradient gather cost without the fold); the C ABI directly, since the package refuses device updates for such a program
    off = Engine(spec, h, tree, dtype=torch.float32, device=dev, lib=lib)
    lib_ = on.lib
    src = np.ascontiguousarray(off.program.grad_src, np.int32)
    n_off = off.program.n_params()
    off._check(lib_.dqmc_set_param_map(off._ctx, src.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), src.size, n_off))
    th = np.zeros(n_off)
    th[src[src >= 0]] = off.program.weights[src >= 0]
    theta_off = torch.as_tensor(th, dtype=torch.float64, device=dev)
    gt_off = torch.empty(n_off, dtype=torch.float64, device=dev)
    theta = on.params_flat()
    r = torch.as_tensor(synthetic_walkers(h, a.walkers, seed=1), dtype=torch.float32, device=dev)
    _, _, g = on.log_psi_vjp(r)
    assert g.numel() == off.program.weights.size

    def wfp(eng, th_):
        eng._check(lib_.dqmc_weights_from_params(eng._ctx, th_.data_ptr()))

    calls = {'weights_from_params_stream': lambda: wfp(on, theta), 'weights_from_params_plain': lambda: wfp(off, theta_off),
             'grad_to_params_stream': lambda: on.grad_to_params(g),
             'grad_to_params_plain': lambda: off._check(lib_.dqmc_grad_to_params(off._ctx, g.data_ptr(), gt_off.data_ptr())),
             'log_psi_vjp': lambda: on.log_psi_vjp(r), 'local_energy': lambda: on.local_energy(r)}
    for f in calls.values():          # warm-up: code objects, workspaces, gather tables, the float64 twin
        f(); f()
    sync()
    t = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            sync()
            t[k].append(1e3 * (time.perf_counter() - t0))
    on.log_psi_vjp(r)
    out = {'system': f'{a.molecule}/transpsiformer', 'electrons': h.n_elec, 'nuclei': h.n_nuc, 'embedding_dim': spec.embedding_dim,
           'layers': spec.n_interactions, 'determinants': spec.n_determinants, 'walkers': a.walkers, 'dtype': 'float32', 'reps': a.reps,
           'vjp_chunks': on.last_chunks()['own'], 'n_params': on.program.n_params(), 'n_weights': int(on.program.weights.size),
           'n_derived': int(on.program.nuclear_stream['n_derived']), 'tiny': bool(a.tiny)}
    for k, v in t.items():
        out[f'{k}_ms'] = round(float(np.median(v)), 4)
        out[f'{k}_min_ms'] = round(min(v), 4)
    out['fold_ms'] = round(out['weights_from_params_stream_ms'] - out['weights_from_params_plain_ms'], 4)
    out['fold_vjp_ms'] = round(out['grad_to_params_stream_ms'] - out['grad_to_params_plain_ms'], 4)
    print(json.dumps(out), flush=True)
    on.close()
    off.close()


if __name__ == '__main__':
    main()
