"""Times the per-walker parameter partials of the nuclear-token stream (option "nuclear_params"): cyclobutadiene (C4H4) /
TransPsiformer at production widths, float32 walkers at defaults on the MI355X, one process, device-synchronised host clock,
warm-up first, median and minimum of --reps, the calls alternated round by round:
  jacobian              log_psi_jacobian + jacobian_to_params: the [B, n_params] rows (the stream's partials per walker included)
  jacobian_to_params    the second call alone
  log_psi_vjp           dqmc_log_psi_vjp + dqmc_grad_to_params of the same context
  kfac_step             one KFACOptimizer step (local energies, dqmc_log_psi_kfac, direction, update) on the walkers of the call
  adam_step             one AdamOptimizer step on the same walkers
  kfac_direction        Engine.kfac_direction alone, from the factors of one dqmc_log_psi_kfac call
and, from device events, the share of the batched adjoint chain and of k_nucb_dw in jacobian_to_params and in kfac_direction.
The Jacobian is B x n_weights plus B x n_params in the context's precision: if the rows do not fit beside the call's workspace
the walkers are halved until they do, and the number used is reported (the model is never shrunk).
Prints one JSON line.  --tiny: narrow widths and few walkers (a rehearsal of the script, not a measurement)."""
import argparse
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
from deepqmc_amd.optimizer import AdamOptimizer, KFACOptimizer  # noqa: E402
from deepqmc_amd.sampling import synthetic_walkers  # noqa: E402
from deepqmc_amd.spec import ANSATZES  # noqa: E402
from deepqmc_amd.wf import NeuralNetworkWaveFunction  # noqa: E402


def timed(calls, reps, sync):
    for f in calls.values():          # warm-up: code objects, workspaces, tables
        f(); f()
    sync()
    t = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            sync()
            t[k].append(1e3 * (time.perf_counter() - t0))
    return t


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
    wf = NeuralNetworkWaveFunction(h, spec, dtype=torch.float32, device=a.device, lib=lib, nuclear_params=True)
    params = wf.init(7, perturb_envelopes=0.1)
    eng = wf.engine(params)
    prog = eng.program
    r = torch.as_tensor(synthetic_walkers(h, a.walkers, seed=1), dtype=torch.float32, device=dev)

    # ---- the Jacobian rows against the VJP: the largest B whose rows fit
    B = a.walkers
    while True:
        try:
            J = torch.empty(B, prog.weights.size, dtype=torch.float32, device=dev)
            Jp = torch.empty(B, prog.n_params(), dtype=torch.float32, device=dev)
            rb = r[:B].contiguous()
            s, l, _ = eng.log_psi_jacobian(rb, out=J)
            eng.jacobian_to_params(J, l, s, out=Jp)
            sync()
            break
        except (torch.OutOfMemoryError, RuntimeError) as e:
            if B == 1 or 'memory' not in str(e).lower():
                raise
            J = Jp = None
            B //= 2

    def jacobian():
        s_, l_, _ = eng.log_psi_jacobian(rb, out=J)
        eng.jacobian_to_params(J, l_, s_, out=Jp)

    def vjp():
        eng.grad_to_params(eng.log_psi_vjp(rb)[2])

    t = timed({'jacobian': jacobian, 'jacobian_to_params': lambda: eng.jacobian_to_params(J, l, s, out=Jp), 'log_psi_vjp': vjp}, a.reps, sync)
    eng.timing(True)
    eng.timing_reset()
    eng.jacobian_to_params(J, l, s, out=Jp)
    rep_j = eng.timing_report()
    eng.timing(False)
    jac_chunks = eng.last_chunks()['own']
    jac_bytes = J.numel() * 4 + Jp.numel() * 4
    J = Jp = None

    # ---- one training step: KFAC against Adam on the walkers of the call, and the direction alone
    batch = (r[None, None], None, None)
    kfac, adam = KFACOptimizer(1e-4).bind(h, wf), AdamOptimizer(1e-5).bind(h, wf)
    st_k, st_a = kfac.init(0, [params], batch), adam.init(0, [params], batch)
    lay = prog.kfac_layout()
    fac = torch.empty(lay['n_factor_doubles'], dtype=torch.float64, device=dev)
    rest = torch.empty(a.walkers, lay['n_rest'], dtype=torch.float32, device=dev)
    cot = torch.randn(a.walkers, dtype=torch.float32, device=dev) / a.walkers
    sign, logpsi, g, _, _ = eng.log_psi_kfac(r, cot, out=(fac, rest))
    gt = eng.grad_to_params(g)
    state = eng.kfac_state()
    out_d = (torch.empty_like(gt), torch.empty(1, dtype=torch.float64, device=dev))
    eng.kfac_direction(gt, fac, rest, logpsi, sign, state, True, 0.95, 1e-3, out=out_d)
    calls = {'kfac_step': lambda: kfac.step(0, [params], st_k, batch), 'adam_step': lambda: adam.step(0, [params], st_a, batch),
             'kfac_direction': lambda: eng.kfac_direction(gt, fac, rest, logpsi, sign, state, False, 0.95, 1e-3, out=out_d)}
    t.update(timed(calls, a.reps, sync))
    eng.timing(True)
    eng.timing_reset()
    eng.kfac_direction(gt, fac, rest, logpsi, sign, state, False, 0.95, 1e-3, out=out_d)
    rep_k = eng.timing_report()
    eng.timing(False)

    blocks, _ = prog.kfac_blocks()
    n_own = int(sum(np.prod(shape) for (m, _), (_, shape) in prog.grad_leaves.items() if m not in blocks and 'nucle' in m))
    out = {'system': f'{a.molecule}/transpsiformer', 'electrons': h.n_elec, 'nuclei': h.n_nuc, 'embedding_dim': spec.embedding_dim,
           'layers': spec.n_interactions, 'determinants': spec.n_determinants, 'walkers': a.walkers, 'dtype': 'float32', 'reps': a.reps,
           'n_weights': int(prog.weights.size), 'n_params': int(prog.n_params()), 'stream_diagonal_elements': n_own,
           'jacobian_walkers': B, 'jacobian_bytes': int(jac_bytes), 'jacobian_bytes_per_walker': int(jac_bytes // B),
           'jacobian_to_params_chunks': jac_chunks, 'tiny': bool(a.tiny)}
    for k, v in t.items():
        out[f'{k}_ms'] = round(float(np.median(v)), 4)
        out[f'{k}_min_ms'] = round(min(v), 4)
    for tag, rep in (('jacobian_to_params', rep_j), ('kfac_direction', rep_k)):
        out[f'{tag}_chain_event_ms'] = round(rep['nuc_rows_chain']['ms'], 4)
        out[f'{tag}_k_nucb_dw_event_ms'] = round(rep['nucb_dw']['ms'], 4)
        out[f'{tag}_k_nucb_dw_share'] = round(rep['nucb_dw']['ms'] / out[f'{tag}_ms'], 4)
    print(json.dumps(out), flush=True)
    wf.release()


if __name__ == '__main__':
    main()
