"""Checks of the per-walker parameter Jacobian of log|psi| (dqmc_log_psi_jacobian) shared by the emulated CPU tests and the GPU
tests: rows against torch.autograd through the float64 oracle, the transpose of the VJP, and the natural-gradient identity."""
import numpy as np
import torch

from deepqmc_amd.engine import Engine
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.params import init_params
from deepqmc_amd.sampling import synthetic_walkers
from oracle import geom
from param_grad_util import leaf_errors, oracle_vjp, small_spec


def jac_engine(name, molname, B, device, lib=None, seed=3, dtype=torch.float64, **spec_kw):
    h = MolecularHamiltonian(mol=Molecule.from_name(molname))
    spec = small_spec(name, **spec_kw)
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=seed, perturb_envelopes=0.1)
    eng = Engine(spec, h, tree, dtype=dtype, device=device, lib=lib, norm_eps=geom.F32_EPS)
    return h, spec, tree, eng, torch.as_tensor(synthetic_walkers(h, B, seed=seed + 1), dtype=dtype, device=device)


def linear_padding_mask(program):
    """Flat weight entries that are padding of a linear weight block (rows >= K or columns >= nout)."""
    pad = np.zeros(program.weights.size, bool)
    for op in program.ops:
        if op.kind != 3:
            continue
        i = op.i
        ldw, w_off, row = (i[21] + 3) // 4 * 4, i[22], 0
        for p in range(i[0]):
            K = i[3 + 4 * p]
            Kp = (K + 3) // 4 * 4
            blk = np.zeros((Kp, ldw), bool)
            blk[K:] = True
            blk[:, i[21]:] = True
            pad[w_off + row * ldw:w_off + (row + Kp) * ldw] = blk.reshape(-1)
            row += Kp
        if i[23] >= 0:
            pad[i[23] + i[21]:i[23] + ldw] = True
    return pad


def check_transpose_of_vjp(eng, r, seed=0, tol=1e-12):
    """J^T c equals log_psi_vjp(r, c) on every flat entry, relative to ||vjp||; linear-layer padding columns of J are 0."""
    B = r.shape[0]
    s, l, J = eng.log_psi_jacobian(r)
    assert J.shape == (B, eng.program.weights.size) and J.dtype == eng.dtype
    c = torch.as_tensor(np.random.default_rng(seed).normal(size=B), dtype=eng.dtype, device=r.device)
    s2, l2, g = eng.log_psi_vjp(r, c)
    assert torch.equal(s, s2) and torch.equal(l, l2)
    jtc = torch.matmul(c.double(), J.double())
    err = float((jtc - g).abs().max() / g.norm())
    assert err < tol, err
    pad = torch.as_tensor(linear_padding_mask(eng.program), device=J.device)
    assert bool((J[:, pad] == 0).all())
    return J, bool(pad.any())


def check_rows_against_oracle(h, spec, tree, eng, r, rows, tol):
    """Rows of unflatten_jacobian(J) against torch.autograd of log|psi(r_b)| through the float64 oracle, leaf-relative."""
    _, _, J = eng.log_psi_jacobian(r)
    Jp = eng.program.unflatten_jacobian(J)
    assert Jp.shape == (r.shape[0], eng.program.n_params()) and Jp.device == J.device and Jp.dtype == J.dtype
    rn = r.cpu().numpy()
    for b in rows:
        ref = oracle_vjp(spec, h, tree, rn[b:b + 1], np.ones(1), geom.F32_EPS)
        err = leaf_errors(eng.program.unflatten_params(Jp[b]), ref)
        worst = max(err, key=err.get)
        assert err[worst] < tol, (b, worst, err[worst])


def check_natgrad(wf, trees, r, damping=1e-3, tol=1e-12):
    """delta of compute_energy_loss_and_natgrad solves (A^T A + damping I) delta = g, A formed here from the Jacobian."""
    from deepqmc_amd.loss import compute_energy_loss_and_natgrad, median_clip_and_mask
    loss, deltas, stats = compute_energy_loss_and_natgrad(None, wf.hamil, wf, trees, r, damping=damping)
    e = stats['E_loc'][0].double()
    for s in range(len(trees)):
        eng = wf.engine(trees[s])
        _, Jp = wf.log_psi_jacobian(trees[s], r[0, s].contiguous())
        Jp = Jp.double()
        _, mask = median_clip_and_mask(e[s])
        m = mask.double().to(Jp.device)
        n_s = m.sum()
        A = (Jp - (m / n_s) @ Jp) * torch.sqrt(m / n_s)[:, None]
        flat = lambda t: torch.as_tensor(np.concatenate([t[mod][leaf].reshape(-1) for (mod, leaf) in eng.program.grad_leaves]),
                                         device=Jp.device)
        d, g = flat(deltas[s]), flat(stats['grad'][s])
        # normwise backward error of the solve, |M d - g| / (|M| |d| + |g|) with M = A^T A + damping I and |M| <= |A|_F^2 + damping:
        # forming A^T (A d) itself rounds at eps |A|^2 |d|, which exceeds eps |g| by up to |A|^2 / damping
        res = A.T @ (A @ d) + damping * d - g
        err = float(res.norm() / ((A.norm() ** 2 + damping) * d.norm() + g.norm()))
        assert err < tol, (s, err)
    return loss, deltas, stats
