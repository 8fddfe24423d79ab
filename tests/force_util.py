"""Shared checks of the coordinate gradients of log|psi| (dqmc_log_psi_grad_coords) and of the Hellmann-Feynman force
estimators (dqmc_hf_force, deepqmc_amd/force.py): torch.autograd of the float64 oracle with respect to r and R, and a
float64 torch restatement of the estimator formulas (Assaraf and Caffarel, J. Chem. Phys. 119, 10536 (2003))."""
import numpy as np
import torch

from deepqmc_amd.engine import Engine
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.params import init_params
from deepqmc_amd.sampling import synthetic_walkers
from oracle import geom
from oracle import wf as owf
from param_grad_util import small_spec


def oracle_grad_coords(spec, h, tree, r, eps):
    """d log|psi| / d r [B, N, 3] and d log|psi| / d R [B, n_nuc, 3] by torch.autograd through the float64 oracle."""
    p = owf.to_torch(tree)
    R0 = torch.as_tensor(np.asarray(h.mol.coords), dtype=torch.float64)
    gr, gR = [], []
    for rb in np.asarray(r, np.float64):
        x = torch.tensor(rb, requires_grad=True)
        R = R0.clone().requires_grad_(True)
        log = owf.wave_function(p, spec, x, R, h.n_up, eps)[1]
        a, c = torch.autograd.grad(log, (x, R))
        gr.append(a.numpy())
        gR.append(c.numpy())
    return np.stack(gr), np.stack(gR)


def walker_errors(got, ref):
    """Normwise relative error per walker: |got_b - ref_b| / |ref_b| over the walker's rows."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    B = ref.shape[0]
    return np.linalg.norm((got - ref).reshape(B, -1), axis=1) / np.maximum(np.linalg.norm(ref.reshape(B, -1), axis=1), 1e-300)


def setup(name, molname, B, device, lib=None, dtype=torch.float64, seed=3, **spec_kw):
    h = MolecularHamiltonian(mol=Molecule.from_name(molname))
    spec = small_spec(name, **spec_kw)
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=seed, perturb_envelopes=0.1)
    eng = Engine(spec, h, tree, dtype=dtype, device=device, lib=lib, norm_eps=geom.F32_EPS)
    r = synthetic_walkers(h, B, seed=seed + 1)
    return h, spec, tree, eng, r


def check_coords_against_oracle(name, molname, B, device, lib=None, tol=1e-9, **spec_kw):
    h, spec, tree, eng, r = setup(name, molname, B, device, lib, **spec_kw)
    sign, log, gr, gR = eng.log_psi_grad_coords(torch.as_tensor(r, device=device))
    ref_r, ref_R = oracle_grad_coords(spec, h, tree, r, geom.F32_EPS)
    er, eR = walker_errors(gr.cpu().numpy(), ref_r), walker_errors(gR.cpu().numpy(), ref_R)
    assert er.max() < tol and eR.max() < tol, (er.max(), eR.max())
    return eng, er, eR


def restated_force(est, r, R, Z, grad_r=None, grad_R=None, e_loc=None, energy=0.0):
    """The estimators written out from their definitions, per walker, float64 [B, n_nuc, 3].  With d = r_i - R_I, u = d / |d|:
    nuclear -dE_nn/dR_I; bare adds -dV_en/dR_I = Z_I sum_i d / |d|^3; the ZVQ family replaces it by grad_r log psi . grad_r Q_I
    with Q_I = Z_I sum_i u; the zero-bias terms add -2 (E_loc - E) times Q_I (ZVZBQ) or d log psi / dR_I (ZB, ZVQZB)."""
    t = lambda x: torch.as_tensor(x).double().cpu()
    r, R, Z = t(r), t(R), t(Z)
    n_nuc = R.shape[0]
    f_nn = torch.zeros(n_nuc, 3, dtype=torch.float64)
    for I in range(n_nuc):
        for J in range(n_nuc):
            if I != J:
                dIJ = R[I] - R[J]
                f_nn[I] += Z[I] * Z[J] * dIJ / dIJ.norm() ** 3
    f = f_nn[None].expand(r.shape[0], -1, -1).clone()
    if est == 'nuclear':
        return f
    d = r[:, None, :, :] - R[None, :, None, :]            # [B, n_nuc, N, 3]
    rho = d.norm(dim=-1, keepdim=True)
    u = d / rho
    if est in ('bare', 'ac_zb'):
        f = f + Z[None, :, None] * (d / rho ** 3).sum(2)
    else:
        g = t(grad_r)[:, None]                              # [B, 1, N, 3]
        f = f + Z[None, :, None] * ((g - (u * g).sum(-1, keepdim=True) * u) / rho).sum(2)
    if est in ('ac_zvzbq', 'ac_zb', 'ac_zvqzb'):
        de = -2 * (t(e_loc) - float(energy))[:, None, None]
        f = f + de * (Z[None, :, None] * u.sum(2) if est == 'ac_zvzbq' else t(grad_R))
    return f


def mirror(r, R, r_cut):
    """The antithetic configuration: electrons within r_cut of their nearest nucleus reflected through it (numpy)."""
    r, R = np.asarray(r, np.float64), np.asarray(R, np.float64)
    out = r.copy()
    for b in range(r.shape[0]):
        for i in range(r.shape[1]):
            d2 = ((r[b, i] - R) ** 2).sum(-1)
            a = int(np.argmin(d2))
            if d2[a] < r_cut ** 2:
                out[b, i] = 2 * R[a] - r[b, i]
    return out
