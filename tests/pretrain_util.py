"""Checks of SCF-orbital pretraining (dqmc_pretrain_target, dqmc_orbitals, dqmc_orbitals_vjp, dqmc_pretrain_loss_grad) shared
by the emulated CPU tests and the GPU tests: a float64 torch restatement of the GTO target and of the loss, a synthetic
dataset in the shape `compute_scf_solution` returns, and torch.autograd through the float64 oracle's orbitals."""
import math

import numpy as np
import torch

from deepqmc_amd.engine import Engine
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.params import init_params
from deepqmc_amd.sampling import synthetic_walkers
from oracle import geom
from oracle import wf as owf
from param_grad_util import leaf_errors, small_spec

DFACT = {-1: 1.0, 1: 1.0, 3: 3.0, 5: 15.0}       # (2 l - 1)!! for l = 0 .. 3


def cartesian_angulars(l):
    return [(lx, ly, l - lx - ly) for lx in range(l, -1, -1) for ly in range(l - lx, -1, -1)]


def restated_aos(shells, r, R):
    """Cartesian GTOs [B, N, n_ao] at the electrons r[B, N, 3] around the nuclei R[n_nuc, 3], float64."""
    r, R = torch.as_tensor(r, dtype=torch.float64), torch.as_tensor(R, dtype=torch.float64)
    d = r[:, :, None, :] - R[None, None]
    d2 = (d ** 2).sum(-1)
    out = []
    for atom, (l, coeffs, zetas) in shells:
        coeffs, zetas = torch.as_tensor(np.asarray(coeffs, np.float64)), torch.as_tensor(np.asarray(zetas, np.float64))
        ls = torch.tensor(cartesian_angulars(l), dtype=torch.float64)
        anorms = torch.tensor([1 / math.sqrt(DFACT[2 * a - 1] * DFACT[2 * b - 1] * DFACT[2 * c - 1]) for a, b, c in cartesian_angulars(l)],
                              dtype=torch.float64)
        rnorms = (2 * zetas / math.pi) ** 0.75 * (4 * zetas) ** (l / 2)
        ang = torch.pow(d[:, :, atom, None, :], ls).prod(-1)                              # [B, N, n_comp]
        radial = (coeffs * rnorms * torch.exp(-torch.abs(zetas * d2[:, :, atom, None]))).sum(-1)
        out.append(anorms * ang * radial[..., None])
    return torch.cat(out, -1)


def restated_target(shells, mo_coeffs, confs, conf_coeffs, r, R):
    """[B, n_conf, N, N]: the molecular orbitals of every configuration, |c|^(1/N) on every column of determinant c and the
    sign of c on its column 0."""
    mos = restated_aos(shells, r, R) @ torch.as_tensor(np.asarray(mo_coeffs, np.float64))      # [B, N, n_mo]
    confs = torch.as_tensor(np.asarray(confs, np.int64))
    c = torch.as_tensor(np.asarray(conf_coeffs, np.float64))
    N = confs.shape[1]
    mos = mos[:, :, confs].permute(0, 2, 1, 3)                                                 # [B, n_conf, N, N]
    first = torch.zeros(N, dtype=torch.float64)
    first[0] = 1
    factors = (c.abs() ** (1 / N))[:, None] * (first[None] * torch.sign(c)[:, None] + (1 - first[None]))
    return mos * factors[None, :, None, :]


def restated_loss(orb, target, n_up, n_total):
    """orb [B, K, N, N], target [B, n_conf, N, N] -> (loss, per_sample_losses [B]): the target tiled to K determinants, its
    up-up block padded with zero columns on the right, its down-down block with zero columns on the left."""
    B, K, N, _ = orb.shape
    T = target.repeat(1, math.ceil(K / target.shape[1]), 1, 1)[:, :K]
    ps = 0
    if n_up > 0:
        t_up = torch.nn.functional.pad(T[:, :, :n_up, :n_up], (0, N - n_up))
        ps = ps + ((orb[:, :, :n_up] - t_up) ** 2).mean((1, 2, 3))
    if N > n_up:
        t_dn = torch.nn.functional.pad(T[:, :, n_up:, n_up:], (n_up, 0))
        ps = ps + ((orb[:, :, n_up:] - t_dn) ** 2).mean((1, 2, 3))
    return ps.sum() / n_total, ps


def synthetic_dataset(h, kind, seed=0, n_states=1):
    """A dataset dict in the shapes of compute_scf_solution.  Per atom two contracted s shells of 3 primitives and one p shell
    of 2, a d shell on the first atom.  kind 'hf': one configuration; 'cas': three, one with a negative coefficient."""
    rng = np.random.default_rng(seed)
    N, n_up, n_dn = h.n_up + h.n_down, h.n_up, h.n_down
    shells = []
    for a in range(h.n_nuc):
        for _ in range(2):
            shells.append((a, (0, rng.uniform(0.2, 0.8, 3), np.sort(rng.uniform(0.1, 3.0, 3))[::-1].copy())))
        shells.append((a, (1, rng.uniform(0.3, 0.9, 2), rng.uniform(0.2, 1.5, 2))))
        if a == 0:
            shells.append((a, (2, np.array([1.0]), np.array([0.6]))))
    n_ao = sum((l + 1) * (l + 2) // 2 for _, (l, _, _) in shells)
    n_mo = N + 3
    mo = rng.normal(size=(1, n_ao, n_mo)) * 0.5
    hf = list(range(n_up)) + list(range(n_dn))
    confs, coeffs = [], []
    for s in range(n_states):
        if kind == 'hf':
            cf, cc = [hf], [1.0]
        else:
            e1, e2 = list(hf), list(hf)
            e1[n_up - 1] = n_up + s                      # one up excitation
            if n_dn:
                e2[N - 1] = n_dn + 1 + s                 # one down excitation
            else:
                e2[0] = n_up + 1 + s
            cf, cc = [hf, e1, e2], [0.9 - 0.1 * s, -0.35, 0.2 + 0.05 * s]
        confs.append([cf])
        coeffs.append([cc])
    return {'centers': np.asarray(h.mol.coords, np.float64), 'shells': shells, 'mo_coeffs': mo,
            'confs': np.asarray(confs, np.int64), 'conf_coeffs': np.asarray(coeffs, np.float64)}


def torch_params(tree):
    return {m: {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in leaves.items()} for m, leaves in tree.items()}


def oracle_orbitals(spec, h, p, r, eps):
    """[B, K, N, N] through the float64 oracle (differentiable in the torch leaves p)."""
    R = torch.as_tensor(np.asarray(h.mol.coords), dtype=torch.float64)
    r = torch.as_tensor(np.asarray(r), dtype=torch.float64)
    return torch.stack([owf.orbitals(p, spec, r[b], R, h.n_up, eps)[0] for b in range(r.shape[0])])


def grads_of(p):
    """({module: {leaf: array}} with zeros where autograd left no gradient, the names of those leaves)."""
    none = sorted(f'{m}:{k}' for m, leaves in p.items() for k, v in leaves.items() if v.grad is None)
    return {m: {k: (v.grad.numpy().copy() if v.grad is not None else np.zeros(v.shape)) for k, v in leaves.items()} for m, leaves in p.items()}, none


def oracle_orbitals_vjp(spec, h, tree, r, cot, eps):
    p = torch_params(tree)
    (oracle_orbitals(spec, h, p, r, eps) * torch.as_tensor(np.asarray(cot, np.float64))).sum().backward()
    return grads_of(p)


def oracle_pretrain(spec, h, tree, r, dataset, state, n_total, eps):
    """(loss share of this state, per-sample losses, gradient tree, leaves without gradient) of the restated loss through the oracle."""
    p = torch_params(tree)
    T = restated_target(dataset['shells'], dataset['mo_coeffs'][0], dataset['confs'][state][0], dataset['conf_coeffs'][state][0], r,
                        h.mol.coords)
    loss, ps = restated_loss(oracle_orbitals(spec, h, p, r, eps), T, h.n_up, n_total)
    loss.backward()
    g, none = grads_of(p)
    return float(loss.detach()), ps.detach().numpy(), g, none


def make(name, molname, B, device, lib=None, dtype=torch.float64, seed=3, small=None):
    h = MolecularHamiltonian(mol=Molecule.from_name(molname))
    spec = small_spec(name, **(small or {}))
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=seed, perturb_envelopes=0.1)
    eng = Engine(spec, h, tree, dtype=dtype, device=device, lib=lib, norm_eps=geom.F32_EPS)
    return h, spec, tree, eng, synthetic_walkers(h, B, seed=seed + 1)


def upload(eng, ds, state=0):
    eng.set_pretrain_target(ds['shells'], ds['mo_coeffs'][0], ds['confs'][state][0], ds['conf_coeffs'][state][0])


def check_target(eng, h, ds, r, rtol, state=0):
    upload(eng, ds, state)
    got = eng.pretrain_target(torch.as_tensor(r, dtype=eng.dtype, device=eng.device)).cpu().double().numpy()
    ref = restated_target(ds['shells'], ds['mo_coeffs'][0], ds['confs'][state][0], ds['conf_coeffs'][state][0], r, h.mol.coords).numpy()
    print('target: largest relative deviation', float(np.max(np.abs(got - ref) / np.abs(ref))))
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=0)
    return got


def check_orbitals_vjp(eng, spec, h, tree, r, tol, seed=0):
    K, N = spec.n_determinants, h.n_up + h.n_down
    cot = np.random.default_rng(seed).normal(size=(r.shape[0], K, N, N))
    orb, g = eng.orbitals_vjp(torch.as_tensor(r, device=eng.device), torch.as_tensor(cot, device=eng.device))
    ref, none = oracle_orbitals_vjp(spec, h, tree, r, cot, geom.F32_EPS)
    got = eng.program.unflatten_grad(g)
    err = leaf_errors(got, ref)
    worst = max(err, key=err.get)
    print('orbitals_vjp: worst leaf', worst, err[worst])
    assert err[worst] < tol, (worst, err[worst])
    for name in none:
        m, k = name.rsplit(':', 1)
        assert np.all(got[m][k] == 0), name
    return orb, none


def check_loss_grad(eng, spec, h, tree, r, ds, tol, loss_rtol=1e-12, ps_rtol=1e-10):
    """pretrain_loss_grad on two walker slices (n_total = B each time) against the one-batch restated loss through autograd."""
    B = r.shape[0]
    upload(eng, ds)
    rt = torch.as_tensor(r, device=eng.device)
    cut = B // 3
    pa, ga = eng.pretrain_loss_grad(rt[:cut], n_total=B)
    pb, gb = eng.pretrain_loss_grad(rt[cut:], n_total=B)
    p1, g1 = eng.pretrain_loss_grad(rt)
    loss_ref, ps_ref, g_ref, _ = oracle_pretrain(spec, h, tree, r, ds, 0, B, geom.F32_EPS)
    ps = torch.cat([pa, pb]).cpu().numpy()
    loss = float(ps.sum()) / B
    print('pretrain_loss_grad: loss', loss, 'reference', loss_ref, 'relative', abs(loss - loss_ref) / abs(loss_ref))
    np.testing.assert_allclose(loss, loss_ref, rtol=loss_rtol)
    np.testing.assert_allclose(float(p1.sum()) / B, loss_ref, rtol=loss_rtol)
    np.testing.assert_allclose(ps, ps_ref, rtol=ps_rtol)
    for g in (ga + gb, g1):
        err = leaf_errors(eng.program.unflatten_grad(g), g_ref)
        worst = max(err, key=err.get)
        print('pretrain_loss_grad: worst leaf', worst, err[worst])
        assert err[worst] < tol, (worst, err[worst])
