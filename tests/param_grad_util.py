"""Checks of the parameter gradient of log|psi| (dqmc_log_psi_vjp) shared by the emulated CPU tests and the GPU tests:
the reference's own golden, and torch.autograd through the float64 oracle."""
import dataclasses
import os

import numpy as np
import torch

from deepqmc_amd.engine import Engine
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.params import init_params
from deepqmc_amd.sampling import synthetic_walkers
from deepqmc_amd.spec import ANSATZES
from oracle import geom
from oracle import wf as owf
from ref_ansatz_util import reference_test_engine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_grad_psi.npz')


def check_grad_golden(kats, device, lib=None):
    """Every leaf of d log|psi| / d theta of the reference's test ansatz at its canonical LiH walker against the reference's
    tests/test_wf/test_grad_psi.npz, at the reference's tolerance (rtol 1e-4, atol 1e-6)."""
    h, P, tree, eng = reference_test_engine(device, lib=lib, norm_eps=geom.F64_EPS)
    r = torch.as_tensor(kats['lih_edges_ne'][0][None], dtype=torch.float64, device=device)
    sign, log, g = eng.log_psi_vjp(r)
    assert int(sign[0]) == int(kats['wf_psi_sign'])
    np.testing.assert_allclose(float(log[0]), float(kats['wf_psi_log']), rtol=0, atol=2e-6)
    got = eng.program.unflatten_grad(g)
    gold = np.load(GOLDEN)
    assert len(gold.files) == 37
    for key in gold.files:
        mod, leaf = key.rsplit(':', 1)
        np.testing.assert_allclose(got[mod][leaf], gold[key], rtol=1e-4, atol=1e-6, err_msg=key)
    return eng


def small_spec(name, **kw):
    return dataclasses.replace(ANSATZES[name](), **kw)


def oracle_vjp(spec, h, tree, r, cot, eps):
    """torch.autograd of sum_b cot[b] log|psi(r_b)| through the float64 oracle -> {module: {leaf: array}}."""
    p = {m: {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in leaves.items()} for m, leaves in tree.items()}
    R = torch.as_tensor(np.asarray(h.mol.coords), dtype=torch.float64)
    r = torch.as_tensor(np.asarray(r), dtype=torch.float64)
    tot = 0
    for b in range(r.shape[0]):
        tot = tot + float(cot[b]) * owf.wave_function(p, spec, r[b], R, h.n_up, eps)[1]
    tot.backward()
    return {m: {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in leaves.items()} for m, leaves in p.items()}


def leaf_errors(got, ref):
    """Largest deviation of every leaf relative to the leaf's norm."""
    out = {}
    for m, leaves in ref.items():
        for k, v in leaves.items():
            g = got.get(m, {}).get(k)
            if g is None:
                assert np.abs(v).max() == 0, (m, k)
                continue
            out[f'{m}:{k}'] = float(np.abs(g - v).max() / max(np.linalg.norm(v), 1e-300))
    return out


def check_against_oracle(name, molname, B, device, lib=None, tol=1e-9, seed=3, **spec_kw):
    h = MolecularHamiltonian(mol=Molecule.from_name(molname))
    spec = small_spec(name, **spec_kw)
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=seed, perturb_envelopes=0.1)
    eng = Engine(spec, h, tree, dtype=torch.float64, device=device, lib=lib, norm_eps=geom.F32_EPS)
    r = synthetic_walkers(h, B, seed=seed + 1)
    cot = np.random.default_rng(seed).normal(size=B)
    _, _, g = eng.log_psi_vjp(torch.as_tensor(r, device=device), torch.as_tensor(cot, device=device))
    err = leaf_errors(eng.program.unflatten_grad(g), oracle_vjp(spec, h, tree, r, cot, geom.F32_EPS))
    worst = max(err, key=err.get)
    assert err[worst] < tol, (worst, err[worst])
    return eng, err
