"""SCF-orbital pretraining through the SIMT emulation of the kernels: the GTO target against a float64 restatement and closed
forms, the device orbitals against the facade's host copy, the orbital VJP and the fused loss step against torch.autograd
through the float64 oracle, chunking and determinism, three Adam steps of `pretrain` against torch.optim.Adam, refusals."""
import math

import numpy as np
import pytest
import torch

from deepqmc_amd.engine import DqmcError, Engine
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.params import init_params
from deepqmc_amd.pretrain import GTOBasis, PretrainTarget, adam, pretrain, pretrain_loss_and_grad
from deepqmc_amd.sampling import synthetic_walkers
from deepqmc_amd.types import PhysicalConfiguration
from deepqmc_amd.wf import NeuralNetworkWaveFunction
from oracle import geom
from param_grad_util import leaf_errors, small_spec
from pretrain_util import (cartesian_angulars, check_loss_grad, check_orbitals_vjp, check_target, make, oracle_orbitals,
                           restated_loss, restated_target, synthetic_dataset, torch_params, upload)
from simt_util import emu_lib

SMALL = dict(embedding_dim=32, n_interactions=1, n_determinants=2)
SMALL4 = {**SMALL, 'n_determinants': 4}       # more determinants than the 3 configurations of the CAS-like dataset: tiling


@pytest.mark.parametrize('kind', ['hf', 'cas'])
def test_target_matches_restatement(kind):
    h, spec, tree, eng, r = make('paulinet', 'LiH', 6, 'cpu', emu_lib(), small=SMALL4)
    ds = synthetic_dataset(h, kind, seed=1)
    t = check_target(eng, h, ds, r, rtol=1e-10)
    assert t.shape == (6, 1 if kind == 'hf' else 3, 4, 4)


def test_angular_order_and_norms_closed_forms():
    """One s, p, d and f shell (one primitive, unit coefficient) on atom 0, mo_coeffs = identity: column mu of the target is
    atomic orbital mu at the electron, N (x^lx y^ly z^lz) exp(-zeta d^2) / sqrt((2lx-1)!! (2ly-1)!! (2lz-1)!!) with
    N = (2 zeta / pi)^(3/4) (4 zeta)^(l/2)."""
    h, spec, tree, eng, r = make('paulinet', 'LiH', 1, 'cpu', emu_lib(), small=SMALL)
    N = 4
    zeta = {0: 0.7, 1: 0.45, 2: 0.6, 3: 0.35}
    shells = [(0, (l, [1.0], [zeta[l]])) for l in range(4)]
    n_ao = 1 + 3 + 6 + 10
    assert [cartesian_angulars(2)[k] for k in (0, 1, 5)] == [(2, 0, 0), (1, 1, 0), (0, 0, 2)]
    assert cartesian_angulars(1) == [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    ao_l = [(l, a) for l in range(4) for a in cartesian_angulars(l)]
    df = {0: 1, 1: 1, 2: 3, 3: 15}
    x, y, z = r[0, 0] - np.asarray(h.mol.coords)[0]
    d2 = x * x + y * y + z * z
    for first in range(0, n_ao, N):                      # N columns of the identity at a time
        cols = [min(first + k, n_ao - 1) for k in range(N)]
        eng.set_pretrain_target(shells, np.eye(n_ao), [cols], [1.0])
        t = eng.pretrain_target(torch.as_tensor(r))[0, 0, 0].numpy()
        for k, ao in enumerate(cols):
            l, (lx, ly, lz) = ao_l[ao]
            ref = ((2 * zeta[l] / math.pi) ** 0.75 * (4 * zeta[l]) ** (l / 2) * x ** lx * y ** ly * z ** lz * math.exp(-zeta[l] * d2)
                   / math.sqrt(df[lx] * df[ly] * df[lz]))
            np.testing.assert_allclose(t[k], ref, rtol=1e-12, err_msg=str((l, lx, ly, lz)))


def _wf(name='paulinet', small=SMALL, **kw):
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    wf = NeuralNetworkWaveFunction(h, small_spec(name, **small), dtype=torch.float64, device='cpu', lib=emu_lib(), norm_eps=geom.F32_EPS, **kw)
    return h, wf


def test_orbitals_equal_return_mos_bit_for_bit():
    h, wf = _wf()
    params = wf.init(0, perturb_envelopes=0.1)
    r = torch.as_tensor(synthetic_walkers(h, 5, seed=2))
    up0, dn0 = wf.apply(params, r, return_mos=True)
    up1, dn1 = wf.orbitals(params, r)
    assert up1.shape == (5, 2, 2, 4) and dn1.shape == (5, 2, 2, 4)
    assert torch.equal(up0, up1) and torch.equal(dn0, dn1)


@pytest.mark.parametrize('name', ['paulinet', 'ferminet'])
def test_orbitals_vjp_matches_oracle_autograd(name):
    h, spec, tree, eng, r = make(name, 'LiH', 6, 'cpu', emu_lib(), small=SMALL)
    orb, none = check_orbitals_vjp(eng, spec, h, tree, r, tol=1e-9)
    assert [n.split('/')[-1] for n in none] == (['conf_coeff:w', 'linear_0:w'] if name == 'paulinet' else [])
    assert all('Jastrow' in n or 'conf_coeff' in n for n in none)
    ref = oracle_orbitals(spec, h, torch_params(tree), r, geom.F32_EPS).detach().numpy()
    np.testing.assert_allclose(orb.numpy(), ref, rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize('kind', ['hf', 'cas'])
def test_pretrain_loss_grad_matches_restated_loss(kind):
    h, spec, tree, eng, r = make('paulinet', 'LiH', 9, 'cpu', emu_lib(), small=SMALL4)
    check_loss_grad(eng, spec, h, tree, r, synthetic_dataset(h, kind, seed=2), tol=1e-9)


def test_two_states_add_up_through_n_total():
    """pretrain_loss_and_grad on r[1, 2, B]: every state's gradient is that of the ONE loss whose means run over both states."""
    from pretrain_util import oracle_pretrain
    h, wf = _wf(small=SMALL4)
    trees = [wf.init(s, perturb_envelopes=0.1) for s in (0, 1)]
    ds = synthetic_dataset(h, 'cas', seed=4, n_states=2)
    B = 5
    r = torch.stack([torch.as_tensor(synthetic_walkers(h, B, seed=30 + s)) for s in (0, 1)])[None]
    loss, grads, ps = pretrain_loss_and_grad(wf, trees, r, ds)
    assert ps.shape == (1, 2, B)
    ref = [oracle_pretrain(wf.spec, h, trees[s], r[0, s].numpy(), ds, s, 2 * B, geom.F32_EPS) for s in (0, 1)]
    np.testing.assert_allclose(loss, ref[0][0] + ref[1][0], rtol=1e-12)
    for s in (0, 1):
        np.testing.assert_allclose(ps[0, s].numpy(), ref[s][1], rtol=1e-10)
        err = leaf_errors(grads[s], ref[s][2])
        worst = max(err, key=err.get)
        assert err[worst] < 1e-9, (s, worst, err[worst])


def test_chunked_equals_unchunked_and_calls_are_bit_identical():
    h, spec, tree, eng, r = make('paulinet', 'LiH', 24, 'cpu', emu_lib(), small=SMALL4)
    upload(eng, synthetic_dataset(h, 'cas', seed=2))
    rt = torch.as_tensor(r)
    cot = torch.as_tensor(np.random.default_rng(1).normal(size=(24, 4, 4, 4)))
    o0, g0 = eng.orbitals_vjp(rt, cot)
    o1, g1 = eng.orbitals_vjp(rt, cot)
    p0, q0 = eng.pretrain_loss_grad(rt)
    p1, q1 = eng.pretrain_loss_grad(rt)
    assert torch.equal(g0, g1) and torch.equal(o0, o1) and torch.equal(p0, p1) and torch.equal(q0, q1)
    assert eng.last_chunks()['own'] == 1
    eng.set_option('ws_budget_mb', 1)
    o2, g2 = eng.orbitals_vjp(rt, cot)
    assert eng.last_chunks()['own'] > 1
    p2, q2 = eng.pretrain_loss_grad(rt)
    assert eng.last_chunks()['own'] > 1
    assert torch.equal(o0, o2) and torch.equal(p0, p2)
    np.testing.assert_allclose(g2.numpy(), g0.numpy(), rtol=1e-12, atol=1e-14 * float(g0.abs().max()))
    np.testing.assert_allclose(q2.numpy(), q0.numpy(), rtol=1e-12, atol=1e-14 * float(q0.abs().max()))
    assert torch.equal(eng.orbitals(rt), o0)


class _FixedSampler:
    """Returns the walkers it was given and its state unchanged."""

    def __init__(self, r):
        self.r, self.calls = r, 0

    def sample(self, rng, state, params, mol_idxs):
        self.calls += 1
        return state, PhysicalConfiguration(None, self.r, None), {}


class _OneMolecule:
    def sample(self):
        return np.zeros(1, np.int64)


def test_three_adam_steps_follow_torch_adam():
    """The end-to-end check: pretrain() with adam() on fixed walkers against torch.optim.Adam on the restated loss through the
    oracle, every leaf after every step."""
    h, wf = _wf(small=SMALL4)
    spec = wf.spec
    params = wf.init(1, perturb_envelopes=0.1)
    ds = synthetic_dataset(h, 'cas', seed=5)
    B, lr = 6, 1e-3
    r = synthetic_walkers(h, B, seed=9)
    p = torch_params(params)
    leaves = [v for lv in p.values() for v in lv.values()]
    opt = torch.optim.Adam(leaves, lr=lr, betas=(0.9, 0.999), eps=1e-8)
    T = restated_target(ds['shells'], ds['mo_coeffs'][0], ds['confs'][0][0], ds['conf_coeffs'][0][0], r, h.mol.coords)
    sampler = _FixedSampler(torch.as_tensor(r)[None, None])
    gen = pretrain(0, h, wf, [params], adam(lr), _OneMolecule(), sampler, {'fixed': True}, ds, None, range(3))
    for step, new_params, ps, mol_idxs in gen:
        opt.zero_grad()
        loss, ps_ref = restated_loss(oracle_orbitals(spec, h, p, r, geom.F32_EPS), T, h.n_up, B)
        loss.backward()
        opt.step()
        np.testing.assert_allclose(ps[0, 0].numpy(), ps_ref.detach().numpy(), rtol=1e-9)
        ref = {m: {k: v.detach().numpy() for k, v in lv.items()} for m, lv in p.items()}
        err = leaf_errors(new_params[0], ref)
        worst = max(err, key=err.get)
        assert err[worst] < 1e-8, (step, worst, err[worst])
        assert new_params[0] is params and list(mol_idxs) == [0]
    assert sampler.calls == 3 and step == 2


def test_merge_keys_average_matching_modules_across_states():
    h, wf = _wf()
    trees = [wf.init(s, perturb_envelopes=0.1) for s in (0, 1)]
    ds = synthetic_dataset(h, 'hf', seed=5, n_states=2)
    r = torch.stack([torch.as_tensor(synthetic_walkers(h, 3, seed=40 + s)) for s in (0, 1)])[None, :]
    sampler = _FixedSampler(r)
    key = 'Backflow'
    next(pretrain(0, h, wf, trees, adam(1e-3), _OneMolecule(), sampler, None, ds, [key], range(1)))
    merged = [m for m in trees[0] if key in m]
    assert merged
    same = {m: all(np.array_equal(trees[0][m][k], trees[1][m][k]) for k in trees[0][m]) for m in trees[0]}
    assert all(same[m] for m in merged)
    assert not any(same[m] for m in same if 'envelopes' in m or 'ElectronGNN' in m or 'electron_gnn' in m.lower())


def test_engine_eviction_uploads_the_table_again():
    h, wf = _wf()
    wf.max_engines = 1
    trees = [wf.init(s, perturb_envelopes=0.1) for s in (0, 1)]
    ds = synthetic_dataset(h, 'cas', seed=6, n_states=2)
    r = torch.stack([torch.as_tensor(synthetic_walkers(h, 3, seed=50 + s)) for s in (0, 1)])[None, :]
    a = pretrain_loss_and_grad(wf, trees, r, ds)
    b = pretrain_loss_and_grad(wf, trees, r, ds)           # the one cached context changes hands between the states
    assert a[0] == b[0] and torch.equal(a[2], b[2])
    wf2 = _wf()[1]
    c = pretrain_loss_and_grad(wf2, trees, r, ds)
    assert a[0] == c[0] and torch.equal(a[2], c[2])


def test_refusals():
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    ds = synthetic_dataset(h, 'hf')
    # attention programs: the same error as the other reverse modes
    spec = small_spec('psiformer', n_interactions=1, n_determinants=2)
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=0)
    eng = Engine(spec, h, tree, dtype=torch.float64, device='cpu', lib=emu_lib(), norm_eps=geom.F32_EPS)
    r = torch.as_tensor(synthetic_walkers(h, 2, seed=0))
    with pytest.raises(DqmcError, match='dqmc error -4'):
        eng.orbitals_vjp(r, torch.zeros(2, 2, 4, 4, dtype=torch.float64))
    upload(eng, ds)
    with pytest.raises(DqmcError, match='dqmc error -4'):
        eng.pretrain_loss_grad(r)
    # spin-factorised determinants
    wf = NeuralNetworkWaveFunction(h, small_spec('paulinet', full_determinant=False, **SMALL), dtype=torch.float64, device='cpu', lib=emu_lib())
    with pytest.raises(NotImplementedError, match='full-determinant'):
        wf.orbitals(None, r)
    with pytest.raises(NotImplementedError, match='full-determinant'):
        wf.orbitals_vjp(None, r, torch.zeros(2, 2, 4, 4))
    with pytest.raises(NotImplementedError, match='full-determinant'):
        pretrain_loss_and_grad(wf, [None], r[None, None], synthetic_dataset(h, 'hf'))
    # malformed tables
    h, spec, tree, eng, _ = make('paulinet', 'LiH', 2, 'cpu', emu_lib(), small=SMALL)
    mo, confs, cc = ds['mo_coeffs'][0], ds['confs'][0][0], ds['conf_coeffs'][0][0]
    with pytest.raises(DqmcError, match='dqmc error -1.*n_ao'):
        eng.set_pretrain_target(ds['shells'], mo[:-1], confs, cc)
    with pytest.raises(DqmcError, match='dqmc error -1.*l = 4'):
        eng.set_pretrain_target(ds['shells'][:-1] + [(0, (4, [1.0], [1.0]))], mo, confs, cc)
    with pytest.raises(DqmcError, match='dqmc error -1.*orbital index'):
        eng.set_pretrain_target(ds['shells'], mo, confs + mo.shape[1], cc)
    with pytest.raises(DqmcError, match='dqmc error -1.*atom'):
        eng.set_pretrain_target([(5, ds['shells'][0][1])] + ds['shells'][1:], mo, confs, cc)
    # no target yet
    with pytest.raises(DqmcError, match='no target set'):
        eng.pretrain_loss_grad(r)
    with pytest.raises(DqmcError, match='no target set'):
        eng.pretrain_target(r)
    with pytest.raises(ValueError, match='l = 4'):
        GTOBasis(ds['centers'], [(0, (4, [1.0], [1.0]))])
    with pytest.raises(ValueError, match='atomic orbitals'):
        PretrainTarget(h, None, ds['centers'], ds['shells'], mo[:-1])
    try:
        import pyscf  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match='pyscf'):
            GTOBasis.from_pyscf(None)


def test_pretrain_target_callable():
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    ds = synthetic_dataset(h, 'cas', seed=7)
    r = synthetic_walkers(h, 3, seed=3)
    fn = PretrainTarget(h, 2, ds['centers'], ds['shells'], ds['mo_coeffs'], dtype=torch.float64, device='cpu', lib=emu_lib())
    got = fn(ds['confs'][0], ds['conf_coeffs'][0], PhysicalConfiguration(None, torch.as_tensor(r), torch.zeros(3, dtype=torch.int32)))
    ref = restated_target(ds['shells'], ds['mo_coeffs'][0], ds['confs'][0][0], ds['conf_coeffs'][0][0], r, h.mol.coords)[:, :2]
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-10)
