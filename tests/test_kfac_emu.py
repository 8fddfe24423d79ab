"""KFAC statistics of the reverse pass (dqmc_log_psi_kfac) through the SIMT emulation of the kernels: the Kronecker factors
against the oracle's recorded linear calls, the layout, the gradient and rest partials against the VJP and the Jacobian,
determinism, chunking and edge cases, and the preconditioner of compute_energy_loss_and_kfac."""
import numpy as np
import pytest
import torch

from deepqmc_amd.engine import DqmcError, Engine
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.loss import (_energy_loss_cotangents, compute_energy_loss_and_kfac, kfac_module_factors,
                              median_clip_and_mask)
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.params import OMNI, init_params
from deepqmc_amd.sampling import synthetic_walkers
from oracle import geom
from param_grad_util import small_spec
from param_jacobian_util import jac_engine
from kfac_util import check_factors_against_oracle
from simt_util import emu_lib

SMALL = dict(embedding_dim=32, n_interactions=1, n_determinants=2)
JASTROW = f'{OMNI}/~/Jastrow/~/mlp/linear_0'


@pytest.mark.parametrize('name', ['paulinet', 'ferminet'])
def test_factors_match_oracle(name):
    h, spec, tree, eng, r = jac_engine(name, 'LiH', 5, 'cpu', emu_lib(), **SMALL)
    check_factors_against_oracle(h, spec, tree, eng, r, tol_a=1e-12, tol_g=1e-9)


@pytest.mark.parametrize('name', ['paulinet', 'ferminet'])
def test_layout_python_and_c_agree_and_every_entry_is_written(name):
    *_, eng, r = jac_engine(name, 'LiH', 4, 'cpu', emu_lib(), **SMALL)
    lay = eng.program.kfac_layout()
    assert eng.kfac_layout() == (lay['n_linear'], lay['n_factor_doubles'], lay['n_rest'])
    fac = torch.full((lay['n_factor_doubles'] + 5,), float('nan'), dtype=torch.float64)
    rest = torch.full((4 * lay['n_rest'] + 7,), float('nan'), dtype=torch.float64)
    s, l, g, factors, rst = eng.log_psi_kfac(r, out=(fac[:-5], rest[:-7].view(4, lay['n_rest'])))
    assert torch.isfinite(fac[:-5]).all() and torch.isnan(fac[-5:]).all()
    assert torch.isfinite(rest[:-7]).all() and torch.isnan(rest[-7:]).all()
    n_valid = int(((s != 0) & torch.isfinite(l)).sum())
    for o, (A, G) in zip(lay['ops'], factors):
        i = eng.program.ops[o['op']].i
        assert torch.equal(A, A.T) and torch.equal(G, G.T)
        col = 0
        for p in range(i[0]):
            K = i[3 + 4 * p]
            assert bool((A[col + K:col + (K + 3) // 4 * 4] == 0).all()) and bool((A[:, col + K:col + (K + 3) // 4 * 4] == 0).all())
            col += (K + 3) // 4 * 4
        assert bool((G[i[21]:] == 0).all()) and bool((G[:, i[21]:] == 0).all())
        if o['has_bias']:
            assert float(A[-1, -1]) == n_valid * o['nrows']


@pytest.mark.parametrize('name', ['paulinet', 'ferminet'])
def test_grad_and_rest_against_vjp_and_jacobian(name):
    *_, eng, r = jac_engine(name, 'LiH', 6, 'cpu', emu_lib(), **SMALL)
    s, l, g, _, rest = eng.log_psi_kfac(r)
    s0, l0, g0 = eng.log_psi_vjp(r)
    assert torch.equal(g, g0) and torch.equal(l, l0) and torch.equal(s, s0)
    cot = torch.as_tensor(np.random.default_rng(2).normal(size=6))
    cot[[1, 4]] = 0
    _, _, gc, _, _ = eng.log_psi_kfac(r, cot)
    _, _, gv = eng.log_psi_vjp(r, cot)
    tree_k, tree_v = eng.program.unflatten_grad(gc), eng.program.unflatten_grad(gv)
    for m in tree_v:
        for k in tree_v[m]:
            ref = tree_v[m][k]
            assert np.abs(tree_k[m][k] - ref).max() <= 1e-12 * max(np.linalg.norm(ref), 1e-300), (m, k)
    _, _, J = eng.log_psi_jacobian(r)
    assert torch.equal(rest, J[:, eng.program.kfac_layout()['rest_index']])


def test_jastrow_G_from_the_jacobian_bias_columns():
    *_, eng, r = jac_engine('paulinet', 'LiH', 6, 'cpu', emu_lib(), **SMALL)
    lay = eng.program.kfac_layout()
    q = next(k for k, o in enumerate(lay['ops']) if o['module'] == JASTROW)
    o = lay['ops'][q]
    assert o['nrows'] == 1
    _, _, _, factors, _ = eng.log_psi_kfac(r)
    _, _, J = eng.log_psi_jacobian(r)
    # one row per walker: walker b's block of the Jacobian is x_b dZ1_b^T (x_b = the Jastrow input), or dZ1_b itself for a bias
    i = eng.program.ops[o['op']].i
    if i[23] >= 0:
        jb = J[:, i[23]:i[23] + o['d_g']]
    else:
        eng.set_option('fused', 0)
        eng.wf_eval(r)
        x = torch.as_tensor(eng.debug_read('x_sum', 6)).reshape(6, -1)[:, :o['d_a']].double()
        jw = J[:, i[22]:i[22] + o['d_a'] * o['d_g']].reshape(6, o['d_a'], o['d_g'])
        jb = torch.einsum('bk,bkn->bn', x, jw) / (x * x).sum(1, keepdim=True)
    ref = jb.T @ jb
    assert float((factors[q][1] - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_repeat_chunked_and_invalid_walkers():
    *_, eng, r = jac_engine('paulinet', 'LiH', 24, 'cpu', emu_lib(), **SMALL)
    cot = torch.as_tensor(np.random.default_rng(1).normal(size=24))
    out0 = eng.log_psi_kfac(r, cot)
    out1 = eng.log_psi_kfac(r, cot)
    assert torch.equal(out0[2], out1[2]) and torch.equal(out0[4], out1[4])
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(out0[3], out1[3]))
    assert eng.last_chunks()['own'] == 1
    eng.set_option('ws_budget_mb', 1)
    out2 = eng.log_psi_kfac(r, cot)
    assert eng.last_chunks()['own'] > 1
    np.testing.assert_allclose(out2[2].numpy(), out0[2].numpy(), rtol=1e-12, atol=1e-12 * float(out0[2].abs().max()))
    for a, b in zip(out2[3], out0[3]):
        for x, y in zip(a, b):
            assert float((x - y).abs().max()) <= 1e-12 * max(float(y.abs().max()), 1e-300)
    assert torch.equal(out2[4], out0[4])


def test_node_and_non_finite_walkers_contribute_nothing():
    *_, eng, r = jac_engine('paulinet', 'LiH', 6, 'cpu', emu_lib(), **SMALL)
    r = r.clone()
    r[1, 1] = r[1, 0]
    r[4, 2, 0] = float('nan')
    s, l, g, factors, rest = eng.log_psi_kfac(r)
    if int(s[1]) != 0:
        r[1, 0, 1] = float('inf')
        s, l, g, factors, rest = eng.log_psi_kfac(r)
    assert int(s[1]) == 0 or not bool(torch.isfinite(l[1]))
    good = [0, 2, 3, 5]
    assert bool((rest[[1, 4]] == 0).all())
    _, _, g_good, f_good, rest_good = eng.log_psi_kfac(r[good].contiguous())
    assert torch.equal(rest[good], rest_good)
    for (A, G), (A2, G2) in zip(factors, f_good):
        assert torch.isfinite(A).all() and torch.isfinite(G).all()
        assert float((A - A2).abs().max()) <= 1e-12 * float(A2.abs().max())
        assert float((G - G2).abs().max()) <= 1e-12 * max(float(G2.abs().max()), 1e-300)


def test_attention_programs_are_unsupported():
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = small_spec('psiformer', n_interactions=1, n_determinants=2)
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=0)
    eng = Engine(spec, h, tree, dtype=torch.float64, device='cpu', lib=emu_lib(), norm_eps=geom.F32_EPS)
    with pytest.raises(DqmcError, match='dqmc error -4'):
        eng.log_psi_kfac(torch.as_tensor(synthetic_walkers(h, 2, seed=0)))


def _wf_and_batch(S=1, B=8, name='paulinet'):
    from deepqmc_amd.wf import NeuralNetworkWaveFunction
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    wf = NeuralNetworkWaveFunction(h, small_spec(name, **SMALL), dtype=torch.float64, device='cpu', lib=emu_lib(),
                                   norm_eps=geom.F32_EPS)
    trees = [wf.init(s, perturb_envelopes=0.1) for s in range(S)]
    r = torch.stack([torch.as_tensor(synthetic_walkers(h, B, seed=30 + s)) for s in range(S)])[None]
    return h, wf, trees, r


def _flat(t, keys):
    return np.concatenate([np.asarray(t[m][k]).reshape(-1) for m, k in keys])


def _state_direction(wf, tree, r, cot, damping, old=None, ema=0.95):
    """The preconditioned direction of one state formed by hand: dense Kronecker solves and the diagonal from the Jacobian."""
    eng = wf.engine(tree)
    prog = eng.program
    s, l, g, factors, _ = eng.log_psi_kfac(r, cot)
    n_v = int(((s != 0) & torch.isfinite(l)).sum())
    gt = prog.unflatten_grad(g)
    mods = kfac_module_factors(prog, factors, n_v)
    out = {}
    for mod, (A, G) in mods.items():
        if old is not None:
            A, G = ema * old['A'][mod] + (1 - ema) * A, ema * old['G'][mod] + (1 - ema) * G
        pi = float(torch.sqrt((torch.trace(A) / A.shape[0]) / (torch.trace(G) / G.shape[0])))
        Ad = A + pi * damping ** 0.5 * torch.eye(A.shape[0], dtype=torch.float64)
        Gd = G + damping ** 0.5 / pi * torch.eye(G.shape[0], dtype=torch.float64)
        gw = np.concatenate([gt[mod]['w'], gt[mod]['b'][None]], 0) if 'b' in gt[mod] else gt[mod]['w']
        # vec(delta) (row-major) solves (A_d kron G_d) vec(delta) = vec(g)
        d = torch.linalg.solve(torch.kron(Ad, Gd), torch.as_tensor(gw).reshape(-1)).reshape(gw.shape).numpy()
        out[mod] = d
    _, Jp = wf.log_psi_jacobian(tree, r)
    other = [(m, k) for (m, k) in prog.grad_leaves if m not in mods]
    sl = prog.leaf_slices()
    cols = np.concatenate([np.arange(sl[key][0].start, sl[key][0].stop) for key in other])
    F = (Jp[:, cols] ** 2).sum(0).numpy() / n_v
    if old is not None:
        F = ema * old['diag'].numpy() + (1 - ema) * F
    diag = _flat(gt, other) / (F + damping)
    return out, diag, other, gt


def test_kronecker_blocks_equal_dense_solves_and_diagonal():
    h, wf, trees, r = _wf_and_batch()
    loss, deltas, stats, state = compute_energy_loss_and_kfac(None, h, wf, trees, r, damping=1e-3)
    _, _, _, cots, _, _ = _energy_loss_cotangents('t', None, h, wf, trees, r, None, median_clip_and_mask)
    kron, diag, other, gt = _state_direction(wf, trees[0], r[0, 0], cots[0], 1e-3)
    assert kron
    for mod, d in kron.items():
        got = np.concatenate([deltas[0][mod]['w'], deltas[0][mod]['b'][None]], 0) if 'b' in deltas[0][mod] else deltas[0][mod]['w']
        assert np.abs(got - d).max() <= 1e-10 * np.abs(d).max(), mod
    np.testing.assert_allclose(_flat(deltas[0], other), diag, rtol=1e-10, atol=0)
    keys = list(wf.engine(trees[0]).program.grad_leaves)
    np.testing.assert_allclose(float(stats['precon_grad_dot'][0]), float(np.dot(_flat(deltas[0], keys), _flat(gt, keys))), rtol=1e-12)


def test_large_damping_tends_to_the_gradient():
    # factored Tikhonov damping: lam delta = g + O(sqrt(|A| |G| / lam)), so the deviation falls as 1 / sqrt(lam)
    h, wf, trees, r = _wf_and_batch()
    keys = list(wf.engine(trees[0]).program.grad_leaves)
    err = {}
    for lam in (1e8, 1e10, 1e16):
        _, deltas, stats, _ = compute_energy_loss_and_kfac(None, h, wf, trees, r, damping=lam)
        d, g = _flat(deltas[0], keys), _flat(stats['grad'][0], keys)
        err[lam] = np.linalg.norm(lam * d - g) / np.linalg.norm(g)
    assert err[1e16] < 1e-6, err
    np.testing.assert_allclose(err[1e8] / err[1e10], 10, rtol=0.05)


def test_ema_mixes_the_factors():
    h, wf, trees, r = _wf_and_batch()
    _, _, _, state = compute_energy_loss_and_kfac(None, h, wf, trees, r)
    r2 = torch.stack([torch.as_tensor(synthetic_walkers(h, 8, seed=77))])[None]
    _, deltas, _, state2 = compute_energy_loss_and_kfac(None, h, wf, trees, r2, state=state, ema=0.9)
    _, _, _, fresh = compute_energy_loss_and_kfac(None, h, wf, trees, r2)
    for key in ('A', 'G'):
        for mod in state[0][key]:
            ref = 0.9 * state[0][key][mod] + (1 - 0.9) * fresh[0][key][mod]
            assert torch.allclose(state2[0][key][mod], ref, rtol=1e-14, atol=0)
    assert torch.allclose(state2[0]['diag'], 0.9 * state[0]['diag'] + (1 - 0.9) * fresh[0]['diag'], rtol=1e-14, atol=0)
    _, _, _, cots, _, _ = _energy_loss_cotangents('t', None, h, wf, trees, r2, None, median_clip_and_mask)
    kron, diag, other, _ = _state_direction(wf, trees[0], r2[0, 0], cots[0], 1e-3, old=state[0], ema=0.9)
    for mod, d in kron.items():
        got = np.concatenate([deltas[0][mod]['w'], deltas[0][mod]['b'][None]], 0) if 'b' in deltas[0][mod] else deltas[0][mod]['w']
        assert np.abs(got - d).max() <= 1e-10 * np.abs(d).max(), mod
    np.testing.assert_allclose(_flat(deltas[0], other), diag, rtol=1e-10, atol=0)


def test_two_states_use_their_own_cotangents():
    h, wf, trees, r = _wf_and_batch(S=2)
    _, deltas, _, state = compute_energy_loss_and_kfac(None, h, wf, trees, r)
    assert len(state) == 2
    _, _, _, cots, _, _ = _energy_loss_cotangents('t', None, h, wf, trees, r, None, median_clip_and_mask)
    for s in range(2):
        kron, diag, other, _ = _state_direction(wf, trees[s], r[0, s], cots[s], 1e-3)
        for mod, d in kron.items():
            got = np.concatenate([deltas[s][mod]['w'], deltas[s][mod]['b'][None]], 0) if 'b' in deltas[s][mod] else deltas[s][mod]['w']
            assert np.abs(got - d).max() <= 1e-10 * np.abs(d).max(), (s, mod)
        np.testing.assert_allclose(_flat(deltas[s], other), diag, rtol=1e-10, atol=0)
