"""Parameter gradient of log|psi| (dqmc_log_psi_vjp) through the SIMT emulation of the kernels: the reference's own golden,
torch.autograd through the float64 oracle, the transpose of the weight packing, chunking and determinism."""
import numpy as np
import pytest
import torch

from deepqmc_amd.engine import DqmcError, Engine
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.params import init_params
from deepqmc_amd.program import compile_program
from deepqmc_amd.sampling import synthetic_walkers
from oracle import geom
from param_grad_util import check_against_oracle, check_grad_golden, small_spec
from simt_util import emu_lib

SMALL = dict(embedding_dim=32, n_interactions=1, n_determinants=2)


def test_reference_grad_golden_through_emulated_hip_path(kats):
    check_grad_golden(kats, 'cpu', emu_lib())


@pytest.mark.parametrize('name', ['paulinet', 'ferminet'])
def test_vjp_matches_oracle_autograd(name):
    check_against_oracle(name, 'LiH', 6, 'cpu', emu_lib(), tol=1e-9, **SMALL)


def _engine(name='paulinet', B=8, seed=5, **kw):
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = small_spec(name, **{**SMALL, **kw})
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=seed, perturb_envelopes=0.1)
    eng = Engine(spec, h, tree, dtype=torch.float64, device='cpu', lib=emu_lib(), norm_eps=geom.F32_EPS)
    return h, spec, tree, eng, torch.as_tensor(synthetic_walkers(h, B, seed=seed))


def test_unflatten_is_the_transpose_of_the_packing():
    h, spec, tree, _, _ = _engine()
    rng = np.random.default_rng(0)
    pack = lambda t: compile_program(spec, t, h.n_up, h.n_down, h.n_nuc).weights
    prog = compile_program(spec, tree, h.n_up, h.n_down, h.n_nuc)
    for _ in range(3):
        v = {m: {k: rng.normal(size=np.shape(x)) for k, x in leaves.items()} for m, leaves in tree.items()}
        g = rng.normal(size=prog.weights.size)
        eps = 1e-3
        moved = {m: {k: np.asarray(x) + eps * v[m][k] for k, x in leaves.items()} for m, leaves in tree.items()}
        lhs = float(np.dot(pack(moved) - pack(tree), g)) / eps
        G = prog.unflatten_grad(g)
        rhs = sum(float(np.sum(v[m][k] * G[m][k])) for m in G for k in G[m])
        assert abs(lhs - rhs) <= 1e-8 * max(1.0, abs(rhs)), (lhs, rhs)


def test_chunked_equals_unchunked_and_calls_are_bit_identical():
    h, spec, tree, eng, r = _engine(B=24)
    cot = torch.as_tensor(np.random.default_rng(1).normal(size=24))
    s0, l0, g0 = eng.log_psi_vjp(r, cot)
    s1, l1, g1 = eng.log_psi_vjp(r, cot)
    assert torch.equal(g0, g1) and torch.equal(l0, l1)
    assert eng.last_chunks()['own'] == 1
    eng.set_option('ws_budget_mb', 1)
    s2, l2, g2 = eng.log_psi_vjp(r, cot)
    assert eng.last_chunks()['own'] > 1
    assert torch.equal(s0, s2)
    np.testing.assert_allclose(l2.numpy(), l0.numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(g2.numpy(), g0.numpy(), rtol=1e-12, atol=1e-14 * float(g0.abs().max()))
    # log|psi| and sign of the vjp are those of the value path
    s3, l3 = eng.wf_eval(r)
    assert torch.equal(s3, s0)
    np.testing.assert_allclose(l3.numpy(), l0.numpy(), rtol=0, atol=1e-12)


def test_padding_and_constants_get_exact_zeros():
    h, spec, tree, eng, r = _engine()
    _, _, g = eng.log_psi_vjp(r)
    src = eng.program.grad_src
    # every padding entry of every linear weight block is exactly zero
    for op in eng.program.ops:
        if op.kind != 3:
            continue
        i = op.i
        ldw, w_off, row = (i[21] + 3) // 4 * 4, i[22], 0
        for p in range(i[0]):
            K = i[3 + 4 * p]
            Kp = (K + 3) // 4 * 4
            blk = g[w_off + row * ldw:w_off + (row + Kp) * ldw].reshape(Kp, ldw).numpy()
            assert np.all(blk[K:] == 0) and np.all(blk[:, i[21]:] == 0)
            assert np.all(src[w_off + row * ldw:w_off + (row + Kp) * ldw].reshape(Kp, ldw)[K:] < 0)
            row += Kp
    # constants (grad_src < 0: padding, the cusp alpha constants, ...) map to nothing: whatever accumulates there does not
    # reach the parameter tree
    const = src < 0
    assert const.any()
    g2 = g.clone()
    g2[torch.as_tensor(const)] = torch.randn(int(const.sum()), dtype=g.dtype)
    t1, t2 = eng.program.unflatten_grad(g), eng.program.unflatten_grad(g2)
    for m in t1:
        for k in t1[m]:
            assert np.array_equal(t1[m][k], t2[m][k]), (m, k)
    # every parameter element receives the gradient of at least one weight entry
    ids = np.unique(src[src >= 0])
    assert ids.size == sum(int(np.prod(sh)) for _, sh in eng.program.grad_leaves.values())


def test_cotangent_weights_walkers_and_wf_facade():
    from deepqmc_amd.wf import NeuralNetworkWaveFunction
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    wf = NeuralNetworkWaveFunction(h, small_spec('paulinet', **SMALL), dtype=torch.float64, device='cpu', lib=emu_lib(),
                                   norm_eps=geom.F32_EPS)
    params = wf.init(0, perturb_envelopes=0.1)
    r = torch.as_tensor(synthetic_walkers(h, 4, seed=2))
    psi, g_all = wf.log_psi_vjp(params, r, torch.ones(4, dtype=torch.float64))
    _, g_a = wf.log_psi_vjp(params, r, torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float64))
    _, g_b = wf.log_psi_vjp(params, r, torch.tensor([0.0, 0.0, 1.0, 1.0], dtype=torch.float64))
    ref = wf.apply(params, r)
    assert torch.equal(psi.sign, ref.sign)
    for m in g_all:
        for k in g_all[m]:
            np.testing.assert_allclose(g_a[m][k] + g_b[m][k], g_all[m][k], rtol=1e-12, atol=1e-12)


def test_attention_programs_are_unsupported():
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = small_spec('psiformer', n_interactions=1, n_determinants=2)
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=0)
    eng = Engine(spec, h, tree, dtype=torch.float64, device='cpu', lib=emu_lib(), norm_eps=geom.F32_EPS)
    with pytest.raises(DqmcError, match='dqmc error -4'):
        eng.log_psi_vjp(torch.as_tensor(synthetic_walkers(h, 2, seed=0)))


def test_energy_loss_gradient_two_states_matches_hand_contraction():
    """compute_energy_loss_and_grad on a [1, 2, B] batch: the masked mean of loss/energy.py:101 divides by the mask count of
    ALL states and walkers, so each state's gradient is its own contraction over that common count."""
    from deepqmc_amd.loss import compute_energy_loss_and_grad, compute_local_energy, median_clip_and_mask
    from deepqmc_amd.wf import NeuralNetworkWaveFunction
    from param_grad_util import leaf_errors, oracle_vjp
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = small_spec('paulinet', **SMALL)
    wf = NeuralNetworkWaveFunction(h, spec, dtype=torch.float64, device='cpu', lib=emu_lib(), norm_eps=geom.F32_EPS)
    trees = [wf.init(s, perturb_envelopes=0.1) for s in (0, 1)]
    B = 8
    r = torch.stack([torch.as_tensor(synthetic_walkers(h, B, seed=20 + s)) for s in (0, 1)])[None]
    loss, grads, _ = compute_energy_loss_and_grad(None, h, wf, trees, r)
    e, _ = compute_local_energy(None, h, wf, trees, r)
    e = e[0].double()
    np.testing.assert_allclose(float(loss), float(e.mean()), rtol=1e-12)
    clipped = [median_clip_and_mask(e[s]) for s in (0, 1)]
    n_mask = sum(float(m.double().sum()) for _, m in clipped)
    assert n_mask == 2 * B
    for s, (ec, _) in enumerate(clipped):
        ref = oracle_vjp(spec, h, trees[s], r[0, s].numpy(), ((ec - ec.mean()) / n_mask).numpy(), geom.F32_EPS)
        err = leaf_errors(grads[s], ref)
        worst = max(err, key=err.get)
        assert err[worst] < 1e-9, (s, worst, err[worst])

