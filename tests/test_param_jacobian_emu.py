"""Per-walker parameter Jacobian of log|psi| (dqmc_log_psi_jacobian) through the SIMT emulation of the kernels: rows against
torch.autograd through the float64 oracle, the transpose of the VJP, the reference's own golden, determinism and chunking,
edge cases, and the natural gradient built on it."""
import numpy as np
import pytest
import torch

from deepqmc_amd.engine import DqmcError, Engine
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.params import init_params
from deepqmc_amd.sampling import synthetic_walkers
from oracle import geom
from param_grad_util import GOLDEN, small_spec
from param_jacobian_util import check_natgrad, check_rows_against_oracle, check_transpose_of_vjp, jac_engine
from ref_ansatz_util import reference_test_engine
from simt_util import emu_lib

SMALL = dict(embedding_dim=32, n_interactions=1, n_determinants=2)


@pytest.mark.parametrize('name', ['paulinet', 'ferminet'])
def test_rows_match_oracle_autograd(name):
    h, spec, tree, eng, r = jac_engine(name, 'LiH', 4, 'cpu', emu_lib(), **SMALL)
    check_rows_against_oracle(h, spec, tree, eng, r, range(4), tol=1e-9)


@pytest.mark.parametrize('name', ['paulinet', 'ferminet'])
def test_jacobian_is_the_transpose_of_the_vjp(name):
    *_, eng, r = jac_engine(name, 'LiH', 6, 'cpu', emu_lib(), **SMALL)
    _, has_padding = check_transpose_of_vjp(eng, r)
    assert has_padding or name == 'ferminet'         # (the small FermiNet's layer widths are multiples of 4)


def test_reference_grad_golden_row(kats):
    h, P, tree, eng = reference_test_engine('cpu', lib=emu_lib(), norm_eps=geom.F64_EPS)
    r = torch.as_tensor(kats['lih_edges_ne'][0][None], dtype=torch.float64)
    sign, log, J = eng.log_psi_jacobian(r)
    assert int(sign[0]) == int(kats['wf_psi_sign'])
    got = eng.program.unflatten_params(eng.program.unflatten_jacobian(J)[0])
    gold = np.load(GOLDEN)
    assert len(gold.files) == 37
    for key in gold.files:
        mod, leaf = key.rsplit(':', 1)
        np.testing.assert_allclose(got[mod][leaf], gold[key], rtol=1e-4, atol=1e-6, err_msg=key)


def test_repeat_and_chunked_calls_are_bit_identical():
    *_, eng, r = jac_engine('paulinet', 'LiH', 24, 'cpu', emu_lib(), **SMALL)
    s0, l0, J0 = eng.log_psi_jacobian(r)
    s1, l1, J1 = eng.log_psi_jacobian(r)
    assert torch.equal(J0, J1) and torch.equal(l0, l1) and torch.equal(s0, s1)
    assert eng.last_chunks()['own'] == 1
    eng.set_option('ws_budget_mb', 1)
    s2, l2, J2 = eng.log_psi_jacobian(r)
    assert eng.last_chunks()['own'] > 1
    assert torch.equal(s0, s2) and torch.equal(J0, J2)


def test_wider_output_keeps_extra_columns():
    *_, eng, r = jac_engine('paulinet', 'LiH', 5, 'cpu', emu_lib(), **SMALL)
    nw = eng.program.weights.size
    out = torch.full((5, nw + 7), float('nan'), dtype=torch.float64)
    _, _, J = eng.log_psi_jacobian(r, out=out)
    assert J.data_ptr() == out.data_ptr()
    assert torch.isnan(out[:, nw:]).all()
    _, _, J_ref = eng.log_psi_jacobian(r)
    assert torch.equal(out[:, :nw], J_ref)
    with pytest.raises(DqmcError):
        eng.log_psi_jacobian(r, out=torch.empty(5, nw - 1, dtype=torch.float64))


def test_node_and_non_finite_walkers_get_zero_rows():
    h, spec, tree, eng, r = jac_engine('paulinet', 'LiH', 6, 'cpu', emu_lib(), **SMALL)
    r = r.clone()
    r[1, 1] = r[1, 0]                     # two spin-up electrons at one position: psi = 0 ...
    r[4, 2, 0] = float('nan')
    s, l, J = eng.log_psi_jacobian(r)
    if int(s[1]) != 0:                    # ... unless round-off in the determinant keeps it off the node: then infinity
        r[1, 0, 1] = float('inf')
        s, l, J = eng.log_psi_jacobian(r)
    assert int(s[1]) == 0 or not bool(torch.isfinite(l[1]))
    assert not bool(torch.isfinite(l[4]))
    for b in (1, 4):
        assert bool((J[b] == 0).all()), b
    good = [0, 2, 3, 5]
    assert bool(torch.isfinite(J[good]).all()) and bool((J[good] != 0).any())


def test_attention_programs_are_unsupported():
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = small_spec('psiformer', n_interactions=1, n_determinants=2)
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=0)
    eng = Engine(spec, h, tree, dtype=torch.float64, device='cpu', lib=emu_lib(), norm_eps=geom.F32_EPS)
    with pytest.raises(DqmcError, match='dqmc error -4'):
        eng.log_psi_jacobian(torch.as_tensor(synthetic_walkers(h, 2, seed=0)))


def test_unflatten_jacobian_rows_equal_unflatten_grad():
    *_, eng, r = jac_engine('ferminet', 'LiH', 3, 'cpu', emu_lib(), **SMALL)
    _, _, J = eng.log_psi_jacobian(r)
    prog = eng.program
    Jp = prog.unflatten_jacobian(J)
    for b in range(3):
        tree = prog.unflatten_grad(J[b])
        flat = np.concatenate([tree[mod][leaf].reshape(-1) for (mod, leaf) in prog.grad_leaves])
        assert np.array_equal(Jp[b].numpy(), flat), b
        back = prog.unflatten_params(Jp[b])
        for (mod, leaf), (sl, shape) in prog.leaf_slices().items():
            assert back[mod][leaf].shape == shape and np.array_equal(back[mod][leaf], tree[mod][leaf])


def _wf_and_batch(S=2, B=8):
    from deepqmc_amd.wf import NeuralNetworkWaveFunction
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    wf = NeuralNetworkWaveFunction(h, small_spec('paulinet', **SMALL), dtype=torch.float64, device='cpu', lib=emu_lib(),
                                   norm_eps=geom.F32_EPS)
    trees = [wf.init(s, perturb_envelopes=0.1) for s in range(S)]
    r = torch.stack([torch.as_tensor(synthetic_walkers(h, B, seed=30 + s)) for s in range(S)])[None]
    return h, wf, trees, r


def test_natgrad_solves_the_damped_fisher_system():
    _, wf, trees, r = _wf_and_batch(S=1)
    check_natgrad(wf, trees, r, damping=1e-3)


def test_natgrad_tends_to_the_gradient_at_large_damping():
    from deepqmc_amd.loss import compute_energy_loss_and_natgrad
    _, wf, trees, r = _wf_and_batch(S=1)
    err = {}
    for damping in (1e6, 1e8, 1e10):
        _, deltas, stats = compute_energy_loss_and_natgrad(None, wf.hamil, wf, trees, r, damping=damping)
        d, g = deltas[0], stats['grad'][0]
        num = sum(float(np.sum((damping * d[m][k] - g[m][k]) ** 2)) for m in g for k in g[m])
        den = sum(float(np.sum(g[m][k] ** 2)) for m in g for k in g[m])
        err[damping] = np.sqrt(num / den)
    # damping delta = g - A^T A delta: the deviation falls as 1 / damping (here ||A^T A|| is a few 1e3)
    assert err[1e10] < 1e-5
    np.testing.assert_allclose([err[1e6] / err[1e8], err[1e8] / err[1e10]], [100, 100], rtol=1e-2)


def test_natgrad_gradient_equals_energy_loss_gradient_two_states():
    from deepqmc_amd.loss import compute_energy_loss_and_grad
    h, wf, trees, r = _wf_and_batch(S=2)
    loss, _, stats = check_natgrad(wf, trees, r)
    loss2, grads, _ = compute_energy_loss_and_grad(None, h, wf, trees, r)
    assert float(loss) == float(loss2)
    for s in range(2):
        g = stats['grad'][s]
        for m in grads[s]:
            for k in grads[s][m]:
                np.testing.assert_allclose(g[m][k], grads[s][m][k], rtol=0, atol=1e-12 * max(1.0, np.abs(grads[s][m][k]).max()))
