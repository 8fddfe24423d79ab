"""The device-resident KFAC step (dqmc_set_kfac_map, dqmc_kfac_direction, dqmc_kfac_apply, optimizer.KFACOptimizer) through the
SIMT emulation of the kernels: the blocked Cholesky solve against dense Kronecker solves, the direction against the tree path,
invalid walkers, determinism, the norm-constrained update and fit_wf against a host loop."""
import numpy as np
import pytest
import torch

from deepqmc_amd.engine import DqmcError, Engine
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.loss import compute_energy_loss_and_kfac, create_loss_fn
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.optimizer import ConstantSchedule, InverseSchedule, KFACOptimizer
from deepqmc_amd.params import init_params
from deepqmc_amd.sampling import synthetic_walkers
from deepqmc_amd.wf import NeuralNetworkWaveFunction
from oracle import geom
from kfac_optimizer_util import (DAMPING, check_flat_against_tree, check_kfac_fit_parity, check_solve_against_kron, check_two_op_module,
                                 covered_shapes, leaf_deviation, norm_constraint_coeff)
from optimizer_util import assert_same_buffers, make_pair
from param_grad_util import small_spec
from param_jacobian_util import jac_engine
from simt_util import emu_lib

SMALL = dict(embedding_dim=32, n_interactions=1, n_determinants=2)
F64 = torch.float64


def _wf_and_batch(S=1, B=8, name='paulinet', seed0=30):
    from deepqmc_amd.wf import NeuralNetworkWaveFunction
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    wf = NeuralNetworkWaveFunction(h, small_spec(name, **SMALL), dtype=F64, device='cpu', lib=emu_lib(), norm_eps=geom.F32_EPS)
    trees = [wf.init(s, perturb_envelopes=0.1) for s in range(S)]
    batch = lambda seed: torch.stack([torch.as_tensor(synthetic_walkers(h, B, seed=seed + s)) for s in range(S)])[None]
    return h, wf, trees, batch(seed0), batch(77)


# ---- 1. the solve kernels on synthetic factors ----
def test_solve_kernels_on_synthetic_factors():
    *_, eng, _ = jac_engine('paulinet', 'LiH', 2, 'cpu', emu_lib(), **SMALL)
    assert eng.KFAC_PANEL == 32
    cov = covered_shapes(eng.program, eng.KFAC_PANEL)
    print(cov)
    # the shapes at which a blocked factorisation goes wrong: dimension 1, a dimension off the panel width, at least two panels
    # plus a remainder, modules with and without a bias
    for key in ('one', 'off_panel', 'two_panels_and_rest', 'bias', 'no_bias'):
        assert cov[key], (key, cov)
    worst = check_solve_against_kron(eng)
    assert len(worst) == len(eng.program.kfac_blocks()[0])


def test_module_with_two_ops():
    *_, eng, _ = jac_engine('paulinet', 'LiH', 2, 'cpu', emu_lib(), **SMALL)
    assert not covered_shapes(eng.program, eng.KFAC_PANEL)['multi_op']       # (else the test above covers it with the program's own tables)
    check_two_op_module(eng)


def test_inconsistent_tables_are_refused():
    *_, eng, _ = jac_engine('paulinet', 'LiH', 2, 'cpu', emu_lib(), **SMALL)
    tabs, layout = eng._kfac_tables()
    for change in ('drop_diag', 'bad_map', 'bad_op'):
        t = {k: v.copy() for k, v in tabs.items()}
        if change == 'drop_diag':        # a parameter element covered by nothing
            t['diag_pos'], t['diag_row'] = t['diag_pos'][:-1].copy(), t['diag_row'][:-1].copy()
        elif change == 'bad_map':        # a row map that is no permutation
            first = int(t['op'][0][4])
            t['maps'][first + 1] = t['maps'][first]
        else:                            # an op that is not in the factor layout
            t['op'][0][0] += 1
        with pytest.raises(DqmcError, match='dqmc error -1'):
            eng.set_kfac_tables(t, layout)
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = small_spec('psiformer', n_interactions=1, n_determinants=2)
    att = Engine(spec, h, init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=0), dtype=F64, device='cpu', lib=emu_lib(), norm_eps=geom.F32_EPS)
    att._param_map_set = True            # (attention programs have no parameter map either; the kfac map must refuse by itself)
    with pytest.raises(DqmcError, match='dqmc error -4'):
        att.set_kfac_tables(tabs, layout)


# ---- 2. the direction against the tree path ----
@pytest.mark.parametrize('name', ['paulinet', 'ferminet'])
def test_direction_against_the_tree_path(name):
    h, wf, trees, r, r2 = _wf_and_batch(name=name)
    check_flat_against_tree(h, wf, trees, r, r2)


def test_two_states_use_their_own_cotangents():
    h, wf, trees, r, r2 = _wf_and_batch(S=2)
    check_flat_against_tree(h, wf, trees, r, r2)


# ---- 3. invalid walkers ----
def test_invalid_walkers_contribute_nothing():
    h, wf, trees, r, _ = _wf_and_batch(B=6)
    eng = wf.engine(trees[0])
    r = r.clone()
    r[0, 0, 1, 1] = r[0, 0, 1, 0]
    r[0, 0, 4, 2, 0] = float('nan')
    s, l = eng.wf_eval(r[0, 0])
    if int(s[1]) != 0:
        r[0, 0, 1, 0, 1] = float('inf')
        s, l = eng.wf_eval(r[0, 0])
    assert int(s[1]) == 0 or not bool(torch.isfinite(l[1]))
    assert not bool(torch.isfinite(l[4])) or int(s[4]) == 0
    cot = torch.as_tensor(np.random.default_rng(5).normal(size=6))
    good = [0, 2, 3, 5]

    def direction(rr, c):
        lay = eng.program.kfac_layout()
        fac = torch.empty(lay['n_factor_doubles'], dtype=F64)
        rest = torch.empty(rr.shape[0], lay['n_rest'], dtype=F64)
        sg, lp, g, _, rest = eng.log_psi_kfac(rr, c, out=(fac, rest))
        st = eng.kfac_state()
        delta, dot = eng.kfac_direction(eng.grad_to_params(g), fac, rest, lp, sg, st, True, 0.95, DAMPING)
        return delta, dot, st
    d_all, dot_all, st_all = direction(r[0, 0].contiguous(), cot)
    d_good, dot_good, st_good = direction(r[0, 0][good].contiguous(), cot[good].contiguous())
    assert torch.isfinite(d_all).all() and torch.isfinite(dot_all).all() and torch.isfinite(st_all).all()
    worst, where = leaf_deviation(eng.program, d_all, eng.program.unflatten_params(d_good))
    print('worst leaf', where, worst)
    assert worst <= 1e-10, (where, worst)
    np.testing.assert_allclose(dot_all.numpy(), dot_good.numpy(), rtol=1e-10)
    np.testing.assert_allclose(st_all.numpy(), st_good.numpy(), rtol=1e-10, atol=1e-10 * float(st_good.abs().max()))


# ---- 4. determinism, and exactly n_params + 1 entries written ----
def test_identical_calls_are_bit_identical_and_nothing_else_is_written():
    *_, eng, r = jac_engine('paulinet', 'LiH', 7, 'cpu', emu_lib(), **SMALL)
    lay = eng.program.kfac_layout()
    fac = torch.empty(lay['n_factor_doubles'], dtype=F64)
    rest = torch.empty(7, lay['n_rest'], dtype=F64)
    cot = torch.as_tensor(np.random.default_rng(1).normal(size=7))
    sg, lp, g, _, rest = eng.log_psi_kfac(r, cot, out=(fac, rest))
    gt = eng.grad_to_params(g)
    n = eng.program.n_params()
    outs = []
    for _ in range(2):
        st = eng.kfac_state()
        eng.kfac_direction(gt, fac, rest, lp, sg, st, True, 0.95, DAMPING)               # a first call, then a mixing one
        buf_d, buf_s = torch.full((n + 6,), float('nan'), dtype=F64), torch.full((1 + 3,), float('nan'), dtype=F64)
        delta, dot = eng.kfac_direction(gt, fac, rest, lp, sg, st, False, 0.9, DAMPING, out=(buf_d[:n], buf_s[:1]))
        assert torch.isfinite(buf_d[:n]).all() and torch.isnan(buf_d[n:]).all()
        assert torch.isfinite(buf_s[:1]).all() and torch.isnan(buf_s[1:]).all()
        outs.append((delta.clone(), dot.clone(), st.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---- 5. dqmc_kfac_apply ----
@pytest.mark.parametrize('case', ['active', 'inactive', 'off'])
def test_kfac_apply_against_the_formula(case):
    h, spec, tree, A, B = make_pair('paulinet', 'LiH', F64, 'cpu', emu_lib(), **SMALL)
    rng = np.random.default_rng(11)
    n = A.program.n_params()
    theta0 = A.params_flat(tree)
    delta = torch.as_tensor(rng.normal(size=n))
    lr = 0.05
    nc = {'active': 1e-3, 'inactive': 1e-3, 'off': 0.0}[case]
    dot = torch.tensor([{'active': 7.0, 'inactive': 0.2, 'off': 7.0}[case]], dtype=F64)      # lr^2 dot = 1.75e-2 / 5e-4 against 1e-3
    coeff = norm_constraint_coeff(lr, float(dot), nc)
    assert (coeff < 1) == (case == 'active')
    A.wf_eval(torch.as_tensor(synthetic_walkers(h, 2, seed=0)))
    before = A.graph_counters()
    theta, norms = theta0.clone(), torch.zeros(4, dtype=F64)
    A.kfac_apply(theta, delta, dot, lr, nc, norms=norms)
    assert A.graph_counters() == before
    want = theta0 + (-lr * coeff) * delta
    assert torch.allclose(theta, want, rtol=1e-15, atol=1e-15 * float(want.abs().max()))
    ref = torch.stack([theta0.norm(), delta.norm(), (lr * coeff * delta).norm(), lr * lr * dot[0]])
    assert torch.allclose(norms, ref, rtol=1e-13, atol=0)
    # the weights after the call: bit for bit dqmc_set_weights from the same doubles
    B.set_params(B.program.unflatten_params(theta))
    assert 0 in assert_same_buffers(B, A)
    # a non-positive <delta, g> switches the constraint off as well
    theta2 = theta0.clone()
    A.kfac_apply(theta2, delta, torch.tensor([-3.0], dtype=F64), lr, 1e-3)
    assert torch.allclose(theta2, theta0 - lr * delta, rtol=1e-15, atol=1e-15 * float(want.abs().max()))


# ---- 6. large damping ----
def test_large_damping_tends_to_the_gradient():
    h, wf, trees, r, _ = _wf_and_batch()
    lam = 1e16
    _, deltas, stats, _ = compute_energy_loss_and_kfac(None, h, wf, trees, r, damping=lam, flat=True)
    d, g = deltas[0], stats['grad'][0]
    err = float((lam * d - g).norm() / g.norm())
    assert err < 1e-6, err


# ---- 7. fit_wf with KFACOptimizer ----
def _lih():
    return MolecularHamiltonian(mol=Molecule.from_name('LiH')), small_spec('paulinet', **SMALL)


def test_fit_wf_one_state_against_the_host_loop():
    """Measured on the reference side (LiH / PauliNet SMALL, 6 walkers, 3 steps, lr 0.05, norm constraint 1e-3): a 1e-10
    relative perturbation of the first direction leaves a relative theta difference of 7.0e-13 after three steps
    (amplification 0.007: the norm constraint is active, so the step scales with the square root of the perturbation, and
    the parameters move by 7e-2 of their size); the device path is allowed 10 x that, 7.0e-12, and deviates by 4e-15.  The
    bound is measured again in every run (kfac_optimizer_util.check_kfac_fit_parity), never taken from the device path."""
    h, spec = _lih()
    stats, state = check_kfac_fit_parity(h, spec, F64, 'cpu', emu_lib(), 1, 6, 3, seed=5)
    for st in stats:
        for key in ('opt/param_norm', 'opt/grad_norm', 'opt/update_norm', 'opt/scaled_grad_norm_sq'):
            assert tuple(st[key].shape) == (1,) and bool(torch.isfinite(st[key]).all()), key
    assert state.opt[0]['count'] == 3 and set(state.opt[0]) == {'theta', 'kfac', 'count', 'norms'}


def test_fit_wf_two_states_merged_against_the_host_loop():
    """As above with two states and merge_keys=['Jastrow']: reference-side difference 1.5e-12 (amplification 0.015), bound
    1.5e-11, device path 1e-15."""
    h, spec = _lih()
    stats, state = check_kfac_fit_parity(h, spec, F64, 'cpu', emu_lib(), 2, 6, 3, seed=6, merge_keys=['Jastrow'])
    t0, t1 = state.opt[0]['theta'], state.opt[1]['theta']
    assert not torch.equal(t0, t1)
    # the merged Jastrow leaves are equal, the others are not
    from optimizer_util import training_setup
    wf = training_setup(h, spec, F64, 'cpu', emu_lib(), 1, 2, 1, 0)[0]
    for (mod, _), (sl, _) in wf.engine(wf.init(0)).program.leaf_slices().items():
        if 'Jastrow' in mod:
            assert torch.equal(t0[sl], t1[sl]), mod


def test_fit_wf_with_a_loss_function_against_the_host_loop():
    """Two states, loss.create_loss_fn(alpha=1): the cotangents of the whole loss enter the reverse pass.  Reference-side
    difference 2.6e-12 (amplification 0.026), bound 2.6e-11, device path 3e-15."""
    h, spec = _lih()
    stats, state = check_kfac_fit_parity(h, spec, F64, 'cpu', emu_lib(), 2, 6, 3, seed=7, loss_kw=dict(alpha=1.0))
    for st in stats:
        assert bool(torch.isfinite(st['loss']).all()) and bool(torch.isfinite(st['overlap/pairwise/mean']).all())


def test_raising_spin_penalty_is_refused():
    from deepqmc_amd.wf import NeuralNetworkWaveFunction
    h, spec = _lih()
    wf = NeuralNetworkWaveFunction(h, spec, dtype=F64, device='cpu', lib=emu_lib(), norm_eps=geom.F32_EPS)
    with pytest.raises(NotImplementedError, match="'raising' spin penalty"):
        KFACOptimizer(loss_fn=create_loss_fn(h, wf, spin_penalty=1.0, spin_penalty_type='raising'))


def test_schedules():
    s = InverseSchedule(0.05, 10000)
    assert s(0) == 0.05 and s(10000) == 0.025 and s(30000) == 0.05 / 4
    assert ConstantSchedule(0.3)(0) == ConstantSchedule(0.3)(17) == 0.3
    import deepqmc_amd.optimizer as O
    assert {'KFACOptimizer', 'InverseSchedule', 'ConstantSchedule'} <= set(O.__all__)
