"""The multi-state training loss through the SIMT emulation of the kernels: dqmc_clip_rows against torch.sort, dqmc_psi_ratio
against the torch ratio, the cotangents of both assembly paths against autograd of the restated reference tangent, the
end-to-end loss and gradients on LiH, the running averages, fit_wf with a loss function against the host-path loop, errors."""
import functools
import math

import numpy as np
import pytest
import torch

from deepqmc_amd.ewm import init_multi_mol_multi_state_ewm
from deepqmc_amd.fit import TrainState, fit_wf
from deepqmc_amd.loss import compute_spin_raising_contributions, create_loss_fn, median_clip_and_mask, psi_ratio_clip_and_mask
from deepqmc_amd.optimizer import NaturalGradientOptimizer, NoOptimizer
from deepqmc_amd.sampling import MoleculeIdxSampler
from loss_util import (F64, SMALL, check_clip_rows, check_clip_rows_nan, check_cotangents, check_end_to_end, check_fit_parity_loss,
                       check_fit_without_loss_fn, check_psi_ratio, check_raising_gradient, lih, lih_batch, ref_cotangents,
                       ref_ewm_init, ref_ewm_update, ref_loss_value, ref_median_clip_and_mask, ref_psi_ratio_clip_and_mask)
from optimizer_util import make_pair, training_setup
from param_grad_util import leaf_errors
from simt_util import emu_lib

FIT_SEED, FIT_LR = 3, 2e-2       # the start of test_optimizer_emu's parity runs


@pytest.fixture(scope='module')
def eng():
    return make_pair('paulinet', 'LiH', torch.float64, 'cpu', emu_lib(), **SMALL)[3]


# ---- 1. dqmc_clip_rows
@pytest.mark.parametrize('n_rows', [1, 9])
@pytest.mark.parametrize('B', [1, 2, 3, 63, 64, 65, 257, 4097])
def test_clip_rows_matches_torch_sort(eng, B, n_rows):
    for median_center in (True, False):
        for median_scale in (True, False):
            for exclude_width in (1.0, math.inf):
                check_clip_rows(eng, B, n_rows, median_center, median_scale, exclude_width)


def test_clip_rows_with_a_nan_returns_and_poisons_only_that_row(eng):
    check_clip_rows_nan(eng)


def test_torch_psi_ratio_clip_is_the_restated_one():
    x = torch.randn(65, dtype=F64, generator=torch.Generator().manual_seed(1))
    x[3] = 50.0
    for got, ref in zip(psi_ratio_clip_and_mask(x, clip_width=4.0, exclude_width=8.0), ref_psi_ratio_clip_and_mask(x, 4.0, 8.0)):
        assert torch.equal(got, ref)


# ---- 2. dqmc_psi_ratio
@pytest.mark.parametrize('B', [5, 257])
@pytest.mark.parametrize('S', [1, 3])
def test_psi_ratio_matches_the_torch_ratio(eng, S, B):
    check_psi_ratio(eng, S, B)


# ---- 3. cotangents from synthetic inputs
@pytest.mark.parametrize('B', [5, 64, 257])
@pytest.mark.parametrize('S', [1, 2, 3])
def test_cotangents_match_autograd_of_the_restated_tangent(eng, S, B):
    for k, scale_overlap_by in enumerate((None, 'energy_gap', 'energy_std', 'max_gap_std')):
        for nan_ewm in (False, True):
            spin_kind = ('squared', 'raising')[(k + nan_ewm) % 2]
            states = None if S == 1 or k % 2 else list(range(S))[1:]          # a proper subset where there is one
            check_cotangents(eng, S, B, scale_overlap_by, nan_ewm, 'energy' if k % 2 == 0 else None, spin_kind, states, seed=k)
    check_cotangents(eng, S, B, 'max_gap_std', False, 'energy', None, None, exclude=False)       # infinite exclude widths, no spin


def test_arbitrary_clip_callables_take_the_torch_path(eng):
    mine = lambda x: median_clip_and_mask(x, clip_width=3.0)
    fn = create_loss_fn(None, None, clip_mask_fn=mine, alpha=1.0)
    assert not fn.kernel_path
    assert create_loss_fn(None, None, functools.partial(functools.partial(median_clip_and_mask, clip_width=3.0), exclude_width=9.0)).kernel_path
    e = torch.randn(2, 7, dtype=F64)
    with pytest.raises(ValueError, match='kernel path'):
        fn.cotangents(e, torch.ones_like(e), torch.ones(2, 2, 7, dtype=F64), path='kernel', engine=eng)


# ---- 4. end to end
@pytest.mark.parametrize('lam', [None, 1.0])
def test_loss_and_gradients_end_to_end(lam):
    h, spec, wf, params, pc, data = lih_batch(2, 16, 'cpu', emu_lib())
    check_end_to_end(h, wf, params, pc, data, lam, 1e-9)


def test_raising_penalty_gradient_matches_autograd_through_the_oracle():
    """B = 3, fixed down_idx: the gradient equals autograd of sum_b [c_b log|psi(r_b)| + k_b L_b(theta)] through the float64 oracle,
    c and k (autograd of the restated tangent) held constant."""
    from oracle import geom
    from oracle import wf as owf
    h, spec, wf, params, pc, data = lih_batch(2, 3, 'cpu', emu_lib())
    beta = h.n_up + h.n_down - 1
    fn = create_loss_fn(h, wf, alpha=4.0, scale_overlap_by='max_gap_std', spin_penalty=1.0, spin_penalty_type='raising')
    loss, grads, (e_loc, ratio, stats) = fn.loss_and_grad(5, params, (pc, None, data), down_idx=beta)
    L = compute_spin_raising_contributions(5, h, wf, pc, params, down_idx=beta)
    w = torch.ones(1, 2, 3, dtype=F64)
    assert abs(float(loss) - float(ref_loss_value(e_loc.double(), w, ratio, L, 4.0, 1.0, [0, 1]))) <= 1e-12 * abs(float(loss))
    c, k = ref_cotangents(e_loc.double()[0], w[0], ratio[0], L[0], data, alpha=4.0, lam=1.0, spin_kind='raising', scale_overlap_by='max_gap_std')
    assert float(k.abs().max()) > 0
    r = pc.r if hasattr(pc, 'r') else pc
    R = torch.as_tensor(np.asarray(h.mol.coords), dtype=F64)
    for s in range(2):
        p = {m: {kk: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for kk, v in lv.items()} for m, lv in params[s].items()}
        tot = 0
        for b in range(3):
            rb = r[0, s, b].double()
            s0, l0 = owf.wave_function(p, spec, rb, R, h.n_up, geom.F32_EPS)
            Lb = 1.0
            for a in range(h.n_up):
                perm = list(range(rb.shape[0]))
                perm[a], perm[beta] = beta, a
                s1, l1 = owf.wave_function(p, spec, rb[perm], R, h.n_up, geom.F32_EPS)
                Lb = Lb - s0.detach() * s1.detach() * torch.exp(l1 - l0)
            assert abs(float(Lb.detach()) - float(L[0, s, b])) <= 1e-9 * max(1.0, abs(float(Lb.detach())))
            tot = tot + c[s, b] * l0 + k[s, b] * Lb
        tot.backward()
        want = {m: {kk: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for kk, v in lv.items()} for m, lv in p.items()}
        err = leaf_errors(grads[s], want)
        worst = max(err, key=err.get)
        print(f'state {s}: worst leaf {worst} {err[worst]:.2e}')
        assert err[worst] <= 1e-9, (worst, err[worst])


def test_raising_penalty_gradient_from_the_jacobians_of_the_swapped_walkers():
    h, spec, wf, params, pc, data = lih_batch(2, 5, 'cpu', emu_lib())
    check_raising_gradient(h, wf, params, pc, data, 1e-9)


def test_the_down_electron_is_drawn_from_the_step_seed():
    from deepqmc_amd.loss import spin_raising_down_idx
    h, _ = lih()
    draws = {spin_raising_down_idx(seed, h) for seed in range(40)}
    assert draws == set(range(h.n_up, h.n_up + h.n_down))
    assert spin_raising_down_idx(11, h) == h.n_up + int(np.random.default_rng([11, 0x5350494e]).integers(h.n_down))


# ---- 5. running averages
def test_ewm_follows_the_restated_update():
    state, update = init_multi_mol_multi_state_ewm((2, 3), window_size=4)
    assert torch.isnan(state.mean).all() and torch.isnan(state.sqerr).all()
    ref = [[ref_ewm_init(4) for _ in range(3)] for _ in range(2)]
    g = torch.Generator().manual_seed(0)
    for k in range(5):                                    # (more updates than the window holds: the decay factors stop shifting)
        sub = None if k % 2 == 0 else [1]
        x = torch.randn(2, 3, generator=g, dtype=F64) - 8.0
        state = update(x if sub is None else x[sub], state, sub)
        for m in range(2):
            if sub is not None and m not in sub:
                continue
            ref[m] = [ref_ewm_update(x[m, s], ref[m][s]) for s in range(3)]
        for key in ('mean', 'var', 'sqerr'):
            want = torch.stack([torch.stack([ref[m][s][key] for s in range(3)]) for m in range(2)])
            got = getattr(state, key)
            assert torch.equal(torch.isnan(got), torch.isnan(want))
            ok = ~torch.isnan(want)
            assert ((got[ok] - want[ok]).abs() <= 1e-14 * want[ok].abs().clamp(min=1.0)).all(), (k, key)
    first = update(torch.full((2, 3), -8.0, dtype=F64), init_multi_mol_multi_state_ewm((2, 3), window_size=4)[0])
    assert torch.equal(first.mean, torch.full((2, 3), -4.0, dtype=F64))        # the reference's under-normalised first mean: x / 2


# ---- 6. fit_wf
def test_fit_wf_with_a_loss_function_matches_the_host_path_loop():
    h, spec = lih()
    check_fit_parity_loss(h, spec, torch.float64, 'cpu', emu_lib(), 48, 5, FIT_LR, FIT_SEED,
                          dict(alpha=4.0, scale_overlap_by='max_gap_std', sort_states_by='energy'))


def test_fit_wf_without_a_loss_function_yields_what_it_yielded():
    h, spec = lih()
    check_fit_without_loss_fn(h, spec, torch.float64, 'cpu', emu_lib(), 16, 3, FIT_LR, FIT_SEED)


def test_other_optimizers_take_the_loss_function():
    """NoOptimizer evaluates loss and ratios without a gradient.  NaturalGradientOptimizer applies -lr delta_s with
    (A_s^T A_s + damping I) delta_s = c_s . J_s, expected here from a DENSE solve: c from autograd of the restated tangent, J from
    log_psi_jacobian, A_s = rows sqrt(m_b / n_s) (J_b - Jbar_s) with the energy clip mask m.  The dense solve is good to
    eps x (|A|^2 + damping) / damping of delta, printed below, and theta moves by lr x delta."""
    h, spec = lih()
    wf, params, sampler, st = training_setup(h, spec, torch.float64, 'cpu', emu_lib(), 2, 8, 2, 1)
    mis = MoleculeIdxSampler(0, 1, 1)
    _, pc, _ = sampler.sample(1 * 1000003, st, params, mis.sample())
    fn = create_loss_fn(h, wf, alpha=4.0)
    nan = torch.full((1, 2), math.nan, dtype=F64)
    batch = (pc, None, {'energy_ewm': nan, 'std_ewm': nan})
    p2, state, e_loc, ratios, stats = NoOptimizer(loss_fn=fn).step(1000003, params, None, batch)
    assert p2 is params and state is None and tuple(ratios.shape) == (1, 2, 2, 8) and torch.isfinite(stats['loss'])
    assert torch.equal(fn.evaluate(1000003, params, batch)['loss'], stats['loss'])
    c, _ = ref_cotangents(e_loc.double()[0], torch.ones(2, 8, dtype=F64), ratios[0], None, batch[2], alpha=4.0)
    r = pc.r if hasattr(pc, 'r') else pc
    damping, lr = 1e-2, 0.05
    deltas = []
    for s in range(2):
        J = wf.log_psi_jacobian(params[s], r[0, s].contiguous())[1].double()
        m = ref_median_clip_and_mask(e_loc.double()[0, s], 5.0, True)[1].to(F64)
        A = torch.sqrt(m / m.sum())[:, None] * (J - (m / m.sum()) @ J)
        F = A.T @ A + damping * torch.eye(J.shape[1], dtype=F64)
        deltas.append(torch.linalg.solve(F, c[s] @ J))
        print(f'state {s}: {J.shape[1]} parameters, condition number {float(torch.linalg.matrix_norm(A, 2)) ** 2 / damping + 1:.1e}')
    prog = wf.engine(params[0]).program
    start = [torch.as_tensor(prog.flatten_params(p)) for p in params]
    opt = NaturalGradientOptimizer(lr, damping=damping, loss_fn=fn)
    for _, state, _, stats in fit_wf(1, h, wf, opt, MoleculeIdxSampler(0, 1, 1), sampler, range(1), TrainState(st, params, None), None):
        for s in range(2):
            moved = (start[s] - state.opt[s]['theta']) / lr
            err = float((moved - deltas[s]).abs().max() / deltas[s].abs().max())
            print(f'state {s}: largest deviation of the applied direction {err:.2e} of max|delta|')
            assert err <= 1e-9, err
        assert 'energy/ewm' in stats and 'overlap/pairwise/mean' in stats


# ---- 7. errors
def test_documented_errors(monkeypatch):
    import torch.distributed as dist
    h, spec = lih()
    wf, params, sampler, st = training_setup(h, spec, torch.float64, 'cpu', emu_lib(), 2, 4, 2, 1)
    _, pc, _ = sampler.sample(3, st, params, MoleculeIdxSampler(0, 1, 1).sample())
    with pytest.raises(ValueError, match='alpha must be set'):
        create_loss_fn(h, wf).loss_and_grad(1, params, (pc, None, {}))
    r = pc.r if hasattr(pc, 'r') else pc
    with pytest.raises(ValueError, match='one molecule|need their geometries'):
        create_loss_fn(h, wf, alpha=1.0).loss_and_grad(1, params, (torch.cat([r, r]), None, {}))
    from deepqmc_amd.types import PhysicalConfiguration
    R2 = torch.as_tensor(np.asarray(h.mol.coords))[None].repeat(2, 1, 1)
    with pytest.raises(ValueError, match='one molecule'):
        create_loss_fn(h, wf, alpha=1.0).loss_and_grad(1, params, (PhysicalConfiguration(R2, torch.cat([r, r]), None), None, {}))
    with pytest.raises(NotImplementedError, match='raising'):
        NaturalGradientOptimizer(loss_fn=create_loss_fn(h, wf, alpha=1.0, spin_penalty=1.0, spin_penalty_type='raising'))
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda *a: 2)
    with pytest.raises(NotImplementedError, match='single process'):
        create_loss_fn(h, wf, alpha=1.0).loss_and_grad(1, params, (pc, None, {}))


def test_attention_programs_raise_what_they_raise_today():
    import dataclasses
    from deepqmc_amd.engine import DqmcError
    from deepqmc_amd.hamil import MolecularHamiltonian
    from deepqmc_amd.molecule import Molecule
    from deepqmc_amd.spec import ANSATZES
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = dataclasses.replace(ANSATZES['psiformer'](), embedding_dim=16, n_interactions=1, n_determinants=1)
    wf, params, sampler, st = training_setup(h, spec, torch.float64, 'cpu', emu_lib(), 1, 4, 2, 1)
    _, pc, _ = sampler.sample(3, st, params, MoleculeIdxSampler(0, 1, 1).sample())
    with pytest.raises(DqmcError, match='dqmc error -4'):
        create_loss_fn(h, wf).loss_and_grad(1, params, (pc, None, {}))
    with pytest.raises(DqmcError, match='dqmc error -4'):
        create_loss_fn(h, wf).loss_and_grad(1, params, (pc, None, {}), flat=True)
