"""What the Engine facade refuses before the C ABI: walkers, geometries and named tensor arguments of the wrong shape, dtype,
layout or device raise DqmcError while the library is replaced by a guard that no entry point may reach; afterwards the
engine computes what it computed before."""
import numpy as np
import pytest
import torch

from deepqmc_amd.engine import DqmcError
from engine_args_util import guarded
from pretrain_util import make, synthetic_dataset, upload
from simt_util import emu_lib

B = 4
F64 = torch.float64


@pytest.fixture(scope='module')
def ctx():
    h, spec, tree, eng, r = make('paulinet', 'LiH', B, 'cpu', emu_lib(), small=dict(embedding_dim=32, n_interactions=1, n_determinants=2))
    upload(eng, synthetic_dataset(h, 'hf', seed=1))
    r = torch.as_tensor(r)
    sign, log = eng.wf_eval(r)
    return dict(h=h, spec=spec, eng=eng, r=r, sign=sign.clone(), log=log.clone())


@pytest.fixture
def eng(ctx):
    with guarded(ctx['eng']) as e:
        yield e


def refused(call, name=None):
    with pytest.raises(DqmcError) as err:
        call()
    if name is not None:
        assert name in str(err.value), str(err.value)


WALKER_CALLS = {
    'wf_eval': lambda e, h, r: e.wf_eval(r),
    'local_energy': lambda e, h, r: e.local_energy(r),
    'psi_and_grad': lambda e, h, r: e.psi_and_grad(r),
    'langevin_update': lambda e, h, r: e.langevin_update(r, 0.1, h.mol.charges),
    'log_psi_vjp': lambda e, h, r: e.log_psi_vjp(r),
    'log_psi_jacobian': lambda e, h, r: e.log_psi_jacobian(r),
    'log_psi_kfac': lambda e, h, r: e.log_psi_kfac(r),
    'log_psi_grad_coords': lambda e, h, r: e.log_psi_grad_coords(r),
    'hf_force': lambda e, h, r: e.hf_force('bare', r),
    'pretrain_target': lambda e, h, r: e.pretrain_target(r),
    'orbitals': lambda e, h, r: e.orbitals(r),
    'orbitals_vjp': lambda e, h, r: e.orbitals_vjp(r, torch.zeros(B, e.spec.n_determinants, e.N, e.N, dtype=F64)),
    'pretrain_loss_grad': lambda e, h, r: e.pretrain_loss_grad(r),
}


@pytest.mark.parametrize('shape', ['B,N+1,3', 'B,3N'])
@pytest.mark.parametrize('method', list(WALKER_CALLS))
def test_bad_walkers_are_refused(ctx, eng, method, shape):
    r = torch.zeros(B, eng.N + 1, 3, dtype=F64) if shape == 'B,N+1,3' else ctx['r'].reshape(B, 3 * eng.N)
    refused(lambda: WALKER_CALLS[method](eng, ctx['h'], r), "'r'")


def test_bad_geometry_is_refused(ctx, eng):
    refused(lambda: eng.wf_eval(ctx['r'], R=torch.zeros(ctx['h'].n_nuc + 1, 3, dtype=F64)), "'R'")


def test_bad_cotangent_is_refused(ctx, eng):
    refused(lambda: eng.log_psi_vjp(ctx['r'], cot=torch.ones(B + 1, dtype=F64)), 'cot')
    refused(lambda: eng.log_psi_kfac(ctx['r'], cot=torch.ones(B + 1, dtype=F64)), 'cot')


@pytest.mark.parametrize('kind', ['float32', 'strided', 'too long', 'meta'])
def test_bad_theta_is_refused(eng, kind):
    n = eng.program.n_params()
    theta = {'float32': lambda: torch.zeros(n, dtype=torch.float32), 'strided': lambda: torch.zeros(2 * n, dtype=F64)[::2],
             'too long': lambda: torch.zeros(n + 1, dtype=F64), 'meta': lambda: torch.empty(n, dtype=F64, device='meta')}[kind]()
    refused(lambda: eng.set_params_flat(theta), 'theta')
    good = torch.zeros(n, dtype=F64)
    refused(lambda: eng.adam_step(theta, good, good, good, lr=0.1), 'theta')
    refused(lambda: eng.apply_update(theta, good), 'theta')
    refused(lambda: eng.kfac_apply(theta, good, torch.zeros(1, dtype=F64), 0.1, 1.0), 'theta')


def test_bad_norms_are_refused(eng):
    v = torch.zeros(eng.program.n_params(), dtype=F64)
    refused(lambda: eng.adam_step(v, v, v, v, lr=0.1, norms=torch.zeros(2, dtype=F64)), 'norms')
    refused(lambda: eng.apply_update(v, v, norms=torch.zeros(2, dtype=F64)), 'norms')


def test_meta_e_loc_is_refused(eng):
    refused(lambda: eng.energy_record(torch.empty(B, dtype=F64, device='meta')), 'e_loc')


def test_float32_factor_buffer_is_refused(ctx, eng):
    n = eng.program.kfac_layout()['n_factor_doubles']
    refused(lambda: eng.log_psi_kfac(ctx['r'], out=(torch.zeros(n, dtype=torch.float32), None)), 'out')


def test_clip_rows_needs_two_dimensions(eng):
    refused(lambda: eng.clip_rows(torch.zeros(B, dtype=F64)), "'x'")


def test_bad_loss_terms_are_refused(eng):
    S = 2
    z = lambda *shape: torch.zeros(*shape, dtype=F64)
    mask = lambda *shape: torch.ones(*shape, dtype=torch.bool)
    overlap = dict(alpha=1.0, r_clip=z(S, S, B), r_mask=mask(S, S, B), r_stats=z(S * S, 4), scale=z(S, S))
    refused(lambda: eng.loss_cotangents(z(S, B), mask(S, B), z(S, 4), rank=torch.arange(S, dtype=torch.int64), **overlap), 'rank')
    refused(lambda: eng.loss_cotangents(z(S, B), mask(S, B + 1), z(S, 4)), 'e_mask')


def sampler_state(eng, r, **over):
    st = {'r': r.clone(), 'log': torch.zeros(B, dtype=F64), 'sign': torch.ones(B, dtype=torch.int32), 'age': torch.zeros(B, dtype=torch.int32),
          'tau': torch.full((1,), 0.3, dtype=F64), 'force': torch.zeros(B, eng.N, 3, dtype=F64)}
    st.update(over)
    return st


SAMPLER_CALLS = {
    'mcmc_steps': lambda e, h, st, **kw: e.mcmc_steps(st, 2, **kw),
    'langevin_steps': lambda e, h, st, **kw: e.langevin_steps(st, 2, h.mol.charges, **kw),
    'exchange_step': lambda e, h, st: e.exchange_step(st, np.zeros(B, np.int64), np.zeros(B, np.int64), torch.full((B,), 0.5, dtype=F64)),
}


@pytest.mark.parametrize('method', list(SAMPLER_CALLS))
def test_bad_sampler_state_is_refused(ctx, eng, method):
    call = SAMPLER_CALLS[method]
    refused(lambda: call(eng, ctx['h'], sampler_state(eng, ctx['r'], age=torch.zeros(B, dtype=F64))), 'age')
    refused(lambda: call(eng, ctx['h'], sampler_state(eng, ctx['r'], log=torch.zeros(B + 1, dtype=F64))), 'log')


@pytest.mark.parametrize('method', ['mcmc_steps', 'langevin_steps'])
def test_bad_noise_is_refused(ctx, eng, method):
    kw = dict(noise=torch.zeros(2, B, eng.N, 2, dtype=F64), unif=torch.full((2, B), 0.5, dtype=F64))
    refused(lambda: SAMPLER_CALLS[method](eng, ctx['h'], sampler_state(eng, ctx['r']), **kw), 'noise')


def test_bad_exchange_indices_are_refused(ctx, eng):
    st = sampler_state(eng, ctx['r'])
    u = torch.full((B,), 0.5, dtype=F64)
    refused(lambda: eng.exchange_step(st, np.zeros(B + 1, np.int64), np.zeros(B, np.int64), u), 'up_idx')
    refused(lambda: eng.langevin_update(ctx['r'], 0.1, np.ones(ctx['h'].n_nuc + 1)), 'mol_charges')


def test_engine_is_unharmed(ctx):
    """After every refusal above (this test runs last): the same values as before the guard was installed, on the real library,
    and a geometry tensor that does not alias the molecule's read-only array."""
    eng = ctx['eng']
    sign, log = eng.wf_eval(ctx['r'])
    assert torch.equal(sign, ctx['sign']) and torch.equal(log, ctx['log'])
    assert not np.shares_memory(eng.R.numpy(), ctx['h'].mol.coords)
    np.testing.assert_array_equal(eng.R.numpy(), np.asarray(ctx['h'].mol.coords, np.float64))
