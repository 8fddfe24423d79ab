"""Ownership of the engine's device memory (DevBuf, csrc/engine.hip) through the SIMT emulation, whose hipMalloc / hipFree
count: every allocation of a context is released with it, a failed dqmc_create releases what it had, a call whose needs fit
the current capacities allocates nothing, and a failed growth leaves the context usable."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import deepqmc_amd.engine as E
from deepqmc_amd.engine import DqmcError, Engine
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.params import init_params
from deepqmc_amd.sampling import synthetic_walkers
from deepqmc_amd.spec import ANSATZES
from oracle import geom
from pretrain_util import synthetic_dataset, upload
from simt_util import emu_lib
from test_ecp import TABLES
from test_pseudo_hamiltonian import synthetic_tables

SMALL = dict(embedding_dim=32, n_interactions=1, n_determinants=2)
DTYPES = {'float32': torch.float32, 'float64': torch.float64}
N_SUB = 2


def counter(name):
    return ctypes.c_longlong.in_dll(emu_lib(), name)


@pytest.fixture(autouse=True)
def no_alloc_limit():
    yield
    counter('simt_alloc_limit').value = 0


def make(dtype, h=None, seed=3):
    h = h or MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = dataclasses.replace(ANSATZES['paulinet'](), **SMALL)
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=seed, perturb_envelopes=0.1)
    return h, Engine(spec, h, tree, dtype=dtype, device='cpu', lib=emu_lib(), norm_eps=geom.F32_EPS)


def walkers(h, eng, n, seed=7):
    return torch.as_tensor(synthetic_walkers(h, n, seed=seed), dtype=eng.dtype)


def sampler_state(eng, r, force=False):
    sign, log = eng.wf_eval(r)
    st = {'r': r.clone(), 'log': log, 'sign': sign, 'age': torch.zeros(r.shape[0], dtype=torch.int32),
          'tau': torch.full((1,), 0.3, dtype=eng.dtype)}
    if force:
        st['force'] = torch.zeros_like(r)
    return st


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_every_allocation_is_released_with_its_context(dtype):
    live = counter('simt_live_allocs')
    before = live.value
    h, eng = make(DTYPES[dtype])
    r = walkers(h, eng, 8)
    eng.wf_eval(r)
    eng.local_energy(r)                      # (float32: creates the twin and the refinement scratch)
    eng.mcmc_steps(sampler_state(eng, r), N_SUB, seed=1)
    eng.langevin_steps(sampler_state(eng, r, force=True), N_SUB, h.mol.charges, seed=1)
    eng.set_params_flat(eng.params_flat())
    eng.set_option('fused_dbg', 1)
    eng.wf_eval(r)
    eng.set_option('fused_dbg', 0)
    eng.log_psi_vjp(r)
    eng.log_psi_jacobian(r)
    sign, log, g, _, rest = eng.log_psi_kfac(r)
    eng.log_psi_grad_coords(r)
    eng._ensure_kfac_map()
    lay = eng.program.kfac_layout()
    fac = torch.empty(lay['n_factor_doubles'], dtype=torch.float64)
    sign, log, g, _, rest = eng.log_psi_kfac(r, out=(fac, None))
    eng.kfac_direction(eng.grad_to_params(g), fac, rest, log, sign, eng.kfac_state(), True, 0.95, 1e-3)
    upload(eng, synthetic_dataset(h, 'hf'))
    eng.pretrain_loss_grad(r)
    assert live.value > before
    others = []
    mol = Molecule.from_name('LiH')
    for kw in (dict(ecp_type='synthetic', ecp_mask=[True, False], ecp_tables=TABLES),
               dict(ecp_type='PH', ecp_mask=[True, False], ph_tables=synthetic_tables())):
        h2, e2 = make(DTYPES[dtype], MolecularHamiltonian(mol=mol, **kw))
        e2.local_energy(walkers(h2, e2, 8), rng=5)
        others.append(e2)
    for e in [eng] + others:
        e.close()
    assert live.value == before


def test_a_failed_create_releases_everything():
    """The malformed program of test_abi.py::test_malformed_program_is_rejected."""
    h, eng = make(torch.float64)
    bad = eng.program
    next(op for op in bad.ops if op.kind == 3).i[17] = 10_000          # destination buffer out of range
    live = counter('simt_live_allocs')
    before = live.value
    orig = E.compile_program
    try:
        E.compile_program = lambda *a, **k: bad
        with pytest.raises(DqmcError, match='malformed op'):
            make(torch.float64)
    finally:
        E.compile_program = orig
    assert live.value == before
    eng.close()


def test_steady_state_allocates_nothing():
    h, eng = make(torch.float32)
    theta = eng.params_flat()
    total = counter('simt_total_allocs')

    def round_(n):
        r = walkers(h, eng, n)
        st = sampler_state(eng, r)
        t0 = total.value
        eng.local_energy(r)
        eng.mcmc_steps(st, N_SUB, seed=1)
        eng.log_psi_vjp(r)
        eng.set_params_flat(theta)
        return total.value - t0

    round_(8)                       # warm-up
    assert round_(8) == 0
    assert round_(4) == 0
    round_(16)                      # (may grow)
    assert round_(8) == 0
    eng.close()


def mc_scratch_bytes(B, N, n_sub, size):
    """The scratch of Engine::mcmc (csrc/engine_mcmc.inl): r_prop, logpsi_prop, sign_prop, noise, unif, each rounded up to 256 bytes."""
    al = lambda x: (x + 255) // 256 * 256
    ns, n_r = max(n_sub, 1), B * N * 3
    return al(size * n_r) + al(size * B) + al(4 * B) + al(size * n_r * ns) + al(size * B * ns)


def test_a_failed_growth_leaves_the_context_usable():
    """A growth the allocator refuses must not leave the old capacity beside a null pointer: the next, smaller call
    re-allocates and answers bit for bit what a context that never saw the failure answers."""
    big, limit = 4096, counter('simt_alloc_limit')
    h, A = make(torch.float32)
    _, fresh = make(torch.float32)
    N = h.n_up + h.n_down
    r = walkers(h, A, 8)
    rng = np.random.default_rng(2)
    noise, unif = rng.normal(size=(N_SUB, 8, N, 3)), rng.uniform(size=(N_SUB, 8))
    for eng in (A, fresh):          # the same warm-up for both
        eng.local_energy(r)
        eng.mcmc_steps(sampler_state(eng, r), N_SUB, noise=noise, unif=unif)
    r_big = walkers(h, A, big)            # (neither refused call gets as far as a kernel)
    st_big = {'r': r_big.clone(), 'log': torch.zeros(big), 'sign': torch.ones(big, dtype=torch.int32),
              'age': torch.zeros(big, dtype=torch.int32), 'tau': torch.full((1,), 0.3)}

    # d_mc
    limit.value = mc_scratch_bytes(big, N, N_SUB, 4) - 1
    assert limit.value > mc_scratch_bytes(8, N, N_SUB, 4)
    with pytest.raises(DqmcError):
        A.mcmc_steps(st_big, N_SUB, seed=1)
    limit.value = 0
    out = []
    for eng in (A, fresh):
        st = sampler_state(eng, r)
        _, acc = eng.mcmc_steps(st, N_SUB, noise=noise, unif=unif, return_accept=True)
        out.append((st, acc))
    (sa, acca), (sf, accf) = out
    assert torch.equal(acca, accf)
    for k in ('r', 'log', 'sign'):
        assert torch.equal(sa[k], sf[k]), k

    # d_flag / d_score: the flag list of `big` walkers is the first thing a float32 local-energy call grows
    limit.value = 4 * (big + 1) - 1
    with pytest.raises(DqmcError):
        A.local_energy(r_big)
    limit.value = 0
    (ea, sta), (ef, stf) = A.local_energy(r), fresh.local_energy(r)
    assert torch.isfinite(ea).all() and torch.equal(ea, ef)
    for k in sta:
        assert torch.equal(sta[k], stf[k]), k
    A.close()
    fresh.close()
