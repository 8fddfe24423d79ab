"""Shared pieces of the tests of the opt-in reverse pass through attention (library option "attention_reverse",
NeuralNetworkWaveFunction(..., attention_reverse=True)): narrow Psiformer contexts with the option on, a training setup whose
wave function carries the flag, the oracle's Kronecker factors including the attention projections, and the checks that the
emulated tests (tests/test_attention_reverse_emu.py) and the GPU tests (tests/test_gpu_attention_reverse.py) both run."""
import copy
import dataclasses
import math

import numpy as np
import torch

from deepqmc_amd.engine import Engine
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.params import init_params
from deepqmc_amd.sampling import (DecorrSampler, MultiElectronicStateSampler, MultiNuclearGeometrySampler,
                                  synthetic_walkers)
from deepqmc_amd.spec import ANSATZES, psiformer
from deepqmc_amd.wf import NeuralNetworkWaveFunction
from kfac_util import library_module_sums, oracle_factors, rel_fro
from optimizer_util import device_path_loop, flat, host_path_loop
from oracle import geom
from oracle import wf as owf

NARROW = dict(embedding_dim=32, n_interactions=1, n_determinants=2)      # 4 heads of width 8
ATT = 'multi_head_attention'


def narrow_psiformer(**kw):
    return dataclasses.replace(psiformer(), **{**NARROW, **kw})


def psiformer_engine(molname, B, device, lib=None, dtype=torch.float64, seed=3, option=1, spec=None, **spec_kw):
    """(spec, h, tree, eng, r [B, N, 3] float64 numpy): a Psiformer context on a named molecule with option
    "attention_reverse" set to `option` (None: left at its default)."""
    h = MolecularHamiltonian(mol=Molecule.from_name(molname))
    spec = spec if spec is not None else narrow_psiformer(**spec_kw)
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=seed, perturb_envelopes=0.1)
    eng = Engine(spec, h, tree, dtype=dtype, device=device, lib=lib, norm_eps=geom.F32_EPS)
    if option is not None:
        eng.set_option('attention_reverse', option)
    return spec, h, tree, eng, synthetic_walkers(h, B, seed=seed + 1)


def psiformer_wf(h, spec, device, lib=None, dtype=torch.float64, attention_reverse=True):
    return NeuralNetworkWaveFunction(h, spec, dtype=dtype, device=device, lib=lib, norm_eps=geom.F32_EPS,
                                     attention_reverse=attention_reverse)


def training_setup_attention(h, spec, dtype, device, lib, n_states, n_walkers, length, seed):
    """optimizer_util.training_setup with a wave function made with attention_reverse=True."""
    wf = psiformer_wf(h, spec, device, lib, dtype)
    params = [wf.init(seed + s, perturb_envelopes=0.1) for s in range(n_states)]
    sampler = MultiNuclearGeometrySampler(MultiElectronicStateSampler(DecorrSampler(h, wf, length=length, tau=0.3), n_states))
    R = torch.as_tensor(h.mol.coords, dtype=dtype, device=device)[None]
    return wf, params, sampler, sampler.init(seed, params, n_walkers, R)


# ---------------------------------------------------------------- chunking and determinism
def check_chunking_and_determinism(eng, r, budget_mb=1):
    """Two identical calls of log_psi_vjp / log_psi_jacobian / log_psi_grad_coords are bit-identical; with a workspace budget
    that forces several walker chunks the Jacobian and the coordinate gradients stay bit-identical and the VJP (whose walker
    sums are regrouped by the chunks) agrees to 1e-12, the bounds of tests/test_param_grad_emu.py."""
    B = r.shape[0]
    cot = torch.as_tensor(np.random.default_rng(1).normal(size=B), dtype=eng.dtype, device=r.device)
    s0, l0, g0 = eng.log_psi_vjp(r, cot)
    s1, l1, g1 = eng.log_psi_vjp(r, cot)
    assert torch.equal(g0, g1) and torch.equal(l0, l1) and torch.equal(s0, s1)
    assert eng.last_chunks()['own'] == 1
    _, _, J0 = eng.log_psi_jacobian(r)
    _, _, J1 = eng.log_psi_jacobian(r)
    assert torch.equal(J0, J1)
    c0 = eng.log_psi_grad_coords(r)
    c1 = eng.log_psi_grad_coords(r)
    assert torch.equal(c0[2], c1[2]) and torch.equal(c0[3], c1[3])
    assert float(g0.abs().max()) > 0 and float(c0[2].abs().max()) > 0
    eng.set_option('ws_budget_mb', budget_mb)
    try:
        s2, l2, g2 = eng.log_psi_vjp(r, cot)
        assert eng.last_chunks()['own'] > 1
        assert torch.equal(s0, s2)
        np.testing.assert_allclose(l2.cpu().numpy(), l0.cpu().numpy(), rtol=0, atol=1e-13)
        np.testing.assert_allclose(g2.cpu().numpy(), g0.cpu().numpy(), rtol=1e-12, atol=1e-14 * float(g0.abs().max()))
        _, _, J2 = eng.log_psi_jacobian(r)
        assert eng.last_chunks()['own'] > 1
        assert torch.equal(J2, J0)
        c2 = eng.log_psi_grad_coords(r)
        assert eng.last_chunks()['own'] > 1
        assert torch.equal(c2[2], c0[2]) and torch.equal(c2[3], c0[3])
    finally:
        eng.set_option('ws_budget_mb', 32 << 10)


# ---------------------------------------------------------------- KFAC factors including the attention projections
def oracle_factors_with_attention(spec, h, tree, r):
    """kfac_util.oracle_factors (the MLPs and the embedding projection) plus the query / key / value / linear modules of every
    attention layer: oracle.wf.attention restated here with each of its four bias-free projections recorded, A = sum x^T x over
    walkers and electrons and G = sum dz^T dz with dz from torch.autograd of log|psi|."""
    rec = []
    orig = owf.attention

    def attention(params, prefix, hx, num_heads, mask=None):
        assert mask is None
        T, D = hx.shape
        hd = D // num_heads

        def lin(name, x):
            z = x @ params[f'{prefix}/{name}']['w']
            z.retain_grad()
            rec.append((f'{prefix}/{name}', x.detach(), z))
            return z
        q, k, v = (lin(nm, hx).reshape(T, num_heads, hd) for nm in ('query', 'key', 'value'))
        w = torch.softmax(torch.einsum('thd,Thd->htT', q, k) / math.sqrt(hd), dim=-1)
        return lin('linear', torch.einsum('htT,Thd->thd', w, v).reshape(T, num_heads * hd))

    owf.attention = attention
    try:
        out = oracle_factors(spec, h, tree, r)
    finally:
        owf.attention = orig
    for name, x, z in rec:      # (every walker's backward has run: z.grad is that walker's dz)
        A, G = out.get(name, (0, 0))
        out[name] = (A + x.T @ x, G + z.grad.T @ z.grad)
    return out


def check_kfac(eng, spec, h, tree, r, tol_a=1e-12, tol_g=1e-9):
    """log_psi_kfac of a Psiformer: the gradient is the VJP's bit for bit, the attention projections have A / G factors of the
    shapes kfac_blocks gives, and every module's factors equal the oracle's (the tolerances of tests/test_kfac_emu.py)."""
    s, l, g, factors, rest = eng.log_psi_kfac(r)
    s0, l0, g0 = eng.log_psi_vjp(r)
    assert torch.equal(g, g0) and torch.equal(l, l0) and torch.equal(s, s0)
    blocks, fallback = eng.program.kfac_blocks()
    got = library_module_sums(eng.program, factors)
    att = [m for m in got if f'/{ATT}/' in m]
    assert sorted(m.rsplit('/', 1)[1] for m in att) == sorted(['query', 'key', 'value', 'linear'] * spec.n_interactions), att
    for m in att:
        blk = blocks[m]
        assert not blk['has_bias'] and m not in fallback
        assert tuple(got[m][0].shape) == (blk['n_in'], blk['n_in']) and tuple(got[m][1].shape) == (blk['n_out'], blk['n_out'])
        assert blk['n_in'] == blk['n_out'] == spec.embedding_dim
    ref = oracle_factors_with_attention(spec, h, tree, r.cpu().numpy())
    assert set(got) == set(ref), set(got) ^ set(ref)
    err_a = {m: rel_fro(got[m][0], A) for m, (A, G) in ref.items()}
    err_g = {m: rel_fro(got[m][1], G) for m, (A, G) in ref.items()}
    ma, mg = max(err_a, key=err_a.get), max(err_g, key=err_g.get)
    print(f'kfac factors: worst A {ma} {err_a[ma]:.2e}, worst G {mg} {err_g[mg]:.2e}')
    assert err_a[ma] < tol_a, ('A', ma, err_a[ma])
    assert err_g[mg] < tol_g, ('G', mg, err_g[mg])
    for m in att:
        assert float(torch.linalg.norm(got[m][1])) > 0, m


# ---------------------------------------------------------------- training
def check_adam_fit_parity(h, spec, device, lib, n_walkers=8, steps=3, lr=1e-3, seed=11, rtol=1e-10):
    """fit_wf + AdamOptimizer against optimizer_util.host_path_loop from the same start, one state: every step's loss and the
    final parameters at optimizer_util.check_fit_parity's rtol (1e-10, the bound tests/test_optimizer_emu.py holds PauliNet to)."""
    wf_h, params_h, sampler_h, st_h = training_setup_attention(h, spec, torch.float64, device, lib, 1, n_walkers, 3, seed)
    losses_h = host_path_loop(seed, h, wf_h, params_h, sampler_h, st_h, steps, lr)
    wf_d, params_d, sampler_d, st_d = training_setup_attention(h, spec, torch.float64, device, lib, 1, n_walkers, 3, seed)
    start = copy.deepcopy(params_d)
    losses_d, state = device_path_loop(seed, h, wf_d, params_d, sampler_d, st_d, steps, lr)
    print('host-path losses  ', losses_h)
    print('device-path losses', losses_d)
    assert all(np.isfinite(losses_h)) and all(np.isfinite(losses_d))
    dev = max(abs(a - b) / abs(a) for a, b in zip(losses_h, losses_d))
    assert dev <= rtol, (losses_h, losses_d)
    prog = wf_d.engine(params_d[0]).program
    th, td, t0 = flat(params_h[0], prog), flat(params_d[0], prog), flat(start[0], prog)
    sl = prog.leaf_slices()
    moved = [m for (m, leaf), (s, _) in sl.items() if f'/{ATT}/' in m and np.abs(td[s] - t0[s]).max() > 0]
    assert len(moved) == 4 * spec.n_interactions, moved          # query, key, value and linear of every layer were stepped
    err = np.abs(th - td).max() / np.abs(th).max()
    print(f'final theta deviation {err:.2e} of max|theta|')
    assert err <= rtol, err


def check_kfac_step(h, spec, device, lib, n_walkers=8, seed=11):
    """One KFACOptimizer step of fit_wf: finite, moves the attention projections, and two runs from the same start are
    bit-identical."""
    from kfac_optimizer_util import device_kfac_loop
    runs = []
    for _ in range(2):
        wf, params, sampler, st = training_setup_attention(h, spec, torch.float64, device, lib, 1, n_walkers, 3, seed)
        start = wf.engine(params[0]).program.flatten_params(params[0])
        thetas, stats, state = device_kfac_loop(seed, h, wf, params, sampler, st, 1, 0.05, 1e-3, 1e-3, 0.95)
        runs.append((thetas[0][0], start, wf.engine(params[0]).program))
    theta, start, prog = runs[0]
    assert np.all(np.isfinite(theta))
    for (m, leaf), (s, _) in prog.leaf_slices().items():
        if f'/{ATT}/' in m:
            assert np.abs(theta[s] - start[s]).max() > 0, m
    assert np.array_equal(theta, runs[1][0])


def check_loss_fn_flat(h, spec, device, lib, n_walkers=8, seed=11):
    """create_loss_fn(h, wf).loss_and_grad: finite with flat=True and flat=False, and the flat gradient is the tree flattened
    (the tolerances of loss_util.check_end_to_end)."""
    from deepqmc_amd.loss import create_loss_fn
    from deepqmc_amd.sampling import MoleculeIdxSampler
    wf, params, sampler, st = training_setup_attention(h, spec, torch.float64, device, lib, 1, n_walkers, 2, seed)
    _, pc, _ = sampler.sample(3, st, params, MoleculeIdxSampler(0, 1, 1).sample())
    fn = create_loss_fn(h, wf)
    loss, grads, _ = fn.loss_and_grad(1, params, (pc, None, {}))
    loss_f, flat_grads, _ = fn.loss_and_grad(1, params, (pc, None, {}), flat=True)
    prog = wf.engine(params[0]).program
    want = prog.flatten_params(grads[0])
    assert np.isfinite(float(loss)) and np.isfinite(float(loss_f)) and np.all(np.isfinite(want))
    assert bool(torch.isfinite(flat_grads[0]).all()) and float(flat_grads[0].abs().max()) > 0
    np.testing.assert_allclose(float(loss_f), float(loss), rtol=1e-12)
    np.testing.assert_allclose(flat_grads[0].cpu().numpy(), want, rtol=1e-12, atol=1e-14)


# ---------------------------------------------------------------- the gate
def check_gate(device, lib):
    """Option off: -4 from log_psi_vjp; on: it runs; off again: -4 again.  A TransPsiformer context with the option on: -4
    from the C ABI and NotImplementedError from wf.log_psi_vjp."""
    import pytest
    from deepqmc_amd.engine import DqmcError
    spec, h, tree, eng, r = psiformer_engine('LiH', 2, device, lib, option=None)
    rt = torch.as_tensor(r, device=device)
    with pytest.raises(DqmcError, match='dqmc error -4'):
        eng.log_psi_vjp(rt)
    eng.set_option('attention_reverse', 1)
    _, _, g = eng.log_psi_vjp(rt)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    eng.set_option('attention_reverse', 0)
    with pytest.raises(DqmcError, match='dqmc error -4: log_psi_vjp: no reverse pass for ATTENTION ops'):
        eng.log_psi_vjp(rt)
    with pytest.raises(DqmcError, match='dqmc error -1'):
        eng.set_option('attention_reverse', 2)
    # TransPsiformer: nuclear tokens (n_const > 0) stay refused with the option on
    tspec = dataclasses.replace(ANSATZES['transpsiformer'](h.mol.charges), **NARROW)
    wf = psiformer_wf(h, tspec, device, lib)
    params = wf.init(0)
    teng = wf.engine(params)
    assert teng.get_option('attention_reverse', 0) == 1
    with pytest.raises(DqmcError, match='dqmc error -4'):
        teng.log_psi_vjp(rt)
    with pytest.raises(DqmcError, match='dqmc error -4'):
        teng.log_psi_grad_coords(rt)
    with pytest.raises(NotImplementedError):
        wf.log_psi_vjp(params, rt)
    # the flag of the wave function: off, the engine refuses as before; on, the Psiformer differentiates
    wf_off = psiformer_wf(h, spec, device, lib, attention_reverse=False)
    with pytest.raises(DqmcError, match='dqmc error -4'):
        wf_off.log_psi_vjp(wf_off.init(0), rt)
    wf_on = psiformer_wf(h, spec, device, lib)
    _, gt = wf_on.log_psi_vjp(wf_on.init(0), rt)
    assert any(f'/{ATT}/query' in m and np.abs(leaves['w']).max() > 0 for m, leaves in gt.items())
