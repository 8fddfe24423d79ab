"""Shared pieces of the tests of TransPsiformer training (library option "nuclear_reverse", Engine(..., nuclear_reverse=True),
NeuralNetworkWaveFunction(..., nuclear_reverse=True)): the nuclear-token stream folded on the device with its backward, and
the attention backward with constant key / value rows.  The emulated tests (tests/test_nuclear_reverse_emu.py) and the GPU
tests (tests/test_gpu_nuclear_reverse.py) run the same checks."""
import copy
import dataclasses

import numpy as np
import pytest
import torch

from deepqmc_amd import checkpoint
from deepqmc_amd.engine import DqmcError, Engine
from deepqmc_amd.fit import TrainState, fit_wf
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.loss import create_loss_fn
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.optimizer import AdamOptimizer, KFACOptimizer, NaturalGradientOptimizer
from deepqmc_amd.params import NUC_EMB, NUC_HEAD, init_params
from deepqmc_amd.program import compile_program
from deepqmc_amd.sampling import (DecorrSampler, MoleculeIdxSampler, MultiElectronicStateSampler, MultiNuclearGeometrySampler,
                                  synthetic_walkers)
from deepqmc_amd.spec import ANSATZES
from deepqmc_amd.wf import NeuralNetworkWaveFunction
from optimizer_util import device_path_loop, flat, host_path_loop, moved_tree
from oracle import geom
from param_grad_util import leaf_errors, oracle_vjp
from pretrain_util import oracle_orbitals_vjp, oracle_pretrain, synthetic_dataset, upload

# (molecule, walkers, what differs from embedding_dim=32, n_determinants=2): the smallest shapes at which each piece can go wrong
CASES = {
    'LiH-1layer': ('LiH', 3, dict(n_interactions=1)),                            # constant rows and zetas only (N = 4, n_nuc = 2, hd = 8)
    'LiH-2layers': ('LiH', 3, dict(n_interactions=2)),                           # layer 0's token update feeds layer 1's K / V
    'LiH-hd9-2layers': ('LiH', 3, dict(embedding_dim=36, n_interactions=2)),     # odd head width, D not a multiple of 8
    'C4H4-2layers': ('cyclobutadiene_square', 2, dict(n_interactions=2)),        # N = 28, n_nuc = 8: two query blocks, 36 keys, 64 edges
}
ATT = 'multi_head_attention'
PER_WALKER = 'no per-walker partials'


def trans_spec(h, **kw):
    return dataclasses.replace(ANSATZES['transpsiformer'](h.mol.charges), **{**dict(embedding_dim=32, n_interactions=1, n_determinants=2), **kw})


def trans_engine(molname, B, device, lib=None, dtype=torch.float64, seed=3, nuclear_reverse=True, **spec_kw):
    """(spec, h, tree, eng, r [B, N, 3] float64 numpy): a narrow TransPsiformer context."""
    h = MolecularHamiltonian(mol=Molecule.from_name(molname))
    spec = trans_spec(h, **spec_kw)
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=seed, perturb_envelopes=0.1)
    eng = Engine(spec, h, tree, dtype=dtype, device=device, lib=lib, norm_eps=geom.F32_EPS, nuclear_reverse=nuclear_reverse)
    return spec, h, tree, eng, synthetic_walkers(h, B, seed=seed + 1)


def trans_wf(h, spec, device, lib=None, dtype=torch.float64, **kw):
    return NeuralNetworkWaveFunction(h, spec, dtype=dtype, device=device, lib=lib, norm_eps=geom.F32_EPS, **{'nuclear_reverse': True, **kw})


def training_setup_nuclear(h, spec, dtype, device, lib, n_states, n_walkers, length, seed):
    """optimizer_util.training_setup with a wave function made with nuclear_reverse=True."""
    wf = trans_wf(h, spec, device, lib, dtype)
    params = [wf.init(seed + s, perturb_envelopes=0.1) for s in range(n_states)]
    sampler = MultiNuclearGeometrySampler(MultiElectronicStateSampler(DecorrSampler(h, wf, length=length, tau=0.3), n_states))
    R = torch.as_tensor(h.mol.coords, dtype=dtype, device=device)[None]
    return wf, params, sampler, sampler.init(seed, params, n_walkers, R)


def grad_tree(eng, g):
    """The device route from the flat weight gradient to a tree: dqmc_grad_to_params, then unflatten_params."""
    return eng.program.unflatten_params(eng.grad_to_params(g))


def nuclear_leaves(tree):
    return [(m, k) for m, leaves in tree.items() for k in leaves
            if m.startswith(NUC_EMB) or m.startswith(NUC_HEAD) or f'/{ATT}/' in m]


# ---------------------------------------------------------------- 1. the gate
def check_gate(device, lib):
    spec, h, tree, eng, r = trans_engine('LiH', 2, device, lib, nuclear_reverse=False)
    rt = torch.as_tensor(r, device=device)
    # flag off: today's refusals, with attention_reverse on as well
    assert eng.program.grad_unsupported and eng.program.nuclear_stream is None
    eng.set_option('attention_reverse', 1)
    with pytest.raises(DqmcError, match='dqmc error -4: log_psi_vjp: no reverse pass for ATTENTION ops'):
        eng.log_psi_vjp(rt)
    with pytest.raises(NotImplementedError):
        eng.params_flat()
    wf_off = trans_wf(h, spec, device, lib, nuclear_reverse=False, attention_reverse=True)
    with pytest.raises(NotImplementedError):
        wf_off.log_psi_vjp(wf_off.init(0), rt)
    # the option needs a registered stream, and takes 0 / 1
    with pytest.raises(DqmcError, match='dqmc error -1'):
        eng.set_option('nuclear_reverse', 1)
    spec, h, tree, on, r = trans_engine('LiH', 2, device, lib)
    with pytest.raises(DqmcError, match='dqmc error -1'):
        on.set_option('nuclear_reverse', 2)
    # flag on: the VJP runs; the per-walker modes keep refusing, and say why
    assert on.program.grad_unsupported is None
    _, _, g = on.log_psi_vjp(rt)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    for call in (on.log_psi_jacobian, on.log_psi_kfac, on.log_psi_grad_coords):
        with pytest.raises(DqmcError, match=f'dqmc error -4: .*{PER_WALKER}'):
            call(rt)
    on.set_option('nuclear_reverse', 0)
    with pytest.raises(DqmcError, match='dqmc error -4: log_psi_vjp: no reverse pass for ATTENTION ops'):
        on.log_psi_vjp(rt)
    on.set_option('nuclear_reverse', 1)
    with pytest.raises(NotImplementedError, match='grad_to_params'):
        on.program.unflatten_grad(g)
    for fn in (on.program.unflatten_jacobian, lambda _: on.program.kfac_blocks()):
        with pytest.raises(NotImplementedError, match=PER_WALKER):
            fn(g[None])
    wf = trans_wf(h, spec, device, lib)
    params = wf.init(0)
    assert wf.attention_reverse and wf.engine(params).get_option('nuclear_reverse', 0) == 1
    _, gt = wf.log_psi_vjp(params, rt)
    assert all(np.abs(gt[m][k]).max() > 0 for m, k in nuclear_leaves(params))
    for call in (wf.log_psi_jacobian, wf.log_psi_kfac, wf.log_psi_grad_coords):
        with pytest.raises(NotImplementedError, match=PER_WALKER):
            call(params, rt)
    for opt in (NaturalGradientOptimizer(hamil=h, ansatz=wf), KFACOptimizer(hamil=h, ansatz=wf)):
        with pytest.raises(NotImplementedError, match=PER_WALKER):
            opt.init(0, [params], None)


# ---------------------------------------------------------------- 2. the fold
def constant_slots(prog):
    """[(first entry, length)] of the weight slots the nuclear stream writes: K and V rows of every layer, the zeta tables."""
    is_const = np.zeros(prog.weights.size, bool)
    is_const[prog.nuclear_stream['sc_col']] = True
    offs = [s[0] for s in prog.weight_slots] + [prog.weights.size]
    out = [(a, b - a) for a, b in zip(offs[:-1], offs[1:]) if is_const[a]]
    assert sum(int(is_const[a:a + n].sum()) for a, n in out) == int(is_const.sum())
    return out


def check_fold_parity(molname, device, lib, dtype, **spec_kw):
    """After a device update the constant slots equal the host fold of the same tree to 1e-10 of the slot's largest magnitude (the
    bound tests/test_program_interp.py gives the folded stream for another summation order); a float32 context's weights are
    the float32 rounding of its double copy."""
    spec, h, tree, eng, _ = trans_engine(molname, 1, device, lib, dtype=dtype, **spec_kw)
    moved = moved_tree(tree, 5)
    eng.set_params_flat(eng.params_flat(moved))
    ref = compile_program(spec, moved, h.n_up, h.n_down, h.n_nuc, R=h.mol.coords, eps=geom.F32_EPS).weights
    if dtype == torch.float64:
        w64 = eng.debug_read_weights(0).view(np.float64)
    else:
        w64 = eng.debug_read_weights(4).view(np.float64)
        w32 = eng.debug_read_weights(0).view(np.float32)
        assert np.array_equal(w32, w64.astype(np.float32))
    slots = constant_slots(eng.program)
    assert len(slots) == 2 * spec.n_interactions + 2
    worst = 0.0
    for a, n in slots:
        dev = np.abs(w64[a:a + n] - ref[a:a + n]).max() / np.abs(ref[a:a + n]).max()
        worst = max(worst, dev)
        assert dev <= 1e-10, (a, n, dev)
    m = eng.program.grad_src >= 0                 # copies of parameters: exact
    assert np.array_equal(w64[m], ref[m])
    print(f'fold parity {molname} {dtype}: worst slot deviation {worst:.2e}')
    return eng


# ---------------------------------------------------------------- 3. the VJP
def check_vjp_against_oracle(case, device, lib, tol=1e-9):
    molname, B, kw = CASES[case]
    spec, h, tree, eng, r = trans_engine(molname, B, device, lib, **kw)
    cot = np.random.default_rng(3).normal(size=B)
    _, _, g = eng.log_psi_vjp(torch.as_tensor(r, device=device), torch.as_tensor(cot, device=device))
    got = grad_tree(eng, g)
    ref = oracle_vjp(spec, h, tree, r, cot, geom.F32_EPS)
    err = leaf_errors(got, ref)
    worst = max(err, key=err.get)
    print(f'{case}: worst leaf {worst} {err[worst]:.2e}')
    assert set(err) == {f'{m}:{k}' for m, leaves in tree.items() for k in leaves}
    assert err[worst] < tol, (worst, err[worst])
    nuc = nuclear_leaves(tree)
    assert len(nuc) >= 4 + 4 * spec.n_interactions + 10
    for m, k in nuc:
        assert np.abs(got[m][k]).max() > 0 and np.abs(ref[m][k]).max() > 0, (m, k)
    return eng


# ---------------------------------------------------------------- 4. the orbital mode
def check_orbitals_and_pretraining(device, lib, tol=1e-9):
    """pretrain_util.check_orbitals_vjp / check_loss_grad with the device route to the tree, LiH with two layers."""
    spec, h, tree, eng, r = trans_engine('LiH', 6, device, lib, n_interactions=2)
    K, N, B = spec.n_determinants, h.n_up + h.n_down, r.shape[0]
    cot = np.random.default_rng(0).normal(size=(B, K, N, N))
    rt = torch.as_tensor(r, device=device)
    _, g = eng.orbitals_vjp(rt, torch.as_tensor(cot, device=device))
    ref, none = oracle_orbitals_vjp(spec, h, tree, r, cot, geom.F32_EPS)
    got = grad_tree(eng, g)
    err = leaf_errors(got, ref)
    worst = max(err, key=err.get)
    print('orbitals_vjp: worst leaf', worst, err[worst])
    assert err[worst] < tol, (worst, err[worst])
    for name in none:
        m, k = name.rsplit(':', 1)
        assert np.all(got[m][k] == 0), name
    for m, k in nuclear_leaves(tree):
        assert np.abs(got[m][k]).max() > 0, (m, k)
    ds = synthetic_dataset(h, 'cas', seed=1)
    upload(eng, ds)
    cut = B // 3
    pa, ga = eng.pretrain_loss_grad(rt[:cut], n_total=B)
    pb, gb = eng.pretrain_loss_grad(rt[cut:], n_total=B)
    p1, g1 = eng.pretrain_loss_grad(rt)
    loss_ref, ps_ref, g_ref, _ = oracle_pretrain(spec, h, tree, r, ds, 0, B, geom.F32_EPS)
    ps = torch.cat([pa, pb]).cpu().numpy()
    np.testing.assert_allclose(float(ps.sum()) / B, loss_ref, rtol=1e-12)
    np.testing.assert_allclose(float(p1.sum()) / B, loss_ref, rtol=1e-12)
    np.testing.assert_allclose(ps, ps_ref, rtol=1e-10)
    for g in (ga + gb, g1):
        err = leaf_errors(grad_tree(eng, g), g_ref)
        worst = max(err, key=err.get)
        print('pretrain_loss_grad: worst leaf', worst, err[worst])
        assert err[worst] < tol, (worst, err[worst])


# ---------------------------------------------------------------- 5. determinism and chunking
def check_chunking_and_determinism(device, lib, B=8, budget_mb=1):
    molname, _, kw = CASES['C4H4-2layers']
    spec, h, tree, eng, r = trans_engine(molname, B, device, lib, **kw)
    rt = torch.as_tensor(r, device=device)
    cot = torch.as_tensor(np.random.default_rng(1).normal(size=B), device=device)
    s0, l0, g0 = eng.log_psi_vjp(rt, cot)
    s1, l1, g1 = eng.log_psi_vjp(rt, cot)
    assert torch.equal(g0, g1) and torch.equal(l0, l1) and torch.equal(s0, s1)
    assert eng.last_chunks()['own'] == 1
    t0, t1 = eng.grad_to_params(g0), eng.grad_to_params(g0)
    assert torch.equal(t0, t1) and float(t0.abs().max()) > 0
    col = torch.as_tensor(eng.program.nuclear_stream['sc_col'].astype(np.int64), device=device)
    assert float(g0[col].abs().max()) > 0
    eng.set_option('ws_budget_mb', budget_mb)
    try:
        s2, l2, g2 = eng.log_psi_vjp(rt, cot)
        assert eng.last_chunks()['own'] > 1
        assert torch.equal(s0, s2)
        np.testing.assert_allclose(l2.cpu().numpy(), l0.cpu().numpy(), rtol=0, atol=1e-13)
        np.testing.assert_allclose(g2.cpu().numpy(), g0.cpu().numpy(), rtol=1e-12, atol=1e-14 * float(g0.abs().max()))
    finally:
        eng.set_option('ws_budget_mb', 32 << 10)


# ---------------------------------------------------------------- 6. freshness after a device step
def check_fresh_after_device_step(device, lib, dtype, n_walkers=6, tol=1e-10):
    """One Engine.adam_step, then wf_eval, local_energy and one mcmc_steps call against a fresh context compiled (host fold) from
    the tree wf.sync_params wrote.  float32: the local energy alone, with refinement forced on, so that it is the float64 twin's."""
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = trans_spec(h, n_interactions=2)
    wf = trans_wf(h, spec, device, lib, dtype)
    params = wf.init(3, perturb_envelopes=0.1)
    eng = wf.engine(params)
    r = torch.as_tensor(synthetic_walkers(h, n_walkers, seed=7), dtype=dtype, device=device)
    if dtype == torch.float32:
        eng.set_option('refine', 2)
        eng.local_energy(r)                       # (the twin exists before the step: it is stepped with the context)
    theta = eng.params_flat()
    start = theta.clone()
    g = torch.as_tensor(np.random.default_rng(2).normal(size=theta.numel()), device=device)
    eng.adam_step(theta, torch.zeros_like(theta), torch.zeros_like(theta), g, lr=1e-2)
    assert wf.params_stale(params)
    wf.sync_params(params)
    assert np.array_equal(eng.program.flatten_params(params), theta.cpu().numpy()) and float((theta - start).abs().min()) > 0
    fresh = Engine(spec, h, params, dtype=dtype, device=device, lib=lib, norm_eps=geom.F32_EPS)
    assert fresh.program.nuclear_stream is None
    if dtype == torch.float32:
        fresh.set_option('refine', 2)
    (ea, _), (eb, _) = eng.local_energy(r), fresh.local_energy(r)
    assert bool(torch.isfinite(ea).all())
    np.testing.assert_allclose(ea.cpu().double().numpy(), eb.cpu().double().numpy(), rtol=tol, atol=tol)
    if dtype == torch.float32:
        assert eng.debug_read_weights(3) is not None      # (the twin served the call)
        return
    (sa, la), (sb, lb) = eng.wf_eval(r), fresh.wf_eval(r)
    assert torch.equal(sa, sb)
    np.testing.assert_allclose(la.cpu().numpy(), lb.cpu().numpy(), rtol=tol, atol=tol)
    noise = torch.as_tensor(np.random.default_rng(4).normal(size=(2, n_walkers, h.n_up + h.n_down, 3)), dtype=dtype, device=device)
    unif = torch.as_tensor(np.random.default_rng(5).uniform(size=(2, n_walkers)), dtype=dtype, device=device)
    out = []
    for e, s, l in ((eng, sa, la), (fresh, sb, lb)):
        st = {'r': r.clone(), 'log': l.clone(), 'sign': s.clone(), 'age': torch.zeros(n_walkers, dtype=torch.int32, device=device),
              'tau': torch.full((1,), 0.3, dtype=dtype, device=device)}
        _, acc = e.mcmc_steps(st, 2, noise=noise, unif=unif, return_accept=True)
        out.append((st, acc))
    assert torch.equal(out[0][1], out[1][1])
    assert torch.equal(out[0][0]['r'], out[1][0]['r'])


# ---------------------------------------------------------------- 7. training parity
def check_adam_fit_parity(device, lib, n_walkers=8, steps=3, lr=1e-3, seed=11, rtol=1e-10):
    """fit_wf + AdamOptimizer (device fold) against optimizer_util.host_path_loop (tree gradients, recompile with the host fold)."""
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = trans_spec(h, embedding_dim=16, n_determinants=1)
    wf_h, params_h, sampler_h, st_h = training_setup_nuclear(h, spec, torch.float64, device, lib, 1, n_walkers, 3, seed)
    losses_h = host_path_loop(seed, h, wf_h, params_h, sampler_h, st_h, steps, lr)
    wf_d, params_d, sampler_d, st_d = training_setup_nuclear(h, spec, torch.float64, device, lib, 1, n_walkers, 3, seed)
    start = copy.deepcopy(params_d)
    losses_d, state = device_path_loop(seed, h, wf_d, params_d, sampler_d, st_d, steps, lr)
    print('host-path losses  ', losses_h)
    print('device-path losses', losses_d)
    assert all(np.isfinite(losses_h)) and all(np.isfinite(losses_d))
    dev = max(abs(a - b) / abs(a) for a, b in zip(losses_h, losses_d))
    assert dev <= rtol, (losses_h, losses_d)
    prog = wf_d.engine(params_d[0]).program
    th, td, t0 = flat(params_h[0], prog), flat(params_d[0], prog), flat(start[0], prog)
    for (m, leaf), (s, _) in prog.leaf_slices().items():
        if m.startswith(NUC_EMB) or m.startswith(NUC_HEAD):
            assert np.abs(td[s] - t0[s]).max() > 0, (m, leaf)
    err = np.abs(th - td).max() / np.abs(th).max()
    print(f'final theta deviation {err:.2e} of max|theta|')
    assert err <= rtol, err


# ---------------------------------------------------------------- 8. several states
def check_two_states(device, lib, n_walkers=6, seed=11):
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = trans_spec(h, embedding_dim=16, n_determinants=1)
    wf, params, sampler, st = training_setup_nuclear(h, spec, torch.float64, device, lib, 2, n_walkers, 2, seed)
    _, pc, _ = sampler.sample(3, st, params, MoleculeIdxSampler(0, 1, 1).sample())
    fn = create_loss_fn(h, wf, alpha=4.0)
    nan = torch.full((1, 2), float('nan'), dtype=torch.float64, device=device)
    data = {'energy_ewm': nan, 'std_ewm': nan}
    loss, grads, _ = fn.loss_and_grad(1, params, (pc, None, data))
    loss_f, flat_grads, _ = fn.loss_and_grad(1, params, (pc, None, data), flat=True)
    np.testing.assert_allclose(float(loss_f), float(loss), rtol=1e-12)
    for s in range(2):
        prog = wf.engine(params[s]).program
        want = prog.flatten_params(grads[s])
        assert np.all(np.isfinite(want)) and float(flat_grads[s].abs().max()) > 0
        np.testing.assert_allclose(flat_grads[s].cpu().numpy(), want, rtol=1e-12, atol=1e-14)
    opt = AdamOptimizer(1e-3, loss_fn=fn)
    for _, state, _, stats in fit_wf(seed, h, wf, opt, MoleculeIdxSampler(0, 1, 1), sampler, range(1), TrainState(st, params, None), None):
        assert np.isfinite(float(stats['loss']))
    for s in range(2):
        assert bool(torch.isfinite(state.opt[s]['theta']).all())


# ---------------------------------------------------------------- 9. checkpoint
def check_checkpoint(device, lib, tmp_path, seed=11):
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = trans_spec(h, embedding_dim=16, n_determinants=1)
    wf, params, sampler, st = training_setup_nuclear(h, spec, torch.float64, device, lib, 1, 4, 2, seed)
    start = copy.deepcopy(params[0])
    gen = fit_wf(1, h, wf, AdamOptimizer(1e-2), MoleculeIdxSampler(0, 1, 1), sampler, range(2), TrainState(st, params, None), None)
    step, state, _, _ = next(gen)
    assert wf.params_stale(params[0])
    checkpoint.save(tmp_path / 'chk.pt', step, state, wf)
    assert not wf.params_stale(params[0])
    _, loaded = checkpoint.load(str(tmp_path / 'chk.pt'))
    prog = wf.engine(params[0]).program
    assert np.array_equal(prog.flatten_params(loaded.params[0]), state.opt[0]['theta'].cpu().numpy())
    for m, k in nuclear_leaves(start):
        assert np.abs(np.asarray(loaded.params[0][m][k]) - start[m][k]).max() > 0, (m, k)
    gen.close()
