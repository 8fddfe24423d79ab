"""Shared checks of the per-walker backward of the nuclear-token stream (library option "nuclear_coords",
Engine(..., nuclear_coords=True), NeuralNetworkWaveFunction(..., nuclear_coords=True)): d log|psi| / dr and d log|psi| / dR of
the TransPsiformer and the zero-bias force estimators that need them.  The emulated tests (tests/test_nuclear_coords_emu.py)
and the GPU tests (tests/test_gpu_nuclear_coords.py) run the same checks.  Every check sets the flag, which neither the library
nor the package knew before.

The reference is torch.autograd of the float64 oracle with respect to r and R (force_util.oracle_grad_coords); it is computed
once per (molecule, walkers, spec) and shared."""
import functools

import numpy as np
import pytest
import torch

from deepqmc_amd import force
from deepqmc_amd import observable as obs
from deepqmc_amd.engine import DqmcError, Engine, _np_ptr
from deepqmc_amd.fit import TrainState, fit_wf
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.optimizer import KFACOptimizer, NaturalGradientOptimizer, NoOptimizer
from deepqmc_amd.params import init_params
from deepqmc_amd.sampling import (DecorrSampler, MoleculeIdxSampler, MultiElectronicStateSampler, MultiNuclearGeometrySampler,
                                  synthetic_walkers)
from deepqmc_amd.types import PhysicalConfiguration
from force_util import oracle_grad_coords, restated_force, walker_errors
from nuclear_reverse_util import CASES, PER_WALKER, trans_engine, trans_spec, trans_wf
from oracle import geom

STREAM_LABEL = 'nuc_coords'      # the timing label of the batched stream backward


def coords_engine(molname, B, device, lib, dtype=torch.float64, **spec_kw):
    """trans_engine with option "nuclear_coords" on."""
    spec, h, tree, eng, r = trans_engine(molname, B, device, lib, dtype=dtype, **spec_kw)
    eng.set_option('nuclear_coords', 1)
    return spec, h, tree, eng, r


@functools.lru_cache(maxsize=None)
def _oracle(molname, B, kw):
    h = MolecularHamiltonian(mol=Molecule.from_name(molname))
    spec = trans_spec(h, **dict(kw))
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=3, perturb_envelopes=0.1)
    gr, gR = oracle_grad_coords(spec, h, tree, synthetic_walkers(h, B, seed=4), geom.F32_EPS)
    gr.setflags(write=False)
    gR.setflags(write=False)
    return gr, gR


def oracle_ref(molname, B, **spec_kw):
    """(grad_r, grad_R) of the oracle at the parameters (seed 3) and walkers (seed 4) of trans_engine; read-only."""
    return _oracle(molname, B, tuple(sorted(spec_kw.items())))


# ---------------------------------------------------------------- 1. oracle parity
def check_against_oracle(case, device, lib, tol=1e-9):
    molname, B, kw = CASES[case]
    spec, h, tree, eng, r = coords_engine(molname, B, device, lib, **kw)
    sign, log, gr, gR = eng.log_psi_grad_coords(torch.as_tensor(r, device=device))
    ref_r, ref_R = oracle_ref(molname, B, **kw)
    er, eR = walker_errors(gr.cpu().numpy(), ref_r), walker_errors(gR.cpu().numpy(), ref_R)
    print(f'{case}: grad_r {er.max():.2e}  grad_R {eR.max():.2e}')
    assert er.max() < tol and eR.max() < tol, (er, eR)


# ---------------------------------------------------------------- 2. row tails and chunks
def check_row_tails_and_chunks(case, B, device, lib, budget_mb, min_chunks, unequal=False, tol=1e-9):
    """B walkers whose token rows are no multiple of the 16-row MFMA tile: the oracle, two identical calls, and the same call
    under a workspace budget of budget_mb, which must cut it into at least min_chunks chunks -- unequal: of different lengths;
    the chunk length c is read off the engine (the smallest B' that takes two chunks is c + 1).  The smallest budget (1 MB)
    holds 9 walkers of the narrow LiH context in one chunk and one C4H4 walker (3 walkers: 1 + 1 + 1); 2 MB hold four C4H4
    walkers, so the three chunks of unequal length are asked of C4H4 with 9 walkers (4 + 4 + 1)."""
    molname, _, kw = CASES[case]
    spec, h, tree, eng, r = coords_engine(molname, B, device, lib, **kw)
    rt = torch.as_tensor(r, device=device)
    out0 = eng.log_psi_grad_coords(rt)
    out1 = eng.log_psi_grad_coords(rt)
    assert all(torch.equal(a, b) for a, b in zip(out0, out1))
    assert eng.last_chunks()['own'] == 1
    ref_r, ref_R = oracle_ref(molname, B, **kw)
    er, eR = walker_errors(out0[2].cpu().numpy(), ref_r), walker_errors(out0[3].cpu().numpy(), ref_R)
    print(f'{case} B={B}: grad_r {er.max():.2e}  grad_R {eR.max():.2e}')
    assert er.max() < tol and eR.max() < tol, (er, eR)
    eng.set_option('ws_budget_mb', budget_mb)
    try:
        out2 = eng.log_psi_grad_coords(rt)
        n = eng.last_chunks()['own']
        assert n >= min_chunks, n
        if n > 1:
            c = next(k for k in range(1, B) if -(-B // k) == n and _chunks(eng, rt[:k + 1]) == 2 and _chunks(eng, rt[:k]) == 1)
            print(f'{n} chunks of at most {c} walkers')
            assert not unequal or B % c, (n, c)
        assert torch.equal(out0[0], out2[0])
        for a, b in zip(out0[1:], out2[1:]):
            np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=1e-12, atol=1e-14 * float(a.abs().max()))
    finally:
        eng.set_option('ws_budget_mb', 32 << 10)


def _chunks(eng, rt):
    eng.log_psi_grad_coords(rt)
    return eng.last_chunks()['own']


# ---------------------------------------------------------------- 3. want_R=False
def check_want_R_false_skips_the_stream(device, lib):
    molname, B, kw = CASES['LiH-2layers']
    spec, h, tree, eng, r = coords_engine(molname, B, device, lib, **kw)
    rt = torch.as_tensor(r, device=device)
    eng.timing(True)
    try:
        eng.timing_reset()
        s1, l1, gr1, none = eng.log_psi_grad_coords(rt, want_R=False)
        rep = eng.timing_report()
        assert none is None and STREAM_LABEL not in rep and rep['attention_bwd']['launches'] == 2, rep
        eng.timing_reset()
        s0, l0, gr0, gR0 = eng.log_psi_grad_coords(rt)
        assert eng.timing_report()[STREAM_LABEL]['launches'] == 1
    finally:
        eng.timing(False)
    assert torch.equal(gr0, gr1) and torch.equal(l0, l1) and torch.equal(s0, s1)
    _, _, none, gR2 = eng.log_psi_grad_coords(rt, want_r=False)
    assert none is None and torch.equal(gR2, gR0)


# ---------------------------------------------------------------- 4. invalid walker
def check_invalid_walker(device, lib):
    """Walker 1: two same-spin electrons at one point, two equal rows in every Slater matrix; walker 3: a NaN coordinate.  A
    walker with sign 0 or a non-finite log|psi| gets all-zero rows, and the rows of the other walkers are those of the call
    without the two, bit for bit.  Walker 3 is always invalid.  Walker 1 is where the two rows come out bit-identical (the SIMT
    emulation: sign 0, log|psi| -inf); on the MI355X the sums of the two attention rows are ordered differently, the
    determinant is 1e-17 of its neighbours' instead of 0 (log|psi| -41.04, sign -1), and the walker is by the rule of
    log_psi_grad_coords a valid one: its rows are then only required not to disturb the others."""
    molname, _, kw = CASES['LiH-2layers']
    spec, h, tree, eng, r = coords_engine(molname, 4, device, lib, **kw)
    assert h.n_down >= 2
    bad = np.array(r)
    bad[1, h.n_up + 1] = bad[1, h.n_up]
    bad[3, 0, 2] = float('nan')
    sign, log, gr, gR = eng.log_psi_grad_coords(torch.as_tensor(bad, device=device))
    invalid = [b for b in (1, 3) if int(sign[b]) == 0 or not np.isfinite(float(log[b]))]
    print('invalid walkers:', invalid, 'log|psi|', log.tolist())
    assert 3 in invalid
    for b in invalid:
        assert torch.all(gr[b] == 0) and torch.all(gR[b] == 0), b
    _, _, gr0, gR0 = eng.log_psi_grad_coords(torch.as_tensor(r, device=device))
    keep = [0, 2]
    assert torch.equal(gr[keep], gr0[keep]) and torch.equal(gR[keep], gR0[keep])
    assert float(gR0[1].abs().max()) > 0 and float(gR0[3].abs().max()) > 0


# ---------------------------------------------------------------- 5. the gate
def empty_kfac_tables():
    i64 = np.int64
    tabs = {'mod': np.zeros((0, 8), i64), 'op': np.zeros((0, 4), i64), 'maps': np.zeros(0, np.int32), 'diag_pos': np.zeros(0, i64),
            'diag_row': np.zeros(0, i64), 'diag_col': np.zeros(0, i64)}
    return tabs, {'size': 0}


def check_gate(device, lib):
    refusal = f'dqmc error -4: .*{PER_WALKER}'
    # option off: today's refusal, word for word
    spec, h, tree, off, r = trans_engine('LiH', 2, device, lib)
    rt = torch.as_tensor(r, device=device)
    today = ('dqmc error -4: log_psi_grad_coords: the nuclear-token stream has no per-walker partials (all walkers share it: one '
             'nuclear backward per walker); only log_psi_vjp, orbitals_vjp and pretrain_loss_grad run with nuclear tokens')
    with pytest.raises(DqmcError) as e:
        off.log_psi_grad_coords(rt)
    assert today in str(e.value)
    assert not off.nuclear_coords
    # the option takes 0 / 1 and needs a registered stream with nuclear_reverse on
    with pytest.raises(DqmcError, match='dqmc error -1'):
        off.set_option('nuclear_coords', 2)
    off.set_option('nuclear_reverse', 0)
    with pytest.raises(DqmcError, match='dqmc error -1'):
        off.set_option('nuclear_coords', 1)
    _, _, _, bare, _ = trans_engine('LiH', 2, device, lib, nuclear_reverse=False)
    with pytest.raises(DqmcError, match='dqmc error -1'):
        bare.set_option('nuclear_coords', 1)
    # option on (the constructor's flag implies nuclear_reverse): the coordinate call runs, every other per-walker call refuses
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=3, perturb_envelopes=0.1)
    on = Engine(spec, h, tree, dtype=torch.float64, device=device, lib=lib, norm_eps=geom.F32_EPS, nuclear_coords=True)
    assert on.nuclear_coords and on.get_option('nuclear_reverse', 0) == 1 and on.get_option('nuclear_coords', 0) == 1
    _, _, gr, gR = on.log_psi_grad_coords(rt)
    assert bool(torch.isfinite(gr).all()) and bool(torch.isfinite(gR).all()) and float(gR.abs().max()) > 0
    for call in (on.log_psi_jacobian, on.log_psi_kfac):
        with pytest.raises(DqmcError, match=refusal):
            call(rt)
    with pytest.raises(DqmcError, match=f'dqmc error -4: dqmc_set_kfac_map: .*{PER_WALKER}'):
        on.set_kfac_tables(*empty_kfac_tables())
    # stale activations (a host upload of the weights, no device fold since): the call that needs them refuses as
    # dqmc_grad_to_params does, the one that does not runs
    w = np.ascontiguousarray(on.program.weights, np.float64)
    on._check(on.lib.dqmc_set_weights(on._ctx, _np_ptr(w), w.size))
    g = torch.zeros(w.size, dtype=torch.float64, device=device)
    with pytest.raises(DqmcError, match='dqmc error -1: dqmc_grad_to_params: the nuclear stream.s activations are older'):
        on.grad_to_params(g)
    with pytest.raises(DqmcError, match='dqmc error -1: log_psi_grad_coords: the nuclear stream.s activations are older'):
        on.log_psi_grad_coords(rt)
    _, _, gr2, none = on.log_psi_grad_coords(rt, want_R=False)      # (constants of the host fold: the last bits may differ)
    assert none is None
    np.testing.assert_allclose(gr2.cpu().numpy(), gr.cpu().numpy(), rtol=1e-9, atol=1e-12)
    on.set_params(tree)                      # (Engine.set_params folds on the device as well)
    assert torch.equal(on.log_psi_grad_coords(rt)[3], gR)
    # the ECP force stays refused
    from test_ecp import TABLES
    he = MolecularHamiltonian(mol=Molecule.from_name('LiH'), ecp_type='synthetic', ecp_tables=TABLES)
    se = trans_spec(he)
    ecp = Engine(se, he, init_params(se, he.n_up, he.n_down, he.n_nuc, seed=3), dtype=torch.float64, device=device, lib=lib,
                 norm_eps=geom.F32_EPS, nuclear_coords=True)
    re_ = torch.as_tensor(synthetic_walkers(he, 2, seed=4), device=device)
    with pytest.raises(DqmcError, match=f'dqmc error -4: ecp_force: .*{PER_WALKER}'):
        ecp.ecp_force('ac_zb', re_, rng=0, e_loc=torch.zeros(2, dtype=torch.float64, device=device))
    # the wave function: the flag implies the two before it
    wf = trans_wf(h, spec, device, lib, nuclear_reverse=False, nuclear_coords=True)
    assert wf.nuclear_coords and wf.nuclear_reverse and wf.attention_reverse
    params = wf.init(0)
    psi, gr, gR = wf.log_psi_grad_coords(params, rt)
    assert bool(torch.isfinite(gR).all()) and float(gR.abs().max()) > 0
    for call in (wf.log_psi_jacobian, wf.log_psi_kfac):
        with pytest.raises(NotImplementedError, match=PER_WALKER):
            call(params, rt)
    for opt in (NaturalGradientOptimizer(hamil=h, ansatz=wf), KFACOptimizer(hamil=h, ansatz=wf)):
        with pytest.raises(NotImplementedError, match=PER_WALKER):
            opt.init(0, [params], None)
    # without the flag the package refuses the coordinate calls, and names the flag that opens them
    wf_off = trans_wf(h, spec, device, lib)
    p_off = wf_off.init(0)
    for call in (lambda: wf_off.log_psi_grad_coords(p_off, rt), lambda: force.make_grad_nuc_log_wf(wf_off)(p_off, rt),
                 lambda: force.evaluate_hf_force_ac_zb(h, wf_off)(None, p_off, rt, torch.zeros(2, dtype=torch.float64, device=device), 0.0)):
        with pytest.raises(NotImplementedError, match=f'{PER_WALKER}.*nuclear_coords=True'):
            call()


# ---------------------------------------------------------------- 6. forces
def check_forces(device, lib, B=6, tol=1e-10):
    """LiH with two layers: make_grad_nuc_log_wf, AC-ZB and AC-ZVQZB against force_util.restated_force fed with the ORACLE's
    gradients, at the 1e-10 of tests/test_force_emu.py::test_estimators_match_restated_formulas; antithetic_wrapper around the
    AC-ZVQZB maker (the wrapper takes estimators of (rng, params, phys_conf): the local energies of each configuration are
    evaluated inside the wrapped callable)."""
    molname, _, kw = CASES['LiH-2layers']
    h = MolecularHamiltonian(mol=Molecule.from_name(molname))
    spec = trans_spec(h, **kw)
    wf = trans_wf(h, spec, device, lib, nuclear_coords=True)
    params = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=3, perturb_envelopes=0.1)
    r_np = synthetic_walkers(h, B, seed=4)
    r = torch.as_tensor(r_np, device=device)
    ref_r, ref_R = oracle_ref(molname, B, **kw)
    R, Z = h.mol.coords, h.mol.charges
    pc = PhysicalConfiguration(torch.as_tensor(R, device=device), r, torch.zeros(B, dtype=torch.int64, device=device))
    e_loc, _ = h.local_energy(wf)(None, params, r)
    energy = float(e_loc.mean())
    gR = force.make_grad_nuc_log_wf(wf)(params, pc)
    assert gR.dtype == torch.float64 and walker_errors(gR.cpu().numpy(), ref_R).max() < 1e-9
    zb, zvqzb = force.evaluate_hf_force_ac_zb(h, wf), force.evaluate_hf_force_ac_zvqzb(h, wf)
    got = {'ac_zb': zb(None, params, pc, e_loc, energy), 'ac_zvqzb': zvqzb(params, pc, e_loc, energy)}
    for est, f in got.items():
        assert f.dtype == torch.float64 and f.shape == (B, h.n_nuc, 3), est
        ref = restated_force(est, r, R, Z, grad_r=np.array(ref_r), grad_R=np.array(ref_R), e_loc=e_loc, energy=energy)
        err = walker_errors(f.cpu().numpy(), ref.numpy()).max()
        print(f'{est}: {err:.2e}')
        assert err < tol, (est, err)
    e_of = h.local_energy(wf)

    def zvqzb_at(rng, params_, c):
        e = e_of(rng, params_, c.r if isinstance(c, PhysicalConfiguration) else c)[0]
        return zvqzb(params_, c, e, energy)

    anti = force.antithetic_wrapper(zvqzb_at, wf, 1.0)(None, params, pc)
    pc_, mirrored = force.antithetic_sampler(pc, 1.0)
    assert not torch.equal(mirrored.r, r)
    log, log_ = wf(params, pc).log.double(), wf(params, mirrored).log.double()
    w_ = 1 / (1 + torch.exp(-2 * (log_ - log)))
    want = (1 - w_)[:, None, None] * zvqzb_at(None, params, pc) + w_[:, None, None] * zvqzb_at(None, params, mirrored)
    assert bool(torch.isfinite(anti).all()) and walker_errors(anti.cpu().numpy(), want.cpu().numpy()).max() < tol


def check_fit_with_force_monitors(device, lib, n_walkers=6, seed=11):
    """One fit_wf step (NoOptimizer, 2 states) with the AC-ZB and AC-ZVQZB monitors: finite [1, S, n_nuc, 3] means, equal to the
    makers called on the walkers of the step."""
    molname, _, kw = CASES['LiH-2layers']
    h = MolecularHamiltonian(mol=Molecule.from_name(molname))
    spec = trans_spec(h, **kw)
    wf = trans_wf(h, spec, device, lib, nuclear_coords=True)
    S = 2
    params = [wf.init(seed + s, perturb_envelopes=0.1) for s in range(S)]
    sampler = MultiNuclearGeometrySampler(MultiElectronicStateSampler(DecorrSampler(h, wf, length=2, tau=0.3), S))
    R = torch.as_tensor(h.mol.coords, dtype=torch.float64, device=device)[None]
    st = sampler.init(seed, params, n_walkers, R)
    opt = NoOptimizer(hamil=h, ansatz=wf)
    seen = {}
    orig_step = opt.step

    def step(rng, params_, opt_state, batch):
        out = orig_step(rng, params_, opt_state, batch)
        seen['pc'], seen['e_loc'] = batch[0], out[2]
        return out
    opt.step = step
    monitors = [obs.ACZBForceMonitor(True, 1), obs.ACZVQZBForceMonitor(True, 1)]
    n = 0
    for _, state, _, stats in fit_wf(seed, h, wf, opt, MoleculeIdxSampler(0, 1, 1), sampler, range(1), TrainState(st, params, None), None,
                                     observable_monitors=monitors):
        n += 1
        pc, e_loc = seen['pc'], seen['e_loc']
        for name, make, rng in (('hf_force_ac_zb', force.evaluate_hf_force_ac_zb, True), ('hf_force_ac_zvqzb', force.evaluate_hf_force_ac_zvqzb, False)):
            mean = stats[f'{name}/mean']
            assert tuple(mean.shape) == (1, S, h.n_nuc, 3) and bool(torch.isfinite(mean).all()), name
            rows = []
            for s in range(S):
                c = PhysicalConfiguration(pc.R[0], pc.r[0, s].contiguous(), None)
                e = e_loc[0, s]
                f = make(h, wf)
                rows.append(f(None, state.params[s], c, e, e.double().mean()) if rng else f(state.params[s], c, e, e.double().mean()))
            want = torch.stack(rows)[None]
            assert torch.equal(stats[f'{name}/samples'], want), name
            assert torch.equal(mean, want.mean(2)), name
    assert n == 1


# ---------------------------------------------------------------- 7. a float32 context
def f32_error_statistics(device, lib, B=256):
    """LiH with two layers, B float32-rounded walkers in a float32 and in a float64 context: (median, 90th percentile) of the
    normwise error per walker, over ALL walkers, of grad_R and of grad_r."""
    molname, _, kw = CASES['LiH-2layers']
    spec, h, tree, e32, r = coords_engine(molname, B, device, lib, dtype=torch.float32, **kw)
    _, _, _, e64, _ = coords_engine(molname, B, device, lib, **kw)
    r32 = torch.as_tensor(r.astype(np.float32), device=device)
    _, _, gr, gR = e32.log_psi_grad_coords(r32)
    _, _, gr64, gR64 = e64.log_psi_grad_coords(r32.double())
    out = {}
    for name, a, b in (('grad_R', gR, gR64), ('grad_r', gr, gr64)):
        err = walker_errors(a.cpu().numpy(), b.cpu().numpy())
        assert err.shape == (B,) and np.all(np.isfinite(err))
        out[name] = (float(np.median(err)), float(np.percentile(err, 90)))
        print(f'float32 {name}: median {out[name][0]:.3e}  90th percentile {out[name][1]:.3e}')
    return out
