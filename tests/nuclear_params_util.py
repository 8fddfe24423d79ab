"""Shared checks of the per-walker parameter partials of the nuclear-token stream (library option "nuclear_params",
Engine(..., nuclear_params=True), NeuralNetworkWaveFunction(..., nuclear_params=True)): the parameter Jacobian of the
TransPsiformer through dqmc_jacobian_to_params, the stream's diagonal elements of the KFAC direction, and the optimisers that
need either.  The emulated tests (tests/test_nuclear_params_emu.py) and the GPU tests (tests/test_gpu_nuclear_params.py) run the
same checks.  Every check sets the flag, which neither the library nor the package knew before.

The reference of the rows is torch.autograd of the float64 oracle (param_grad_util.oracle_vjp with a unit cotangent on one
walker); it is computed once per (case, walkers) and shared."""
import functools

import numpy as np
import pytest
import torch

from deepqmc_amd.engine import DqmcError, Engine, _np_ptr
from deepqmc_amd.fit import TrainState, fit_wf
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.loss import compute_energy_loss_and_kfac, compute_energy_loss_and_natgrad
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.optimizer import KFACOptimizer, NaturalGradientOptimizer
from deepqmc_amd.params import NUC_EMB, NUC_HEAD, init_params
from deepqmc_amd.sampling import (DecorrSampler, MoleculeIdxSampler, MultiElectronicStateSampler, MultiNuclearGeometrySampler,
                                  synthetic_walkers)
from attention_reverse_util import psiformer_engine
from kfac_optimizer_util import DAMPING, damped_module_factors, module_blocks, read_state
from nuclear_coords_util import empty_kfac_tables
from nuclear_reverse_util import CASES, PER_WALKER, trans_engine, trans_spec, trans_wf
from oracle import geom
from param_grad_util import leaf_errors, oracle_vjp
from param_jacobian_util import check_natgrad, jac_engine


# (case, walkers, ws_budget_mb, chunks of log_psi_jacobian at least, of unequal lengths, chunks of jacobian_to_params at least or None).
# The first three are the cases of the coords suite.  There 2 MB cut the 9 C4H4 walkers of the coordinate mode into 4 + 4 + 1; the
# Jacobian mode also reserves its split-K partials, 2 MB hold three of its walkers, and 9 walkers make 3 + 3 + 3.  That case
# keeps its three chunks, and chunks of unequal lengths are asked of 10 walkers at the same budget (3 + 3 + 3 + 1).
CHUNK_CASES = [('LiH-2layers', 9, 1, 1, False, None), ('C4H4-2layers', 3, 1, 3, False, None), ('C4H4-2layers', 9, 2, 3, False, None),
               ('C4H4-2layers', 10, 2, 4, True, None), ('C4H4-2layers', 20, 1, 3, False, 3)]


def params_engine(molname, B, device, lib, dtype=torch.float64, **spec_kw):
    """trans_engine with option "nuclear_params" on."""
    spec, h, tree, eng, r = trans_engine(molname, B, device, lib, dtype=dtype, **spec_kw)
    eng.set_option('nuclear_params', 1)
    return spec, h, tree, eng, r


def theta_rows(eng, rt):
    """(sign, logpsi, Jp [B, n_params]): log_psi_jacobian taken onto the parameters on the device."""
    s, l, J = eng.log_psi_jacobian(rt)
    return s, l, eng.jacobian_to_params(J, l, s)


def stream_leaves(prog):
    """[(module, leaf, slice)] of the leaves only the stream reads: nuclei_embedding and nuclear_gnn_head."""
    return [(m, k, sl) for (m, k), (sl, _) in prog.leaf_slices().items() if m.startswith(NUC_EMB) or m.startswith(NUC_HEAD)]


@functools.lru_cache(maxsize=None)
def _oracle_rows(molname, B, kw):
    h = MolecularHamiltonian(mol=Molecule.from_name(molname))
    spec = trans_spec(h, **dict(kw))
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=3, perturb_envelopes=0.1)
    r = synthetic_walkers(h, B, seed=4)
    return tuple(oracle_vjp(spec, h, tree, r[b:b + 1], np.ones(1), geom.F32_EPS) for b in range(B))


def oracle_rows(molname, B, **spec_kw):
    """Per walker, the oracle's tree of d log|psi(r_b)| / d params at the parameters (seed 3) and walkers (seed 4) of trans_engine."""
    return _oracle_rows(molname, B, tuple(sorted(spec_kw.items())))


# ---------------------------------------------------------------- 1. oracle rows, 2. transpose
def check_rows_against_oracle(case, device, lib, tol=1e-9):
    """Every row of jacobian_to_params(log_psi_jacobian(r)) against autograd of the oracle, leaf-relative at the 1e-9 of
    param_jacobian_util.check_rows_against_oracle, every leaf; the stream's own leaves are nonzero on both sides.  Then
    c^T J_theta against grad_to_params(log_psi_vjp(r, c)) at 1e-12 of its norm."""
    molname, B, kw = CASES[case]
    spec, h, tree, eng, r = params_engine(molname, B, device, lib, **kw)
    rt = torch.as_tensor(r, device=device)
    s, l, Jp = theta_rows(eng, rt)
    assert Jp.shape == (B, eng.program.n_params()) and Jp.dtype == torch.float64 and Jp.device.type == torch.device(device).type
    refs = oracle_rows(molname, B, **kw)
    leaves = {f'{m}:{k}' for m, lv in tree.items() for k in lv}
    own = stream_leaves(eng.program)
    assert len(own) >= 10
    for b in range(B):
        got = eng.program.unflatten_params(Jp[b])
        err = leaf_errors(got, refs[b])
        worst = max(err, key=err.get)
        print(f'{case} row {b}: worst leaf {worst} {err[worst]:.2e}')
        assert set(err) == leaves
        assert err[worst] < tol, (b, worst, err[worst])
        for m, k, _ in own:
            assert np.abs(got[m][k]).max() > 0 and np.abs(refs[b][m][k]).max() > 0, (b, m, k)
    c = torch.as_tensor(np.random.default_rng(0).normal(size=B), device=device)
    s2, l2, g = eng.log_psi_vjp(rt, c)
    assert torch.equal(s, s2) and torch.equal(l, l2)
    gt = eng.grad_to_params(g)
    dev = float((torch.matmul(c, Jp) - gt).abs().max() / gt.norm())
    print(f'{case}: transpose {dev:.2e}')
    assert dev < 1e-12, dev
    return eng, rt, Jp


# ---------------------------------------------------------------- 3. programs without a stream
def check_no_stream_agreement(device, lib, B=5):
    """jacobian_to_params against Program.unflatten_jacobian on a Psiformer and a PauliNet context.  Both sum an element's
    copies in ascending entry order in the Jacobian's precision, so the two are bit-identical."""
    _, _, _, psi, r = psiformer_engine('LiH', B, device, lib)
    _, _, _, pauli, rp = jac_engine('paulinet', 'LiH', B, device, lib)
    for name, eng, rt in (('psiformer', psi, torch.as_tensor(r, device=device)), ('paulinet', pauli, rp)):
        s, l, J = eng.log_psi_jacobian(rt)
        got, ref = eng.jacobian_to_params(J, l, s), eng.program.unflatten_jacobian(J)
        assert float(ref.abs().max()) > 0
        assert torch.equal(got, ref), (name, float((got - ref).abs().max()))


# ---------------------------------------------------------------- 4. row tails, chunks, determinism
def check_row_tails_and_chunks(case, B, device, lib, budget_mb, min_chunks, unequal=False, fold_chunks=None):
    """B walkers off the tiles: two identical calls are bit-identical; under a workspace budget of budget_mb the rows match the
    unchunked ones to rtol 1e-12; a walker with a NaN coordinate gets an all-zero row and leaves the other rows' bits alone.
    The budget must cut log_psi_jacobian into at least min_chunks chunks (unequal: of different lengths), as it cuts
    log_psi_grad_coords in the coords suite.  The stream's arenas are much smaller than the reverse pass's workspace: 1 MB, the
    smallest budget, holds those of 8 C4H4 walkers, so the cases of that suite run dqmc_jacobian_to_params in ONE chunk, and a
    case of its own (20 walkers at 1 MB) asserts fold_chunks chunks of different lengths of it."""
    molname, _, kw = CASES[case]
    spec, h, tree, eng, r = params_engine(molname, B, device, lib, **kw)
    rt = torch.as_tensor(r, device=device)
    s, l, J = eng.log_psi_jacobian(rt)
    assert eng.last_chunks()['own'] == 1
    j0, j1 = eng.jacobian_to_params(J, l, s), eng.jacobian_to_params(J, l, s)
    assert torch.equal(j0, j1) and eng.last_chunks()['own'] == 1
    own = stream_leaves(eng.program)
    assert all(float(j0[:, sl].abs().max()) > 0 for _, _, sl in own)
    eng.set_option('ws_budget_mb', budget_mb)
    try:
        s2, l2, J2 = eng.log_psi_jacobian(rt)
        n = eng.last_chunks()['own']
        assert n >= min_chunks, n
        if n > 1:
            c = _chunk_len(lambda k: eng.log_psi_jacobian(rt[:k]), eng, B, n)
            print(f'log_psi_jacobian: {n} chunks of at most {c} walkers')
            assert not unequal or B % c, (n, c)
        j2 = eng.jacobian_to_params(J2, l2, s2)
        nf = eng.last_chunks()['own']
        print(f'{case} B={B} at {budget_mb} MB: jacobian_to_params in {nf} chunks')
        if fold_chunks is not None:
            assert nf >= fold_chunks, nf
            c = _chunk_len(lambda k: eng.jacobian_to_params(J2[:k], l2[:k].contiguous(), s2[:k].contiguous()), eng, B, nf)
            print(f'jacobian_to_params: {nf} chunks of at most {c} walkers')
            assert B % c, (nf, c)
        assert torch.equal(s, s2)
        np.testing.assert_allclose(j2.cpu().numpy(), j0.cpu().numpy(), rtol=1e-12, atol=1e-14 * float(j0.abs().max()))
    finally:
        eng.set_option('ws_budget_mb', 32 << 10)
    bad = np.array(r)
    bad[1, 0, 2] = float('nan')
    sb, lb, Jb = eng.log_psi_jacobian(torch.as_tensor(bad, device=device))
    jb = eng.jacobian_to_params(Jb, lb, sb)
    assert int(sb[1]) == 0 or not np.isfinite(float(lb[1]))
    assert torch.all(jb[1] == 0)
    keep = [b for b in range(B) if b != 1]
    assert torch.equal(jb[keep], j0[keep])


def _chunk_len(call, eng, B, n):
    """The chunk length c of a call that took n chunks for B walkers: the smallest B' that takes two chunks is c + 1."""
    def chunks(k):
        call(k)
        return eng.last_chunks()['own']
    return next(k for k in range(1, B) if -(-B // k) == n and chunks(k + 1) == 2 and chunks(k) == 1)


# ---------------------------------------------------------------- 5. the stream's diagonal elements of the KFAC direction
def check_kfac_diagonal(case, device, lib, damping=DAMPING, ema=0.9):
    """log_psi_kfac then kfac_direction(first): the F of the stream's own elements in the state equal sum_b Jp[b, i]^2 / n_v
    formed in torch from the rows of jacobian_to_params, and their delta g / (F + damping), both at 1e-12, at the project's
    damping of 1e-3.  A second call with first=False on other walkers mixes the F.  Then the module blocks against the dense
    Kronecker solve with the damped factors at 1e-10 (torch's Cholesky pair inside that bound, as
    kfac_optimizer_util.check_solve_against_kron asserts), from the same factors and a state of its own.

    The damping of that last call.  The forward error of a float64 solve is about cond 2^-53, and it hits the dense LU solve, the
    Cholesky pair and the kernels alike.  These factors are real ones of 2 - 3 walkers, of rank 2 - 3 times the rows per walker:
    damped by 1e-3, cond(A_d) cond(G_d) reaches 1e7 on LiH and 1e10 on C4H4, where the REFERENCE pair is 4.2e-08 from the dense
    solve (the kernels equal the pair in the digits shown; against a solution refined with 80-bit residuals the pair and the
    kernels are at 8.5e-09, the dense solve at 3.9e-08).  A bound of 1e-10 can be asked only where the reference holds it with
    room: kron_damping takes the smallest 1e-3 x 10^k at which cond(A_d) cond(G_d) 2^-53 <= 1e-11, a tenth of the bound, for every
    module -- a rule on the reference's factors alone.  At that damping the largest eigenvalue of a damped factor is still 1e2 -
    1e5 times its damping term, so a wrong factor, map or solve moves the blocks far beyond the bound.  The errors at 1e-3 are
    printed, not asserted."""
    molname, B, kw = CASES[case]
    spec, h, tree, eng, r = params_engine(molname, B, device, lib, **kw)
    prog = eng.program
    rt = torch.as_tensor(r, device=device)
    _, _, Jp = theta_rows(eng, rt)
    lay = eng.kfac_state_layout()
    elems = torch.as_tensor(lay['diag_elems'], device=device)
    is_own = np.zeros(prog.n_params(), bool)
    for _, _, sl in stream_leaves(prog):
        is_own[sl] = True
    own = torch.as_tensor(is_own[lay['diag_elems']], device=device)
    assert int(own.sum()) == int(is_own.sum()) > 0      # every element of the stream's own leaves is a diagonal element
    cot = torch.as_tensor(np.random.default_rng(1).normal(size=B), device=device)

    def direction(rt_, state, first):
        fac = torch.empty(prog.kfac_layout()['n_factor_doubles'], dtype=torch.float64, device=device)
        sign, logpsi, g, _, rest = eng.log_psi_kfac(rt_, cot, out=(fac, None))
        gt = eng.grad_to_params(g)
        delta, dot = eng.kfac_direction(gt, fac, rest, logpsi, sign, state, first, ema, damping)
        return fac, gt, delta, dot, (rest, logpsi, sign)

    state = eng.kfac_state()
    fac, gt, delta, dot, (rest, logpsi, sign) = direction(rt, state, True)
    F = read_state(eng, state)['diag']
    F_ref = (Jp * Jp).sum(0)[elems] / B
    np.testing.assert_allclose(F[own].cpu().numpy(), F_ref[own].cpu().numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(F.cpu().numpy(), F_ref.cpu().numpy(), rtol=1e-12, atol=1e-300)      # (and the other diagonal elements)
    assert float(F[own].max()) > 0 and int((F[own] > 0).sum()) > int(own.sum()) // 2      # (rows of w that meet an absent atom type stay 0)
    np.testing.assert_allclose(delta[elems].cpu().numpy(), (gt[elems] / (F + damping)).cpu().numpy(), rtol=1e-12, atol=0)
    assert torch.allclose(dot, (delta * gt).sum()[None], rtol=1e-12, atol=0)
    # the second call: other walkers, the EMA
    r2 = torch.as_tensor(synthetic_walkers(h, B, seed=9), device=device)
    _, _, Jp2 = theta_rows(eng, r2)
    F_old = F.clone()
    _, gt2, delta2, _, _ = direction(r2, state, False)
    F2 = read_state(eng, state)['diag']
    F2_ref = ema * F_old + (1 - ema) * (Jp2 * Jp2).sum(0)[elems] / B
    np.testing.assert_allclose(F2[own].cpu().numpy(), F2_ref[own].cpu().numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(delta2[elems][own].cpu().numpy(), (gt2[elems] / (F2 + damping))[own].cpu().numpy(), rtol=1e-12, atol=0)
    assert float((F2[own] - F_old[own]).abs().max()) > 0
    # the module blocks: printed at the project's damping, asserted at the damping the reference can hold the bound at
    gb = module_blocks(prog, gt)

    def block_errors(d, delta_d):
        got, worst = module_blocks(prog, delta_d), []
        mods = damped_module_factors(prog, fac, B, d)
        assert len(mods) >= 6
        for mod, (Ad, Gd) in mods.items():
            g = gb[mod].cpu()
            ref = torch.linalg.solve(torch.kron(Ad.cpu(), Gd.cpu()), g.reshape(-1)).reshape(g.shape)
            ch = torch.cholesky_solve(g, torch.linalg.cholesky(Ad.cpu()))
            ch = torch.cholesky_solve(ch.T.contiguous(), torch.linalg.cholesky(Gd.cpu())).T
            worst.append((float((ch - ref).abs().max() / ref.abs().max()), float((got[mod].cpu() - ref).abs().max() / ref.abs().max())))
        return max(w[0] for w in worst), max(w[1] for w in worst)

    ref_err, err = block_errors(damping, delta)
    print(f'{case} damping {damping:g}: kernels {err:.2e}  torch Cholesky pair {ref_err:.2e} (not asserted)')
    d_k = kron_damping(prog, fac, B)
    delta_k, _ = eng.kfac_direction(gt, fac, rest, logpsi, sign, eng.kfac_state(), True, ema, d_k)
    ref_err, err = block_errors(d_k, delta_k)
    print(f'{case} damping {d_k:g}: kernels {err:.2e}  torch Cholesky pair {ref_err:.2e}')
    assert ref_err <= 1e-10, ('the reference pair', ref_err)
    assert err <= 1e-10, ('the kernels', err)
    np.testing.assert_allclose(delta_k[elems].cpu().numpy(), (gt[elems] / (F_old + d_k)).cpu().numpy(), rtol=1e-12, atol=0)


def kron_damping(prog, fac, n_v, bound=1e-10):
    """The smallest damping 1e-3 x 10^k at which every module's cond(A_d) cond(G_d) 2^-53 is at most a tenth of `bound`."""
    d = 1e-3
    while d < 1e9:
        cond = max(float(torch.linalg.cond(Ad.cpu()) * torch.linalg.cond(Gd.cpu())) for Ad, Gd in damped_module_factors(prog, fac, n_v, d).values())
        if cond * 2.0 ** -53 <= 0.1 * bound:
            return d
        d *= 10
    raise AssertionError('no damping conditions the factors')


# ---------------------------------------------------------------- 6. the optimisers
def _training_setup(h, spec, device, lib, n_walkers, seed):
    wf = trans_wf(h, spec, device, lib, nuclear_params=True)
    params = [wf.init(seed, perturb_envelopes=0.1)]
    sampler = MultiNuclearGeometrySampler(MultiElectronicStateSampler(DecorrSampler(h, wf, length=2, tau=0.3), 1))
    R = torch.as_tensor(h.mol.coords, dtype=torch.float64, device=device)[None]
    return wf, params, sampler, sampler.init(seed, params, n_walkers, R)


def check_optimizer_steps(make_opt, device, lib, n_walkers=8, steps=3, seed=11):
    """Three fit_wf steps on LiH with 8 walkers: finite losses and parameters, the stream's own leaves move, and two runs from the
    same start are bit-identical."""
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = trans_spec(h, embedding_dim=16, n_determinants=1)
    runs = []
    for _ in range(2):
        wf, params, sampler, st = _training_setup(h, spec, device, lib, n_walkers, seed)
        prog = wf.engine(params[0]).program
        start = prog.flatten_params(params[0])
        losses, state = [], TrainState(st, params, None)
        for _, state, _, stats in fit_wf(seed, h, wf, make_opt(), MoleculeIdxSampler(0, 1, 1), sampler, range(steps), state, None):
            losses.append(float(stats['local_energy/mean'].reshape(-1)[0]))
        runs.append((state.opt[0]['theta'].cpu().numpy().copy(), losses))
    theta, losses = runs[0]
    print('energies', losses)
    assert len(losses) == steps and np.all(np.isfinite(losses)) and np.all(np.isfinite(theta))
    for m, k, sl in stream_leaves(prog):
        assert np.abs(theta[sl] - start[sl]).max() > 0, (m, k)
    assert np.array_equal(theta, runs[1][0]) and losses == runs[1][1]


def check_natgrad_identity(device, lib, B=6):
    """param_jacobian_util.check_natgrad on the TransPsiformer wave function; the tree path of KFAC stays refused, the flat one
    runs."""
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = trans_spec(h, n_interactions=2)
    wf = trans_wf(h, spec, device, lib, nuclear_params=True)
    assert wf.nuclear_params and wf.nuclear_reverse and wf.attention_reverse and not wf.nuclear_coords
    params = [wf.init(3, perturb_envelopes=0.1)]
    r = torch.as_tensor(synthetic_walkers(h, B, seed=4), device=device)[None, None]
    _, deltas, stats = check_natgrad(wf, params, r, tol=1e-12)
    for m, k, _ in stream_leaves(wf.engine(params[0]).program):
        assert np.abs(deltas[0][m][k]).max() > 0, (m, k)
    _, d_flat, _ = compute_energy_loss_and_natgrad(None, h, wf, params, r, flat=True)
    assert bool(torch.isfinite(d_flat[0]).all())
    with pytest.raises(NotImplementedError, match=PER_WALKER):
        compute_energy_loss_and_kfac(None, h, wf, params, r)
    _, d_kfac, st, state = compute_energy_loss_and_kfac(None, h, wf, params, r, flat=True)
    assert bool(torch.isfinite(d_kfac[0]).all()) and float(st['precon_grad_dot'][0]) > 0


# ---------------------------------------------------------------- 7. the gate
def check_gate(device, lib):
    refusal = f'dqmc error -4: .*{PER_WALKER}'
    # option off: today's refusals
    spec, h, tree, off, r = trans_engine('LiH', 2, device, lib)
    rt = torch.as_tensor(r, device=device)
    today = ('the nuclear-token stream has no per-walker partials (all walkers share it: one nuclear backward per walker); only '
             'log_psi_vjp, orbitals_vjp and pretrain_loss_grad run with nuclear tokens')
    for name, call in (('log_psi_jacobian', off.log_psi_jacobian), ('log_psi_kfac', off.log_psi_kfac)):
        with pytest.raises(DqmcError) as e:
            call(rt)
        assert f'dqmc error -4: {name}: {today}' in str(e.value)
    with pytest.raises(DqmcError) as e:
        off.set_kfac_tables(*empty_kfac_tables())
    assert f'dqmc error -4: dqmc_set_kfac_map: {today}' in str(e.value)
    J = torch.zeros(2, off.program.weights.size, dtype=torch.float64, device=device)
    lp, sg = torch.zeros(2, dtype=torch.float64, device=device), torch.ones(2, dtype=torch.int32, device=device)
    with pytest.raises(DqmcError, match=f'dqmc error -4: dqmc_jacobian_to_params: .*{PER_WALKER}'):
        off.jacobian_to_params(J, lp, sg)
    assert not off.nuclear_params and not off.program.nuclear_params
    for fn in (off.program.unflatten_jacobian, lambda _: off.program.kfac_blocks()):
        with pytest.raises(NotImplementedError, match=PER_WALKER):
            fn(J)
    with pytest.raises(NotImplementedError, match=f'{PER_WALKER}.*jacobian_to_params'):
        off.program.unflatten_jacobian(J)
    # the option takes 0 / 1 and needs a registered stream with nuclear_reverse on
    with pytest.raises(DqmcError, match='dqmc error -1'):
        off.set_option('nuclear_params', 2)
    off.set_option('nuclear_reverse', 0)
    with pytest.raises(DqmcError, match='dqmc error -1'):
        off.set_option('nuclear_params', 1)
    _, _, _, bare, _ = trans_engine('LiH', 2, device, lib, nuclear_reverse=False)
    with pytest.raises(DqmcError, match='dqmc error -1'):
        bare.set_option('nuclear_params', 1)
    # option on (the constructor's flag implies nuclear_reverse)
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=3, perturb_envelopes=0.1)
    on = Engine(spec, h, tree, dtype=torch.float64, device=device, lib=lib, norm_eps=geom.F32_EPS, nuclear_params=True)
    assert on.nuclear_params and on.program.nuclear_params and not on.nuclear_coords
    assert on.get_option('nuclear_reverse', 0) == 1 and on.get_option('nuclear_params', 0) == 1
    s, l, Jp = theta_rows(on, rt)
    assert bool(torch.isfinite(Jp).all()) and float(Jp.abs().max()) > 0
    on.program.kfac_blocks()
    with pytest.raises(NotImplementedError, match='jacobian_to_params'):      # (the host transpose has no stream)
        on.program.unflatten_jacobian(J)
    with pytest.raises(DqmcError, match=f'dqmc error -4: log_psi_grad_coords: .*{PER_WALKER}'):
        on.log_psi_grad_coords(rt)
    on.set_option('nuclear_coords', 1)      # (the two flags are independent)
    assert bool(torch.isfinite(on.log_psi_grad_coords(rt)[3]).all())
    assert torch.equal(theta_rows(on, rt)[2], Jp)
    # stale activations (a host upload of the weights, no device fold since)
    w = np.ascontiguousarray(on.program.weights, np.float64)
    on._check(on.lib.dqmc_set_weights(on._ctx, _np_ptr(w), w.size))
    s1, l1, J1 = on.log_psi_jacobian(rt)      # (needs no activations of the stream)
    with pytest.raises(DqmcError, match='dqmc error -1: dqmc_jacobian_to_params: the nuclear stream.s activations are older'):
        on.jacobian_to_params(J1, l1, s1)
    on.set_params(tree)
    assert torch.equal(theta_rows(on, rt)[2], Jp)
    # the ECP force stays refused
    from test_ecp import TABLES
    he = MolecularHamiltonian(mol=Molecule.from_name('LiH'), ecp_type='synthetic', ecp_tables=TABLES)
    se = trans_spec(he)
    ecp = Engine(se, he, init_params(se, he.n_up, he.n_down, he.n_nuc, seed=3), dtype=torch.float64, device=device, lib=lib,
                 norm_eps=geom.F32_EPS, nuclear_params=True)
    re_ = torch.as_tensor(synthetic_walkers(he, 2, seed=4), device=device)
    with pytest.raises(DqmcError, match=f'dqmc error -4: ecp_force: .*{PER_WALKER}'):
        ecp.ecp_force('ac_zb', re_, rng=0, e_loc=torch.zeros(2, dtype=torch.float64, device=device))
    # the wave function: off, the refusals name the flag; on, the calls run and the coordinate call stays refused
    wf_off = trans_wf(h, spec, device, lib)
    p_off = wf_off.init(0)
    for call in (lambda: wf_off.log_psi_jacobian(p_off, rt), lambda: wf_off.log_psi_kfac(p_off, rt),
                 lambda: NaturalGradientOptimizer(hamil=h, ansatz=wf_off).init(0, [p_off], None),
                 lambda: KFACOptimizer(hamil=h, ansatz=wf_off).init(0, [p_off], None)):
        with pytest.raises(NotImplementedError, match=f'{PER_WALKER}.*nuclear_params=True'):
            call()
    wf = trans_wf(h, spec, device, lib, nuclear_reverse=False, nuclear_params=True)
    params = wf.init(0)
    psi, Jw = wf.log_psi_jacobian(params, rt)
    assert Jw.shape == (2, wf.engine(params).program.n_params()) and float(Jw.abs().max()) > 0
    _, gtree, factors, rest = wf.log_psi_kfac(params, rt)
    assert all(np.abs(gtree[m][k]).max() > 0 for m, k, _ in stream_leaves(wf.engine(params).program))
    with pytest.raises(NotImplementedError, match=PER_WALKER):
        wf.log_psi_grad_coords(params, rt)
    for opt in (NaturalGradientOptimizer(hamil=h, ansatz=wf), KFACOptimizer(hamil=h, ansatz=wf)):
        assert opt.init(0, [params], None) is not None


# ---------------------------------------------------------------- 8. a float32 context
def f32_error_statistics(device, lib, B=256):
    """LiH with two layers, B float32-rounded walkers in a float32 and in a float64 context: (median, 90th percentile) over the
    walkers of the normwise error of the row restricted to the stream's own leaves."""
    molname, _, kw = CASES['LiH-2layers']
    spec, h, tree, e32, r = params_engine(molname, B, device, lib, dtype=torch.float32, **kw)
    _, _, _, e64, _ = params_engine(molname, B, device, lib, **kw)
    r32 = torch.as_tensor(r.astype(np.float32), device=device)
    J32, J64 = theta_rows(e32, r32)[2], theta_rows(e64, r32.double())[2]
    assert J32.dtype == torch.float32
    cols = torch.as_tensor(np.concatenate([np.arange(sl.start, sl.stop) for _, _, sl in stream_leaves(e64.program)]), device=device)
    a, b = J32[:, cols].double(), J64[:, cols]
    err = ((a - b).norm(dim=1) / b.norm(dim=1)).cpu().numpy()
    assert err.shape == (B,) and np.all(np.isfinite(err))
    out = (float(np.median(err)), float(np.percentile(err, 90)))
    print(f'float32 stream rows: median {out[0]:.3e}  90th percentile {out[1]:.3e}')
    return out
