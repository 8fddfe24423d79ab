"""Checks of the device-resident KFAC step (dqmc_set_kfac_map, dqmc_kfac_direction, dqmc_kfac_apply, optimizer.KFACOptimizer)
shared by the emulated CPU tests and the GPU tests."""
import numpy as np
import torch

from deepqmc_amd.fit import TrainState, fit_wf
from deepqmc_amd.loss import _kfac_directions_tree, compute_energy_loss_and_kfac, create_loss_fn, kfac_module_factors
from deepqmc_amd.optimizer import KFACOptimizer
from deepqmc_amd.pretrain import apply_updates, merge_states
from deepqmc_amd.sampling import MoleculeIdxSampler
from optimizer_util import training_setup

DAMPING = 1e-3


def synthetic_inputs(eng, B, seed):
    """A factor buffer of per-op X X^T / D D^T (X, D random with twice as many columns as rows, scaled so that the module
    factors are O(1) after the normalisation by n_v R and n_v), a random gradient, zero rest partials and B valid walkers."""
    prog = eng.program
    lay = prog.kfac_layout()
    blocks, _ = prog.kfac_blocks()
    R_of = {q: blk['R'] for blk in blocks.values() for q in blk['ops']}
    rng = np.random.default_rng(seed)
    fac = np.zeros(lay['n_factor_doubles'])
    for q, o in enumerate(lay['ops']):
        for off, d, norm in ((o['a_off'], o['d_a'], B * R_of.get(q, 1)), (o['g_off'], o['d_g'], B)):
            X = rng.normal(size=(d, 2 * d)) * np.sqrt(norm / (2 * d))
            fac[off:off + d * d] = (X @ X.T).reshape(-1)
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device=eng.device).contiguous()
    return dict(fac=t(fac), g=t(rng.normal(size=prog.n_params())), rest=torch.zeros(B, lay['n_rest'], dtype=eng.dtype, device=eng.device),
                logpsi=torch.zeros(B, dtype=eng.dtype, device=eng.device), sign=torch.ones(B, dtype=torch.int32, device=eng.device))


def factor_views(prog, fac):
    return [(fac[o['a_off']:o['a_off'] + o['d_a'] ** 2].view(o['d_a'], o['d_a']), fac[o['g_off']:o['g_off'] + o['d_g'] ** 2].view(o['d_g'], o['d_g']))
            for o in prog.kfac_layout()['ops']]


def damped_module_factors(prog, fac, n_v, damping):
    """{module: (A_d, G_d)} of the first call (no EMA), torch float64 on fac's device."""
    out = {}
    for mod, (A, G) in kfac_module_factors(prog, factor_views(prog, fac), n_v).items():
        pi = torch.sqrt((torch.trace(A) / A.shape[0]) / (torch.trace(G) / G.shape[0]))
        eye = lambda M: torch.eye(M.shape[0], dtype=M.dtype, device=M.device)
        out[mod] = (A + pi * damping ** 0.5 * eye(A), G + damping ** 0.5 / pi * eye(G))
    return out


def module_blocks(prog, vec):
    """{module: [W; b] (d_A x d_G) torch matrix} of a parameter-ordered device vector."""
    sl = prog.leaf_slices()
    out = {}
    for mod, blk in prog.kfac_blocks()[0].items():
        w = vec[sl[(mod, 'w')][0]].reshape(blk['n_in'], blk['n_out'])
        out[mod] = torch.cat([w, vec[sl[(mod, 'b')][0]][None]], 0) if blk['has_bias'] else w
    return out


def covered_shapes(prog, panel):
    """What the solve kernels meet in this program: the factor dimensions and the properties a blocked factorisation can trip over."""
    blocks, _ = prog.kfac_blocks()
    dims = sorted({d for blk in blocks.values() for d in (blk['n_in'] + int(blk['has_bias']), blk['n_out'])})
    return dict(dims=dims, one=1 in dims, off_panel=any(d % panel for d in dims if d > 1),
                two_panels_and_rest=any(d > 2 * panel and d % panel for d in dims),
                bias=any(blk['has_bias'] for blk in blocks.values()), no_bias=any(not blk['has_bias'] for blk in blocks.values()),
                multi_op=any(len(blk['ops']) > 1 for blk in blocks.values()))


def check_solve_against_kron(eng, B=6, seed=0, tol=1e-10):
    """Engine.kfac_direction on synthetic SPD factors against the dense solve of (A_d kron G_d) vec(delta) = vec(g), per module;
    the diagonal elements against g / damping (zero rest partials)."""
    prog = eng.program
    x = synthetic_inputs(eng, B, seed)
    state = eng.kfac_state()
    delta, dot = eng.kfac_direction(x['g'], x['fac'], x['rest'], x['logpsi'], x['sign'], state, True, 0.95, DAMPING)
    got, gb = module_blocks(prog, delta), module_blocks(prog, x['g'])
    worst = {}
    for mod, (Ad, Gd) in damped_module_factors(prog, x['fac'], B, DAMPING).items():
        g = gb[mod]
        ref = torch.linalg.solve(torch.kron(Ad.cpu(), Gd.cpu()), g.cpu().reshape(-1)).reshape(g.shape)
        # the reference alone has to sit inside the bound: torch's Cholesky pair against the dense LU solve
        ch = torch.cholesky_solve(g.cpu(), torch.linalg.cholesky(Ad.cpu()))
        ch = torch.cholesky_solve(ch.T.contiguous(), torch.linalg.cholesky(Gd.cpu())).T
        ref_err = float((ch - ref).abs().max() / ref.abs().max())
        err = float((got[mod].cpu() - ref).abs().max() / ref.abs().max())
        worst[mod] = (tuple(g.shape), err, ref_err)
        assert ref_err <= tol, (mod, ref_err)
        assert err <= tol, (mod, tuple(g.shape), err)
    lay = eng.kfac_state_layout()
    el = torch.as_tensor(lay['diag_elems'], device=eng.device)
    if el.numel():
        assert torch.allclose(delta[el], x['g'][el] / DAMPING, rtol=1e-14, atol=0)
    assert torch.allclose(dot, (delta * x['g']).sum()[None], rtol=1e-12, atol=0)
    return worst


def read_state(eng, state):
    """The device state as the tree path's dict {'A': {module: matrix}, 'G': ..., 'diag': vector}."""
    lay = eng.kfac_state_layout()
    out = {'A': {}, 'G': {}}
    for mod, m in lay['modules'].items():
        for key in ('A', 'G'):
            off, d = m[key]
            out[key][mod] = state[off:off + d * d].view(d, d)
    off, n = lay['diag']
    out['diag'] = state[off:off + n]
    return out


def leaf_deviation(prog, delta_flat, delta_tree):
    """Largest |flat - tree| over a leaf, relative to the leaf's largest tree entry -> (worst ratio, its leaf)."""
    got = prog.unflatten_params(delta_flat)
    worst, where = 0.0, None
    for m in delta_tree:
        for k in delta_tree[m]:
            ref = np.asarray(delta_tree[m][k])
            e = np.abs(got[m][k] - ref).max() / max(np.abs(ref).max(), 1e-300)
            if e > worst:
                worst, where = e, (m, k)
    return worst, where


def check_flat_against_tree(h, wf, trees, r, r2=None, tol=1e-10, state_rtol=1e-13):
    """compute_energy_loss_and_kfac(flat=True) against flat=False on the batch r [1, S, B, N, 3]; with r2, a second call with
    ema = 0.9 and the states of both paths."""
    _, d_tree, st_tree, state_tree = compute_energy_loss_and_kfac(None, h, wf, trees, r, damping=DAMPING)
    _, d_flat, st_flat, state_flat = compute_energy_loss_and_kfac(None, h, wf, trees, r, damping=DAMPING, flat=True)
    S = len(trees)

    def compare(d_tree, d_flat, st_tree, st_flat):
        for s in range(S):
            prog = wf.engine(trees[s]).program
            assert torch.isfinite(d_flat[s]).all()
            worst, where = leaf_deviation(prog, d_flat[s], d_tree[s])
            print(f'state {s}: worst leaf {where} {worst:.2e}')
            assert worst <= tol, (s, where, worst)
        np.testing.assert_allclose(st_flat['precon_grad_dot'].cpu().numpy(), st_tree['precon_grad_dot'].numpy(), rtol=1e-10)
    compare(d_tree, d_flat, st_tree, st_flat)
    if S > 1:       # the states' own cotangents: the directions differ between the states
        assert float((d_flat[0] - d_flat[1]).abs().max()) > 0
    if r2 is None:
        return
    _, d_tree, st_tree, state_tree = compute_energy_loss_and_kfac(None, h, wf, trees, r2, state=state_tree, damping=DAMPING, ema=0.9)
    _, d_flat, st_flat, state_flat2 = compute_energy_loss_and_kfac(None, h, wf, trees, r2, state=state_flat, damping=DAMPING, ema=0.9, flat=True)
    assert all(a is b for a, b in zip(state_flat, state_flat2))          # updated in place
    compare(d_tree, d_flat, st_tree, st_flat)
    for s in range(S):
        got = read_state(wf.engine(trees[s]), state_flat[s])
        for key in ('A', 'G'):
            for mod, ref in state_tree[s][key].items():
                np.testing.assert_allclose(got[key][mod].cpu().numpy(), ref.cpu().numpy(), rtol=state_rtol, atol=0, err_msg=f'{key} {mod}')
        np.testing.assert_allclose(got['diag'].cpu().numpy(), state_tree[s]['diag'].cpu().numpy(), rtol=state_rtol, atol=0)


# ---------------------------------------------------------------- training loop
def norm_constraint_coeff(lr, dot, norm_constraint):
    """kfac_jax's norm constraint with momentum 0."""
    if norm_constraint <= 0 or dot <= 0:
        return 1.0
    return min(1.0, float(np.sqrt(norm_constraint / (lr * lr * dot))))


def host_kfac_loop(rng, h, wf, params, sampler, smpl_state, steps, lr, norm_constraint, damping, ema, merge_keys=None, loss_kw=None,
                   first_direction_factor=1.0):
    """The KFAC training loop from the public host-path pieces: the tree direction (compute_energy_loss_and_kfac(flat=False),
    or, with a loss function, its body on the cotangents of loss_and_cotangents), the norm constraint, the host parameter
    update, wf.invalidate, sampler.update.  Returns the flat parameter vectors [step][state] after every step."""
    from deepqmc_amd.ewm import init_multi_mol_multi_state_ewm
    fn = create_loss_fn(h, wf, **loss_kw) if loss_kw is not None else None
    mis = MoleculeIdxSampler(0, 1, 1)
    S = len(params)
    dev = wf.engine(params[0]).device
    ewm, upd = init_multi_mol_multi_state_ewm((1, S), device=dev)
    sewm, _ = init_multi_mol_multi_state_ewm((1, S), device=dev)
    state, thetas = None, []
    for k in range(steps):
        seed = int(rng) * 1000003 + k
        smpl_state, pc, _ = sampler.sample(seed, smpl_state, params, mis.sample())
        if fn is None:
            _, deltas, stats, state = compute_energy_loss_and_kfac(seed, h, wf, params, pc, state, damping, ema)
        else:
            v, c, _ = fn.loss_and_cotangents(seed, params, (pc, None, {'energy_ewm': ewm.mean, 'std_ewm': sewm.mean}))
            _, deltas, stats, state = _kfac_directions_tree(wf, params, v['r'], v['Rs'], v['loss'], list(c), dict(v['stats']), state,
                                                            damping, ema)
            e64 = v['stats']['E_loc'].double()
            ewm, sewm = upd(e64.mean(-1), ewm), upd(e64.std(-1, unbiased=False), sewm)
        for s, p in enumerate(params):
            f = first_direction_factor if k == 0 else 1.0
            lr_k = lr(k) if callable(lr) else lr
            dot = float(stats['precon_grad_dot'][s]) * f
            scale = -lr_k * norm_constraint_coeff(lr_k, dot, norm_constraint) * f
            apply_updates(p, {m: {leaf: scale * np.asarray(v) for leaf, v in leaves.items()} for m, leaves in deltas[s].items()})
        merge_states(params, merge_keys)
        for p in params:
            wf.invalidate(p)
        smpl_state = sampler.update(smpl_state, params)
        thetas.append([wf.engine(p).program.flatten_params(p) for p in params])
    return thetas


def device_kfac_loop(rng, h, wf, params, sampler, smpl_state, steps, lr, norm_constraint, damping, ema, merge_keys=None, loss_kw=None):
    """fit_wf with KFACOptimizer from the same start -> (theta [step][state], the stats of every step)."""
    kw = {'loss_fn': create_loss_fn(h, wf, **loss_kw)} if loss_kw is not None else {}
    opt = KFACOptimizer(lr, norm_constraint=norm_constraint, damping=damping, ema=ema, **kw)
    thetas, all_stats = [], []
    state = TrainState(smpl_state, params, None)
    for _, state, _, stats in fit_wf(rng, h, wf, opt, MoleculeIdxSampler(0, 1, 1), sampler, range(steps), state, merge_keys):
        thetas.append([st['theta'].cpu().numpy().copy() for st in state.opt])
        all_stats.append(stats)
    return thetas, all_stats, state


def theta_deviation(a, b):
    """Largest |a - b| / max|a| over the steps and states of two trajectories."""
    return max(np.abs(x - y).max() / np.abs(x).max() for sa, sb in zip(a, b) for x, y in zip(sa, sb))


def check_kfac_fit_parity(h, spec, dtype, device, lib, n_states, n_walkers, steps, seed, lr=0.05, norm_constraint=1e-3, damping=DAMPING,
                          ema=0.95, merge_keys=None, loss_kw=None, length=3):
    """fit_wf + KFACOptimizer against host_kfac_loop.  The bound is measured on the reference side: the host loop twice, the
    second time with its step-0 direction multiplied by 1 + 1e-10 (the one-step bound of the direction tests); the device path
    may deviate from the host loop by 10 x the largest relative theta difference of those two runs."""
    run = lambda f: host_kfac_loop(seed, h, *_setup(h, spec, dtype, device, lib, n_states, n_walkers, length, seed), steps, lr,
                                   norm_constraint, damping, ema, merge_keys, loss_kw, first_direction_factor=f)
    th_a, th_b = run(1.0), run(1.0 + 1e-10)
    amp = theta_deviation(th_a, th_b)
    wf, params, sampler, st = _setup(h, spec, dtype, device, lib, n_states, n_walkers, length, seed)
    th_d, stats, state = device_kfac_loop(seed, h, wf, params, sampler, st, steps, lr, norm_constraint, damping, ema, merge_keys, loss_kw)
    dev = theta_deviation(th_a, th_d)
    moved = np.abs(th_a[-1][0] - th_a[0][0]).max() / np.abs(th_a[0][0]).max()
    print(f'reference-side deviation after {steps} steps from a 1e-10 perturbation of the first direction: {amp:.3e} '
          f'(amplification {amp / 1e-10:.2f}); bound {10 * amp:.3e}; device path against the host loop: {dev:.3e}; '
          f'theta moved by {moved:.2e} between the first and the last step')
    assert amp > 0 and moved > 0
    assert dev <= 10 * amp, (dev, amp)
    return stats, state


def _setup(h, spec, dtype, device, lib, n_states, n_walkers, length, seed):
    return training_setup(h, spec, dtype, device, lib, n_states, n_walkers, length, seed)


# ---------------------------------------------------------------- a module with two ops, through tables of the test's own
def check_two_op_module(eng, B=5, seed=4, tol=1e-10):
    """No program this library compiles today lets kfac_blocks group two LINEAR ops into one module, so the gather over a
    module's ops is exercised with tables written here: two modules of equal shape are declared ONE module with two ops (both
    ops' factors are summed into the first module's A_hat and G_hat, R = the sum of their rows per walker) and the second
    module's parameters join the diagonal set without rest columns (F = 0, delta = g / damping).  Reference: the dense
    Kronecker solve with factors summed in numpy through the ops' row / column maps."""
    tabs, layout = eng._kfac_tables()
    mod, op, maps = tabs['mod'], tabs['op'], tabs['maps']
    a, b = next((a, b) for a in range(len(mod)) for b in range(a + 1, len(mod))
                if tuple(mod[a][:3]) == tuple(mod[b][:3]) and mod[a][7] == mod[b][7] == 1 and mod[a][0] * mod[a][1] > 1
                and tuple(op[mod[a][6]][2:4]) == tuple(op[mod[b][6]][2:4]))
    oa, ob = int(mod[a][6]), int(mod[b][6])
    order = [q for q in range(len(op)) if q != ob]
    order.insert(order.index(oa) + 1, ob)
    newpos = {old: new for new, old in enumerate(order)}
    new_mod = []
    for k, m in enumerate(mod):
        if k == b:
            continue
        m = m.copy()
        m[6] = newpos[int(m[6])]
        if k == a:
            m[7], m[3] = 2, mod[a][3] + mod[b][3]
        new_mod.append(m)
    n_in, n_out, hb = (int(v) for v in mod[b][:3])
    extra = np.concatenate([np.arange(mod[b][4], mod[b][4] + n_in * n_out)] + ([np.arange(mod[b][5], mod[b][5] + n_out)] if hb else []))
    new = dict(mod=np.ascontiguousarray(np.stack(new_mod)), op=np.ascontiguousarray(op[order]), maps=maps,
               diag_pos=np.ascontiguousarray(np.concatenate([tabs['diag_pos'], extra]).astype(np.int64)),
               diag_row=np.ascontiguousarray(np.concatenate([tabs['diag_row'], np.full(extra.size, tabs['diag_row'][-1])]).astype(np.int64)),
               diag_col=tabs['diag_col'])
    off, mods = 0, {}
    for k, m in enumerate(new['mod']):
        da, dg = int(m[0] + m[2]), int(m[1])
        mods[k] = {'A': (off, da), 'G': (off + da * da, dg)}
        off += da * da + dg * dg
    eng.set_kfac_tables(new, {'modules': mods, 'diag': (off, new['diag_pos'].size), 'diag_elems': new['diag_pos'], 'size': off + new['diag_pos'].size})
    x = synthetic_inputs(eng, B, seed)
    delta, dot = eng.kfac_direction(x['g'], x['fac'], x['rest'], x['logpsi'], x['sign'], eng.kfac_state(), True, 0.95, DAMPING)
    fac, g, d = x['fac'].cpu().numpy(), x['g'].cpu().numpy(), delta.cpu().numpy()
    da, dg = int(mod[a][0] + mod[a][2]), int(mod[a][1])
    A, G = np.zeros((da, da)), np.zeros((dg, dg))
    for q in (oa, ob):
        a_off, g_off, d_a, d_g, r0, c0 = (int(v) for v in op[q])
        rows, cols = maps[r0:r0 + d_a], maps[c0:c0 + d_g]
        Al, Gl = fac[a_off:a_off + d_a * d_a].reshape(d_a, d_a), fac[g_off:g_off + d_g * d_g].reshape(d_g, d_g)
        A[np.ix_(rows[rows >= 0], rows[rows >= 0])] += Al[np.ix_(rows >= 0, rows >= 0)]
        G[np.ix_(cols[cols >= 0], cols[cols >= 0])] += Gl[np.ix_(cols >= 0, cols >= 0)]
    A, G = A / (B * int(mod[a][3] + mod[b][3])), G / B
    pi = np.sqrt((np.trace(A) / da) / (np.trace(G) / dg))
    Ad, Gd = A + pi * DAMPING ** 0.5 * np.eye(da), G + DAMPING ** 0.5 / pi * np.eye(dg)
    w0, b0 = int(mod[a][4]), int(mod[a][5])
    blk = lambda v: np.concatenate([v[w0:w0 + int(mod[a][0]) * dg].reshape(-1, dg)] + ([v[b0:b0 + dg][None]] if mod[a][2] else []), 0)
    ref = np.linalg.solve(np.kron(Ad, Gd), blk(g).reshape(-1)).reshape(da, dg)
    err = np.abs(blk(d) - ref).max() / np.abs(ref).max()
    print(f'two ops in one module, block {da} x {dg}: {err:.2e}')
    assert err <= tol, err
    np.testing.assert_allclose(d[extra], g[extra] / DAMPING, rtol=1e-14, atol=0)
    return da, dg


def check_solve_residual(eng, B=8, seed=0):
    """Engine.kfac_direction on synthetic SPD factors at dimensions where the dense Kronecker matrix is out of reach: the residual
    max|A_d delta G_d - g| / max|g| of every module, against the residual torch's own cholesky / cholesky_solve pair leaves on
    the same inputs.  Returns (largest residual of the kernels, of torch, per-module list)."""
    prog = eng.program
    x = synthetic_inputs(eng, B, seed)
    delta, _ = eng.kfac_direction(x['g'], x['fac'], x['rest'], x['logpsi'], x['sign'], eng.kfac_state(), True, 0.95, DAMPING)
    got, gb = module_blocks(prog, delta), module_blocks(prog, x['g'])
    rows = []
    for mod, (Ad, Gd) in damped_module_factors(prog, x['fac'], B, DAMPING).items():
        g = gb[mod]
        ch = torch.cholesky_solve(g, torch.linalg.cholesky(Ad))
        ch = torch.cholesky_solve(ch.T.contiguous(), torch.linalg.cholesky(Gd)).T
        res = lambda d: float((Ad @ d @ Gd - g).abs().max() / g.abs().max())
        assert torch.isfinite(got[mod]).all(), mod
        rows.append((mod.split('/~/', 2)[-1], tuple(g.shape), res(got[mod]), res(ch)))
    return max(r[2] for r in rows), max(r[3] for r in rows), rows
