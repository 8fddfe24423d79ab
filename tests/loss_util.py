"""Checks of the multi-state training loss (dqmc_psi_ratio, dqmc_clip_rows, dqmc_loss_cotangents, deepqmc_amd/loss.py
create_loss_fn, ewm.py, fit.py) shared by the emulated CPU tests and the GPU tests.

The first half is a torch-float64 restatement of the reference's formulas (loss/loss_function.py, loss/energy.py, loss/overlap.py,
loss/spin.py, loss/clip.py, ewm.py), written as the reference writes them -- tangents as functions of a `log_psi_tangent[1, S, B]`
variable -- so that the expected cotangents are torch.autograd of the tangent and never the library's closed form."""
import dataclasses
import math

import numpy as np
import torch

from deepqmc_amd.fit import TrainState, fit_wf
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.loss import compute_mean_spin, compute_psi_ratio, compute_spin_contributions, create_loss_fn
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.optimizer import AdamOptimizer
from deepqmc_amd.pretrain import adam, apply_updates, merge_states
from deepqmc_amd.sampling import MoleculeIdxSampler
from deepqmc_amd.spec import ANSATZES
from optimizer_util import flat, training_setup
from param_grad_util import leaf_errors

F64 = torch.float64
SMALL = dict(embedding_dim=32, n_interactions=1, n_determinants=2)


# ---------------------------------------------------------------- restated reference formulas
def ref_median(x):
    xs = torch.sort(x).values
    n = xs.shape[0]
    return 0.5 * (xs[(n - 1) // 2] + xs[n // 2])


def ref_median_clip_and_mask(x, clip_width, median_center, exclude_width=math.inf):
    center = ref_median(x) if median_center else x.mean()
    abs_diff = (x - center).abs()
    mad = abs_diff.mean()
    return torch.minimum(torch.maximum(x, center - clip_width * mad), center + clip_width * mad), abs_diff < exclude_width


def ref_psi_ratio_clip_and_mask(x, clip_width=10.0, exclude_width=math.inf):
    center = ref_median(x)
    deviation = (x - center).abs()
    sigma = ref_median(deviation)
    return torch.minimum(torch.maximum(x, center - clip_width * sigma), center + clip_width * sigma), (x - center).abs() < exclude_width


def ref_rows(fn, x):
    """vmap of a [B] -> ([B], [B]) function over the leading axes."""
    lead = x.shape[:-1]
    out = [fn(row) for row in x.reshape(-1, x.shape[-1])]
    return torch.stack([o[0] for o in out]).reshape(*lead, -1), torch.stack([o[1] for o in out]).reshape(*lead, -1)


def masked_mean(x, mask, dim=None):
    x = torch.where(mask, x, torch.zeros_like(x))
    return x.sum() / mask.sum() if dim is None else x.sum(dim) / mask.sum(dim)


def triu_flat(x):
    i, j = torch.triu_indices(x.shape[-1], x.shape[-1], 1)
    return x[..., i, j]


def ref_symmetrize(x):
    return torch.sign(x) * torch.sqrt(torch.clamp(x * x.transpose(-1, -2), min=0.0))


def ref_mean_overlap(psi_ratio, weight):
    non_symm = (weight[:, None, :, :] * psi_ratio).mean(-1)
    symm = ref_symmetrize(non_symm)
    return triu_flat(symm ** 2).sum(-1).mean(), symm


def ref_scale(kind, data, min_gap):
    def gap():
        e = data['energy_ewm']
        return torch.clamp(torch.nan_to_num((e[:, :, None] - e[:, None]).abs(), nan=1.0), min_gap, 5.0)

    def std():
        return torch.clamp(torch.nan_to_num(data['std_ewm'].mean(0), nan=5.0), min_gap, 5.0)[:, None]
    return {None: lambda: torch.tensor(1.0, dtype=F64), 'energy_gap': gap, 'energy_std': std,
            'max_gap_std': lambda: torch.maximum(gap(), std())}[kind]()


def ref_ordering(sort_states_by, data, S):
    if sort_states_by == 'energy':
        return torch.argsort(data['energy_ewm'], dim=-1, stable=True)
    return torch.arange(S)[None]


def ref_energy_tangent(e_clip, weight, t, mask):
    per_state_mean = (e_clip * weight).mean(-1, keepdim=True)
    return masked_mean((e_clip - per_state_mean) * t * weight, mask)


def ref_overlap_tangent(r_clip, weight, t, r_mask, scale, ordering):
    weight, t = weight[:, None, :, :], t[:, None, :, :]
    mean_ratio = (weight * r_clip).mean(-1)
    ot = (r_clip - mean_ratio[..., None]) * weight * t
    ot = masked_mean(ot, r_mask, dim=-1)
    ot = 2 * ot * mean_ratio.transpose(-1, -2)
    ot = ot * scale
    ot = torch.stack([m[o][:, o] for m, o in zip(ot, ordering)])
    return triu_flat(ot).sum(-1).mean()


def ref_spin_tangent(spin, weight, t, mask, states):
    sw, st, sm = weight[:, states], t[:, states], mask[:, states]
    mean = (spin * sw).mean(-1, keepdim=True)
    return masked_mean((spin - mean) * st * sw, sm)


def ref_spin_raising_tangent(l_clip, l_tangent, weight, t, mask, states):
    """spin.py:175-222 with ONE deliberate departure: the reference indexes the [M, n_states, B] mask of the clipped L by the state
    NUMBERS a second time (spin.py:207-209, `gradient_mask[:, state] for state in states`), which for a proper subset such as
    [1, 2] picks clamped or shifted rows; here row q of the mask belongs to states[q], like row q of L itself."""
    sw, st = weight[:, states], t[:, states]
    mean = (l_clip * sw).mean(-1, keepdim=True)
    self_adjoint = (l_clip - mean) * st
    return masked_mean(mean * sw * (2 * self_adjoint + l_tangent), mask)


def ref_loss_value(e_loc, weight, psi_ratio, spin, alpha, lam, states):
    """loss_function.py:141-189: unclipped means.  All [1, ...]; spin [1, n_states, B] or None."""
    loss = (e_loc * weight).mean()
    if e_loc.shape[1] > 1:
        loss = loss + alpha * ref_mean_overlap(psi_ratio, weight)[0]
    if spin is not None:
        loss = loss + lam * (spin * weight[:, states]).mean()
    return loss


def ref_cotangents(e_loc, weight, psi_ratio=None, spin=None, data=None, *, e_clip_kw=None, r_clip_kw=None, alpha=None, lam=None,
                   spin_kind='squared', states=None, scale_overlap_by=None, sort_states_by=None, min_gap=0.1):
    """d(loss tangent)/d(log_psi_tangent) by autograd -> (c [S, B], k [n_states, B] or None: d/d(spin_raising_tangent)).
    Inputs [S, B], [S, S, B], [n_states, B] (one molecule)."""
    e_clip_kw = e_clip_kw or dict(clip_width=5.0, median_center=True)
    r_clip_kw = r_clip_kw or {}
    S, B = e_loc.shape
    e, w = e_loc[None], weight[None]
    t = torch.zeros(1, S, B, dtype=F64, requires_grad=True)
    states = list(range(S)) if states is None else list(states)
    lt = torch.zeros(1, len(states), B, dtype=F64, requires_grad=True)
    e_clip, e_mask = ref_rows(lambda x: ref_median_clip_and_mask(x, **e_clip_kw), e)
    tangent = ref_energy_tangent(e_clip, w, t, e_mask)
    if S > 1:
        r_clip, r_mask = ref_rows(lambda x: ref_psi_ratio_clip_and_mask(x, **r_clip_kw), psi_ratio[None])
        tangent = tangent + alpha * ref_overlap_tangent(r_clip, w, t, r_mask, ref_scale(scale_overlap_by, data, min_gap),
                                                        ref_ordering(sort_states_by, data, S))
    if lam is not None:
        if spin_kind == 'squared':
            tangent = tangent + lam * ref_spin_tangent(spin[None], w, t, e_mask, states)
        else:
            l_clip, l_mask = ref_rows(lambda x: ref_median_clip_and_mask(x, **e_clip_kw), spin[None])
            tangent = tangent + lam * ref_spin_raising_tangent(l_clip, lt, w, t, l_mask, states)
    c, k = torch.autograd.grad(tangent, (t, lt), allow_unused=True)
    return c[0], (k[0] if k is not None else None)


def ref_ewm_init(window_size):
    return dict(step=0, alpha=torch.zeros(window_size, dtype=F64), buffer=torch.zeros(window_size, dtype=F64),
                mean=torch.tensor(math.nan, dtype=F64), var=torch.tensor(math.nan, dtype=F64), sqerr=torch.tensor(math.nan, dtype=F64))


def ref_ewm_update(x, state, max_alpha=0.999, decay_alpha=10.0):
    """ewm.py:72-114 for one scalar estimator."""
    alpha = state['alpha']
    buffer = torch.cat([x.reshape(1), state['buffer'][:-1]])
    if not state['step'] + 1 >= len(alpha):
        alpha = torch.cat([torch.tensor([max(1 - max_alpha, 1 / (2 + state['step'] / decay_alpha))], dtype=F64), alpha[:-1]])
    beta = torch.cat([torch.ones(1, dtype=F64), torch.cumprod(1 - alpha[:-1], 0)])
    weights = alpha * beta
    mean = (weights * buffer).sum()
    variance = weights * (buffer - mean) ** 2
    return dict(step=state['step'] + 1, alpha=alpha, buffer=buffer, mean=mean, var=variance.sum(), sqerr=(weights * variance).sum())


# ---------------------------------------------------------------- synthetic inputs of the assembly
def synthetic(S, B, seed, nan_ewm=False, n_spin=None):
    """E_loc [S, B] with outliers, non-uniform weights of mean 1, ratios [S, S, B] with outliers (diagonal: ones), spin rows and
    finite or NaN running averages whose energy order is not the identity."""
    g = torch.Generator().manual_seed(seed)
    e = -8.0 + 0.3 * torch.arange(S, dtype=F64)[:, None] + 0.2 * torch.randn(S, B, generator=g, dtype=F64)
    e[0, 1] += 30.0                                   # far out: clipped, and masked out under a finite exclude_width
    e[-1, 2] -= 5.0
    w = torch.rand(S, B, generator=g, dtype=F64) + 0.5
    w = w / w.mean(-1, keepdim=True)
    ratio = 0.3 * torch.randn(S, S, B, generator=g, dtype=F64) + 0.2
    ratio[0, S - 1, 0] += 40.0
    ratio[S - 1, 0, 3] -= 25.0
    for s in range(S):
        ratio[s, s] = 1.0
    n_spin = S if n_spin is None else n_spin
    spin = 0.75 + 0.4 * torch.randn(n_spin, B, generator=g, dtype=F64)
    spin[0, 4] += 20.0
    if nan_ewm:
        data = {'energy_ewm': torch.full((1, S), math.nan, dtype=F64), 'std_ewm': torch.full((1, S), math.nan, dtype=F64)}
    else:
        data = {'energy_ewm': torch.tensor([[-7.9, -8.3, -8.05][:S]], dtype=F64), 'std_ewm': torch.tensor([[0.4, 0.05, 2.0][:S]], dtype=F64)}
    return e, w, ratio, spin, data


def to_dev(x, device):
    if isinstance(x, dict):
        return {k: to_dev(v, device) for k, v in x.items()}
    return x.to(device).contiguous() if isinstance(x, torch.Tensor) else x


def check_cotangents(eng, S, B, scale_overlap_by, nan_ewm, sort_states_by, spin_kind, states, seed=0, exclude=True):
    """Kernel path and torch path of LossFunction.cotangents against autograd of the restated tangent: 1e-12 of the largest |c|
    of the state (float64 sums of B terms in another order: B eps ~ 6e-14 for B = 257, with margin for the S^2 rows that are
    added); two kernel calls bit-equal.  Returns the largest deviations."""
    import functools
    from deepqmc_amd.loss import median_clip_and_mask, psi_ratio_clip_and_mask
    n_spin = S if states is None else len(states)
    e, w, ratio, spin, data = synthetic(S, B, seed, nan_ewm, n_spin)
    e_kw = dict(clip_width=3.0, median_center=True, exclude_width=10.0 if exclude else math.inf)
    r_kw = dict(clip_width=6.0, exclude_width=15.0 if exclude else math.inf)
    alpha, lam = (4.0 if S > 1 else None), (1.5 if spin_kind else None)
    c_ref, k_ref = ref_cotangents(e, w, ratio, spin, data, e_clip_kw=e_kw, r_clip_kw=r_kw, alpha=alpha, lam=lam, spin_kind=spin_kind or 'squared',
                                  states=states, scale_overlap_by=scale_overlap_by, sort_states_by=sort_states_by)
    # the inputs exercise what they are meant to: masked-out samples in an energy row and a ratio row, no row fully masked
    e_mask = ref_rows(lambda x: ref_median_clip_and_mask(x, **e_kw), e)[1]
    r_mask = ref_rows(lambda x: ref_psi_ratio_clip_and_mask(x, **r_kw), ratio)[1]
    if exclude:
        assert (~e_mask).any()
        assert S == 1 or (~r_mask).any()
    assert e_mask.any(-1).all() and r_mask.any(-1).all()
    if sort_states_by == 'energy' and S > 1 and not nan_ewm:
        assert not torch.equal(ref_ordering('energy', data, S)[0], torch.arange(S))
    fn = create_loss_fn(None, None, functools.partial(median_clip_and_mask, **e_kw), functools.partial(psi_ratio_clip_and_mask, **r_kw),
                        alpha=alpha, spin_penalty=lam, spin_penalty_type=spin_kind or 'squared', spin_penalty_states=states,
                        scale_overlap_by=scale_overlap_by, sort_states_by=sort_states_by)
    assert fn.kernel_path
    dev = eng.device
    args = [to_dev(x, dev) for x in (e, w, ratio if S > 1 else None, spin if spin_kind else None, data)]
    worst = {}
    outs = {}
    for path in ('kernel', 'torch'):
        c, k = fn.cotangents(*args, path=path, engine=eng)
        outs[path] = (c, k)
        c = c.cpu()
        assert torch.isfinite(c).all()
        scale = c_ref.abs().amax(-1, keepdim=True)
        err = float(((c - c_ref).abs() / scale).max())
        print(f'S={S} B={B} {scale_overlap_by} nan_ewm={nan_ewm} sort={sort_states_by} spin={spin_kind} states={states} {path}: '
              f'max |c - c_ref| / max|c| = {err:.2e}')
        worst[path] = err
        if spin_kind == 'raising':
            kerr = float(((k.cpu() - k_ref).abs() / k_ref.abs().amax(-1, keepdim=True)).max())
            print(f'    k: {kerr:.2e}')
            worst[path] = max(err, kerr)
        else:
            assert k is None
    c2, k2 = fn.cotangents(*args, path='kernel', engine=eng)
    assert torch.equal(c2, outs['kernel'][0]) and (k2 is None or torch.equal(k2, outs['kernel'][1]))
    assert max(worst.values()) <= 1e-12, worst
    return worst


# ---------------------------------------------------------------- dqmc_clip_rows / dqmc_psi_ratio
def clip_rows_cases(B, n_rows, seed=0):
    """x [n_rows, B]: random rows, and among them a row with ties (small integers), a constant row and a descending one."""
    g = torch.Generator().manual_seed(seed + 1000 * B + n_rows)
    x = torch.randn(n_rows, B, generator=g, dtype=F64) * 2.0 - 1.0
    w = torch.rand(n_rows, B, generator=g, dtype=F64) + 0.5
    if n_rows >= 9:
        x[2] = torch.randint(-2, 3, (B,), generator=g).to(F64)
        x[4] = 3.25
        x[6] = torch.sort(x[6], descending=True).values
    else:
        x[0, : B // 2] = torch.randint(-2, 3, (B // 2,), generator=g).to(F64)        # ties inside a random row
    return x, w


def check_clip_rows(eng, B, n_rows, median_center, median_scale, exclude_width, clip_width=2.0):
    """dqmc_clip_rows against torch.sort: median centre and median-based scale bit-equal, the other numbers to 1e-12 relative
    (B eps for the longest row, B = 4097: 9e-13), masks equal."""
    x, w = clip_rows_cases(B, n_rows)
    xd, wd = x.to(eng.device), w.to(eng.device)
    xc, mask, st = (o.cpu() for o in eng.clip_rows(xd, wd, median_center=median_center, median_scale=median_scale, clip_width=clip_width,
                                                   exclude_width=exclude_width))
    xc2, mask2, st2 = (o.cpu() for o in eng.clip_rows(xd, wd, median_center=median_center, median_scale=median_scale,
                                                      clip_width=clip_width, exclude_width=exclude_width))
    assert torch.equal(xc, xc2) and torch.equal(mask, mask2) and torch.equal(st, st2)
    rel = lambda a, b: float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))
    for r in range(n_rows):
        center = ref_median(x[r]) if median_center else x[r].mean()
        if median_center:
            assert st[r, 0] == center, (r, st[r, 0], center)
        else:
            assert abs(float(st[r, 0] - center)) <= 1e-12 * max(abs(float(center)), float(x[r].abs().max()))
        # (the deviations are measured from the library's centre: equal to torch's for the median, within 1e-12 for the mean)
        dev = (x[r] - st[r, 0]).abs()
        scale = ref_median(dev) if median_scale else dev.mean()
        if median_scale:
            assert st[r, 1] == scale, (r, st[r, 1], scale)
        else:
            assert abs(float(st[r, 1] - scale)) <= 1e-12 * max(float(scale), 1e-300) or float(scale) == 0.0 == float(st[r, 1])
        lo, hi = st[r, 0] - clip_width * st[r, 1], st[r, 0] + clip_width * st[r, 1]
        ref = torch.minimum(torch.maximum(x[r], lo), hi)
        assert rel(xc[r], ref) <= 1e-12, (r, rel(xc[r], ref))
        assert torch.equal(mask[r], dev < exclude_width)
        assert abs(float(st[r, 2] - (w[r] * ref).mean())) <= 1e-12 * float((w[r] * ref).abs().mean() + 1e-300)
        assert float(st[r, 3]) == float(mask[r].sum())
    return st


def check_clip_rows_nan(eng, B=65):
    x, _ = clip_rows_cases(B, 9)
    x[3, B // 2] = math.nan
    xc, mask, st = (o.cpu() for o in eng.clip_rows(x.to(eng.device), median_center=True, median_scale=True))
    assert not torch.isfinite(xc[3]).any() and not torch.isfinite(st[3, :3]).any()
    keep = [r for r in range(9) if r != 3]
    assert torch.isfinite(xc[keep]).all() and torch.isfinite(st[keep]).all()


def torch_psi_ratio(sign, log):
    """The ratio exactly as loss.compute_psi_ratio forms it from (sign, log) [S, S, B]."""
    mean_log = log.mean(dim=(1, 2))
    shifted = log - mean_log[:, None, None]
    diag = torch.diagonal(shifted, dim1=0, dim2=1).permute(1, 0)
    sdiag = torch.diagonal(sign, dim1=0, dim2=1).permute(1, 0)
    return sign * sdiag[None] * torch.exp(shifted - diag[None])


def check_psi_ratio(eng, S, B, seed=0):
    """dqmc_psi_ratio against torch_psi_ratio, 1e-14 relative.  log|psi_i| = offset_i + noise with offsets spread over +-300, so the
    shifted and the unshifted logs differ by hundreds.  The ratio is exp of a DIFFERENCE of numbers of magnitude ~1e2, so two correct
    evaluations agree to 1e-14 only if their means agree to ~1e-16 absolute; the logs are therefore multiples of 2^-20 (their
    sums, < 2^53 x 2^-20, are exact in any order) and what is compared is the shift, the exponential and the signs -- not the
    order of a sum."""
    g = torch.Generator().manual_seed(seed + 10 * S + B)
    offset = torch.linspace(-300.0, 300.0, S).to(F64) if S > 1 else torch.tensor([300.0], dtype=F64)
    log = offset[:, None, None] + 3.0 * torch.randn(S, S, B, generator=g, dtype=F64)
    log = torch.round(log * 2 ** 20) / 2 ** 20
    sign = torch.where(torch.rand(S, S, B, generator=g) < 0.5, -1.0, 1.0).to(F64)
    ref = torch_psi_ratio(sign, log)
    assert torch.isfinite(ref).all()
    got = eng.psi_ratio(log.to(eng.device), sign.to(eng.device)).cpu()
    err = float(((got - ref).abs() / ref.abs()).max())
    print(f'psi_ratio S={S} B={B}: max relative deviation {err:.2e}')
    assert err <= 1e-14
    return err


# ---------------------------------------------------------------- end to end
def lih_batch(S, B, device, lib, small=True, seed=3):
    """S LiH / PauliNet states in float64, one sampled [1, S, B] batch and finite running averages."""
    h, spec = lih(small)
    wf, params, sampler, st = training_setup(h, spec, torch.float64, device, lib, S, B, 3, seed)
    _, pc, _ = sampler.sample(7, st, params, MoleculeIdxSampler(0, 1, 1).sample())
    data = {'energy_ewm': torch.tensor([[-7.9, -8.1]], dtype=F64, device=device), 'std_ewm': torch.tensor([[0.5, 0.3]], dtype=F64, device=device)}
    return h, spec, wf, params, pc, data


def check_end_to_end(h, wf, params, pc, data, lam, grad_tol):
    """Loss against the restated loss from the library's own E_loc, psi ratios and spin rows (1e-12); every state's gradient
    against (autograd cotangent of the restated tangent) . (log_psi_jacobian rows), leaf-relative."""
    S = len(params)
    fn = create_loss_fn(h, wf, alpha=4.0, scale_overlap_by='max_gap_std', spin_penalty=lam)
    loss, grads, (e_loc, ratio, stats) = fn.loss_and_grad(5, params, (pc, None, data))
    r = pc.r if hasattr(pc, 'r') else pc
    B = r.shape[2]
    assert tuple(e_loc.shape) == (1, S, B) and tuple(ratio.shape) == (1, S, S, B)
    ratio_t, _ = compute_psi_ratio(wf, params, pc)
    w = torch.ones(1, S, B, dtype=F64, device=ratio_t.device)
    spin = None
    if lam is not None:
        spin = compute_spin_contributions(h, wf, params, pc)
        from deepqmc_amd.physics import evaluate_spin
        rows = torch.stack([evaluate_spin(h, wf)(params[s], r[0, s].contiguous()) for s in range(S)])
        assert torch.equal(spin[0], rows)
        mean, sstats = compute_mean_spin(spin, w)
        assert torch.equal(stats['spin/mean'], sstats['spin/mean']) and tuple(stats['spin/std'].shape) == (1, S)
    ref = ref_loss_value(e_loc.double().cpu(), w.cpu(), ratio_t.cpu(), None if spin is None else spin.cpu(), 4.0, lam, list(range(S)))
    print('loss', float(loss), 'restated', float(ref))
    assert abs(float(loss) - float(ref)) <= 1e-12 * abs(float(ref))
    assert tuple(stats['overlap/pairwise/mean'].shape) == (1, S, S)
    c, _ = ref_cotangents(e_loc.double()[0].cpu(), w[0].cpu(), ratio_t[0].cpu(), None if spin is None else spin[0].cpu(),
                          {k: v.cpu() for k, v in data.items()}, alpha=4.0, lam=lam, scale_overlap_by='max_gap_std')
    _, flat_grads, _ = fn.loss_and_grad(5, params, (pc, None, data), flat=True)
    for s in range(S):
        _, Jp = wf.log_psi_jacobian(params[s], r[0, s].contiguous())
        prog = wf.engine(params[s]).program
        want = prog.unflatten_params((c[s].to(Jp.device) @ Jp.double()).cpu().numpy())
        err = leaf_errors(grads[s], want)
        worst = max(err, key=err.get)
        print(f'state {s}: worst leaf {worst} {err[worst]:.2e}')
        assert err[worst] <= grad_tol, (worst, err[worst])
        np.testing.assert_allclose(flat_grads[s].cpu().numpy(), prog.flatten_params(grads[s]), rtol=1e-12, atol=1e-14)


def swapped_walkers(r, alpha, beta):
    """P_{alpha beta} r: electrons alpha and beta of every walker r[B, N, 3] exchanged."""
    perm = list(range(r.shape[1]))
    perm[alpha], perm[beta] = beta, alpha
    return r[:, perm].contiguous()


def check_raising_gradient(h, wf, params, pc, data, grad_tol, seed=5):
    """The raising kind end to end, from pieces the loss function does not use: with rho_b,a = psi(P_a r_b) / psi(r_b) from wf_eval
    on walkers swapped here, L_b = 1 - sum_a rho_b,a and (c, k) = autograd of the restated tangent, the gradient of state s is
        (c_s + k_s sum_a rho_a) . J(r_s) - sum_a (k_s rho_a) . J(P_a r_s)
    with J the per-walker Jacobians of log|psi| (log_psi_jacobian), n_up + 1 of them: leaf-relative `grad_tol`."""
    S = len(params)
    beta = h.n_up + h.n_down - 1
    fn = create_loss_fn(h, wf, alpha=4.0, scale_overlap_by='max_gap_std', spin_penalty=1.0, spin_penalty_type='raising')
    loss, grads, (e_loc, ratio, stats) = fn.loss_and_grad(seed, params, (pc, None, data), down_idx=beta)
    r = pc.r if hasattr(pc, 'r') else pc
    B = r.shape[2]
    rho, jac = [], []
    for s in range(S):
        eng = wf.engine(params[s])
        rs = r[0, s].contiguous()
        s0, l0 = eng.wf_eval(rs)
        rows, js = [], [wf.log_psi_jacobian(params[s], rs)[1].double()]
        for a in range(h.n_up):
            ra = swapped_walkers(rs, a, beta)
            s1, l1 = eng.wf_eval(ra)
            rows.append((s0 * s1).double() * torch.exp(l1.double() - l0.double()))
            js.append(wf.log_psi_jacobian(params[s], ra)[1].double())
        rho.append(torch.stack(rows, -1))
        jac.append(js)
    rho = torch.stack(rho)                                                # [S, B, n_up]
    L = (1.0 - rho.sum(-1)).cpu()
    w = torch.ones(1, S, B, dtype=F64)
    ref = ref_loss_value(e_loc.double().cpu(), w, ratio.cpu(), L[None], 4.0, 1.0, list(range(S)))
    assert abs(float(loss) - float(ref)) <= 1e-12 * abs(float(ref)), (float(loss), float(ref))
    c, k = ref_cotangents(e_loc.double()[0].cpu(), w[0], ratio[0].cpu(), L, {kk: v.cpu() for kk, v in data.items()}, alpha=4.0, lam=1.0,
                          spin_kind='raising', scale_overlap_by='max_gap_std')
    assert float(k.abs().max()) > 0
    for s in range(S):
        dev = rho.device
        cs, ks = c[s].to(dev), k[s].to(dev)
        g = (cs + ks * rho[s].sum(-1)) @ jac[s][0]
        for a in range(h.n_up):
            g = g - (ks * rho[s][:, a]) @ jac[s][1 + a]
        want = wf.engine(params[s]).program.unflatten_params(g.cpu().numpy())
        err = leaf_errors(grads[s], want)
        worst = max(err, key=err.get)
        print(f'raising, state {s}: worst leaf {worst} {err[worst]:.2e}')
        assert err[worst] <= grad_tol, (worst, err[worst])


# ---------------------------------------------------------------- training loop
def lih(small=True):
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = ANSATZES['paulinet']()
    return h, dataclasses.replace(spec, **SMALL) if small else spec


def host_path_loop_loss(rng, h, wf, params, sampler, smpl_state, steps, lr, loss_kw):
    """The training loop of a loss function from the public host-path pieces: loss_and_grad(flat=False) trees, pretrain.adam,
    wf.invalidate, sampler.update, and the running averages through ewm.py.  Returns the loss of every step."""
    from deepqmc_amd.ewm import init_multi_mol_multi_state_ewm
    fn = create_loss_fn(h, wf, **loss_kw)
    opt = adam(lr)
    opt_state = [opt.init(p) for p in params]
    mis = MoleculeIdxSampler(0, 1, 1)
    S = len(params)
    dev = wf.engine(params[0]).device
    ewm, upd = init_multi_mol_multi_state_ewm((1, S), device=dev)
    sewm, _ = init_multi_mol_multi_state_ewm((1, S), device=dev)
    losses = []
    for k in range(steps):
        seed = int(rng) * 1000003 + k
        smpl_state, pc, _ = sampler.sample(seed, smpl_state, params, mis.sample())
        loss, grads, (e_loc, _, _) = fn.loss_and_grad(seed, params, (pc, None, {'energy_ewm': ewm.mean, 'std_ewm': sewm.mean}))
        for s, p in enumerate(params):
            u, opt_state[s] = opt.update(grads[s], opt_state[s], p)
            apply_updates(p, u)
        for p in params:
            wf.invalidate(p)
        smpl_state = sampler.update(smpl_state, params)
        e64 = e_loc.double()
        ewm, sewm = upd(e64.mean(-1), ewm), upd(e64.std(-1, unbiased=False), sewm)
        losses.append(float(loss))
    return losses


def check_fit_parity_loss(h, spec, dtype, device, lib, n_walkers, steps, lr, seed, loss_kw, rtol=1e-10, length=3):
    """fit_wf with a loss function against host_path_loop_loss from the same start (two states): every step's loss and the final
    theta at `rtol`, as optimizer_util.check_fit_parity; the shape of `ratios` and the energy/* keys."""
    S = 2
    wf_h, params_h, sampler_h, st_h = training_setup(h, spec, dtype, device, lib, S, n_walkers, length, seed)
    losses_h = host_path_loop_loss(seed, h, wf_h, params_h, sampler_h, st_h, steps, lr, loss_kw)
    wf_d, params_d, sampler_d, st_d = training_setup(h, spec, dtype, device, lib, S, n_walkers, length, seed)
    opt = AdamOptimizer(lr, loss_fn=create_loss_fn(h, wf_d, **loss_kw))
    losses_d, state = [], TrainState(st_d, params_d, None)
    gen = fit_wf(seed, h, wf_d, opt, MoleculeIdxSampler(0, 1, 1), sampler_d, range(steps), state, None)
    ratios_shapes = []
    orig_step = opt.step

    def step(*a):
        out = orig_step(*a)
        ratios_shapes.append(tuple(out[3].shape))
        return out
    opt.step = step
    for _, state, _, stats in gen:
        losses_d.append(float(stats['loss']))
        for key in ('energy/ewm', 'energy/ewm_error', 'energy/std_ewm', 'overlap/pairwise/mean'):
            assert key in stats and isinstance(stats[key], torch.Tensor), key
        assert tuple(stats['energy/ewm'].shape) == (1, S)
    assert ratios_shapes == [(1, S, S, n_walkers)] * steps
    print('host-path losses  ', losses_h)
    print('device-path losses', losses_d)
    dev_ = max(abs(a - b) / abs(a) for a, b in zip(losses_h, losses_d))
    print('largest relative loss deviation', dev_)
    assert dev_ <= rtol, (losses_h, losses_d)
    for s in range(S):
        prog = wf_d.engine(params_d[s]).program
        th, td = flat(params_h[s], prog), flat(params_d[s], prog)
        err = np.abs(th - td).max() / np.abs(th).max()
        print(f'state {s}: final theta deviation {err:.2e} of max|theta|')
        assert err <= rtol, err
    return losses_h, losses_d


def nearby_states_setup(h, spec, dtype, device, lib, n_walkers, length, seed, noise):
    """Two states with real overlap: state 0 = wf.init(seed), state 1 = the same tree with `noise` x N(0, 1) added to every leaf
    (optimizer_util.moved_tree), and a two-state sampler initialised for them."""
    from optimizer_util import moved_tree
    from oracle import geom
    from deepqmc_amd.sampling import DecorrSampler, MultiElectronicStateSampler, MultiNuclearGeometrySampler
    from deepqmc_amd.wf import NeuralNetworkWaveFunction
    wf = NeuralNetworkWaveFunction(h, spec, dtype=dtype, device=device, lib=lib, norm_eps=geom.F32_EPS)
    p0 = wf.init(seed, perturb_envelopes=0.1)
    params = [p0, moved_tree(p0, seed + 1, noise)]
    sampler = MultiNuclearGeometrySampler(MultiElectronicStateSampler(DecorrSampler(h, wf, length=length, tau=0.3), 2))
    R = torch.as_tensor(h.mol.coords, dtype=dtype, device=device)[None]
    return wf, params, sampler, sampler.init(seed, params, n_walkers, R)


def fixed_set_overlap(wf, params, r, log0=None):
    """|overlap/pairwise/mean[0, 1]| of `params` on the fixed walkers r [1, 2, n, N, 3], which follow |psi_j|^2 of the START
    parameters.  log0 [2, n] = log|psi_j| of the start on its own walkers reweights them to the present |psi_j|^2
    (w_jb ~ exp(2 (log|psi_j(r_jb)| - log0_jb)), mean 1 per state), so the estimate stays consistent while the states move.
    Returns (|overlap|, log|psi_j| on its own walkers [2, n], the effective sample size per state)."""
    from deepqmc_amd.loss import compute_mean_overlap
    own = torch.stack([wf.engine(params[s]).wf_eval(r[0, s].contiguous())[1].double() for s in range(2)])
    w = torch.ones_like(own) if log0 is None else torch.exp(2.0 * (own - log0))
    w = w / w.mean(-1, keepdim=True)
    ratio, _ = compute_psi_ratio(wf, params, r)
    _, stats = compute_mean_overlap(ratio, w[None])
    ess = w.sum(-1) ** 2 / (w * w).sum(-1)
    return abs(float(stats['overlap/pairwise/mean'][0, 0, 1])), own, ess.cpu().numpy()


TODAYS_KEYS = {'hamil/V_el', 'hamil/E_kin', 'hamil/V_loc', 'hamil/V_nl', 'hamil/lap', 'hamil/quantum_force', 'local_energy/mean',
               'local_energy/std', 'local_energy/min', 'local_energy/max', 'opt/param_norm', 'opt/grad_norm', 'opt/update_norm'}


def check_fit_without_loss_fn(h, spec, dtype, device, lib, n_walkers, steps, lr, seed):
    """loss_fn=None: today's keys (those of the sampler aside) and values; and the single-state energy-only loss function walks
    the same trajectory as the path without one (rtol 1e-10: the two assemblies sum in different orders)."""
    runs = {}
    for label, mk in (('none', lambda wf: AdamOptimizer(lr, loss_fn=None)), ('plain', lambda wf: AdamOptimizer(lr)),
                      ('loss_fn', lambda wf: AdamOptimizer(lr, loss_fn=create_loss_fn(h, wf)))):
        wf, params, sampler, st = training_setup(h, spec, dtype, device, lib, 1, n_walkers, 3, seed)
        out = []
        for _, state, _, stats in fit_wf(seed, h, wf, mk(wf), MoleculeIdxSampler(0, 1, 1), sampler, range(steps), TrainState(st, params, None), None):
            out.append(stats)
        runs[label] = (out, state.opt[0]['theta'].clone())
    for stats in runs['none'][0]:
        assert {k for k in stats if not k.startswith('sampling/')} == TODAYS_KEYS
    for a, b in zip(runs['none'][0], runs['plain'][0]):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k])), k
    assert torch.equal(runs['none'][1], runs['plain'][1])
    for a, b in zip(runs['none'][0], runs['loss_fn'][0]):
        assert set(b) - set(a) == {'loss', 'energy/ewm', 'energy/ewm_error', 'energy/std_ewm'}
        np.testing.assert_allclose(float(b['local_energy/mean']), float(a['local_energy/mean']), rtol=1e-10)
        np.testing.assert_allclose(float(b['loss']), float(a['local_energy/mean']), rtol=1e-10)
    np.testing.assert_allclose(runs['loss_fn'][1].cpu().numpy(), runs['none'][1].cpu().numpy(), rtol=1e-10, atol=1e-12)


def check_overlap_penalty_separates(h, spec, dtype, device, lib, n_train, n_eval, steps, lr, seed, noise):
    """`steps` Adam steps of fit_wf from nearby_states_setup with alpha = 4 (max_gap_std) and, as the control, with alpha = 0, both
    from the same start and with the same seeds; |overlap/pairwise/mean[0, 1]| of the start and of the two ends on ONE fixed set of
    n_eval walkers per state (equilibrated under the start, reweighted to the states they are evaluated for: fixed_set_overlap).
    Returns {'start', 4.0, 0.0: |overlap|, 'ess': {alpha: effective sample sizes [2]}}."""
    mis = MoleculeIdxSampler(0, 1, 1)
    wf, params, sampler, st = nearby_states_setup(h, spec, dtype, device, lib, n_eval, 3, seed, noise)
    for k in range(4):
        st, pc, _ = sampler.sample(100 + k, st, params, mis.sample())
    r_fix = (pc.r if hasattr(pc, 'r') else pc).clone()
    out = {'ess': {}}
    out['start'], log0, _ = fixed_set_overlap(wf, params, r_fix)
    for alpha in (4.0, 0.0):
        wf, params, sampler, st = nearby_states_setup(h, spec, dtype, device, lib, n_train, 3, seed, noise)
        opt = AdamOptimizer(lr, loss_fn=create_loss_fn(h, wf, alpha=alpha, scale_overlap_by='max_gap_std'))
        for _ in fit_wf(seed, h, wf, opt, mis, sampler, range(steps), TrainState(st, params, None), None):
            pass
        out[alpha], _, out['ess'][alpha] = fixed_set_overlap(wf, params, r_fix, log0)
    print(f"|overlap[0,1]| on {n_eval} fixed walkers per state: start {out['start']:.4f}, after {steps} steps alpha=4 {out[4.0]:.4f} "
          f"(effective samples {out['ess'][4.0].round()}), alpha=0 {out[0.0]:.4f} (effective samples {out['ess'][0.0].round()})")
    return out
