"""Batch-level callers of the hot path: `compute_local_energy` (reference
src/deepqmc/loss/energy.py:19-60), `compute_psi_ratio` (loss/overlap.py:19-99) and the training gradient of the
energy loss `compute_energy_loss_and_grad` (loss/loss_function.py:191-226) with its natural-gradient form
`compute_energy_loss_and_natgrad` and its KFAC form `compute_energy_loss_and_kfac`, with the
reference's `[molecule, electronic state, walker]` batch axes.  The molecule and state axes are
host loops over HIP contexts (one per state's parameter set; the geometry of a molecule is an argument
of the call); the walker axis is the GPU batch.  `phys_conf` is either the electron tensor r[M,S,B,N,3]
(M = 1, the Hamiltonian's geometry) or a `PhysicalConfiguration(R[M,n_nuc,3], r[M,S,B,N,3], mol_idx)` as
`MultiNuclearGeometrySampler.sample` returns it.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from .hamil import STAT_KEYS


def _unpack(phys_conf):
    """-> (r[M,S,B,N,3], [R_m or None per molecule])."""
    if hasattr(phys_conf, 'r'):
        r, R = phys_conf.r, phys_conf.R
    else:
        r, R = phys_conf, None
    if r.dim() != 5:
        raise ValueError('expected r[M, S, B, N, 3]')
    M = r.shape[0]
    if R is None:
        if M != 1:
            raise ValueError('M > 1 molecules need their geometries: pass a PhysicalConfiguration(R[M,n_nuc,3], r, mol_idx)')
        return r, [None]
    R = torch.as_tensor(R)
    while R.dim() > 3:            # the samplers tile R over the state / walker axes (electron_samplers.py:165-173)
        R = R[:, 0]
    if R.dim() == 2:
        R = R[None]
    if R.shape[0] != M:
        raise ValueError('R and r disagree on the number of molecules')
    return r, [R[m] for m in range(M)]


def compute_local_energy(rng, hamil, ansatz, params: Sequence, phys_conf_r: torch.Tensor, static_io: bool = False):
    """loss/energy.py:19-60: returns (E_loc[M,S,B], stats{key: [M,S]} = per-(molecule,state)
    means over the walkers, energy.py:59).  `params` = one parameter tree per state.  `static_io`: Engine.local_energy's
    (training loops: the same device pointers at every step, so the captured pass is replayed)."""
    from .types import PhysicalConfiguration
    r, Rs = _unpack(phys_conf_r)
    M, S = r.shape[0], r.shape[1]
    assert len(params) == S
    es, stats = [], {k: [] for k in STAT_KEYS}
    for m in range(M):
        em, sm = [], {k: [] for k in STAT_KEYS}
        for s in range(S):
            rr = r[m, s].contiguous()
            pc = rr if Rs[m] is None else PhysicalConfiguration(Rs[m], rr, None)
            e, st = ansatz.engine(params[s], Rs[m]).local_energy(pc, rng=rng, static_io=static_io)
            em.append(e)
            for k in STAT_KEYS:
                sm[k].append(st[k].mean())
        es.append(torch.stack(em))
        for k in STAT_KEYS:
            stats[k].append(torch.stack(sm[k]))
    return torch.stack(es), {k: torch.stack(v) for k, v in stats.items()}


def compute_psi_ratio(ansatz, params: Sequence, phys_conf_r: torch.Tensor):
    """loss/overlap.py:77-99 + :40-75: R[m, i, j, b] = psi_i(r_b ~ psi_j^2) / psi_j(r_b ~ psi_j^2),
    computed from log-shifted values (shift = mean log|psi| of each state i over all samples).  Returns the reference's
    tuple `(psi_ratio, stats)`; `stats` is the (empty) dict of compute_wave_function_values, overlap.py:19-50."""
    r, Rs = _unpack(phys_conf_r)
    M, S, B = r.shape[0], r.shape[1], r.shape[2]
    out = []
    for m in range(M):
        sign = torch.empty(S, S, B, dtype=torch.float64, device=r.device)
        log = torch.empty(S, S, B, dtype=torch.float64, device=r.device)
        r_all = r[m].reshape(S * B, *r.shape[3:]).contiguous()      # the samples of ALL states as one batch
        for i in range(S):                       # wave function i on the samples of every state j: ONE evaluation of
            eng = ansatz.engine(params[i], Rs[m])                     # S * B walkers per parameter set instead of S
            sg, lg = eng.wf_eval(r_all, Rs[m])                        # (the reference vmaps over both axes, overlap.py:40-49)
            sign[i], log[i] = sg.double().reshape(S, B), lg.double().reshape(S, B)
        mean_log = log.mean(dim=(1, 2))                                   # overlap.py:92-94
        shifted = log - mean_log[:, None, None]
        diag = torch.diagonal(shifted, dim1=0, dim2=1).permute(1, 0)     # [S(j), B]
        log_ratio = shifted - diag[None]
        sdiag = torch.diagonal(sign, dim1=0, dim2=1).permute(1, 0)
        out.append(sign * sdiag[None] * torch.exp(log_ratio))
    return torch.stack(out), {}


def symmetrize_overlap_with_clipped_geometric_mean(x: torch.Tensor) -> torch.Tensor:
    """loss/overlap.py:102-121: y_ij = sign(x_ij) sqrt(max(0, x_ij x_ji))."""
    return torch.sign(x) * torch.sqrt(torch.clamp(x * x.transpose(-1, -2), min=0.0))


def compute_mean_overlap(psi_ratio: torch.Tensor, weight: torch.Tensor):
    """loss/overlap.py:124-149: weighted mean of the psi ratios over the walkers of ALL ranks (the reference's
    all_device_mean; here one all-reduce of an [M,S,S] tensor), symmetrised; returns (sum_{i<j} S_ij^2 averaged
    over molecules, {'overlap/pairwise/mean': S[M,S,S]}).  psi_ratio [M,S,S,B], weight [M,S,B]."""
    import torch.distributed as dist
    s = (weight[:, None, :, :] * psi_ratio).sum(-1)
    n = torch.tensor(float(psi_ratio.shape[-1]), dtype=s.dtype, device=s.device)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        packed = torch.cat([s.reshape(-1), n.reshape(1)])          # sums and walker count in ONE all-reduce
        dist.all_reduce(packed)
        s, n = packed[:-1].reshape(s.shape), packed[-1]
    symm = symmetrize_overlap_with_clipped_geometric_mean(s / n)
    S = symm.shape[-1]
    iu = torch.triu_indices(S, S, offset=1, device=symm.device)
    loss = (symm[:, iu[0], iu[1]] ** 2).sum(-1).mean()
    return loss, {'overlap/pairwise/mean': symm}


def median_clip_and_mask(x: torch.Tensor, clip_width: float = 5.0, median_center: bool = True,
                         exclude_width: float = float('inf')):
    """loss/clip.py:73-98 for one [B] batch: clip to center +- clip_width x mean absolute deviation (center = the median,
    the mean of the two middle values for even B as jnp.median, or the mean); mask = deviation < exclude_width."""
    if median_center:
        xs = torch.sort(x).values
        n = xs.shape[0]
        center = 0.5 * (xs[(n - 1) // 2] + xs[n // 2])
    else:
        center = x.mean()
    abs_diff = (x - center).abs()
    mad = abs_diff.mean()
    return torch.clamp(x, center - clip_width * mad, center + clip_width * mad), abs_diff < exclude_width


def compute_energy_loss_and_grad(rng, hamil, ansatz, params: Sequence, phys_conf, weight=None, clip_mask_fn=median_clip_and_mask,
                                 flat: bool = False):
    """The energy part of the reference's training step for a [1, S, B] batch: loss/loss_function.py:191-226 with
    compute_mean_energy / compute_mean_energy_tangent (loss/energy.py:63-102) and clip_local_energy (loss/clip.py:31-47).
    Per state s the loss gradient is one vector-Jacobian product of log|psi| (dqmc_log_psi_vjp),
        grad_s = sum_b c_sb d log|psi_s(r_sb)| / d theta_s,   c_sb = mask_sb w_sb (clip(E)_sb - mean_b(clip(E)_s w_s)) / sum_sb mask_sb,
    the mask count taken over all states and walkers, as the reference's masked_mean over [M, S, B].
    Returns (loss = mean(E_loc w) over [1, S, B], [grad tree per state], stats: the hamiltonian statistics of
    compute_local_energy and 'E_loc' [1, S, B]).  The overlap and spin penalties are not included.
    flat=True: the gradients are float64 device vectors in parameter order (Program.grad_leaves, Engine.grad_to_params)
    instead of host trees -- what the device-resident optimisers (deepqmc_amd/optimizer.py) consume -- and nothing of the
    call waits for the host."""
    r, Rs, loss, cots, masks, stats = _energy_loss_cotangents('compute_energy_loss_and_grad', rng, hamil, ansatz, params, phys_conf,
                                                             weight, clip_mask_fn, static_io=flat)
    grads = []
    for s, cot in enumerate(cots):
        pc, eng = _state_conf(ansatz, params[s], r, Rs, s)
        if flat:
            if eng.program.grad_unsupported:
                raise NotImplementedError(f'compute_energy_loss_and_grad: unsupported for this program ({eng.program.grad_unsupported})')
            _, _, g = eng.log_psi_vjp(r[0, s].contiguous(), cot.to(eng.dtype).to(eng.device).contiguous(), Rs[0])
            grads.append(eng.grad_to_params(g))
            continue
        _, grad = ansatz.log_psi_vjp(params[s], pc, cot.to(eng.dtype).to(eng.device).contiguous())
        grads.append(grad)
    return loss, grads, stats


def _energy_loss_cotangents(name, rng, hamil, ansatz, params, phys_conf, weight, clip_mask_fn, static_io=False):
    """-> (r, Rs, loss, [cotangent c_s [B] per state], [clip mask [B] per state], stats) of the energy loss on a [1, S, B] batch."""
    r, Rs = _unpack(phys_conf)
    if r.shape[0] != 1:
        raise ValueError(f'{name}: one molecule per batch ([1, S, B])')
    e_loc, stats = compute_local_energy(rng, hamil, ansatz, params, phys_conf, static_io=static_io)
    S, B = r.shape[1], r.shape[2]
    e64 = e_loc.double()
    w = torch.ones_like(e64) if weight is None else torch.as_tensor(weight, dtype=torch.float64, device=e64.device).reshape(e64.shape)
    loss = (e64 * w).mean()
    # masked_mean over the whole [1, S, B] batch (loss/energy.py:101, utils.py:51-54): ONE mask count for all states
    clipped = [clip_mask_fn(e64[0, s]) for s in range(S)]
    n_mask = sum(mask.to(torch.float64).sum() for _, mask in clipped)
    cots = []
    for s, (e_clip, mask) in enumerate(clipped):
        mean_e = (e_clip * w[0, s]).mean()
        cots.append(mask.to(torch.float64) * w[0, s] * (e_clip - mean_e) / n_mask)
    stats = dict(stats)
    stats['E_loc'] = e_loc
    return r, Rs, loss, cots, [mask for _, mask in clipped], stats


def _state_conf(ansatz, params_s, r, Rs, s):
    from .types import PhysicalConfiguration
    rr = r[0, s].contiguous()
    pc = rr if Rs[0] is None else PhysicalConfiguration(Rs[0], rr, None)
    return pc, ansatz.engine(params_s, Rs[0])


def compute_energy_loss_and_natgrad(rng, hamil, ansatz, params: Sequence, phys_conf, damping=1e-3, weight=None,
                                    clip_mask_fn=median_clip_and_mask, flat: bool = False):
    """compute_energy_loss_and_grad preconditioned by the damped Fisher matrix of the per-walker log|psi| gradients (natural
    gradient / stochastic reconfiguration), in the MinSR form that needs only a B x B solve.  Per state s, with the per-walker
    rows O_b = d log|psi_s(r_sb)| / d theta_s (NeuralNetworkWaveFunction.log_psi_jacobian), the clip mask m_b, its count n_s over
    the state's walkers and the masked mean Obar_s = sum_b m_b O_b / n_s:
        g_s     = sum_b c_sb O_b                                 (the gradient of compute_energy_loss_and_grad, same c_sb)
        A_s     = rows sqrt(m_b / n_s) (O_b - Obar_s)
        delta_s = (A_s^T A_s + damping I)^-1 g_s = (g_s - A_s^T (A_s A_s^T + damping I)^-1 A_s g_s) / damping.
    The Gram matrix A_s A_s^T is formed with torch.matmul in the Jacobian's dtype, its Cholesky solve runs in float64, and one
    step of iterative refinement removes the cancellation of the Woodbury form at small damping.
    Returns (loss, [delta_s tree per state], stats): stats as compute_energy_loss_and_grad's, plus 'grad' = [g_s tree per state].
    flat=True: delta_s and g_s are float64 device vectors in parameter order instead of host trees.
    Single process only: the Jacobians of other ranks are not gathered."""
    if not damping > 0:
        raise ValueError('damping must be positive')
    r, Rs, loss, cots, masks, stats = _energy_loss_cotangents('compute_energy_loss_and_natgrad', rng, hamil, ansatz, params, phys_conf,
                                                             weight, clip_mask_fn, static_io=flat)
    return _natgrad_directions('compute_energy_loss_and_natgrad', ansatz, params, r, Rs, loss, cots, masks, stats, damping, flat)


def _natgrad_directions(name, ansatz, params, r, Rs, loss, cots, masks, stats, damping, flat):
    """The body of compute_energy_loss_and_natgrad for given cotangents c_s and masks m_s (the penalties of create_loss_fn
    enter through c_s only)."""
    deltas, gs = [], []
    for s, cot in enumerate(cots):
        pc, eng = _state_conf(ansatz, params[s], r, Rs, s)
        _, Jp = ansatz.log_psi_jacobian(params[s], pc)
        dt, dev = Jp.dtype, Jp.device
        c = cot.to(dt).to(dev)                                  # the cotangent log_psi_vjp receives
        g = torch.matmul(c, Jp).double()
        m = masks[s].to(torch.float64).to(dev)
        n_s = m.sum()
        obar = torch.matmul((m / n_s).to(dt), Jp)
        A = Jp.sub_(obar).mul_(torch.sqrt(m / n_s).to(dt)[:, None])          # in place: Jp is this call's own tensor
        gram = torch.matmul(A, A.transpose(0, 1)).double()
        gram.diagonal().add_(damping)
        chol = torch.linalg.cholesky(gram)
        Av = lambda v: torch.matmul(A, v.to(dt)).double()
        AtV = lambda v: torch.matmul(v.to(dt), A).double()

        def solve(v):                     # (A^T A + damping I)^-1 v, Woodbury
            z = torch.cholesky_solve(Av(v)[:, None], chol)[:, 0]
            return (v - AtV(z)) / damping

        delta = solve(g)
        delta = delta + solve(g - AtV(Av(delta)) - damping * delta)      # one step of iterative refinement
        prog = eng.program
        deltas.append(delta.contiguous() if flat else prog.unflatten_params(delta))
        gs.append(g.contiguous() if flat else prog.unflatten_params(g))
        del A, Jp
    stats['grad'] = gs
    return loss, deltas, stats



def kfac_module_factors(prog, factors, n_valid):
    """The KFAC-expand factors of every Kronecker module of kfac_blocks in haiku layout (bias as the last row of A):
    A_hat = sum_l A_l / (n_valid R_mod), G_hat = sum_l G_l / n_valid over the module's ops -> {module: (A_hat, G_hat)}."""
    blocks, _ = prog.kfac_blocks()
    out = {}
    for mod, blk in blocks.items():
        dev = factors[0][0].device
        da, dg = blk['n_in'] + int(blk['has_bias']), blk['n_out']
        A = torch.zeros(da, da, dtype=torch.float64, device=dev)
        G = torch.zeros(dg, dg, dtype=torch.float64, device=dev)
        for q, rows, cols in zip(blk['ops'], blk['rows'], blk['cols']):
            Al, Gl = factors[q]
            sr, sc = torch.as_tensor(rows >= 0, device=dev), torch.as_tensor(cols >= 0, device=dev)
            ri, ci = torch.as_tensor(rows[rows >= 0], device=dev), torch.as_tensor(cols[cols >= 0], device=dev)
            A[ri[:, None], ri[None, :]] += Al[sr][:, sr]
            G[ci[:, None], ci[None, :]] += Gl[sc][:, sc]
        out[mod] = (A / (n_valid * blk['R']), G / n_valid)
    return out


def _rest_gather(prog, elems):
    """Per source multiplicity, the rest columns that hold a copy of each parameter element of `elems` (-1: none)."""
    lay = prog.kfac_layout()
    pos = np.full(prog.weights.size, -1, np.int64)
    pos[lay['rest_index']] = np.arange(lay['n_rest'])
    tabs = []
    for idx, has in prog._jacobian_gather():
        col = np.where(has[elems], pos[idx[elems]], -1)
        if (has[elems] & (col < 0)).any():
            raise NotImplementedError('compute_energy_loss_and_kfac: a diagonal parameter is held by a linear layer of a module '
                                      'that kfac_blocks cannot factor')
        tabs.append(col)
    return tabs


def compute_energy_loss_and_kfac(rng, hamil, ansatz, params: Sequence, phys_conf, state=None, damping=1e-3, ema=0.95, weight=None,
                                 clip_mask_fn=median_clip_and_mask, flat: bool = False):
    """compute_energy_loss_and_grad preconditioned by KFAC (Kronecker-factored approximate curvature of the Fisher matrix of
    log|psi|), one dqmc_log_psi_kfac call per state.  With n_v valid walkers (sign != 0, finite log|psi|) and, per module of
    Program.kfac_blocks, R_mod the rows per walker of its ops:
        A_hat = sum_l A_l / (n_v R_mod),  G_hat = sum_l G_l / n_v        (KFAC-expand normalisation, bias = last row of A_hat)
        F <- ema F_old + (1 - ema) F_new  (the first call takes F_new; the factors live in `state`)
        pi = sqrt((tr A_hat / dim A_hat) / (tr G_hat / dim G_hat))
        delta [W; b] = (A_hat + pi sqrt(damping) I)^-1 [grad W; grad b] (G_hat + sqrt(damping) / pi I)^-1   (float64, every call)
    Every other parameter element (envelopes, cusp alphas, conf_coeff, modules kfac_blocks cannot factor) takes a diagonal
    block: with o_bi = d log|psi_b| / d theta_i (its copies' rest columns summed), F_ii = sum_b o_bi^2 / n_v (same EMA) and
    delta_i = g_i / (F_ii + damping).  This normalisation is this library's definition; it is not pinned to kfac_jax, which
    may, for instance, scale G by a constant of its predictive distribution.
    Returns (loss, [delta tree per state], stats, state): stats as compute_energy_loss_and_grad's plus 'grad' (the gradient
    trees) and 'precon_grad_dot' = [<delta_s, g_s>] (what the reference's norm constraint needs); state = one dict of factors
    per electronic state, to pass to the next call.  Single process only: the factors of other ranks are not summed.
    flat=True: the same arithmetic on the device (Engine.kfac_direction): the deltas and 'grad' are float64 device vectors in
    parameter order, 'precon_grad_dot' is a device tensor [S], and `state` is one float64 device tensor per electronic
    state (Engine.kfac_state_layout) that is updated in place; nothing of the call waits for the host."""
    if not damping > 0:
        raise ValueError('damping must be positive')
    r, Rs, loss, cots, masks, stats = _energy_loss_cotangents('compute_energy_loss_and_kfac', rng, hamil, ansatz, params, phys_conf,
                                                             weight, clip_mask_fn, static_io=flat)
    if flat:
        return _kfac_directions_flat(ansatz, params, r, Rs, loss, cots, stats, state, damping, ema)
    return _kfac_directions_tree(ansatz, params, r, Rs, loss, cots, stats, state, damping, ema)


def _kfac_directions_tree(ansatz, params, r, Rs, loss, cots, stats, state, damping, ema):
    """The body of compute_energy_loss_and_kfac(flat=False) for given cotangents c_s: host trees, torch Cholesky per module."""
    S = len(cots)
    state = list(state) if state is not None else [None] * S
    if len(state) != S:
        raise ValueError('state holds the factors of a different number of states')
    sq = damping ** 0.5
    mix = lambda old, new: new if old is None else ema * old + (1 - ema) * new
    deltas, gs, dots = [], [], []
    for s, cot in enumerate(cots):
        pc, eng = _state_conf(ansatz, params[s], r, Rs, s)
        prog = eng.program
        if prog.nuclear_stream is not None:      # (the stream's diagonal elements are formed on the device only: flat=True)
            raise NotImplementedError(f'compute_energy_loss_and_kfac(flat=False): {prog.PER_WALKER_NUCLEAR}; the tree path stays '
                                      'refused with nuclear_params=True, use flat=True')
        rr = pc.r if hasattr(pc, 'r') else pc
        RR = pc.R if hasattr(pc, 'R') else None
        sign, logpsi, g, factors, rest = eng.log_psi_kfac(rr, cot.to(eng.dtype).to(eng.device).contiguous(), RR)
        dev = g.device
        valid = (sign != 0) & torch.isfinite(logpsi)
        n_v = max(int(valid.sum()), 1)
        gtree = prog.unflatten_grad(g)
        old = state[s] or {}
        new = {'A': {}, 'G': {}}
        delta = {m: {k: np.zeros_like(v) for k, v in leaves.items()} for m, leaves in gtree.items()}
        for mod, (A, G) in kfac_module_factors(prog, factors, n_v).items():
            A = mix(old.get('A', {}).get(mod), A)
            G = mix(old.get('G', {}).get(mod), G)
            new['A'][mod], new['G'][mod] = A, G
            pi = float(torch.sqrt((torch.trace(A) / A.shape[0]) / (torch.trace(G) / G.shape[0])))
            gw = torch.as_tensor(gtree[mod]['w'], device=dev)
            if 'b' in gtree[mod]:
                gw = torch.cat([gw, torch.as_tensor(gtree[mod]['b'], device=dev)[None]], 0)
            Ad = A + pi * sq * torch.eye(A.shape[0], dtype=A.dtype, device=dev)
            Gd = G + sq / pi * torch.eye(G.shape[0], dtype=G.dtype, device=dev)
            d = torch.cholesky_solve(gw, torch.linalg.cholesky(Ad))
            d = torch.cholesky_solve(d.T.contiguous(), torch.linalg.cholesky(Gd)).T
            d = d.cpu().numpy()
            delta[mod]['w'] = d[:gw.shape[0] - int('b' in gtree[mod])]
            if 'b' in gtree[mod]:
                delta[mod]['b'] = d[-1]
        # the diagonal block: every parameter element outside the Kronecker modules
        kron = set(new['A'])
        elems = np.concatenate([np.arange(base, base + int(np.prod(shape))) for (mod, leaf), (base, shape) in prog.grad_leaves.items()
                                if mod not in kron] or [np.zeros(0, np.int64)]).astype(np.int64)
        if elems.size:
            o = torch.zeros(rest.shape[0], elems.size, dtype=torch.float64, device=dev)
            for col in _rest_gather(prog, elems):
                sel = torch.as_tensor(col >= 0, device=dev)
                o[:, sel] += rest[:, torch.as_tensor(col[col >= 0], device=dev)].double()
            F = mix(old.get('diag'), (o * o).sum(0) / n_v)
            new['diag'] = F
            gflat = np.concatenate([np.asarray(gtree[mod][leaf]).reshape(-1) for (mod, leaf) in prog.grad_leaves])
            dflat = gflat[elems] / (F.cpu().numpy() + damping)
            pos = 0
            for (mod, leaf), (base, shape) in prog.grad_leaves.items():
                if mod in kron:
                    continue
                n = int(np.prod(shape))
                delta[mod][leaf] = dflat[pos:pos + n].reshape(shape)
                pos += n
        state[s] = new
        deltas.append(delta)
        gs.append(gtree)
        dots.append(sum(float(np.sum(delta[m][k] * gtree[m][k])) for m in gtree for k in gtree[m]))
    stats['grad'] = gs
    stats['precon_grad_dot'] = torch.tensor(dots, dtype=torch.float64)
    return loss, deltas, stats, state


def _kfac_directions_flat(ansatz, params, r, Rs, loss, cots, stats, state, damping, ema):
    """compute_energy_loss_and_kfac(flat=True) for given cotangents c_s (the penalties of create_loss_fn enter through c_s
    only; the factors are those of the unit cotangent either way).  state: None or a list with, per electronic state, None
    (first call) or the device tensor of the last call."""
    S = len(cots)
    state = list(state) if state is not None else [None] * S
    if len(state) != S:
        raise ValueError('state holds the factors of a different number of states')
    deltas, gs, dots = [], [], []
    for s, cot in enumerate(cots):
        pc, eng = _state_conf(ansatz, params[s], r, Rs, s)
        if eng.program.grad_unsupported:
            raise NotImplementedError(f'compute_energy_loss_and_kfac: unsupported for this program ({eng.program.grad_unsupported})')
        lay = eng.program.kfac_layout()
        rr = r[0, s].contiguous()
        fac = torch.empty(lay['n_factor_doubles'], dtype=torch.float64, device=eng.device)
        rest = torch.empty(rr.shape[0], lay['n_rest'], dtype=eng.dtype, device=eng.device)
        sign, logpsi, g, _, rest = eng.log_psi_kfac(rr, cot.to(eng.dtype).to(eng.device).contiguous(), Rs[0], out=(fac, rest))
        gt = eng.grad_to_params(g)
        first = state[s] is None
        if first:
            state[s] = eng.kfac_state()
        delta, dot = eng.kfac_direction(gt, fac, rest, logpsi, sign, state[s], first, ema, damping)
        deltas.append(delta)
        gs.append(gt)
        dots.append(dot)
    stats['grad'] = gs
    stats['precon_grad_dot'] = torch.cat(dots)
    return loss, deltas, stats, state


# ---- the training loss of several electronic states: energy + overlap penalty + spin penalty (loss/loss_function.py:107-308) ----

def psi_ratio_clip_and_mask(x: torch.Tensor, clip_width: float = 10.0, exclude_width: float = float('inf')):
    """loss/clip.py:144-174 for one [B] batch of wave-function ratios: clip to median +- clip_width x the median absolute
    deviation from it (both medians exact, the mean of the two middle values for even B); mask = deviation < exclude_width."""
    def median(v):
        vs = torch.sort(v).values
        n = vs.shape[0]
        return 0.5 * (vs[(n - 1) // 2] + vs[n // 2])
    center = median(x)
    deviation = (x - center).abs()
    sigma = median(deviation)
    return torch.clamp(x, center - clip_width * sigma, center + clip_width * sigma), deviation < exclude_width


def no_scaling(data):
    """loss/overlap.py:158-160."""
    return torch.tensor(1.0, dtype=torch.float64)


def scale_by_energy_gap(data, min_gap_scale_factor: float = 0.1):
    """loss/overlap.py:163-170: clip(nan_to_num(|E_i - E_j|, nan=1), min_gap_scale_factor, 5) of the running energies
    data['energy_ewm'] [M, S] -> [M, S, S]."""
    e = data['energy_ewm']
    return torch.clamp(torch.nan_to_num((e[:, :, None] - e[:, None]).abs(), nan=1.0), min_gap_scale_factor, 5.0)


def scale_by_energy_std(data, min_gap_scale_factor: float = 0.01):
    """loss/overlap.py:173-177: clip(nan_to_num(mean over molecules of data['std_ewm'], nan=5), min_gap_scale_factor, 5) -> [S, 1]."""
    return torch.clamp(torch.nan_to_num(data['std_ewm'].mean(dim=0), nan=5.0), min_gap_scale_factor, 5.0)[:, None]


def scale_by_max_gap_std(data, min_gap_scale_factor: float = 0.1):
    """loss/overlap.py:180-184."""
    return torch.maximum(scale_by_energy_gap(data, min_gap_scale_factor), scale_by_energy_std(data, min_gap_scale_factor))


def _states(states, S):
    return list(range(S)) if states is None else [int(s) for s in states]


def compute_spin_contributions(hamil, ansatz, params: Sequence, phys_conf, states=None):
    """loss/spin.py:13-46: <S^2> per walker (physics.evaluate_spin) of the states `states` (default: all) on their own
    samples -> float64 [1, n_states, B]."""
    r, Rs = _unpack(phys_conf)
    if r.shape[0] != 1:
        raise ValueError('compute_spin_contributions: one molecule per batch ([1, S, B])')
    from .physics import evaluate_spin
    spin = evaluate_spin(hamil, ansatz)
    return torch.stack([spin(params[s], _state_conf(ansatz, params[s], r, Rs, s)[0]) for s in _states(states, r.shape[1])])[None]


def spin_raising_down_idx(rng, hamil) -> int:
    """The down electron of the stochastic spin-raising operator for the integer step seed `rng`: ONE index for the whole
    batch, as the reference draws it (loss/spin.py:151-154), by the rule
        down_idx = n_up + numpy.random.default_rng([rng mod 2^64, 0x5350494e]).integers(n_down)."""
    if not isinstance(rng, (int, np.integer)):
        raise ValueError('the spin-raising penalty needs an integer step seed `rng` (or an explicit down_idx)')
    return hamil.n_up + int(np.random.default_rng([int(rng) & (2 ** 64 - 1), 0x5350494e]).integers(hamil.n_down))


def compute_spin_raising_contributions(rng, hamil, ansatz, phys_conf, params: Sequence, states=None, down_idx=None, return_ratios=False):
    """loss/spin.py:118-172: L_b = 1 - sum_{alpha in up} psi(P_{alpha beta} r_b) / psi(r_b) for one down electron beta of the
    whole batch, drawn from the step seed by spin_raising_down_idx unless `down_idx` fixes it -> float64 [1, n_states, B].
    return_ratios: also the ratios rho[n_states, B, n_up] the direct term of the gradient is weighted with."""
    from .physics import _ratios
    r, Rs = _unpack(phys_conf)
    if r.shape[0] != 1:
        raise ValueError('compute_spin_raising_contributions: one molecule per batch ([1, S, B])')
    beta = spin_raising_down_idx(rng, hamil) if down_idx is None else int(down_idx)
    if not hamil.n_up <= beta < hamil.n_up + hamil.n_down:
        raise ValueError(f'down_idx must lie in [{hamil.n_up}, {hamil.n_up + hamil.n_down})')
    rows, rhos = [], []
    for s in _states(states, r.shape[1]):
        pc, eng = _state_conf(ansatz, params[s], r, Rs, s)
        up = torch.arange(hamil.n_up, device=eng.device)
        rho = _ratios(ansatz, params[s], pc, up, torch.full_like(up, beta))          # [B, n_up]
        rows.append(1.0 - rho.sum(-1))
        rhos.append(rho)
    out = torch.stack(rows)[None]
    return (out, torch.stack(rhos), beta) if return_ratios else out


def compute_mean_spin(spin_contributions: torch.Tensor, weight: torch.Tensor, states=None):
    """loss/spin.py:49-73: (mean over [1, n_states, B] of spin x weight, {'spin/mean', 'spin/std'}: the weighted average and
    standard deviation per state [1, n_states])."""
    sw = weight[:, _states(states, weight.shape[1])]
    mean = (spin_contributions * sw).sum(-1) / sw.sum(-1)
    var = ((spin_contributions - mean[..., None]) ** 2 * sw).sum(-1) / sw.sum(-1)
    return (spin_contributions * sw).mean(), {'spin/mean': mean, 'spin/std': torch.sqrt(var)}


def _library_clip(fn, base, defaults):
    """The keyword values of `fn` if it is `base` itself or a functools.partial (of partials) of it, else None."""
    import functools
    import inspect
    args, kw = (), {}
    while isinstance(fn, functools.partial):
        args, kw = fn.args + args, {**fn.keywords, **kw}
        fn = fn.func
    if fn is not base:
        return None
    try:
        bound = inspect.signature(base).bind_partial(None, *args, **kw)
    except TypeError:
        return None
    out = dict(defaults)
    out.update({k: v for k, v in bound.arguments.items() if k != 'x'})
    return out


def _single_process(name):
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError(f'{name}: single process only (the medians and means of other ranks are not gathered)')


class LossFunction:
    """The object create_loss_fn returns; see there."""

    def __init__(self, hamil, ansatz, clip_mask_fn, clip_mask_overlap_fn, alpha, spin_penalty, spin_penalty_type, spin_penalty_states,
                 scale_overlap_by, sort_states_by, min_gap_scale_factor):
        import functools
        if spin_penalty_type not in ('squared', 'raising'):
            raise ValueError("spin_penalty_type must be 'squared' or 'raising'")
        scale_fns = {None: no_scaling, 'energy_gap': scale_by_energy_gap, 'energy_std': scale_by_energy_std, 'max_gap_std': scale_by_max_gap_std}
        if scale_overlap_by not in scale_fns:
            raise ValueError(f'scale_overlap_by must be one of {list(scale_fns)}')
        if sort_states_by not in (None, 'energy'):
            raise ValueError("sort_states_by must be None or 'energy'")
        self.hamil, self.ansatz = hamil, ansatz
        self.clip_mask_fn, self.clip_mask_overlap_fn = clip_mask_fn, clip_mask_overlap_fn
        self.alpha, self.spin_penalty, self.spin_penalty_type = alpha, spin_penalty, spin_penalty_type
        self.spin_penalty_states = None if spin_penalty_states is None else [int(s) for s in spin_penalty_states]
        self.scale_overlap_by, self.sort_states_by = scale_overlap_by, sort_states_by
        # (loss_function.py:121-135: every factory is called with THIS min_gap_scale_factor, scale_by_energy_std included)
        self.scale_fn = no_scaling if scale_overlap_by is None else functools.partial(scale_fns[scale_overlap_by],
                                                                                     min_gap_scale_factor=min_gap_scale_factor)
        self._e_clip = _library_clip(clip_mask_fn, median_clip_and_mask, dict(clip_width=5.0, median_center=True, exclude_width=float('inf')))
        self._r_clip = _library_clip(clip_mask_overlap_fn, psi_ratio_clip_and_mask, dict(clip_width=10.0, exclude_width=float('inf')))
        self.kernel_path = self._e_clip is not None and (self._r_clip is not None or clip_mask_overlap_fn is None)
        self._index_cache = {}

    # -- pieces ------------------------------------------------------------
    def _states_index(self, states, device):
        """The spin states as an index tensor on `device`: uploaded once, so that no step copies it from the host."""
        key = (tuple(states), str(device))
        if key not in self._index_cache:
            self._index_cache[key] = torch.tensor(states, dtype=torch.long, device=device)
        return self._index_cache[key]

    def ordering(self, data, S, device):
        """data['ordering'] of loss_function.py:136-139, 228 for molecule 0 -> (ordering [S], rank [S] int32 = its inverse)."""
        if self.sort_states_by == 'energy':
            order = torch.argsort(data['energy_ewm'][0].to(device), dim=-1, stable=True)
        else:
            order = torch.arange(S, device=device)
        rank = torch.empty_like(order)
        rank[order] = torch.arange(S, device=device)
        return order, rank.to(torch.int32)

    def overlap_scale(self, data, S, device):
        """scale[S, S] of the configured factory for molecule 0."""
        if self.scale_overlap_by is None:
            return torch.ones(S, S, dtype=torch.float64, device=device)
        sc = torch.as_tensor(self.scale_fn(data), dtype=torch.float64).to(device)
        if sc.dim() == 3:
            sc = sc[0]
        return sc.expand(S, S).contiguous()

    def cotangents(self, e_loc, weight, psi_ratio=None, spin=None, data=None, path=None, engine=None, return_mask=False):
        """The loss assembly on its own: from E_loc [S, B], the weights [S, B], the ratios [S, S, B] (S > 1), the spin rows
        [n_states, B] (squared: <S^2>, raising: L) and data -> (c [S, B], k [n_states, B] or None), float64 on the device
        of the inputs.  path: 'kernel' (dqmc_clip_rows + dqmc_loss_cotangents on `engine`'s stream), 'torch' (the same formulas in
        torch, any clip callable), default: the kernel path when the clip functions are the library's own.
        return_mask: also the energy clip mask, bool [S, B] (what the natural gradient centres its Fisher matrix with).
        Row q of `spin` belongs to state states[q], and so does row q of the raising kind's clip mask: the reference indexes
        that [M, n_states, B] mask by the state NUMBERS once more (spin.py:207-209), which for a proper subset of the states
        picks clamped or shifted rows; that is not reproduced."""
        path = path or ('kernel' if self.kernel_path else 'torch')
        S, B = e_loc.shape
        if S > 1 and self.alpha is None:
            raise ValueError('alpha must be set for the overlap loss of more than one state')
        data = data or {}
        if S > 1 and 'energy_ewm' not in data and (self.sort_states_by or self.scale_overlap_by in ('energy_gap', 'max_gap_std')):
            raise ValueError("data['energy_ewm'] is required")
        if path == 'kernel':
            if not self.kernel_path:
                raise ValueError('the kernel path needs the library\'s own clip functions (median_clip_and_mask, psi_ratio_clip_and_mask)')
            c, k, e_mask = self._cotangents_kernel(engine, e_loc, weight, psi_ratio, spin, data)
        elif path == 'torch':
            c, k, e_mask = self._cotangents_torch(e_loc, weight, psi_ratio, spin, data)
        else:
            raise ValueError("path must be 'kernel' or 'torch'")
        return (c, k, e_mask) if return_mask else (c, k)

    def _cotangents_kernel(self, eng, e, w, ratio, spin, data):
        S, B = e.shape
        ec = self._e_clip
        kw = {}
        e_clip, e_mask, e_stats = eng.clip_rows(e, w, median_center=bool(ec['median_center']), median_scale=False,
                                                clip_width=ec['clip_width'], exclude_width=ec['exclude_width'])
        if S > 1:
            rc = self._r_clip
            w_rows = w[None].expand(S, S, B).reshape(S * S, B).contiguous()           # row (i, j) is weighted with w_j
            r_clip, r_mask, r_stats = eng.clip_rows(ratio.reshape(S * S, B), w_rows, median_center=True, median_scale=True,
                                                    clip_width=rc['clip_width'], exclude_width=rc['exclude_width'])
            kw.update(alpha=self.alpha, r_clip=r_clip.view(S, S, B), r_mask=r_mask.view(S, S, B), r_stats=r_stats,
                      scale=self.overlap_scale(data, S, e.device), rank=self.ordering(data, S, e.device)[1])
        if self.spin_penalty is not None:
            states = _states(self.spin_penalty_states, S)
            kw.update(spin_kind=self.spin_penalty_type, spin_penalty=self.spin_penalty, states=states)
            if self.spin_penalty_type == 'squared':
                kw['spin'] = spin.contiguous()
            else:
                l_clip, l_mask, l_stats = eng.clip_rows(spin.contiguous(), w[self._states_index(states, w.device)], median_center=bool(ec['median_center']),
                                                        median_scale=False, clip_width=ec['clip_width'], exclude_width=ec['exclude_width'])
                kw.update(spin=l_clip, spin_mask=l_mask, spin_stats=l_stats)
        c, k = eng.loss_cotangents(e_clip, e_mask, e_stats, w, **kw)
        return c, k, e_mask

    def _cotangents_torch(self, e, w, ratio, spin, data):
        S, B = e.shape
        f64 = torch.float64
        clipped = [self.clip_mask_fn(e[s]) for s in range(S)]
        e_clip = torch.stack([c for c, _ in clipped])
        e_mask_b = torch.stack([m for _, m in clipped])
        e_mask = e_mask_b.to(f64)
        c = e_mask * w * (e_clip - (e_clip * w).mean(-1, keepdim=True)) / e_mask.sum()
        if S > 1:
            if self.clip_mask_overlap_fn is None:
                raise ValueError('clip_mask_overlap_fn must be set for more than one state')
            pairs = [[self.clip_mask_overlap_fn(ratio[i, j]) for j in range(S)] for i in range(S)]
            r_clip = torch.stack([torch.stack([p[0] for p in row]) for row in pairs])
            r_mask = torch.stack([torch.stack([p[1] for p in row]) for row in pairs]).to(f64)
            x = (r_clip * w[None]).mean(-1)                                           # x_ij = mean_b(w_jb rho^_ijb)
            scale = self.overlap_scale(data, S, e.device)
            rank = self.ordering(data, S, e.device)[1]
            lower = (rank[:, None] < rank[None, :]).to(f64)                           # [i, j]: rank(i) < rank(j)
            coef = self.alpha * lower * 2.0 * x.transpose(0, 1) * scale / r_mask.sum(-1)
            c = c + (coef[:, :, None] * r_mask * (r_clip - x[:, :, None]) * w[None]).sum(0)
        k = None
        if self.spin_penalty is not None:
            states = _states(self.spin_penalty_states, S)
            idx = self._states_index(states, w.device)
            sw = w[idx]
            if self.spin_penalty_type == 'squared':
                m = e_mask[idx]
                add = self.spin_penalty * m * sw * (spin - (spin * sw).mean(-1, keepdim=True)) / m.sum()
            else:
                clipped = [self.clip_mask_fn(spin[q]) for q in range(len(states))]
                l_clip = torch.stack([cl for cl, _ in clipped])
                m = torch.stack([mk for _, mk in clipped]).to(f64)
                mu = (l_clip * sw).mean(-1, keepdim=True)
                k = self.spin_penalty * m * mu * sw / m.sum()
                add = k * 2.0 * (l_clip - mu)
            c = c.index_add(0, idx, add)
        return c, k, e_mask_b

    def _psi_ratio(self, params, r, Rs):
        """compute_psi_ratio with the log shift on the device (dqmc_psi_ratio) -> [1, S, S, B]."""
        S, B = r.shape[1], r.shape[2]
        eng0 = self.ansatz.engine(params[0], Rs[0])
        sign = torch.empty(S, S, B, dtype=torch.float64, device=eng0.device)
        log = torch.empty(S, S, B, dtype=torch.float64, device=eng0.device)
        r_all = r[0].reshape(S * B, *r.shape[3:]).contiguous()
        for i in range(S):
            sg, lg = self.ansatz.engine(params[i], Rs[0]).wf_eval(r_all, Rs[0])
            sign[i], log[i] = sg.reshape(S, B), lg.reshape(S, B)
        return eng0.psi_ratio(log, sign)[None]

    # -- the whole step --------------------------------------------------------
    def evaluate(self, rng, params, batch, static_io=False, down_idx=None):
        """The value side (loss_function.py:141-189): -> dict(loss, e_loc [1,S,B], weight [1,S,B], psi_ratio [1,S,S,B] or None,
        spin [n_states, B] or None, rho, stats, r, Rs)."""
        phys_conf, weight = batch[0], batch[1] if len(batch) > 1 else None
        _single_process('create_loss_fn')
        r, Rs = _unpack(phys_conf)
        if r.shape[0] != 1:
            raise ValueError('create_loss_fn: one molecule per batch ([1, S, B])')
        S, B = r.shape[1], r.shape[2]
        if S > 1 and self.alpha is None:
            raise ValueError('alpha must be set for the overlap loss of more than one state')
        e_loc, stats = compute_local_energy(rng, self.hamil, self.ansatz, params, phys_conf, static_io=static_io)
        e64 = e_loc.double()
        w = torch.ones_like(e64) if weight is None else torch.as_tensor(weight, dtype=torch.float64, device=e64.device).reshape(e64.shape)
        out = dict(e_loc=e_loc, e64=e64, weight=w, r=r, Rs=Rs, psi_ratio=None, spin=None, rho=None, beta=None)
        loss = (e64 * w).mean()
        stats = dict(stats)
        if S > 1:
            psi_ratio = self._psi_ratio(params, r, Rs) if self.kernel_path else compute_psi_ratio(self.ansatz, params, phys_conf)[0]
            overlap_loss, ostats = compute_mean_overlap(psi_ratio, w)
            loss = loss + self.alpha * overlap_loss
            stats.update(ostats)
            out['psi_ratio'] = psi_ratio
        if self.spin_penalty is not None:
            if self.spin_penalty_type == 'squared':
                spin = compute_spin_contributions(self.hamil, self.ansatz, params, phys_conf, self.spin_penalty_states)
            else:
                spin, out['rho'], out['beta'] = compute_spin_raising_contributions(rng, self.hamil, self.ansatz, phys_conf, params,
                                                                                   self.spin_penalty_states, down_idx, return_ratios=True)
            mean_spin, sstats = compute_mean_spin(spin, w, self.spin_penalty_states)
            loss = loss + self.spin_penalty * mean_spin
            stats.update(sstats)
            out['spin'] = spin[0]
        stats['E_loc'] = e_loc
        out.update(loss=loss, stats=stats)
        return out

    def loss_and_cotangents(self, rng, params, batch, static_io=False, down_idx=None, path=None):
        """evaluate + cotangents: -> (values dict of evaluate, which gains 'e_mask' bool [S, B], c [S, B], k or None)."""
        v = self.evaluate(rng, params, batch, static_io=static_io, down_idx=down_idx)
        data = batch[2] if len(batch) > 2 and batch[2] is not None else {}
        eng = self.ansatz.engine(params[0], v['Rs'][0])
        c, k, v['e_mask'] = self.cotangents(v['e64'][0].contiguous(), v['weight'][0].contiguous(),
                                            None if v['psi_ratio'] is None else v['psi_ratio'][0], v['spin'], data, path=path, engine=eng,
                                            return_mask=True)
        return v, c, k

    def loss_and_grad(self, rng, params, batch, flat: bool = False, down_idx=None, path=None):
        """-> (loss, [grad per state], (E_loc [1,S,B], psi_ratio [1,S,S,B] or None, stats)).  Per state one dqmc_log_psi_vjp call with
        the cotangent c_s; the raising kind runs it on the stack [r_s ; P_alpha r_s, alpha < n_up] with the cotangents
        [c_sb + k_sb sum_alpha rho_b,alpha ; -k_sb rho_b,alpha].  flat=True: float64 device vectors in parameter order
        (Engine.grad_to_params) and nothing waits for the host; else host trees."""
        from .physics import _swapped
        v, c, k = self.loss_and_cotangents(rng, params, batch, static_io=flat, down_idx=down_idx, path=path)
        r, Rs = v['r'], v['Rs']
        S, B = r.shape[1], r.shape[2]
        states = _states(self.spin_penalty_states, S)
        grads = []
        for s in range(S):
            eng = self.ansatz.engine(params[s], Rs[0])
            if flat and eng.program.grad_unsupported:
                raise NotImplementedError(f'create_loss_fn: unsupported for this program ({eng.program.grad_unsupported})')
            rr, cot = r[0, s].contiguous(), c[s]
            if k is not None and s in states:
                q = states.index(s)
                rho, n_up = v['rho'][q], self.hamil.n_up                               # [B, n_up]
                up = torch.arange(n_up, device=eng.device)
                rp = _swapped(torch.as_tensor(rr, dtype=eng.dtype, device=eng.device), up, torch.full_like(up, v['beta']))   # [B, n_up, N, 3]
                rr = torch.cat([torch.as_tensor(rr, dtype=eng.dtype, device=eng.device), rp.reshape(B * n_up, *rp.shape[2:])])
                cot = torch.cat([cot + k[q] * rho.sum(-1), (-k[q][:, None] * rho).reshape(-1)])
            _, _, g = eng.log_psi_vjp(rr, cot.to(eng.dtype).contiguous(), Rs[0])
            grads.append(eng.grad_to_params(g) if flat else self.ansatz._grad_tree(eng, g))
        return v['loss'], grads, (v['e_loc'], v['psi_ratio'], v['stats'])

    __call__ = loss_and_grad


def create_loss_fn(hamil, ansatz, clip_mask_fn=median_clip_and_mask, clip_mask_overlap_fn=psi_ratio_clip_and_mask, alpha=None,
                   spin_penalty=None, spin_penalty_type='squared', spin_penalty_states=None, scale_overlap_by=None, sort_states_by=None,
                   min_gap_scale_factor=0.1):
    """loss/loss_function.py:107-308 for a [1, S, B] batch: the energy loss of compute_energy_loss_and_grad plus
    alpha x the overlap penalty between the states and spin_penalty x a spin penalty ('squared': <S^2> of physics.evaluate_spin,
    'raising': the stochastic spin-raising estimator), over `spin_penalty_states` (default: all).  Returns a LossFunction whose
        loss_and_grad(rng, params, batch, flat=False) -> (loss, [grad per state], (E_loc [1,S,B], psi_ratio [1,S,S,B] or None, stats))
    takes batch = (phys_conf, weight, data), data = {'energy_ewm': [1, S], 'std_ewm': [1, S]} float64 device tensors (the
    running averages of fit_wf; NaN before the first update).  The loss VALUE uses the unclipped overlap and spin means
    (loss_function.py:141-189); stats gains 'overlap/pairwise/mean' [1,S,S], 'spin/mean' and 'spin/std' [1, n_states].

    Every penalty tangent is a linear functional of the tangent of log|psi_s| on state s's own samples, so the gradient of
    state s is ONE vector-Jacobian product with the cotangent (w weights, hats clipped values, m masks)
        c_sb  = m_sb w_sb (E^_sb - mean_b(E^_s w_s)) / sum_{s,b} m_sb
        c_jb += alpha sum_{i: rank(i) < rank(j)} 2 x_ji scale_ij m_ijb (rho^_ijb - x_ij) w_jb / sum_b m_ijb,  x_ij = mean_b(w_jb rho^_ijb)
        c_sb += lambda m_sb w_sb (s_sb - mean_b(s_s w_s)) / sum_{s in states, b} m_sb                              ('squared')
        c_sb += lambda m_sb mu_s w_sb 2 (L^_sb - mu_s) / n, mu_s = mean_b(L^_s w_s), plus the direct term sum_b k_sb dL_sb,
                k_sb = lambda m_sb mu_s w_sb / n                                                                   ('raising')
    rank = the inverse of the state ordering (sort_states_by='energy': argsort of data['energy_ewm']), scale_ij from
    scale_overlap_by (None, 'energy_gap', 'energy_std', 'max_gap_std').  The assembly runs as HIP kernels (dqmc_clip_rows,
    dqmc_loss_cotangents) when the clip functions are median_clip_and_mask / psi_ratio_clip_and_mask or functools.partial of
    them, and as the same formulas in torch for any other callable.  One molecule, single process (NotImplementedError under
    an initialised process group of more than one rank); S > 1 without alpha is a ValueError."""
    return LossFunction(hamil, ansatz, clip_mask_fn, clip_mask_overlap_fn, alpha, spin_penalty, spin_penalty_type, spin_penalty_states,
                        scale_overlap_by, sort_states_by, min_gap_scale_factor)
