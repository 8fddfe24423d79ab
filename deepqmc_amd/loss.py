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
                                 clip_mask_fn=median_clip_and_mask):
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
    per electronic state, to pass to the next call.  Single process only: the factors of other ranks are not summed."""
    if not damping > 0:
        raise ValueError('damping must be positive')
    r, Rs, loss, cots, masks, stats = _energy_loss_cotangents('compute_energy_loss_and_kfac', rng, hamil, ansatz, params, phys_conf,
                                                             weight, clip_mask_fn)
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
