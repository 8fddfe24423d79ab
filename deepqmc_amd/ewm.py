"""Exponentially weighted running averages of the training loop (reference src/deepqmc/ewm.py), as torch on the device: one
independent estimator per (molecule, electronic state).  fit_wf keeps one of the states' energies and one of their standard
deviations; the overlap penalty of loss.create_loss_fn is scaled and ordered by them.

Each estimator holds a window of the most recent observations (newest first) and their decay factors.  An update shifts the
observation in, and -- while fewer than `window_size` updates were made -- the factor a_t = max(1 - max_alpha, 1 / (2 + t /
decay_alpha)) of update t = 0, 1, ...; with beta_k = prod_{l<k} (1 - a_l) the weights are a_k beta_k and
    mean = sum_k weight_k x_k,  var = sum_k weight_k (x_k - mean)^2,  sqerr = sum_k weight_k^2 (x_k - mean)^2.
The state starts with mean = var = sqerr = NaN, and -- as in the reference -- the weights of the first updates do not sum to
one (the first mean is x / 2): the early averages are under-normalised on purpose of parity; consumers read the NaN start
through nan_to_num.
"""
from __future__ import annotations

from collections import namedtuple
from math import ceil

import torch

__all__ = ['EWMState', 'init_multi_mol_multi_state_ewm']

EWMState = namedtuple('EWMState', 'step params buffer mean var sqerr')


def init_multi_mol_multi_state_ewm(shape, max_alpha: float = 0.999, decay_alpha: float = 10.0, window_size=None, device='cpu'):
    """ewm.py:119-182: -> (state, update).  state: EWMState of float64 tensors of leading shape `shape` (typically (n_mols, S)) on
    `device` (step: int64 [*shape]; params['alpha'], buffer: [*shape, window_size]).  update(x, state, sub_idxs=None) -> state
    advances every estimator with x [*shape], or only the entries `sub_idxs` of the leading axis with x [len(sub_idxs),
    *shape[1:]].  Nothing waits for the host."""
    if window_size is None:
        window_size = ceil(decay_alpha * (1 / (1 - max_alpha) - 2))
    shape = tuple(shape)
    f64 = dict(dtype=torch.float64, device=device)
    state = EWMState(step=torch.zeros(shape, dtype=torch.int64, device=device),
                     params={'max_alpha': max_alpha, 'decay_alpha': decay_alpha, 'alpha': torch.zeros(*shape, window_size, **f64)},
                     buffer=torch.zeros(*shape, window_size, **f64), mean=torch.full(shape, float('nan'), **f64),
                     var=torch.full(shape, float('nan'), **f64), sqerr=torch.full(shape, float('nan'), **f64))

    def update_all(x, step, alpha, buffer):
        x = torch.as_tensor(x, dtype=torch.float64, device=buffer.device)
        buffer = torch.cat([x[..., None], buffer[..., :-1]], dim=-1)
        new = torch.clamp(1.0 / (2.0 + step.to(torch.float64) / decay_alpha), min=1.0 - max_alpha)
        shifted = torch.cat([new[..., None], alpha[..., :-1]], dim=-1)
        alpha = torch.where((step + 1 >= window_size)[..., None], alpha, shifted)
        beta = torch.cat([torch.ones_like(alpha[..., :1]), torch.cumprod(1.0 - alpha[..., :-1], dim=-1)], dim=-1)
        weights = alpha * beta
        mean = (weights * buffer).sum(-1)
        variance = weights * (buffer - mean[..., None]) ** 2
        return step + 1, alpha, buffer, mean, variance.sum(-1), (weights * variance).sum(-1)

    def update(x, state, sub_idxs=None):
        if sub_idxs is None:
            step, alpha, buffer, mean, var, sqerr = update_all(x, state.step, state.params['alpha'], state.buffer)
            return EWMState(step, {**state.params, 'alpha': alpha}, buffer, mean, var, sqerr)
        idx = torch.as_tensor(sub_idxs, dtype=torch.long, device=state.buffer.device)
        new = update_all(x, state.step[idx], state.params['alpha'][idx], state.buffer[idx])
        old = (state.step, state.params['alpha'], state.buffer, state.mean, state.var, state.sqerr)
        step, alpha, buffer, mean, var, sqerr = (o.index_copy(0, idx, n) for o, n in zip(old, new))
        return EWMState(step, {**state.params, 'alpha': alpha}, buffer, mean, var, sqerr)

    return state, update
