"""Optimisers of the variational training loop with the surface of the reference's `optimizer.py` (`init(rng, params,
batch)`, `step(rng, params, opt_state, batch) -> (params, opt_state, E_loc, ratios, stats)`), backed by the device-resident
optimiser step of the HIP library (include/dqmc.h: dqmc_set_param_map ... dqmc_apply_update).

The parameters of electronic state s live in a float64 device vector `theta` (the order of Program.grad_leaves) inside the
optimiser state, next to Adam's moments.  A step evaluates the energy loss and its gradient as flat device vectors
(loss.compute_energy_loss_and_grad(..., flat=True)), updates theta in one fused kernel and re-packs the context's weights
on the device: no parameter crosses the host, no layer program is recompiled, and the captured forward-Laplacian graph of the
context stays valid.  The parameter TREES handed to `step` are returned as the same objects -- they key the context cache
(wf.py) -- with leaves that are stale until `NeuralNetworkWaveFunction.sync_params` (fit.fit_wf does that every `sync_every`
steps and when it ends).

`batch` = `(phys_conf, weight)` or `(phys_conf, weight, data)` as in the reference: phys_conf r[1, S, B, N, 3] or a
PhysicalConfiguration of it, weight [1, S, B] or None.  KFACOptimizer forms its direction on the device as well
(loss.compute_energy_loss_and_kfac(..., flat=True), dqmc_kfac_direction / dqmc_kfac_apply); the tree-based KFAC direction
(flat=False) remains for host-side use.
"""
from __future__ import annotations

import torch

from .loss import (_kfac_directions_flat, _natgrad_directions, _unpack, compute_energy_loss_and_grad, compute_energy_loss_and_kfac,
                   compute_energy_loss_and_natgrad, compute_local_energy, median_clip_and_mask)

__all__ = ['NoOptimizer', 'AdamOptimizer', 'NaturalGradientOptimizer', 'KFACOptimizer', 'InverseSchedule', 'ConstantSchedule',
           'merge_states_flat']


class InverseSchedule:
    """optimizer.py (reference): init_value / (1 + n / decay_rate) at step count n."""

    def __init__(self, init_value, decay_rate):
        self.init_value, self.decay_rate = init_value, decay_rate

    def __call__(self, n):
        return self.init_value / (1 + n / self.decay_rate)


class ConstantSchedule:
    """The same value at every step count."""

    def __init__(self, value):
        self.value = value

    def __call__(self, n):
        return self.value


class _Optimizer:
    changes_params = True

    def __init__(self, *, hamil=None, ansatz=None, clip_mask_fn=median_clip_and_mask, loss_fn=None):
        """loss_fn: a loss.create_loss_fn object (energy + overlap + spin penalties, its own clip functions); None: the energy
        loss of compute_energy_loss_and_grad with `clip_mask_fn`, exactly as without the argument."""
        self.hamil, self.ansatz, self.clip_mask_fn, self.loss_fn = hamil, ansatz, clip_mask_fn, loss_fn
        if loss_fn is not None and hamil is None:
            self.hamil, self.ansatz = loss_fn.hamil, loss_fn.ansatz

    def bind(self, hamil, ansatz):
        """The Hamiltonian and the wave function the loss is evaluated with (fit_wf binds an optimiser built without them)."""
        self.hamil, self.ansatz = hamil, ansatz
        return self

    def _engines(self, params, phys_conf):
        if self.ansatz is None:
            raise ValueError('optimizer is not bound to a Hamiltonian and an ansatz: pass them at construction or call bind()')
        Rs = [None] if phys_conf is None else _unpack(phys_conf)[1]
        return [self.ansatz.engine(p, Rs[0]) for p in params]

    def _refuse_nuclear_stream(self, params, batch):
        """The optimisers that need per-walker partials of log|psi| (Jacobian rows, KFAC factors) take a program whose
        nuclear-token stream is shared by all walkers only with nuclear_params=True (the stream's partials per walker)."""
        for eng in self._engines(params, batch[0] if batch is not None else None):
            if eng.program.nuclear_stream is not None and not eng.nuclear_params:
                raise NotImplementedError(f'{type(self).__name__}: {eng.program.PER_WALKER_NUCLEAR}')

    @staticmethod
    def _batch(batch):
        phys_conf, weight = batch[0], batch[1] if len(batch) > 1 else None
        return phys_conf, weight

    def _new_state(self, params, batch, moments):
        engines = self._engines(params, batch[0] if batch is not None else None)
        state = []
        for p, eng in zip(params, engines):
            # a context that was already stepped on the device holds the current values; otherwise the tree does
            theta = eng.params_flat() if eng.params_ahead else eng.params_flat(p)
            st = {'theta': theta, 'count': 0, 'norms': torch.zeros(3, dtype=torch.float64, device=theta.device)}
            if moments:
                st['mu'], st['nu'] = torch.zeros_like(theta), torch.zeros_like(theta)
            state.append(st)
        return state

    @staticmethod
    def _opt_stats(opt_state):
        norms = torch.stack([st['norms'] for st in opt_state])      # [S, 3]: (param, grad, update) per electronic state
        return {'opt/param_norm': norms[:, 0], 'opt/grad_norm': norms[:, 1], 'opt/update_norm': norms[:, 2]}


class NoOptimizer(_Optimizer):
    """optimizer.py:74-102: evaluates the local energies, leaves the parameters alone."""

    changes_params = False

    def init(self, rng, params, batch):
        return None

    def step(self, rng, params, opt_state, batch):
        phys_conf, _ = self._batch(batch)
        if self.loss_fn is not None:       # the loss value and the ratios, no gradient
            v = self.loss_fn.evaluate(rng, params, batch, static_io=True)
            stats = dict(v['stats'])
            e_loc = stats.pop('E_loc')
            return params, opt_state, e_loc, v['psi_ratio'], {'loss': v['loss'], **stats}
        e_loc, stats = compute_local_energy(rng, self.hamil, self.ansatz, params, phys_conf, static_io=True)
        return params, opt_state, e_loc, None, dict(stats)


class AdamOptimizer(_Optimizer):
    """optimizer.py:105-158 with optax.adam(learning_rate, b1, b2, eps): the update of pretrain.adam on device vectors
    (dqmc_adam_step).  `learning_rate` may be a callable of the count of steps taken so far.  State: per electronic state
    {'theta', 'mu', 'nu', 'norms'} float64 device tensors and the integer 'count'."""

    def __init__(self, learning_rate=1e-3, b1=0.9, b2=0.999, eps=1e-8, **kw):
        super().__init__(**kw)
        self.lr, self.b1, self.b2, self.eps = learning_rate, b1, b2, eps

    def init(self, rng, params, batch):
        return self._new_state(params, batch, moments=True)

    def step(self, rng, params, opt_state, batch):
        phys_conf, weight = self._batch(batch)
        ratios, extra = None, {}
        if self.loss_fn is not None:
            loss, grads, (_, ratios, stats) = self.loss_fn.loss_and_grad(rng, params, batch, flat=True)
            extra = {'loss': loss}
        else:
            _, grads, stats = compute_energy_loss_and_grad(rng, self.hamil, self.ansatz, params, phys_conf, weight, self.clip_mask_fn,
                                                           flat=True)
        for eng, st, g in zip(self._engines(params, phys_conf), opt_state, grads):
            lr = self.lr(st['count']) if callable(self.lr) else self.lr
            eng.adam_step(st['theta'], st['mu'], st['nu'], g, lr=lr, b1=self.b1, b2=self.b2, eps=self.eps, t=st['count'] + 1,
                          norms=st['norms'])
            st['count'] += 1
        stats = dict(stats)
        e_loc = stats.pop('E_loc')
        return params, opt_state, e_loc, ratios, {**self._opt_stats(opt_state), **extra, **stats}


class NaturalGradientOptimizer(_Optimizer):
    """Stochastic reconfiguration on the flat natural gradient (loss.compute_energy_loss_and_natgrad(..., flat=True)):
    theta <- theta - learning_rate (F + damping I)^-1 g, the direction formed on the device and applied by dqmc_apply_update.
    'opt/grad_norm' is the norm of the preconditioned direction, as the reference reports for KFAC (optimizer.py:211)."""

    def __init__(self, learning_rate=1e-2, damping=1e-3, **kw):
        super().__init__(**kw)
        self.lr, self.damping = learning_rate, damping
        if self.loss_fn is not None and self.loss_fn.spin_penalty is not None and self.loss_fn.spin_penalty_type == 'raising':
            raise NotImplementedError("NaturalGradientOptimizer: the 'raising' spin penalty has a direct term that is not a "
                                      'contraction with the Jacobian of log|psi|')

    def init(self, rng, params, batch):
        self._refuse_nuclear_stream(params, batch)
        return self._new_state(params, batch, moments=False)

    def step(self, rng, params, opt_state, batch):
        phys_conf, weight = self._batch(batch)
        ratios, extra = None, {}
        if self.loss_fn is not None:
            # g_s = c_s J_s with the cotangent of the whole loss, preconditioned by the Fisher matrix of the energy path
            v, c, _ = self.loss_fn.loss_and_cotangents(rng, params, batch, static_io=True)
            ratios, extra = v['psi_ratio'], {'loss': v['loss']}
            _, deltas, stats = _natgrad_directions('NaturalGradientOptimizer', self.ansatz, params, v['r'], v['Rs'], v['loss'],
                                                   list(c), list(v['e_mask']), dict(v['stats']), self.damping, flat=True)
        else:
            _, deltas, stats = compute_energy_loss_and_natgrad(rng, self.hamil, self.ansatz, params, phys_conf, self.damping, weight,
                                                               self.clip_mask_fn, flat=True)
        for eng, st, d in zip(self._engines(params, phys_conf), opt_state, deltas):
            lr = self.lr(st['count']) if callable(self.lr) else self.lr
            eng.apply_update(st['theta'], d, scale=-lr, norms=st['norms'])
            st['count'] += 1
        stats = dict(stats)
        e_loc = stats.pop('E_loc')
        stats.pop('grad', None)
        return params, opt_state, e_loc, ratios, {**self._opt_stats(opt_state), **extra, **stats}


class KFACOptimizer(_Optimizer):
    """The reference's default optimiser (conf/task/opt/kfac.yaml: kfac_jax with learning rate InverseSchedule(0.05, 10000),
    norm_constraint 1e-3, damping 1e-3, inverse_update_period 1, momentum 0) on the flat device vectors: the direction of
    loss.compute_energy_loss_and_kfac (its docstring is the definition) formed by dqmc_kfac_direction with the factors in a
    device state, and theta <- theta - lr min(1, sqrt(norm_constraint / (lr^2 <delta, g>))) delta applied by
    dqmc_kfac_apply.  `learning_rate` and `damping` may be callables of the count of steps taken so far.  State per electronic
    state: {'theta', 'kfac' (the factor state, Engine.kfac_state_layout), 'count', 'norms' [4]}.  Stats: 'opt/param_norm',
    'opt/grad_norm' (the norm of the preconditioned direction, as the reference reports), 'opt/update_norm' and
    'opt/scaled_grad_norm_sq' = lr^2 <delta, g>.  Momentum, adaptive damping and an inverse_update_period other than 1 are
    not implemented; single process, one molecule per batch."""

    def __init__(self, learning_rate=InverseSchedule(0.05, 10000), norm_constraint=1e-3, damping=1e-3, ema=0.95, **kw):
        super().__init__(**kw)
        self.lr, self.norm_constraint, self.damping, self.ema = learning_rate, norm_constraint, damping, ema
        if self.loss_fn is not None and self.loss_fn.spin_penalty is not None and self.loss_fn.spin_penalty_type == 'raising':
            raise NotImplementedError("KFACOptimizer: the 'raising' spin penalty has a direct term that is not a "
                                      'contraction with the Jacobian of log|psi|')

    def init(self, rng, params, batch):
        self._refuse_nuclear_stream(params, batch)
        state = self._new_state(params, batch, moments=False)
        for st in state:
            st['kfac'] = None          # allocated by the first step (Engine.kfac_state), which overwrites it
            st['norms'] = torch.zeros(4, dtype=torch.float64, device=st['theta'].device)
        return state

    def step(self, rng, params, opt_state, batch):
        phys_conf, weight = self._batch(batch)
        ratios, extra = None, {}
        count = opt_state[0]['count']
        damping = self.damping(count) if callable(self.damping) else self.damping
        kstate = [st['kfac'] for st in opt_state]
        if self.loss_fn is not None:
            # the cotangent of the whole loss enters the reverse pass; the factors are those of the unit cotangent either way
            v, c, _ = self.loss_fn.loss_and_cotangents(rng, params, batch, static_io=True)
            ratios, extra = v['psi_ratio'], {'loss': v['loss']}
            if not damping > 0:
                raise ValueError('damping must be positive')
            _, deltas, stats, kstate = _kfac_directions_flat(self.ansatz, params, v['r'], v['Rs'], v['loss'], list(c), dict(v['stats']),
                                                             kstate, damping, self.ema)
        else:
            _, deltas, stats, kstate = compute_energy_loss_and_kfac(rng, self.hamil, self.ansatz, params, phys_conf, kstate, damping,
                                                                    self.ema, weight, self.clip_mask_fn, flat=True)
        dots = stats['precon_grad_dot']
        for s, (eng, st, d) in enumerate(zip(self._engines(params, phys_conf), opt_state, deltas)):
            lr = self.lr(st['count']) if callable(self.lr) else self.lr
            st['kfac'] = kstate[s]
            eng.kfac_apply(st['theta'], d, dots[s:s + 1], lr, self.norm_constraint, norms=st['norms'])
            st['count'] += 1
        stats = dict(stats)
        e_loc = stats.pop('E_loc')
        stats.pop('grad', None)
        stats.pop('precon_grad_dot', None)
        norms = torch.stack([st['norms'] for st in opt_state])
        opt = {'opt/param_norm': norms[:, 0], 'opt/grad_norm': norms[:, 1], 'opt/update_norm': norms[:, 2],
               'opt/scaled_grad_norm_sq': norms[:, 3]}
        return params, opt_state, e_loc, ratios, {**opt, **extra, **stats}


def merge_states_flat(ansatz, params, opt_state, merge_keys, phys_conf=None):
    """optimizer.py:227-249 on the device vectors: the elements of every module whose name contains one of `merge_keys` are
    replaced by their mean over the electronic states (torch, through Program.leaf_slices), and every context is re-packed
    from its merged theta.  Nothing happens for a single state, without keys, or without a device-resident state."""
    if not merge_keys or opt_state is None or len(params) < 2:
        return
    Rs = [None] if phys_conf is None else _unpack(phys_conf)[1]
    engines = [ansatz.engine(p, Rs[0]) for p in params]
    thetas = [st['theta'] for st in opt_state]
    touched = False
    for (mod, _), (sl, _) in engines[0].program.leaf_slices().items():
        if any(key in mod for key in merge_keys):
            mean = torch.stack([t[sl] for t in thetas]).mean(dim=0)
            for t in thetas:
                t[sl] = mean
            touched = True
    if touched:
        for eng, t in zip(engines, thetas):
            eng.set_params_flat(t)
