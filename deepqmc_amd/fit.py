"""The variational training loop (reference src/deepqmc/fit.py: `fit_wf` and its train step) on the device-resident
optimiser step: sample, `opt.step`, merge the electronic states, refresh the sampler's psi -- per step no parameter crosses
the host and the captured forward-Laplacian graphs of the contexts are replayed.  With an optimiser that carries a loss function
(loss.create_loss_fn) the loop keeps the reference's running averages of the states' energies (ewm.py) and hands them to the
loss as `data`.  With `observable_monitors` (deepqmc_amd/observable.py) the loop calls every monitor after the optimiser step
and the sampler update of a step, as the reference's loop does (fit.py:93-113), and merges what they return into the yielded
stats; without them nothing of this is constructed or called.
"""
from __future__ import annotations

import numpy as np
import torch

from .checkpoint import TrainState
from .ewm import init_multi_mol_multi_state_ewm
from .optimizer import merge_states_flat
from .types import Psi

__all__ = ['fit_wf', 'TrainState']


def _host_mean(x):
    """Sampler statistics arrive as nested lists over molecules / states of host floats."""
    return float(np.mean(np.asarray(x, np.float64)))


def _sampler_psi(smpl_state, mol):
    """Psi(sign, log) [1, S, B] of molecule `mol` from the state of MultiNuclearGeometrySampler over MultiElectronicStateSampler
    (or over a single-state sampler); None for a sampler state of another shape."""
    try:
        states = smpl_state['elec'][mol]
        states = [states] if isinstance(states, dict) else list(states)
        return Psi(torch.stack([st['psi'].sign for st in states])[None], torch.stack([st['psi'].log for st in states])[None])
    except (KeyError, IndexError, TypeError, AttributeError):
        return None


def fit_wf(rng, hamil, ansatz, opt, molecule_idx_sampler, sampler, steps, train_state, merge_keys, sync_every=None,
           observable_monitors=None):
    """fit.py:34-162 as a generator: one training step per element of `steps`, yielding
    `(step, TrainState(sampler, params, opt), mol_idxs, stats)`.

    `rng`: an integer seed (step k samples with rng * 1000003 + k, as pretrain does); `opt`: an optimiser of
    deepqmc_amd/optimizer.py (bound to `hamil` / `ansatz` here if it is not yet); `sampler.sample(rng, smpl_state, params,
    mol_idxs)` -> (smpl_state, phys_conf r[1, S, B, N, 3], stats) as MultiNuclearGeometrySampler over
    MultiElectronicStateSampler gives it; `train_state`: TrainState(sampler state, [parameter tree per electronic state],
    optimiser state or None).  `merge_keys`: module-name substrings whose parameters are averaged over the states after every
    step.  stats: the sampler's statistics (host floats), 'hamil/*' and 'local_energy/{mean,std,min,max}' and 'opt/*' (device
    tensors: reading them is the caller's synchronisation, the loop itself never waits for the device).

    The yielded parameter trees are the objects of `train_state.params` throughout -- they key the context cache -- and
    their leaves are brought up to date (NeuralNetworkWaveFunction.sync_params) every `sync_every` steps and when the
    generator finishes or is closed; in between they are stale and `ansatz.params_stale(tree)` says so.

    If `opt.loss_fn` is set (fit.py:115-160): running averages of 'local_energy/mean' and 'local_energy/std' per (molecule,
    state) are kept on the device, passed to the optimiser as data = {'energy_ewm', 'std_ewm'} [1, S] (NaN before the first
    update) and reported as 'energy/ewm', 'energy/ewm_error' and 'energy/std_ewm' (device tensors [1, S]); stats also
    carries the loss function's 'loss', 'overlap/pairwise/mean' and 'spin/*'.  Without a loss function nothing of this
    happens and the yielded stats are what they were.

    `observable_monitors`: a list of observable.ObservableMonitor.  They are finalized once with (hamil, ansatz); after the
    optimiser step and the sampler update of every step, monitor q is called with (step, seed * 131 + q, the updated params,
    the phys_conf of the step, the sampler's refreshed psi as Psi [1, S, B], e_loc [1, S, B], the ratios `opt.step` returned) and
    what it returns -- `name/mean`, `name/std`, `name/samples`, device tensors -- is merged into stats
    (observable.split_samples takes the samples out again).  The monitors work on the contexts' device-resident weights, so
    they are right between syncs too.  None: nothing is constructed or called; the keys and values are those above."""
    if hasattr(opt, 'bind') and (getattr(opt, 'hamil', None) is None or getattr(opt, 'ansatz', None) is None):
        opt.bind(hamil, ansatz)
    smpl_state, params, opt_state = train_state
    params = list(params)
    merge_keys = tuple(merge_keys) if merge_keys is not None else None
    if opt_state is None:
        opt_state = opt.init(rng, params, None)
    with_loss = getattr(opt, 'loss_fn', None) is not None
    ewm_state = update_ewm = None
    idx_cache = {}
    monitors = [m.finalize(hamil, ansatz) for m in observable_monitors] if observable_monitors else []
    try:
        for k, step in enumerate(steps):
            seed = int(rng) * 1000003 + k
            mol_idxs = molecule_idx_sampler.sample()
            smpl_state, phys_conf, smpl_stats = sampler.sample(seed, smpl_state, params, mol_idxs)
            data = {}
            if with_loss:
                if ewm_state is None:
                    r_ = phys_conf.r if hasattr(phys_conf, 'r') else phys_conf
                    # one batch of estimators [n_mols, 2, S]: row 0 the energies, row 1 their standard deviations (one update)
                    shape = (getattr(molecule_idx_sampler, 'n_mols', 1), 2, r_.shape[1])
                    ewm_state, update_ewm = init_multi_mol_multi_state_ewm(shape, device=r_.device)
                mol = int(np.asarray(mol_idxs).reshape(-1)[0])
                one_mol = ewm_state.mean.shape[0] == 1       # (then an update is the whole batch: no gather, no scatter)
                if not one_mol and mol not in idx_cache:     # one upload per molecule index, then no step copies anything from the host
                    idx_cache[mol] = torch.tensor([mol], dtype=torch.long, device=ewm_state.mean.device)
                idx = None if one_mol else idx_cache[mol]
                data = {'energy_ewm': ewm_state.mean[mol:mol + 1, 0], 'std_ewm': ewm_state.mean[mol:mol + 1, 1]}
            params, opt_state, e_loc, ratios, stats = opt.step(seed, params, opt_state, (phys_conf, None, data))
            if getattr(opt, 'changes_params', True):
                merge_states_flat(ansatz, params, opt_state, merge_keys, phys_conf)
                if hasattr(sampler, 'update'):      # psi of the walkers under the new parameters (fit.py:90-92)
                    smpl_state = sampler.update(smpl_state, params)
            e64 = e_loc.double()
            out = {k_: _host_mean(v) for k_, v in smpl_stats.items()}
            out.update({k_ if '/' in k_ or k_ == 'loss' else f'hamil/{k_}': v for k_, v in stats.items()})
            out.update({'local_energy/mean': e64.mean(dim=-1), 'local_energy/std': e64.std(dim=-1, unbiased=False),
                        'local_energy/min': e64.amin(dim=-1), 'local_energy/max': e64.amax(dim=-1)})
            if with_loss:
                ewm_state = update_ewm(torch.stack([out['local_energy/mean'], out['local_energy/std']], dim=1), ewm_state, idx)
                out.update({'energy/ewm': ewm_state.mean[mol:mol + 1, 0], 'energy/ewm_error': torch.sqrt(ewm_state.sqerr[mol:mol + 1, 0]),
                            'energy/std_ewm': ewm_state.mean[mol:mol + 1, 1]})
            if monitors:
                psi = _sampler_psi(smpl_state, int(np.asarray(mol_idxs).reshape(-1)[0]))
                for q, monitor in enumerate(monitors):
                    out.update(monitor(step, seed * 131 + q, params, phys_conf, psi, e_loc, ratios))
            if sync_every and (k + 1) % int(sync_every) == 0:
                for p in params:
                    ansatz.sync_params(p)
            yield step, TrainState(smpl_state, params, opt_state), mol_idxs, out
    finally:
        for p in params:
            ansatz.sync_params(p)
