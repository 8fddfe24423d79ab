"""Observable monitors of the training loop (reference src/deepqmc/observable.py): objects that `fit.fit_wf` calls after every
step with the walkers, the updated parameters, psi, the local energies and the psi ratios of the step, and that return
`name/mean`, `name/std` (and `name/samples`) every `period` steps.

    monitors = [SpinMonitor(False, 10), ACZVQForceMonitor(False, 10), OscillatorStrengthMonitor(False, 1)]
    for step, state, mol_idxs, stats in fit_wf(..., observable_monitors=monitors):
        samples, stats = split_samples(stats)

Shapes are this package's: `phys_conf.r` is [1, S, B, N, 3] (one molecule, S electronic states, B walkers per state), `params` one
parameter tree per state, `psi` a Psi of [1, S, B] tensors, `local_energy` [1, S, B], `psi_ratios` [1, S, S, B] or None.
Samples are [1, S, B, ...], statistics [1, S, ...]: float64 device tensors (the std is the population std, as jnp.std).  `rng`
is an integer seed.  Nothing in a monitor waits for the host: reading a statistic is the caller's synchronisation.

Every monitor that evaluates something obtains its HIP context through `wf.engine(params[s], R)` and so works on the context's
device-resident weights: on the device path of `fit_wf` the leaves of the parameter trees are stale between syncs and are
never read here.

The states are a host loop over contexts, as everywhere in this package.  Cartesian nuclear coordinates only (no
`coordinate_transform`), one molecule per batch, one process.  The AC-ZV and AC-ZVZB monitors are not provided: their ZV term is
the local energy of d psi / dR, which is not built (`observable_monitor_from_name` says so).
"""
from __future__ import annotations

import torch

from . import ecp_force as _ecp_force
from . import force as _force
from .loss import _single_process, _unpack
from .physics import evaluate_spin
from .types import PhysicalConfiguration

__all__ = ['ObservableMonitor', 'ElectronPositionMonitor', 'NuclearPositionMonitor', 'WaveFunctionMonitor', 'EnergyMonitor',
           'PsiRatioMonitor', 'SpinMonitor', 'BareForceMonitor', 'BareForceAntiMonitor', 'ACZVQForceMonitor', 'ACZVQForceAntiMonitor',
           'ACZVZBQForceMonitor', 'ACZBForceMonitor', 'ACZVQZBForceMonitor', 'FiniteDifferenceForceMonitor',
           'OscillatorStrengthMonitor', 'default_observable_monitors', 'observable_monitor_from_name', 'split_samples',
           'compute_mean_and_std']


def compute_mean_and_std(name, observable_samples, axis=2):
    """observable.py:60-66: {name/mean, name/std} over `axis` (the population std) in float64."""
    x = observable_samples.double()
    return {f'{name}/mean': x.mean(dim=axis), f'{name}/std': x.std(dim=axis, unbiased=False)}


def split_samples(stats):
    """(samples, stats): the `*/samples` entries of a stats dict of `fit_wf` apart from the statistics."""
    samples = {k: v for k, v in stats.items() if k.endswith('/samples')}
    return samples, {k: v for k, v in stats.items() if k not in samples}


def _gaussian_ecp(hamil):
    pot = getattr(hamil, 'pot', None)
    return pot is not None and not hasattr(pot, 'rv_l2')


def _one_molecule(phys_conf):
    """(r [S, B, N, 3], R [n_nuc, 3] or None) of a batch of one molecule."""
    r, Rs = _unpack(phys_conf)
    if r.shape[0] != 1:
        raise ValueError('observable monitors take one molecule per batch')
    return r[0], Rs[0]


class ObservableMonitor:
    """observable.py:69-190.  Subclasses set `name` and build `observable_fn(rng, params_s, phys_conf_s[, e_loc_s, energy_s]) ->
    [B, ...]` in `finalize`; `requires_energy` says which of the two signatures it has."""

    name: str
    observable_fn = None
    requires_energy = False

    def __init__(self, save_samples: bool, period: int):
        assert period > 0
        self.save_samples, self.period = save_samples, period
        self.hamil = self.wf = None

    def finalize(self, hamil, wf):
        """Bind the monitor to the Hamiltonian and the wave function (once, before the loop); returns self."""
        self.hamil, self.wf = hamil, wf
        return self

    def compute_observable(self, rng, params, phys_conf, psi, local_energy, psi_ratios):
        """-> (samples [1, S, B, ...], {name/mean, name/std} [1, S, ...]).  State s is evaluated on its own walkers with its own
        parameters; estimators that take the energy get local_energy[0, s] and its mean (a device tensor)."""
        assert self.observable_fn is not None, 'call ObservableMonitor.finalize first'
        r, R = _one_molecule(phys_conf)
        rows = []
        for s in range(r.shape[0]):
            rs = r[s].contiguous()
            pc = PhysicalConfiguration(R, rs, None) if R is not None else rs
            if self.requires_energy:
                e = local_energy[0, s]
                rows.append(self.observable_fn(rng, params[s], pc, e, e.double().mean()))
            else:
                rows.append(self.observable_fn(rng, params[s], pc))
        samples = torch.stack(rows)[None].double()
        return samples, compute_mean_and_std(self.name, samples, axis=2)

    def __call__(self, step, rng, params, phys_conf, psi, local_energy, psi_ratios):
        """The statistics of this step, or {} on steps that are no multiple of `period`."""
        if self.wf is None:
            raise RuntimeError(f'{type(self).__name__}: call ObservableMonitor.finalize(hamil, wf) first')
        if step % self.period:
            return {}
        samples, stats = self.compute_observable(rng, params, phys_conf, psi, local_energy, psi_ratios)
        stats = dict(stats)
        if self.save_samples and samples is not None:
            stats[f'{self.name}/samples'] = samples
        return stats


def _no_rng(fn):
    """observable.py rng_wrapper: an estimator that takes no seed, behind the signature of one that does."""
    return lambda rng, *args: fn(*args)


class SpinMonitor(ObservableMonitor):
    """<S^2> from the swapped configurations (physics.evaluate_spin)."""

    name = 'spin'

    def finalize(self, hamil, wf):
        self.observable_fn = _no_rng(evaluate_spin(hamil, wf))
        return super().finalize(hamil, wf)


class _ForceMonitor(ObservableMonitor):
    """Base of the Hellmann-Feynman force monitors: `evaluate_hf_force(hamil, wf)` builds the estimator, samples [1, S, B, n_nuc, 3]."""

    def finalize(self, hamil, wf):
        self.observable_fn = self.evaluate_hf_force(hamil, wf)
        return super().finalize(hamil, wf)

    @staticmethod
    def evaluate_hf_force(hamil, wf):
        raise NotImplementedError


def _refuse_ecp(hamil, what):
    if getattr(hamil, 'pot', None) is not None:      # observable.py:361: assert not jnp.any(hamil.ecp_mask)
        raise NotImplementedError(f'{what}: not defined for Hamiltonians with an effective core potential; the bare and AC-ZB '
                                  'monitors are')


class BareForceMonitor(_ForceMonitor):
    """The bare estimator; Hamiltonians with a Gaussian-type ECP are routed to deepqmc_amd.ecp_force."""

    name = 'hf_force_bare'

    @staticmethod
    def evaluate_hf_force(hamil, wf):
        return (_ecp_force if _gaussian_ecp(hamil) else _force).evaluate_hf_force_bare(hamil, wf)


class BareForceAntiMonitor(BareForceMonitor):
    """The bare estimator averaged with its antithetic mirror (force.antithetic_wrapper)."""

    name = 'hf_force_bare_anti'

    def __init__(self, save_samples: bool, period: int, cutoff: float = 0.3):
        super().__init__(save_samples, period)
        self.cutoff = cutoff

    def finalize(self, hamil, wf):
        self.observable_fn = _force.antithetic_wrapper(self.evaluate_hf_force(hamil, wf), wf, self.cutoff)
        return ObservableMonitor.finalize(self, hamil, wf)


class ACZBForceMonitor(_ForceMonitor):
    """AC-ZB; Hamiltonians with a Gaussian-type ECP are routed to deepqmc_amd.ecp_force."""

    name = 'hf_force_ac_zb'
    requires_energy = True

    @staticmethod
    def evaluate_hf_force(hamil, wf):
        return (_ecp_force if _gaussian_ecp(hamil) else _force).evaluate_hf_force_ac_zb(hamil, wf)


class ACZVQForceMonitor(_ForceMonitor):
    """AC-ZVQ; refuses Hamiltonians with an ECP."""

    name = 'hf_force_ac_zvq'

    def finalize(self, hamil, wf):
        _refuse_ecp(hamil, type(self).__name__)
        return super().finalize(hamil, wf)

    @staticmethod
    def evaluate_hf_force(hamil, wf):
        return _no_rng(_force.evaluate_hf_force_ac_zvq(hamil, wf))


class ACZVQForceAntiMonitor(ACZVQForceMonitor):
    """AC-ZVQ averaged with its antithetic mirror; refuses Hamiltonians with an ECP."""

    name = 'hf_force_ac_zvq_anti'

    def __init__(self, save_samples: bool, period: int, cutoff: float = 0.3):
        super().__init__(save_samples, period)
        self.cutoff = cutoff

    def finalize(self, hamil, wf):
        _refuse_ecp(hamil, type(self).__name__)
        self.observable_fn = _force.antithetic_wrapper(_force.evaluate_hf_force_ac_zvq(hamil, wf), wf, self.cutoff)
        return ObservableMonitor.finalize(self, hamil, wf)


class ACZVZBQForceMonitor(ACZVQForceMonitor):
    """AC-ZVZBQ; refuses Hamiltonians with an ECP."""

    name = 'hf_force_ac_zvzbq'
    requires_energy = True

    @staticmethod
    def evaluate_hf_force(hamil, wf):
        return _no_rng(_force.evaluate_hf_force_ac_zvzbq(hamil, wf))


class ACZVQZBForceMonitor(ACZVQForceMonitor):
    """AC-ZVQ with the zero-bias term of AC-ZB; refuses Hamiltonians with an ECP."""

    name = 'hf_force_ac_zvqzb'
    requires_energy = True

    @staticmethod
    def evaluate_hf_force(hamil, wf):
        return _no_rng(_force.evaluate_hf_force_ac_zvqzb(hamil, wf))


class FiniteDifferenceForceMonitor(ObservableMonitor):
    """force.evaluate_finite_difference_force with step `h`: 3 n_nuc value and local-energy evaluations per call."""

    name = 'finite_difference_force'
    requires_energy = True

    def __init__(self, save_samples: bool, period: int, h: float = 1e-3):
        super().__init__(save_samples, period)
        self.h = h

    def finalize(self, hamil, wf):
        self.observable_fn = _force.evaluate_finite_difference_force(hamil, wf, self.h)
        return super().finalize(hamil, wf)


class EnergyMonitor(ObservableMonitor):
    """observable.py:459-480: mean, std, min and max of the local energies -- the four keys and values `fit_wf` reports."""

    name = 'local_energy'

    def compute_observable(self, rng, params, phys_conf, psi, local_energy, psi_ratios):
        e64 = local_energy.double()
        return e64, {f'{self.name}/mean': e64.mean(dim=-1), f'{self.name}/std': e64.std(dim=-1, unbiased=False),
                     f'{self.name}/min': e64.amin(dim=-1), f'{self.name}/max': e64.amax(dim=-1)}


class PsiRatioMonitor(ObservableMonitor):
    """The ratios the loss returned, [1, S, S, B]: samples only."""

    name = 'psi_ratio'

    def compute_observable(self, rng, params, phys_conf, psi, local_energy, psi_ratios):
        assert psi_ratios is not None, 'PsiRatioMonitor needs the psi ratios of a multi-state loss'
        return psi_ratios.double(), {}


class ElectronPositionMonitor(ObservableMonitor):
    """The walkers, [1, S, B, N, 3]: samples only."""

    name = 'r'

    def compute_observable(self, rng, params, phys_conf, psi, local_energy, psi_ratios):
        return _unpack(phys_conf)[0].double(), {}


class NuclearPositionMonitor(ObservableMonitor):
    """The geometry of every state's walkers, [1, S, n_nuc, 3]: samples only."""

    name = 'R'

    def compute_observable(self, rng, params, phys_conf, psi, local_energy, psi_ratios):
        r, R = _one_molecule(phys_conf)
        R = torch.as_tensor(self.hamil.mol.coords if R is None else R, device=r.device).double()
        return R[None, None].expand(1, r.shape[0], -1, -1).contiguous(), {}


class WaveFunctionMonitor(ObservableMonitor):
    """The sampler's psi, {'sign', 'log'} of [1, S, B]: samples only."""

    name = 'psi'

    def compute_observable(self, rng, params, phys_conf, psi, local_energy, psi_ratios):
        return {'sign': psi.sign.double(), 'log': psi.log.double()}, {}


class OscillatorStrengthMonitor(ObservableMonitor):
    """observable.py:556-605 in two launches (Engine.oscillator_strength, dqmc_oscillator_strength): `oscillator_strength/mean`
    and `oscillator_strength/err`, [1, S, S]; no samples.  Needs the psi ratios of a multi-state loss."""

    name = 'oscillator_strength'

    def compute_observable(self, rng, params, phys_conf, psi, local_energy, psi_ratios):
        if psi_ratios is None:
            raise ValueError('OscillatorStrengthMonitor needs the psi ratios of a multi-state loss (psi_ratios is None)')
        _single_process('OscillatorStrengthMonitor')
        r, R = _one_molecule(phys_conf)
        eng = self.wf.engine(params[0], R)
        os_mean, os_err, _, _ = eng.oscillator_strength(r, psi_ratios[0].contiguous(), local_energy[0])
        return None, {f'{self.name}/mean': os_mean[None], f'{self.name}/err': os_err[None]}


_MONITORS = (ElectronPositionMonitor, NuclearPositionMonitor, WaveFunctionMonitor, EnergyMonitor, SpinMonitor, PsiRatioMonitor,
             OscillatorStrengthMonitor, BareForceMonitor, BareForceAntiMonitor, ACZVQForceMonitor, ACZVQForceAntiMonitor,
             ACZBForceMonitor, ACZVZBQForceMonitor, FiniteDifferenceForceMonitor, ACZVQZBForceMonitor)
_NOT_BUILT = ('hf_force_ac_zv', 'hf_force_ac_zvzb')


def default_observable_monitors():
    """observable.py:608-612."""
    return [WaveFunctionMonitor(save_samples=True, period=1)]


def observable_monitor_from_name(name):
    """observable.py:615-638: the monitor of that `name` with save_samples=True, period=1."""
    for monitor in _MONITORS:
        if monitor.name == name:
            return monitor(save_samples=True, period=1)
    if name in _NOT_BUILT:
        raise NotImplementedError(f'{name}: the ZV term (the local energy of d psi / dR, make_zv_term_via_jvp) is not built')
    raise ValueError(f'Unknown observable monitor: {name}')
