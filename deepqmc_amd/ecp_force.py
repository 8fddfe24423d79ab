"""Hellmann-Feynman forces on the nuclei for Hamiltonians with a Gaussian-type effective core potential (reference
src/deepqmc/force.py:286-299 with hamil.pot.grad_nonloc_potential, ecp/gaussian_type_ecp.py:257-330, ecp/ecp_force_utils.py),
batched over walkers.  The all-electron estimators live in `deepqmc_amd.force`, which refuses ECP Hamiltonians.

Per walker, float64 [B, n_nuc, 3] on the device, with Z the valence charges `hamil.ns_valence`:

    F_I = F_nuc,I(Z)  -  dV_loc/dR_I  -  G_I

V_loc is the -Z_I / rho attraction plus the local r^-1, r^0, r^1 Gaussians of the masked nuclei; G is the gradient of the
non-local term, assembled from the psi ratios of the 12-point quadrature and d log|psi| / dr, d log|psi| / dR at the quadrature
configurations (one coordinate reverse pass per walker chunk; formulas at dqmc_ecp_force in include/dqmc.h).  All of it runs
in the HIP library (csrc/kernels_ecp.hip, csrc/engine_ecp_force.inl).

    f = evaluate_hf_force_bare(hamil, ansatz)
    F = f(rng, params, phys_conf)                 # [B, n_nuc, 3]; rng: the int seed of the quadrature rotation

rows='own' (default) keeps, for each non-local nucleus I, only row I of the ratio gradient -- what the reference computes
(`wf_ratio_grad[:, nucleus_index, :]`); rows='all' keeps every row, the full dV_nl/dR, at no extra cost.

Differences from the reference, on purpose:
  * the reference stores the row of the j-th non-local nucleus at row j, which is right only when every nucleus has a non-local
    channel; here it is stored at row nuc_with_nl_pot[j];
  * the reference's gradient path draws one rotation angle for all (nucleus, electron) pairs of a call; here the angle is keyed
    exactly as in the local energy (the seed `rng`, or explicit `ecp_phi` [B, n_nl, N]), so the same seed gives the vertices
    of the E_loc call;
  * Cartesian nuclear coordinates only;
  * the derivative of the quadrature frame is singular for an electron on the z axis through a nucleus, as the reference's
    autograd is; it is not special-cased.
Pseudo-Hamiltonians are not supported (NotImplementedError).
"""
from __future__ import annotations

from . import force as _force
from .force import _split


def _check_hamil(hamil, name):
    pot = getattr(hamil, 'pot', None)
    if pot is None:
        raise NotImplementedError(f'{name}: an all-electron Hamiltonian has no effective core potential; use deepqmc_amd.force')
    if hasattr(pot, 'rv_l2'):
        raise NotImplementedError(f'{name}: pseudo-Hamiltonians are not supported, only Gaussian-type effective core potentials')


def _call(wf, est, rows, rng, params, phys_conf, ecp_phi=None, e_loc=None, energy=0.0, return_parts=False):
    r, R = _split(phys_conf)
    eng = wf.engine(params, R)
    if est == 'ac_zb':
        e_loc, energy = _force._centred(eng, e_loc, energy)      # (a device-tensor energy is subtracted on the device)
    return eng.ecp_force(est, r, R, rng=rng, ecp_phi=ecp_phi, e_loc=e_loc, energy=float(energy), rows=rows,
                         return_parts=return_parts)


def evaluate_hf_force_bare(hamil, wf, rows='own'):
    """force.py evaluate_hf_force_bare for a Gaussian-type ECP: f(rng, params, phys_conf, ecp_phi=None) ->
    F_nuc - dV_loc/dR - G per walker."""
    _check_hamil(hamil, 'evaluate_hf_force_bare')

    def f(rng, params, phys_conf, ecp_phi=None):
        return _call(wf, 'bare', rows, rng, params, phys_conf, ecp_phi)

    f.takes_rng, f.needs_energy, f.estimator = True, False, 'bare'
    return f


def evaluate_hf_force_ac_zb(hamil, wf, rows='own'):
    """force.py evaluate_hf_force_ac_zb for a Gaussian-type ECP: f(rng, params, phys_conf, e_loc, energy, ecp_phi=None) ->
    bare - 2 (e_loc - energy) d log|psi| / dR_I, the gradient from the same reverse pass."""
    _check_hamil(hamil, 'evaluate_hf_force_ac_zb')

    def f(rng, params, phys_conf, e_loc, energy, ecp_phi=None):
        return _call(wf, 'ac_zb', rows, rng, params, phys_conf, ecp_phi, e_loc, energy)

    f.takes_rng, f.needs_energy, f.estimator = True, True, 'ac_zb'
    return f


def grad_nonloc_potential(hamil, wf, rows='own'):
    """gaussian_type_ecp.py grad_nonloc_potential: f(rng, params, phys_conf, ecp_phi=None) -> +G per walker, [B, n_nuc, 3]."""
    _check_hamil(hamil, 'grad_nonloc_potential')

    def f(rng, params, phys_conf, ecp_phi=None):
        return -_call(wf, 'bare', rows, rng, params, phys_conf, ecp_phi, return_parts=True)[1][1]

    return f


def grad_local_potential(hamil, wf):
    """f(params, phys_conf) -> dV_loc/dR per walker, [B, n_nuc, 3]: the gradient of the -Z/rho attraction and of the local
    ECP terms (gaussian_type_ecp.py:127-159).  Taken from the force call (the first part minus the nuclear repulsion force),
    so it costs what that call costs."""
    _check_hamil(hamil, 'grad_local_potential')

    def f(params, phys_conf):
        part0 = _call(wf, 'bare', 'own', 0, params, phys_conf, return_parts=True)[1][0]
        return _force.nuclear_force(hamil.mol.coords if _split(phys_conf)[1] is None else _split(phys_conf)[1], phys_conf,
                                    hamil.ns_valence) - part0

    return f


__all__ = ['evaluate_hf_force_bare', 'evaluate_hf_force_ac_zb', 'grad_nonloc_potential', 'grad_local_potential']
