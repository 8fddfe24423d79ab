"""Hellmann-Feynman forces on the nuclei (reference src/deepqmc/force.py), batched over walkers.

Every estimator returns the per-walker force as float64 [B, n_nuc, 3] on the device; averaging over walkers (and ranks) is
the caller's.  The per-walker arithmetic is one HIP kernel (dqmc_hf_force); its inputs come from the library:
grad_r log|psi| from the forward-Laplacian pass (dqmc_psi_grad, every ansatz, with the float32 -> float64 refinement) and
grad_R log|psi| from the coordinate reverse pass (dqmc_log_psi_grad_coords, the programs log_psi_vjp supports).

    f = evaluate_hf_force_ac_zvq(hamil, ansatz)
    F = f(params, phys_conf)                      # [B, n_nuc, 3]

Cartesian nuclear coordinates only (no coordinate_transform).  Hamiltonians with an effective core potential or a
pseudo-Hamiltonian are not supported by the estimators of this module (NotImplementedError): the reference's ZVQ family
rejects them, and the bare ECP force needs the gradient of the non-local term, which `deepqmc_amd.ecp_force` provides for
Gaussian-type ECPs (evaluate_hf_force_bare, evaluate_hf_force_ac_zb; they work with `antithetic_wrapper` below).  The AC-ZV
and AC-ZVZB estimators (the local energy of d psi / d R, make_zv_term_via_jvp) are not provided.

`evaluate_finite_difference_force` needs no derivative of psi and no restriction on the Hamiltonian: one launch displaces the
walkers with every nuclear coordinate (dqmc_fd_displace), the engine evaluates log|psi| and E_loc at the 3 n_nuc displaced
copies, and one launch forms the importance-weighted quotient (dqmc_fd_force).  The estimators that take `(e_loc, energy)`
accept `energy` as a float or as a device tensor; the latter never waits for the host (`_centred`).
"""
from __future__ import annotations

import torch

from .types import PhysicalConfiguration


def _split(phys_conf):
    if isinstance(phys_conf, PhysicalConfiguration):
        return phys_conf.r, phys_conf.R
    return phys_conf, None


def _check_hamil(hamil, name):
    if hamil.pot is not None:
        raise NotImplementedError(f'{name}: Hamiltonians with an effective core potential or a pseudo-Hamiltonian are not '
                                  'supported (the ZVQ family rejects them; the bare force needs the non-local ECP gradient)')


def _centred(eng, e_loc, energy):
    """(e_loc [B] in the engine's dtype, energy as a float) for the estimators with a zero-bias term.  A float `energy` crosses
    the C ABI by value.  A device tensor (what the observable monitors pass: the mean of e_loc) is subtracted from e_loc on the
    device instead, in float64, so that nothing waits for the host; the kernel then sees energy 0.  In a float64 context the two
    ways are bit-identical; in a float32 one the centred energies are rounded to float32 once."""
    e_loc = eng._t(e_loc).reshape(-1)
    if isinstance(energy, torch.Tensor):
        return (e_loc.double() - energy.to(e_loc.device).double()).to(eng.dtype), 0.0
    return e_loc, float(energy)


def nuclear_force(R, phys_conf, nuclear_charges):
    """force.py nuclear_force: -grad_R of the nuclear repulsion, F_I = sum_{J != I} Z_I Z_J (R_I - R_J) / |R_I - R_J|^3, for every
    walker of phys_conf ([B, n_nuc, 3] float64; the same row for each walker).  A geometry-only term of n_nuc^2 pairs."""
    r, _ = _split(phys_conf)
    r = torch.as_tensor(r)
    R = torch.as_tensor(R, dtype=torch.float64, device=r.device)
    R = R[0] if R.dim() == 3 else R
    Z = torch.as_tensor(nuclear_charges, dtype=torch.float64, device=r.device)
    d = R[:, None, :] - R[None, :, :]
    dist = d.norm(dim=-1) + torch.eye(len(Z), dtype=torch.float64, device=r.device)     # (diagonal: d = 0)
    f = ((Z[:, None] * Z[None, :] / dist ** 3)[..., None] * d).sum(1)
    return f[None].expand(r.shape[0], -1, -1).contiguous()


def Q(r, R, c):
    """force.py Q (Assaraf-Caffarel 2003): Q_I = c_I sum_i (r_i - R_I) / |r_i - R_I| per walker, [B, n_nuc, 3] float64."""
    r = torch.as_tensor(r).double()
    R = torch.as_tensor(R, dtype=torch.float64, device=r.device)
    R = R[0] if R.dim() == 3 else R
    c = torch.as_tensor(c, dtype=torch.float64, device=r.device)
    d = r[:, None, :, :] - R[None, :, None, :]                    # [B, n_nuc, N, 3]
    return c[None, :, None] * (d / d.norm(dim=-1, keepdim=True)).sum(2)


def make_grad_nuc_log_wf(wf):
    """force.py make_grad_nuc_log_wf: f(params, phys_conf) -> d log|psi| / d R per walker, [B, n_nuc, 3] float64.
    Independent of the Hamiltonian (ECP Hamiltonians included); the programs log_psi_vjp supports (a TransPsiformer: a wave
    function made with `nuclear_coords=True`)."""

    def grad_nuc_log_wf(params, phys_conf):
        r, R = _split(phys_conf)
        eng = wf.engine(params, R)
        if eng.program.grad_unsupported:
            raise NotImplementedError(f'make_grad_nuc_log_wf: unsupported for this program ({eng.program.grad_unsupported})')
        if eng.program.nuclear_stream is not None and not eng.nuclear_coords:
            raise NotImplementedError(f'make_grad_nuc_log_wf: {eng.program.PER_WALKER_NUCLEAR}')
        return eng.log_psi_grad_coords(r, R, want_r=False)[3].double()

    return grad_nuc_log_wf


def _estimator(hamil, wf, est, *, takes_rng, needs_energy):
    _check_hamil(hamil, f'evaluate_hf_force_{est}')
    zvq = est in ('ac_zvq', 'ac_zvzbq', 'ac_zvqzb')
    nuc = est in ('ac_zb', 'ac_zvqzb')

    def force(params, phys_conf, e_loc=None, energy=None):
        r, R = _split(phys_conf)
        eng = wf.engine(params, R)
        r = eng._t(r)
        grad_r = grad_R = None
        if zvq:
            grad_r = eng.psi_and_grad(r, R)[2].contiguous()
        if nuc:
            if eng.program.grad_unsupported:
                raise NotImplementedError(f'evaluate_hf_force_{est}: unsupported for this program ({eng.program.grad_unsupported})')
            if eng.program.nuclear_stream is not None and not eng.nuclear_coords:
                raise NotImplementedError(f'evaluate_hf_force_{est}: {eng.program.PER_WALKER_NUCLEAR}')
            grad_R = eng.log_psi_grad_coords(r, R, want_r=False)[3]
        if needs_energy:
            e_loc, energy = _centred(eng, e_loc, energy)
        return eng.hf_force(est, r, R, grad_r=grad_r, grad_R=grad_R, e_loc=e_loc if needs_energy else None,
                            energy=energy if needs_energy else 0.0)

    if takes_rng and needs_energy:
        f = lambda rng, params, phys_conf, e_loc, energy: force(params, phys_conf, e_loc, energy)
    elif takes_rng:
        f = lambda rng, params, phys_conf: force(params, phys_conf)
    elif needs_energy:
        f = lambda params, phys_conf, e_loc, energy: force(params, phys_conf, e_loc, energy)
    else:
        f = lambda params, phys_conf: force(params, phys_conf)
    f.takes_rng, f.needs_energy, f.estimator = takes_rng, needs_energy, est
    return f


def evaluate_hf_force_bare(hamil, wf):
    """force.py evaluate_hf_force_bare (all-electron): f(rng, params, phys_conf) -> F_nuc + Z_I sum_i (r_i - R_I) / |r_i - R_I|^3."""
    return _estimator(hamil, wf, 'bare', takes_rng=True, needs_energy=False)


def evaluate_hf_force_ac_zvq(hamil, wf):
    """force.py evaluate_hf_force_ac_zvq: f(params, phys_conf) -> F_nuc + grad_r log|psi| . grad_r Q_I (every ansatz)."""
    return _estimator(hamil, wf, 'ac_zvq', takes_rng=False, needs_energy=False)


def evaluate_hf_force_ac_zvzbq(hamil, wf):
    """force.py evaluate_hf_force_ac_zvzbq: f(params, phys_conf, e_loc, energy) -> AC-ZVQ - 2 (e_loc - energy) Q_I."""
    return _estimator(hamil, wf, 'ac_zvzbq', takes_rng=False, needs_energy=True)


def evaluate_hf_force_ac_zb(hamil, wf):
    """force.py evaluate_hf_force_ac_zb: f(rng, params, phys_conf, e_loc, energy) -> bare - 2 (e_loc - energy) d log|psi| / d R_I."""
    return _estimator(hamil, wf, 'ac_zb', takes_rng=True, needs_energy=True)


def evaluate_hf_force_ac_zvqzb(hamil, wf):
    """AC-ZVQ with the zero-bias term of AC-ZB: f(params, phys_conf, e_loc, energy) -> AC-ZVQ - 2 (e_loc - energy) d log|psi| / d R_I.
    (No function of this name in the reference: its zero-variance part is AC-ZVQ's, its zero-bias part AC-ZB's.)"""
    return _estimator(hamil, wf, 'ac_zvqzb', takes_rng=False, needs_energy=True)


def evaluate_finite_difference_force(hamil, wf, step_size):
    """force.py evaluate_finite_difference_force: f(rng, params, phys_conf, e_loc, energy=None, return_parts=False) ->
    [B, n_nuc, 3] float64, the one force estimator that needs no derivative of psi.  For every displacement d = (n0, j0) of the
    D = 3 n_nuc nuclear coordinates, with the reference's signs (formulas at dqmc_fd_displace in include/dqmc.h):

        R_d = R - h e_(n0, j0),   r_d[b, e, j0] = r[b, e, j0] + h w[b, n0, e],   w = softmax_n(-|R_n - r_be|)
        F[b, n0, j0] = exp(2 (log|psi|(r_d, R_d) - log|psi|(r, R))) (E_loc(r_d, R_d) - e_loc[b]) / h

    One launch forms all displaced copies (dqmc_fd_displace, w in float64), D value evaluations and D local-energy calls of the
    engine follow -- `wf.engine(params, R_d)`, so ansatzes that fold the geometry get a context per displaced geometry, and
    the same `rng` keys the ECP quadrature of every displaced call -- and one launch forms the quotient (dqmc_fd_force).
    `energy` is accepted for uniformity and unused.  Hamiltonians with an ECP or a pseudo-Hamiltonian are evaluated as
    `hamil.local_energy` evaluates them.  return_parts: (F, (r_d [D, B, N, 3], R_d [D, n_nuc, 3], log_d [D, B], e_d [D, B])).

    The quotient divides the error of E_loc by h: with float32 local energies (relative error ~1e-5 after the refinement)
    and h = 1e-3 the per-walker force carries an error of order 1e-2 |E_loc|.  A float64 context is what the estimator is
    meant for."""
    h = float(step_size)
    n_nuc = hamil.n_nuc

    def force(rng, params, phys_conf, e_loc, energy=None, return_parts=False):
        r, R = _split(phys_conf)
        eng = wf.engine(params, R)
        r, Rt, B = eng._walkers(r, R)
        r_d, R_d = eng.fd_displace(r, Rt, h)
        log_0 = eng.wf_eval(r, Rt)[1]
        log_d = torch.empty(3 * n_nuc, B, dtype=eng.dtype, device=eng.device)
        e_d = torch.empty_like(log_d)
        for d in range(3 * n_nuc):
            eng_d = wf.engine(params, R_d[d])
            log_d[d] = eng_d.wf_eval(r_d[d], R_d[d])[1]
            e_d[d] = eng_d.local_energy(PhysicalConfiguration(R_d[d], r_d[d], None), rng=rng)[0]
        F = eng.fd_force(log_d, log_0, e_d, eng._t(e_loc).reshape(-1), h)
        return (F, (r_d, R_d, log_d, e_d)) if return_parts else F

    force.takes_rng, force.needs_energy, force.estimator = True, True, 'finite_difference'
    return force


def antithetic_sampler(phys_conf, r_cut, R=None):
    """force.py antithetic_sampler: (phys_conf, mirrored) where every electron within r_cut of its nearest nucleus is reflected
    through that nucleus.  Works on [B, N, 3] device tensors (R from phys_conf, else `R`)."""
    r, R0 = _split(phys_conf)
    r = torch.as_tensor(r)
    R = torch.as_tensor(R0 if R0 is not None else R, dtype=r.dtype, device=r.device)
    R = R[0] if R.dim() == 3 else R
    d = r[:, :, None, :] - R[None, None, :, :]                    # [B, N, n_nuc, 3]
    d2 = (d * d).sum(-1)
    idx = d2.argmin(-1)
    near = torch.gather(d, 2, idx[..., None, None].expand(-1, -1, 1, 3))[:, :, 0]
    mask = (torch.gather(d2, 2, idx[..., None])[..., 0] < r_cut ** 2)[..., None]
    r_ = r - 2 * near * mask
    if isinstance(phys_conf, PhysicalConfiguration):
        return phys_conf, PhysicalConfiguration(phys_conf.R, r_, phys_conf.mol_idx)
    return r, r_


def antithetic_wrapper(evaluate_force, wf, r_cut):
    """force.py antithetic_wrapper: f(rng, params, phys_conf) -> the average of `evaluate_force` at phys_conf and at its
    antithetic mirror, weighted by softmax(0, 2 (log|psi(mirror)| - log|psi|)).  Only estimators that take no local energy
    (evaluate_hf_force_bare, evaluate_hf_force_ac_zvq), as in the reference."""
    if getattr(evaluate_force, 'needs_energy', False):
        raise ValueError('antithetic_wrapper: only estimators that do not take the local energy (bare, AC-ZVQ)')
    takes_rng = getattr(evaluate_force, 'takes_rng', True)

    def evaluate_force_antithetic(rng, params, phys_conf):
        pc, pc_ = antithetic_sampler(phys_conf, r_cut, R=wf.hamil.mol.coords)
        log = wf(params, pc).log.double()
        log_ = wf(params, pc_).log.double()
        w = torch.softmax(torch.stack((torch.zeros_like(log), 2 * (log_ - log))), 0)
        call = (lambda c: evaluate_force(rng, params, c)) if takes_rng else (lambda c: evaluate_force(params, c))
        f, f_ = call(pc), call(pc_)
        return w[0][:, None, None] * f + w[1][:, None, None] * f_

    return evaluate_force_antithetic


__all__ = ['nuclear_force', 'Q', 'make_grad_nuc_log_wf', 'evaluate_hf_force_bare', 'evaluate_hf_force_ac_zvq',
           'evaluate_hf_force_ac_zvzbq', 'evaluate_hf_force_ac_zb', 'evaluate_hf_force_ac_zvqzb', 'evaluate_finite_difference_force',
           'antithetic_sampler',
           'antithetic_wrapper']
