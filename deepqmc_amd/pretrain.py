"""Pretraining of the ansatz orbitals to (MC-)SCF orbitals (reference src/deepqmc/pretrain/pretraining.py,
pretraining_target.py, gto.py; train.py:194-251).

The SCF itself is not run here: the boundary is the reference's `dataset` dict, as `pyscfext.compute_scf_solution` returns
it wherever pyscf exists,

    dataset = {'centers': [n_nuc, 3], 'shells': [(atom, (l, coeffs, zetas)), ...], 'mo_coeffs': [M, n_ao, n_mo],
               'confs': [S, M, n_conf, N], 'conf_coeffs': [S, M, n_conf]}

with Cartesian GTO shells, one contraction each.  Target, loss and its parameter gradient are evaluated on the GPU
(include/dqmc.h: dqmc_set_pretrain_target, dqmc_pretrain_target, dqmc_pretrain_loss_grad); this module is the host loop:
one HIP context per electronic state, Adam on the haiku-shaped gradient trees, the generator `pretrain`.

    loss = mean((orb_up - T_up)^2) + mean((orb_dn - T_dn)^2)     over (molecule, state, walker, determinant, row, column)

One molecule per batch (M = 1), any number of states, a single process.
"""
from __future__ import annotations

import dataclasses
from typing import Sequence

import numpy as np
import torch

from .types import PhysicalConfiguration

L_MAX = 3


def get_cartesian_angulars(l: int):
    """gto.py:9-12: the order of the Cartesian components of a shell."""
    return [(lx, ly, l - lx - ly) for lx in range(l, -1, -1) for ly in range(l - lx, -1, -1)]


class GTOBasis:
    """A Cartesian GTO basis of a molecule (gto.py:39-74): validates `shells` = [(atom, (l, coeffs, zetas)), ...] against
    `centers` [n_nuc, 3] and keeps them in the form `Engine.set_pretrain_target` packs.  The orbitals are centred on the
    nuclei of the physical configuration they are evaluated at; `centers` is kept for reference only, as in the reference."""

    def __init__(self, centers, shells):
        self.centers = np.asarray(centers, np.float64).reshape(-1, 3)
        self.shells = []
        for atom, (l, coeffs, zetas) in shells:
            atom, l = int(atom), int(l)
            coeffs, zetas = np.asarray(coeffs, np.float64).reshape(-1), np.asarray(zetas, np.float64).reshape(-1)
            if not 0 <= atom < len(self.centers):
                raise ValueError(f'shell on atom {atom}: the molecule has {len(self.centers)} centers')
            if not 0 <= l <= L_MAX:
                raise ValueError(f'shell with l = {l}: angular momenta 0 .. {L_MAX} are supported')
            if coeffs.size != zetas.size or coeffs.size == 0:
                raise ValueError('a shell needs one contraction coefficient per exponent')
            self.shells.append((atom, (l, coeffs, zetas)))
        self.n_ao = sum((l + 1) * (l + 2) // 2 for _, (l, _, _) in self.shells)

    @classmethod
    def from_pyscf(cls, mol):
        """gto.py:55-74: (centers, shells) of a pyscf molecule with Cartesian GTOs (`mol.cart == True`)."""
        try:
            import pyscf  # noqa: F401
        except ImportError as e:
            raise ImportError('GTOBasis.from_pyscf needs pyscf; build the dataset where pyscf is installed and pass its '
                              "'centers' and 'shells' to GTOBasis / PretrainTarget") from e
        assert mol.cart
        shells = []
        for i in range(mol.nbas):
            for coeffs in mol.bas_ctr_coeff(i).T:
                shells.append((mol.bas_atom(i), (mol.bas_angular(i), coeffs, mol.bas_exp(i))))
        return mol.atom_coords(), shells


class PretrainTarget:
    """An (MC-)SCF wave function as pretraining target (pretraining_target.py:17-45).  `__call__(confs, conf_coeffs,
    phys_conf)` -> [B, n_conf, N, N] on the GPU: the molecular orbitals of every configuration, the CI coefficient folded
    into the orbitals of its determinant.  confs [M, n_conf, N], conf_coeffs [M, n_conf], mo_coeffs [M, n_ao, n_mo]; the
    molecule is `phys_conf.mol_idx` (0 without one)."""

    def __init__(self, hamil, n_determinants, centers, shells, mo_coeffs, *, dtype=torch.float64, device='cuda', lib=None):
        self.hamil, self.n_determinants = hamil, n_determinants
        self.basis = GTOBasis(centers, shells)
        self.mo_coeffs = np.asarray(mo_coeffs, np.float64)
        if self.mo_coeffs.ndim == 2:
            self.mo_coeffs = self.mo_coeffs[None]
        if self.mo_coeffs.shape[1] != self.basis.n_ao:
            raise ValueError(f'mo_coeffs has {self.mo_coeffs.shape[1]} rows, the basis {self.basis.n_ao} atomic orbitals')
        self.dtype, self.device, self._lib = dtype, device, lib
        self._engine = None

    def upload(self, eng, confs, conf_coeffs, mol_idx=0):
        eng.set_pretrain_target(self.basis.shells, self.mo_coeffs[mol_idx], np.asarray(confs)[mol_idx], np.asarray(conf_coeffs)[mol_idx])

    def __call__(self, confs, conf_coeffs, phys_conf):
        from .engine import Engine
        from .params import init_params
        from .spec import ANSATZES
        r = phys_conf.r if isinstance(phys_conf, PhysicalConfiguration) else phys_conf
        R = phys_conf.R if isinstance(phys_conf, PhysicalConfiguration) else None
        mol_idx = getattr(phys_conf, 'mol_idx', None)
        m = 0 if mol_idx is None else int(torch.as_tensor(mol_idx).reshape(-1)[0])
        if self._engine is None:     # the target kernel belongs to a context; this one is only its host (smallest ansatz, never evaluated)
            h = self.hamil
            spec = dataclasses.replace(ANSATZES['paulinet'](), embedding_dim=8, n_interactions=1, n_determinants=1)
            self._engine = Engine(spec, h, init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=0), dtype=self.dtype,
                                  device=self.device, lib=self._lib)
        self.upload(self._engine, confs, conf_coeffs, m)
        t = self._engine.pretrain_target(r, R)
        return t if self.n_determinants is None else t[:, :self.n_determinants]


def pretrain_loss_and_grad(wf, params: Sequence, phys_conf_r, dataset, target_fn=None):
    """The loss of pretraining.py:66-95 and its gradient, per electronic state: returns (loss, [grad tree per state],
    per_sample_losses [1, S, B] float64).  `params`: one parameter tree per state; `phys_conf_r`: r[1, S, B, N, 3] or a
    PhysicalConfiguration of it.  State s evaluates `dqmc_pretrain_loss_grad` in its own context with n_total = M S B, so the
    per-state gradients are those of the one loss over all states.  The target table is uploaded into every context that does
    not hold it yet (contexts are cached and evicted by `wf.engine`)."""
    from .loss import _unpack
    r, Rs = _unpack(phys_conf_r)
    M, S, B = r.shape[:3]
    if M != 1:
        raise NotImplementedError('pretraining takes one molecule per batch (M = 1)')
    if len(params) != S:
        raise ValueError(f'{len(params)} parameter trees for {S} electronic states')
    if not wf.spec.full_determinant:
        raise NotImplementedError('pretraining: only full-determinant programs expose their orbital matrices')
    if target_fn is None:
        target_fn = PretrainTarget(wf.hamil, None, dataset['centers'], dataset['shells'], dataset['mo_coeffs'])
    confs, conf_coeffs = np.asarray(dataset['confs']), np.asarray(dataset['conf_coeffs'])
    if confs.ndim != 4 or confs.shape[0] != S or conf_coeffs.shape[:2] != confs.shape[:2]:
        raise ValueError(f"expected dataset['confs'] [S = {S}, M, n_conf, N] and dataset['conf_coeffs'] [S, M, n_conf]")
    n_total = M * S * B
    loss, grads, ps = 0.0, [], []
    for s in range(S):
        eng = wf.engine(params[s], Rs[0])
        if eng.program.grad_unsupported:
            raise NotImplementedError(f'pretraining: unsupported for this program ({eng.program.grad_unsupported})')
        key = (id(target_fn), s)
        if getattr(eng, '_pretrain_key', None) != key:
            target_fn.upload(eng, confs[s], conf_coeffs[s], 0)
            eng._pretrain_key, eng._pretrain_target_ref = key, target_fn      # (the reference keeps id() from being recycled)
        p, g = eng.pretrain_loss_grad(r[0, s].contiguous(), Rs[0], n_total=n_total)
        loss = loss + float(p.sum()) / n_total
        # (a device-folded nuclear stream is transposed on the device: Engine.grad_to_params)
        grads.append(wf._grad_tree(eng, g))
        ps.append(p)
    return loss, grads, torch.stack(ps)[None]


class _Adam:
    """optax.adam on {module: {leaf: ndarray}} trees: `init(params) -> state`, `update(grads, state, params=None) ->
    (updates, state)`; the caller adds the updates to the parameters (optax.apply_updates)."""

    def __init__(self, learning_rate, b1, b2, eps):
        self.lr, self.b1, self.b2, self.eps = learning_rate, b1, b2, eps

    def init(self, params):
        zeros = lambda: {m: {k: np.zeros(np.shape(v), np.float64) for k, v in leaves.items()} for m, leaves in params.items()}
        return {'count': 0, 'mu': zeros(), 'nu': zeros()}

    def update(self, grads, state, params=None):
        t = state['count'] + 1
        mu = {m: {k: self.b1 * state['mu'][m][k] + (1 - self.b1) * np.asarray(g, np.float64) for k, g in lv.items()} for m, lv in grads.items()}
        nu = {m: {k: self.b2 * state['nu'][m][k] + (1 - self.b2) * np.asarray(g, np.float64) ** 2 for k, g in lv.items()} for m, lv in grads.items()}
        lr = self.lr(state['count']) if callable(self.lr) else self.lr
        c1, c2 = 1 - self.b1 ** t, 1 - self.b2 ** t
        upd = {m: {k: -lr * (mu[m][k] / c1) / (np.sqrt(nu[m][k] / c2) + self.eps) for k in lv} for m, lv in grads.items()}
        return upd, {'count': t, 'mu': mu, 'nu': nu}


def adam(learning_rate, b1=0.9, b2=0.999, eps=1e-8):
    """optax.adam(learning_rate, b1, b2, eps) for the gradient trees of this package (optax is not a dependency)."""
    return _Adam(learning_rate, b1, b2, eps)


def apply_updates(params, updates):
    """optax.apply_updates in place: the leaves of `params` keep their identity (and dtype), so the cached contexts of the
    tree are refreshed with `wf.invalidate(params)`."""
    for m, lv in updates.items():
        for k, u in lv.items():
            leaf = params[m][k]
            if isinstance(leaf, np.ndarray):
                leaf += u.astype(leaf.dtype)
            else:
                params[m][k] = np.asarray(leaf) + u
    return params


def merge_states(params: Sequence, merge_keys):
    """optimizer.py:227-249: the leaves of every module whose name contains one of `merge_keys` are replaced by their mean
    over the electronic states, in place."""
    if not merge_keys or len(params) < 2:
        return params
    for m in params[0]:
        if not any(key in m for key in merge_keys):
            continue
        for k in params[0][m]:
            mean = np.mean([np.asarray(p[m][k], np.float64) for p in params], axis=0)
            for p in params:
                p[m][k] = mean.astype(np.asarray(p[m][k]).dtype)
    return params


def pretrain(rng, hamil, ansatz, params: Sequence, opt, molecule_idx_sampler, sampler, smpl_state, dataset, merge_keys, steps):
    """pretraining.py:19-140 as a generator: one pretraining step per element of `steps`, yielding (step, params,
    per_sample_losses [1, S, B], mol_idxs).  `params`: one parameter tree per electronic state, updated in place;
    `opt`: `adam(...)` or any object with optax's `init(params)` / `update(grads, state, params)`; `sampler.sample(rng,
    smpl_state, params, mol_idxs)` -> (smpl_state, phys_conf r[1, S, B, N, 3], stats) as MultiNuclearGeometrySampler over
    MultiElectronicStateSampler gives it; `rng`: an integer seed."""
    if not (hasattr(opt, 'init') and hasattr(opt, 'update')):
        raise NotImplementedError('opt must provide init(params) and update(grads, state, params)')
    target_fn = PretrainTarget(hamil, None, dataset['centers'], dataset['shells'], dataset['mo_coeffs'])
    params = list(params)
    opt_state = [opt.init(p) for p in params]
    for k, step in enumerate(steps):
        mol_idxs = molecule_idx_sampler.sample()
        smpl_state, phys_conf, _ = sampler.sample(int(rng) * 1000003 + k, smpl_state, params, mol_idxs)
        _, grads, per_sample_losses = pretrain_loss_and_grad(ansatz, params, phys_conf, dataset, target_fn)
        for s, p in enumerate(params):
            updates, opt_state[s] = opt.update(grads[s], opt_state[s], p)
            apply_updates(p, updates)
        merge_states(params, tuple(merge_keys) if merge_keys is not None else None)
        for p in params:
            ansatz.invalidate(p)
        if hasattr(sampler, 'update'):      # log|psi| of the walkers under the new parameters (fit.py:92)
            smpl_state = sampler.update(smpl_state, params)
        yield step, params, per_sample_losses, mol_idxs


__all__ = ['GTOBasis', 'PretrainTarget', 'pretrain_loss_and_grad', 'adam', 'apply_updates', 'merge_states', 'pretrain',
           'get_cartesian_angulars']
