"""`NeuralNetworkWaveFunction`: the ansatz surface (`init` / `apply`) of the reference
(src/deepqmc/types.py:107-150, wf/nn_wave_function.py:42-173) backed by the HIP engine.

    ansatz = NeuralNetworkWaveFunction(hamil, 'paulinet')
    params = ansatz.init(seed)                 # haiku-shaped parameter tree (NumPy leaves)
    psi    = ansatz.apply(params, phys_conf)   # Psi(sign[B], log[B]) on the GPU

`apply` evaluates a whole batch (the reference vmaps its single-walker apply,
sampling/electron_samplers.py:76-81).  One engine (HIP context) is kept per live parameter
tree OBJECT: the cache holds a reference to the tree and matches it with `is`, so a recycled
`id()` can never alias an engine holding other weights.  Pass a new tree object after an
optimiser step and its weights are uploaded into the least recently used context; leaves
mutated in place are not detected -- call `invalidate(params)` after doing that.

A device-resident optimiser step (Engine.adam_step / apply_update / set_params_flat, deepqmc_amd/optimizer.py) changes a
context's weights without touching the tree it is cached under: the engine is marked (`Engine.params_ahead`), and
`sync_params(tree)` downloads the current values into the tree's leaves.  The cache does that by itself before it
re-targets or drops such a context.
"""
from __future__ import annotations

import torch

from .engine import Engine
from .hamil import MolecularHamiltonian
from .params import init_params
from .spec import ANSATZES, AnsatzSpec
from .types import PhysicalConfiguration, Psi


class NeuralNetworkWaveFunction:
    def __init__(self, hamil: MolecularHamiltonian, spec='paulinet', *, dtype=torch.float32, device='cuda',
                 norm_eps=None, lib=None, attention_reverse=False, nuclear_reverse=False, nuclear_coords=False,
                 nuclear_params=False):
        """`attention_reverse`: opt in to the reverse pass through attention ops (library option "attention_reverse"), which
        the parameter- and coordinate-gradient entry points below, the force and ECP-force estimators, pretraining,
        `create_loss_fn` and the optimisers of `fit_wf` need for a Psiformer.  Off (the default) those calls fail with
        `dqmc error -4` for an attention ansatz.  The TransPsiformer stays unsupported with this flag alone (its nuclear tokens
        are folded on the host).
        `nuclear_reverse` (implies `attention_reverse`): the nuclear-token stream of a TransPsiformer is also folded on the
        device and has a backward there (library option "nuclear_reverse"), which opens `log_psi_vjp`, `orbitals_vjp`,
        pretraining, `create_loss_fn` and `fit_wf` with AdamOptimizer / NoOptimizer.  The per-walker modes (log_psi_jacobian,
        log_psi_kfac, log_psi_grad_coords, NaturalGradientOptimizer, KFACOptimizer, forces) stay refused: the stream is shared
        by all walkers and has no per-walker partials.
        `nuclear_coords` (implies `nuclear_reverse` and `attention_reverse`): the stream's backward also runs per walker, adjoints
        only, down to the nuclear coordinates (library option "nuclear_coords"), which opens `log_psi_grad_coords`,
        `force.make_grad_nuc_log_wf`, `evaluate_hf_force_ac_zb` / `_ac_zvqzb` and their `fit_wf` monitors.  The Jacobian, KFAC,
        NaturalGradientOptimizer, KFACOptimizer and the ECP force stay refused.
        `nuclear_params` (implies `nuclear_reverse` and `attention_reverse`; independent of `nuclear_coords`): the stream's
        parameter partials are formed per walker on the device (library option "nuclear_params"), which opens `log_psi_jacobian`
        (through Engine.jacobian_to_params), `log_psi_kfac`, `compute_energy_loss_and_natgrad`,
        `compute_energy_loss_and_kfac(flat=True)`, NaturalGradientOptimizer and KFACOptimizer.  In the KFAC direction the
        stream's own parameters (nuclei_embedding, nuclear_gnn_head) are diagonal elements.  The ECP force stays refused."""
        self.hamil = hamil
        if spec == 'transpsiformer':
            self.spec: AnsatzSpec = ANSATZES[spec](hamil.mol.charges)      # atom types of the nuclei embedding
        else:
            self.spec = ANSATZES[spec]() if isinstance(spec, str) else spec
        self.dtype, self.device, self.norm_eps, self._lib = dtype, device, norm_eps, lib
        self.nuclear_coords = bool(nuclear_coords) and bool(self.spec.nuclei_tokens)
        self.nuclear_params = bool(nuclear_params) and bool(self.spec.nuclei_tokens)
        self.nuclear_reverse = (bool(nuclear_reverse) or bool(nuclear_coords) or bool(nuclear_params)) and bool(self.spec.nuclei_tokens)
        self.attention_reverse = bool(attention_reverse) or bool(nuclear_reverse) or bool(nuclear_coords) or bool(nuclear_params)
        self._engines = []       # [(params tree, Engine)], most recently used last (one per electronic state)
        self.max_engines = 8
        self._evictions = 0

    def init(self, rng=0, phys_conf=None, **kw):
        """types.py:121-133.  `rng`: an integer seed (the JAX key stream is not reproduced)."""
        h = self.hamil
        return init_params(self.spec, h.n_up, h.n_down, h.n_nuc, seed=int(rng), **kw)

    def _geometry_key(self, R):
        """Ansatzes with nuclear tokens fold the geometry into the program: one context per (tree, geometry).
        Everything else takes R per call and shares one context across geometries."""
        if R is None or not self.spec.nuclei_tokens:
            return None
        import numpy as np
        R = np.asarray(R.detach().cpu() if hasattr(R, 'detach') else R, np.float64).reshape(-1, self.hamil.n_nuc, 3)
        if R.shape[0] > 1 and not np.array_equal(R, np.broadcast_to(R[:1], R.shape)):
            raise ValueError('an ansatz with nuclear tokens takes ONE geometry per call (per-walker geometries differ)')
        R = np.ascontiguousarray(R[0])
        return None if np.array_equal(R, self.hamil.mol.coords) else R.tobytes()

    def engine(self, params, R=None) -> Engine:
        """One HIP context per live parameter tree (e.g. per electronic state, the leading `S` axis of
        the reference's params, wf/base.py:27).  The cache entry keeps the tree alive and is matched by
        identity; once `max_engines` trees are alive the least recently used context is re-targeted
        with `set_params` (no new allocation)."""
        gkey = self._geometry_key(R)
        for k, (tree, key, eng) in enumerate(self._engines):
            if tree is params and key == gkey:
                self._engines.append(self._engines.pop(k))
                return eng
        reuse = [k for k, (_, key, _) in enumerate(self._engines) if key == gkey]
        if len(self._engines) >= self.max_engines and reuse:
            old_tree, _, eng = self._engines.pop(reuse[0])
            self._sync_tree(old_tree, eng)      # (a context stepped on the device holds the only copy of its tree's current values)
            eng.set_params(params)
        else:
            if len(self._engines) >= self.max_engines:
                # the evicted context leaves the cache; its device memory (workspace, float64 twin, captured graphs) goes back
                # when its LAST reference goes -- now, if the cache held the only one (Engine keeps no reference cycle:
                # tests/test_facade_emu.py::test_engine_is_released_by_reference_count), otherwise when the caller that
                # still holds it drops it.  Nothing is closed under a caller's feet.
                self._sync_tree(*self._engines.pop(0)[::2])
                self._evictions += 1
                if self._evictions == 4 * self.max_engines:
                    import warnings
                    warnings.warn(f'NeuralNetworkWaveFunction: {self._evictions} HIP contexts evicted from a cache of '
                                  f'{self.max_engines}; raise `max_engines` to (geometries x states) in use')
            import numpy as np
            R0 = None if gkey is None else np.frombuffer(gkey, np.float64).reshape(self.hamil.n_nuc, 3)
            eng = Engine(self.spec, self.hamil, params, dtype=self.dtype, device=self.device,
                         norm_eps=self.norm_eps, lib=self._lib, R=R0, nuclear_reverse=self.nuclear_reverse,
                         nuclear_coords=self.nuclear_coords, nuclear_params=self.nuclear_params)
            if self.attention_reverse:      # before any set_kfac_map or graph capture (setting an option bumps the graph epoch)
                eng.set_option('attention_reverse', 1)
        self._engines.append((params, gkey, eng))
        return eng

    def release(self):
        """Close every cached HIP context (device workspaces, twins, captured graphs) NOW, whoever still refers to them:
        an `Engine` obtained from `engine()` before this call raises a clear "engine closed" error afterwards."""
        while self._engines:
            self._engines.pop()[2].close()

    @staticmethod
    def _sync_tree(tree, eng):
        if not eng.params_ahead:
            return
        theta = eng.params_flat().cpu().numpy()
        import numpy as np
        for (mod, leaf), (sl, shape) in eng.program.leaf_slices().items():
            cur = tree[mod][leaf]
            if isinstance(cur, np.ndarray) and cur.shape == tuple(shape) and cur.flags.writeable:
                cur[...] = theta[sl].reshape(shape).astype(cur.dtype)
            else:
                tree[mod][leaf] = theta[sl].reshape(shape).copy()
        eng.params_ahead = False

    def sync_params(self, params=None):
        """Bring the leaves of `params` (every cached tree if None) up to date with their context after device-resident
        optimiser steps, in place: one device-to-host copy of the parameter vector per stale tree.  Returns `params`."""
        for tree, _, eng in self._engines:
            if params is None or tree is params:
                self._sync_tree(tree, eng)
        return params

    def params_stale(self, params) -> bool:
        """True if a cached context of `params` was stepped on the device since the tree's leaves were last written."""
        return any(tree is params and eng.params_ahead for tree, _, eng in self._engines)

    def invalidate(self, params=None):
        """Re-upload the weights of `params` (all cached trees if None) after their leaves were changed in place."""
        for tree, _, eng in self._engines:
            if params is None or tree is params:
                eng.set_params(tree)

    def apply(self, params, phys_conf, return_mos: bool = False) -> Psi:
        """types.py:135-150 (batched)."""
        r = phys_conf.r if isinstance(phys_conf, PhysicalConfiguration) else phys_conf
        R = phys_conf.R if isinstance(phys_conf, PhysicalConfiguration) else None
        eng = self.engine(params, R)
        if return_mos:
            # wf/nn_wave_function.py:127,144-145: the (backflow-transformed) molecular orbitals the determinants are taken of,
            # `(orb_up, orb_down)` -- the pretraining hook.  They are the Slater-matrix buffer of the value path: read back
            # through the debug interface (a host copy: this is not a hot path) as [B, K, n_up | n_down, n_orb].
            if not self.spec.full_determinant:
                raise NotImplementedError('return_mos (wf/nn_wave_function.py:144): only full-determinant programs expose '
                                          'their orbital matrices; spin-factorised ones store block-diagonal matrices')
            import numpy as np
            prev_fused = eng.get_option('fused', 1)
            eng.set_option('fused', 0)              # every activation buffer stays readable (include/dqmc.h: "fused")
            try:
                eng.wf_eval(r, R)
                B = torch.as_tensor(r).shape[0]
                N, K = self.hamil.n_elec, self.spec.n_determinants
                A = eng.debug_read('orbitals', B)[:, :, 0, :N * N].reshape(B, K, N, N)     # rows = electrons, columns = orbitals
            finally:
                eng.set_option('fused', prev_fused)      # (the caller's own choice, not the default)
            A = torch.as_tensor(np.ascontiguousarray(A), dtype=self.dtype, device=self.device)
            return A[:, :, :self.hamil.n_up], A[:, :, self.hamil.n_up:]
        sign, log = eng.wf_eval(r, R)
        return Psi(sign, log)

    __call__ = apply

    @staticmethod
    def _grad_tree(eng, g):
        """Flat gradient over the weight buffer -> tree.  Programs with a device-folded nuclear stream take the device route
        (Engine.grad_to_params transposes the fold there), every other program the host transpose of the packing."""
        prog = eng.program
        if prog.nuclear_stream is not None:
            return prog.unflatten_params(eng.grad_to_params(g))
        return prog.unflatten_grad(g)

    def _per_walker_check(self, name, eng, coords=False):
        if eng.program.grad_unsupported:
            raise NotImplementedError(f'{name}: unsupported for this program ({eng.program.grad_unsupported})')
        if eng.program.nuclear_stream is not None and not (eng.nuclear_coords if coords else eng.nuclear_params):
            raise NotImplementedError(f'{name}: {eng.program.PER_WALKER_NUCLEAR}')

    def _orbital_engine(self, name, params, phys_conf):
        if not self.spec.full_determinant:
            raise NotImplementedError(f'{name}: only full-determinant programs expose their orbital matrices; spin-factorised '
                                      'ones store block-diagonal matrices')
        r = phys_conf.r if isinstance(phys_conf, PhysicalConfiguration) else phys_conf
        R = phys_conf.R if isinstance(phys_conf, PhysicalConfiguration) else None
        return self.engine(params, R), r, R

    def orbitals(self, params, phys_conf):
        """`apply(..., return_mos=True)` without the host copy: `(orb_up [B, K, n_up, N], orb_down [B, K, n_down, N])`, views of
        one device tensor written by the value pass (Engine.orbitals)."""
        eng, r, R = self._orbital_engine('orbitals', params, phys_conf)
        A = eng.orbitals(r, R)
        return A[:, :, :self.hamil.n_up], A[:, :, self.hamil.n_up:]

    def orbitals_vjp(self, params, phys_conf, cotangent):
        """jax.vjp of the batched `apply(..., return_mos=True)`: `cotangent` = `(cot_up [B, K, n_up, N], cot_down
        [B, K, n_down, N])` or one [B, K, N, N] tensor; returns ((orb_up, orb_down), grad tree {module: {leaf: ndarray}}) with
        grad = sum cot * d orbitals / d params.  Leaves no path leads from to the orbitals (the Jastrow factor, conf_coeff)
        get exact zeros.  The same programs as log_psi_vjp are supported."""
        eng, r, R = self._orbital_engine('orbitals_vjp', params, phys_conf)
        if eng.program.grad_unsupported:
            raise NotImplementedError(f'orbitals_vjp: unsupported for this program ({eng.program.grad_unsupported})')
        if isinstance(cotangent, (tuple, list)):
            cotangent = torch.cat([torch.as_tensor(c, dtype=self.dtype, device=self.device) for c in cotangent], dim=2)
        A, g = eng.orbitals_vjp(r, cotangent, R)
        return (A[:, :, :self.hamil.n_up], A[:, :, self.hamil.n_up:]), self._grad_tree(eng, g)

    def log_psi_vjp(self, params, phys_conf, cotangent=None):
        """jax.vjp of vmap(ansatz.apply)(params, r).log (loss/loss_function.py:59-75) with one cotangent per walker:
        returns (Psi(sign, log), grad tree {module: {leaf: ndarray}}) with grad = sum_b cotangent[b] d log|psi(r_b)| / d params.
        cotangent None = all ones.  Programs with attention ops (Psiformer) are supported when the wave function was made
        with `attention_reverse=True`; programs whose packing is not a copy of the parameters (nuclear tokens:
        TransPsiformer) are not supported."""
        r = phys_conf.r if isinstance(phys_conf, PhysicalConfiguration) else phys_conf
        R = phys_conf.R if isinstance(phys_conf, PhysicalConfiguration) else None
        eng = self.engine(params, R)
        if self.attention_reverse and eng.program.grad_unsupported:
            raise NotImplementedError(f'log_psi_vjp: unsupported for this program ({eng.program.grad_unsupported})')
        sign, log, g = eng.log_psi_vjp(r, cotangent, R)
        return Psi(sign, log), self._grad_tree(eng, g)

    def log_psi_jacobian(self, params, phys_conf):
        """The per-walker rows of the Jacobian that log_psi_vjp contracts: returns (Psi(sign, log), Jp) with
        Jp[b] = d log|psi(r_b)| / d params as a [B, n_params] tensor on the device, in the wave function's dtype, columns in
        the program's grad_leaves order (eng.program.leaf_slices / unflatten_params map them back onto the tree).  The same
        programs as log_psi_vjp are supported; a TransPsiformer needs `nuclear_params=True` and takes the device route
        (Engine.jacobian_to_params: the stream's parameter partials are formed per walker there)."""
        r = phys_conf.r if isinstance(phys_conf, PhysicalConfiguration) else phys_conf
        R = phys_conf.R if isinstance(phys_conf, PhysicalConfiguration) else None
        eng = self.engine(params, R)
        self._per_walker_check('log_psi_jacobian', eng)          # before the B x n_weights allocation
        sign, log, J = eng.log_psi_jacobian(r, R)
        Jp = eng.jacobian_to_params(J, log, sign) if eng.program.nuclear_stream is not None else eng.program.unflatten_jacobian(J)
        del J
        return Psi(sign, log), Jp

    def log_psi_kfac(self, params, phys_conf, cotangent=None):
        """log_psi_vjp plus the KFAC statistics of the same reverse pass (Engine.log_psi_kfac): returns (Psi(sign, log), grad
        tree, factors, rest) with factors the per-LINEAR-op (A, G) float64 tensors and rest the [B, n_rest] per-walker partials
        of the entries no LINEAR op owns (Program.kfac_layout / kfac_blocks map both onto the parameters).  The same programs
        as log_psi_vjp are supported."""
        r = phys_conf.r if isinstance(phys_conf, PhysicalConfiguration) else phys_conf
        R = phys_conf.R if isinstance(phys_conf, PhysicalConfiguration) else None
        eng = self.engine(params, R)
        self._per_walker_check('log_psi_kfac', eng)
        sign, log, g, factors, rest = eng.log_psi_kfac(r, cotangent, R)
        return Psi(sign, log), self._grad_tree(eng, g), factors, rest

    def log_psi_grad_coords(self, params, phys_conf):
        """jax.grad of ansatz.apply(.).log with respect to the electron and the nuclear coordinates (reference force.py
        make_grad_log_wf / make_grad_nuc_log_wf), per walker, from the reverse pass (Engine.log_psi_grad_coords): returns
        (Psi(sign, log), grad_r [B, N, 3], grad_R [B, n_nuc, 3]) on the device, in the wave function's dtype.  The same
        programs as log_psi_vjp are supported; a TransPsiformer needs `nuclear_coords=True`."""
        r = phys_conf.r if isinstance(phys_conf, PhysicalConfiguration) else phys_conf
        R = phys_conf.R if isinstance(phys_conf, PhysicalConfiguration) else None
        eng = self.engine(params, R)
        self._per_walker_check('log_psi_grad_coords', eng, coords=True)
        sign, log, gr, gR = eng.log_psi_grad_coords(r, R)
        return Psi(sign, log), gr, gR
