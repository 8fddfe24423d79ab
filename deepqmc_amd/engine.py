"""Engine: one HIP context (`dqmc_ctx`) = one ansatz + parameter set on one GPU.

Host glue only: compiles the layer program (program.py), hands it to the C ABI
(include/dqmc.h) and moves raw device pointers of torch tensors across it.  torch is used
for device memory and streams, nothing else.  The library trusts those pointers: `Engine._arg` and
`Engine._walkers` are where a wrong dtype, layout, device or shape is stopped.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .hamil import STAT_KEYS, MolecularHamiltonian
from .program import DqmcSystem, Program, compile_program
from .spec import AnsatzSpec
from .types import PhysicalConfiguration

F32_EPS = float(np.finfo(np.float32).eps)
F64_EPS = float(np.finfo(np.float64).eps)
# estimator codes of dqmc_hf_force (include/dqmc.h: DQMC_FORCE_*), in code order
FORCE_ESTIMATORS = ('nuclear', 'bare', 'ac_zvq', 'ac_zvzbq', 'ac_zb', 'ac_zvqzb')
SAMPLER_STAT_KEYS = ('sampling/acceptance', 'sampling/tau', 'sampling/age/mean', 'sampling/age/max',
                     'sampling/log_psi/mean', 'sampling/log_psi/std', 'sampling/dists/mean')


class DqmcError(RuntimeError):
    pass


def nuclear_energy(coords: np.ndarray, charges: np.ndarray) -> float:
    """sum_{a<b} Z_a Z_b / R_ab (reference physics.py:112-116).  Host-side helper (reports, tests); the
    library recomputes the term on the device from the R of every call."""
    e = 0.0
    for a in range(len(charges)):
        for b in range(a + 1, len(charges)):
            e += charges[a] * charges[b] / float(np.linalg.norm(coords[a] - coords[b]))
    return e


def _np_ptr(a: np.ndarray, ctype=ctypes.c_double, or_null=False):
    """The data of a contiguous host array as a `ctype*`; or_null: an empty array crosses as NULL."""
    return None if or_null and not a.size else a.ctypes.data_as(ctypes.POINTER(ctype))


def _ptr(t):
    """The device pointer of an optional tensor (None -> NULL)."""
    return t.data_ptr() if t is not None else None


class Engine:
    def __init__(self, spec: AnsatzSpec, hamil: MolecularHamiltonian, params, *, dtype=torch.float32,
                 device='cuda', norm_eps: Optional[float] = None, lib=None, R=None, compiler=None, nuclear_reverse=False,
                 nuclear_coords=False, nuclear_params=False):
        """`R` [n_nuc,3]: the geometry this context is compiled for (default: the Hamiltonian's).  It matters only
        for ansatzes with nuclear tokens, whose nuclear stream is folded into the program; every other ansatz
        takes the geometry per call.  `compiler(params) -> Program` replaces the default `compile_program(spec, ...)`
        (e.g. program_featurewise.compile_featurewise for the reference's test ansatz family); `spec` may then be
        any object with `n_determinants` and `nuclei_tokens`.  `nuclear_reverse`: for an ansatz with nuclear tokens, register
        the nuclear stream with the library (dqmc_set_nuclear_stream) and switch on options "attention_reverse" and
        "nuclear_reverse": device updates fold the stream on the device and grad_to_params transposes it, so the
        walker-summed gradients (log_psi_vjp, orbitals_vjp, pretrain_loss_grad) and the Adam step run.  `nuclear_coords` (implies
        `nuclear_reverse`): option "nuclear_coords" as well, which opens log_psi_grad_coords -- the stream's backward runs per
        walker, adjoints only, down to R.  `self.nuclear_coords` says whether it is on.  `nuclear_params` (implies
        `nuclear_reverse`, independent of `nuclear_coords`): option "nuclear_params", which opens log_psi_jacobian, log_psi_kfac,
        jacobian_to_params and the KFAC tables -- the stream's parameter partials are formed per walker.  `self.nuclear_params`
        says whether it is on (set_option('nuclear_params', ...) keeps it and Program.nuclear_params current)."""
        nuclear_reverse = bool(nuclear_reverse) or bool(nuclear_coords) or bool(nuclear_params)
        self.lib = lib if lib is not None else _lib.load()
        self.spec, self.hamil = spec, hamil
        self.dtype = dtype
        self.device = torch.device(device)
        if dtype not in (torch.float32, torch.float64):
            raise ValueError('dtype must be float32 or float64')
        # eps under the safe norm is the compute dtype's machine eps (reference utils.py:79-85)
        self.norm_eps = norm_eps if norm_eps is not None else (F32_EPS if dtype == torch.float32 else F64_EPS)
        self.R0 = np.asarray(hamil.mol.coords if R is None else R, np.float64).reshape(hamil.n_nuc, 3)
        R0_, eps_ = self.R0, self.norm_eps      # (no `self` in the closure: a cycle would leave the context -- tens of GB of
        self._compile = compiler if compiler is not None else (       # workspace -- to the cyclic collector instead of the reference count)
            lambda p_: compile_program(spec, p_, hamil.n_up, hamil.n_down, hamil.n_nuc, R=R0_, eps=eps_,
                                       nuclear_reverse=bool(nuclear_reverse) and bool(spec.nuclei_tokens)))
        self.program: Program = self._compile(params)
        self._theta_ref = None         # the device vector of the last device update (params_flat)
        self.params_ahead = False      # set by a device update: the context's weights are newer than the tree it is cached under
        self._param_map_set = self._kfac_map_set = False      # dqmc_set_param_map / dqmc_set_kfac_map done
        self._kfac_layout = None       # the state layout of the installed KFAC tables (set_kfac_tables)
        self._static_io = {}           # B -> the buffers of local_energy(static_io=True)
        self._options = {}             # what set_option was given
        self.pretrain_n_conf = None    # configurations of the uploaded pretraining target
        self._ecp_phi = None
        self.N = hamil.n_up + hamil.n_down
        sysd = DqmcSystem(hamil.n_up, hamil.n_down, hamil.n_nuc, spec.n_determinants,
                          0 if dtype == torch.float32 else 1, 0, self.norm_eps, 0.0)
        p = self.program
        self._bufs, self._ops = p.c_bufs(), p.c_ops()
        w = self._w_host = np.ascontiguousarray(p.weights, np.float64)      # (params_flat reads theta back from it)
        it = np.ascontiguousarray(p.itable if p.itable.size else np.zeros(1, np.int32), np.int32)
        ch = np.ascontiguousarray(hamil.ns_valence, np.float64)
        stream = 0
        dev_index = 0
        if self.device.type == 'cuda':
            dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
            stream = torch.cuda.current_stream(self.device).cuda_stream
        ctx = ctypes.c_void_p()
        rc = self.lib.dqmc_create(ctypes.byref(ctx), dev_index, ctypes.c_void_p(stream), ctypes.byref(sysd), _np_ptr(ch), self._bufs,
                                  len(p.bufs), self._ops, len(p.ops), _np_ptr(w), w.size, _np_ptr(it, ctypes.c_int32), p.itable.size)
        self._ctx = ctx
        self._check(rc)
        pot = getattr(hamil, 'pot', None)
        if pot is not None and hasattr(pot, 'rv_l2'):       # pseudo-Hamiltonian tables -> device
            mask = np.ascontiguousarray(pot.ecp_mask, np.int32)
            self._check(self.lib.dqmc_set_pseudo_hamiltonian(self._ctx, pot.rv_loc.shape[1], pot.r_max, _np_ptr(pot.rv_loc, or_null=True),
                                                             _np_ptr(pot.rv_l2, or_null=True), _np_ptr(mask, ctypes.c_int32)))
        elif pot is not None:                               # Gaussian-type ECP tables -> device
            self._check(self.lib.dqmc_set_ecp(self._ctx, pot.loc_params.shape[3], _np_ptr(pot.loc_params, or_null=True),
                                              pot.nl_params.shape[1], pot.nl_params.shape[3], _np_ptr(pot.nl_params, or_null=True)))
        self.R = torch.tensor(self.R0, dtype=dtype, device=self.device)      # (a copy: R0 may be the molecule's read-only array)
        self._theta_host = None        # nuclear stream: the parameters of the last host upload (some leaves have no copy in the weights)
        if p.nuclear_stream is not None:
            self._theta_host = p.flatten_params(params)
            self._register_nuclear_stream()
            self.set_option('attention_reverse', 1)
            self.set_option('nuclear_reverse', 1)
        self.nuclear_coords = bool(nuclear_coords) and p.nuclear_stream is not None
        if self.nuclear_coords:
            self.set_option('nuclear_coords', 1)
        self.nuclear_params = False
        if nuclear_params and p.nuclear_stream is not None:
            self.set_option('nuclear_params', 1)

    def _register_nuclear_stream(self):
        """dqmc_set_nuclear_stream from Program.nuclear_stream and the current parameters."""
        self._ensure_param_map()
        ns = self.program.nuclear_stream
        lin = (_lib.DqmcNucLinear * len(ns['lin']))()
        for k, (w, b, n_in, n_out, act) in enumerate(ns['lin']):
            lin[k].w, lin[k].b, lin[k].n_in, lin[k].n_out, lin[k].act = w, b, n_in, n_out, act
        types = np.ascontiguousarray(ns['nuc_types'], np.int32)
        Rn = np.ascontiguousarray(ns['R'], np.float64)
        row = np.ascontiguousarray(ns['sc_row'], np.int64)
        col = np.ascontiguousarray(ns['sc_col'], np.int32)
        theta = np.ascontiguousarray(self._theta_host, np.float64)
        d = _lib.DqmcNucStream(self.hamil.n_nuc, ns['n_layers'], ns['heads'], ns['dim'], ns['n_det'], ns['n_env'], ns['n_edge_lin'],
                               ns['n_embed_lin'], ns['n_mlp_lin'], len(ns['lin']), lin, ns['zbias'][0], ns['zbias'][1],
                               _np_ptr(types, ctypes.c_int32), _np_ptr(Rn), ns['n_derived'], _np_ptr(row, ctypes.c_int64),
                               _np_ptr(col, ctypes.c_int32), _np_ptr(theta))
        self._check(self.lib.dqmc_set_nuclear_stream(self._ctx, ctypes.byref(d)))

    # ------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != 0:
            if getattr(self, '_ctx', None) is None:
                raise DqmcError('engine closed: its HIP context was destroyed (Engine.close / NeuralNetworkWaveFunction.release); '
                                'obtain a new one with NeuralNetworkWaveFunction.engine(params)')
            raise DqmcError(f'dqmc error {rc}: {self.lib.dqmc_last_error().decode()}')

    def close(self):
        if getattr(self, '_ctx', None):
            self.lib.dqmc_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _t(self, x, dtype=None):
        return torch.as_tensor(x, dtype=dtype or self.dtype, device=self.device).contiguous()

    # ---- what crosses the C ABI as a raw pointer: the layout must be exactly the documented one ----
    def _arg(self, name, t, dtype, shape, optional=False):
        """`t` if it is a contiguous `dtype` tensor of `shape` (None: any extent) on the engine's device type, else DqmcError.
        A bool tensor for a uint8 slot is viewed as uint8; `optional`: None passes."""
        if t is None and optional:
            return None
        if dtype == torch.uint8 and isinstance(t, torch.Tensor) and t.dtype == torch.bool:
            t = t.view(torch.uint8)
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or t.device.type != self.device.type \
                or t.dim() != len(shape) or any(n is not None and n != m for n, m in zip(shape, t.shape)):
            want = ', '.join('*' if n is None else str(n) for n in shape)
            got = f'{t.dtype} {list(t.shape)} on {t.device}' if isinstance(t, torch.Tensor) else type(t).__name__
            raise DqmcError(f"'{name}' must be a contiguous {dtype} tensor of shape [{want}] on {self.device}, got {got}")
        return t

    def check_walker_vector(self, name, t, n=None):
        """A [B] tensor about to cross the C ABI as a raw pointer: dtype, layout and device must be the context's."""
        return self._arg(name, t, self.dtype, (n,))

    def _walkers(self, r, R=None):
        """The prologue of every entry point that takes walkers: (r [B, N, 3] as a contiguous tensor of the engine's dtype on
        its device, the geometry tensor of the call, B)."""
        r = self._arg('r', self._t(r), self.dtype, (None, self.N, 3))
        return r, self._R(R), r.shape[0]

    def _cot(self, cot, B):
        return None if cot is None else self._arg('cot', self._t(cot).reshape(-1), self.dtype, (B,))

    def _psi_out(self, B):
        """New (logpsi [B], sign [B]) outputs."""
        return torch.empty(B, dtype=self.dtype, device=self.device), torch.empty(B, dtype=torch.int32, device=self.device)

    def _R(self, R):
        if R is None:
            return self.R
        R = self._t(R)
        if R.dim() == 3:      # reference tiles R per walker (electron_samplers.py:165-173)
            R = R[0].contiguous()
        self._arg('R', R, self.dtype, (self.hamil.n_nuc, 3))
        if self.spec.nuclei_tokens and not torch.equal(R, self.R):
            raise DqmcError('this ansatz folds the nuclear stream at the geometry of its Hamiltonian; '
                            'build a new engine for a different R')
        return R

    def _read(self, fn, ctype, keys) -> dict:
        """{key: value} of a getter `fn(ctx, ctype out[len(keys)])`."""
        out = (ctype * len(keys))()
        self._check(fn(self._ctx, out))
        return dict(zip(keys, out))

    def set_params(self, params):
        """New parameter tree after an optimiser step (same structure)."""
        prog = self._compile(params)
        w = self._w_host = np.ascontiguousarray(prog.weights, np.float64)
        self._check(self.lib.dqmc_set_weights(self._ctx, _np_ptr(w), w.size))
        self.params_ahead, self._theta_ref = False, None
        if prog.nuclear_stream is not None:
            # the host upload carries constants folded on the host; the transpose of the fold needs the activations of a device
            # fold of the same parameters (include/dqmc.h: the invariant of dqmc_set_nuclear_stream), so fold them there as well
            self._theta_host = prog.flatten_params(params)
            theta = torch.as_tensor(self._theta_host, dtype=torch.float64, device=self.device).contiguous()
            self._check(self.lib.dqmc_weights_from_params(self._ctx, theta.data_ptr()))
            if self.device.type == 'cuda':
                torch.cuda.current_stream(self.device).synchronize()      # (theta is a temporary)

    # ---- device-resident parameters and optimiser step (dqmc_set_param_map ... dqmc_apply_update) ----
    def _ensure_param_map(self):
        """Upload Program.grad_src on first use (dqmc_set_param_map)."""
        if not self._param_map_set:
            prog = self.program
            if prog.grad_unsupported:
                raise NotImplementedError(f'device-resident parameters: unsupported for this program ({prog.grad_unsupported})')
            src = np.ascontiguousarray(prog.grad_src, np.int32)
            self._check(self.lib.dqmc_set_param_map(self._ctx, _np_ptr(src, ctypes.c_int32), src.size, prog.n_params()))
            self._param_map_set = True

    def _thetas(self, norms=None, n_norms=3, **vectors):
        """Check float64 [n_params] device vectors, given by name, and the optional `norms` [n_norms]."""
        n = self.program.n_params()
        for name, t in vectors.items():
            self._arg(name, t, torch.float64, (n,))
        self._arg('norms', norms, torch.float64, (n_norms,), optional=True)

    def params_flat(self, params=None):
        """The context's current parameters as a float64 device vector in Program.grad_leaves order: the theta of
        set_params_flat / adam_step / apply_update.  After a device update: a copy of the vector that update used; before
        one: read back from the weights of the last host upload (every parameter element is copied into the weight buffer
        verbatim); with `params`: that tree, flattened.  The returned vector is the caller's."""
        if params is not None:
            return torch.as_tensor(self.program.flatten_params(params), dtype=torch.float64, device=self.device).contiguous()
        if self._theta_ref is not None:
            return self._theta_ref.clone()
        prog = self.program
        if prog.grad_unsupported:
            raise NotImplementedError(f'params_flat: unsupported for this program ({prog.grad_unsupported})')
        if self._theta_host is not None:
            return torch.as_tensor(self._theta_host, dtype=torch.float64, device=self.device).contiguous()
        m = prog.grad_src >= 0
        theta = np.zeros(prog.n_params(), np.float64)
        theta[prog.grad_src[m]] = self._w_host[m]
        return torch.as_tensor(theta, dtype=torch.float64, device=self.device).contiguous()

    def set_params_flat(self, theta):
        """New parameter values from a float64 device vector (dqmc_weights_from_params): weights, twin, tape and fused planes
        are rewritten on the device, nothing goes through the host and captured graphs stay valid."""
        self._thetas(theta=theta)
        self._ensure_param_map()
        self._check(self.lib.dqmc_weights_from_params(self._ctx, theta.data_ptr()))
        self.params_ahead, self._theta_ref = True, theta

    def grad_to_params(self, g):
        """Flat gradient over the weight buffer (log_psi_vjp) -> float64 [n_params] device vector: unflatten_grad flattened in
        leaf order, without leaving the device (dqmc_grad_to_params)."""
        self._arg('g', g, torch.float64, (self.program.weights.size,))
        self._ensure_param_map()
        out = torch.empty(self.program.n_params(), dtype=torch.float64, device=self.device)
        self._check(self.lib.dqmc_grad_to_params(self._ctx, g.data_ptr(), out.data_ptr()))
        return out

    def jacobian_to_params(self, J, logpsi, sign, out=None):
        """Per-walker Jacobian over the weight buffer (log_psi_jacobian, with the logpsi and sign of that call) -> [B, n_params]
        in the engine's dtype on its device: row b is the transpose of the packing applied to J[b], the per-walker form of
        grad_to_params (dqmc_jacobian_to_params).  Without a nuclear stream it equals Program.unflatten_jacobian(J); with one
        (nuclear_params=True) the stream's parameter partials of every walker are added on the device.  Rows of invalid
        walkers are zero.  `out`: a preallocated contiguous [B, n_params] tensor."""
        if not isinstance(J, torch.Tensor) or J.dim() != 2 or J.dtype != self.dtype or J.device.type != self.device.type or \
                J.shape[1] != self.program.weights.size or J.stride(1) != 1 or J.stride(0) < J.shape[1]:
            raise DqmcError(f"'J' must be a [B, {self.program.weights.size}] {self.dtype} tensor on {self.device} with unit column stride")
        B = J.shape[0]
        self._arg('logpsi', logpsi, self.dtype, (B,))
        self._arg('sign', sign, torch.int32, (B,))
        self._ensure_param_map()
        n = self.program.n_params()
        if out is None:
            out = torch.empty(B, n, dtype=self.dtype, device=self.device)
        self._arg('out', out, self.dtype, (B, n))
        self._check(self.lib.dqmc_jacobian_to_params(self._ctx, J.data_ptr(), J.stride(0), B, logpsi.data_ptr(), sign.data_ptr(),
                                                     out.data_ptr(), n))
        return out

    def adam_step(self, theta, mu, nu, grad_theta, *, lr, b1=0.9, b2=0.999, eps=1e-8, t=1, norms=None):
        """One optax.adam step in place on the device vectors theta, mu, nu, then the re-pack (dqmc_adam_step).  t: 1-based count.
        norms: optional float64 [3] device tensor receiving (param, grad, update) 2-norms."""
        self._thetas(norms, theta=theta, mu=mu, nu=nu, grad_theta=grad_theta)
        self._ensure_param_map()
        self._check(self.lib.dqmc_adam_step(self._ctx, theta.data_ptr(), mu.data_ptr(), nu.data_ptr(), grad_theta.data_ptr(),
                                            self.program.n_params(), float(lr), float(b1), float(b2), float(eps), int(t), _ptr(norms)))
        self.params_ahead, self._theta_ref = True, theta

    def apply_update(self, theta, delta, scale=1.0, norms=None):
        """theta += scale * delta on the device, then the re-pack (dqmc_apply_update)."""
        self._thetas(norms, theta=theta, delta=delta)
        self._ensure_param_map()
        self._check(self.lib.dqmc_apply_update(self._ctx, theta.data_ptr(), delta.data_ptr(), float(scale), _ptr(norms)))
        self.params_ahead, self._theta_ref = True, theta

    # ---- KFAC preconditioner on the flat device vectors (dqmc_set_kfac_map, dqmc_kfac_direction, dqmc_kfac_apply) ----
    KFAC_PANEL = 32     # DQMC_KFAC_PANEL: panel width of the blocked Cholesky factorisation and triangular solves

    def _kfac_tables(self):
        """The host tables of dqmc_set_kfac_map from Program.kfac_blocks / kfac_layout / leaf_slices and loss._rest_gather,
        and the layout of the state they imply."""
        from .loss import _rest_gather
        prog = self.program
        blocks, _ = prog.kfac_blocks()
        lay = prog.kfac_layout()
        sl = prog.leaf_slices()
        mod, op, maps, n_maps = [], [], [], 0
        layout = {'modules': {}, 'diag': None}
        off = 0
        for name, blk in blocks.items():
            da, dg = blk['n_in'] + int(blk['has_bias']), blk['n_out']
            b_pos = sl[(name, 'b')][0].start if blk['has_bias'] else -1
            mod.append([blk['n_in'], blk['n_out'], int(blk['has_bias']), blk['R'], sl[(name, 'w')][0].start, b_pos, len(op), len(blk['ops'])])
            for q, rows, cols in zip(blk['ops'], blk['rows'], blk['cols']):
                o = lay['ops'][q]
                op.append([o['a_off'], o['g_off'], o['d_a'], o['d_g'], n_maps, n_maps + len(rows)])
                maps += [np.asarray(rows, np.int32), np.asarray(cols, np.int32)]
                n_maps += len(rows) + len(cols)
            layout['modules'][name] = {'A': (off, da), 'G': (off + da * da, dg)}
            off += da * da + dg * dg
        elems = np.concatenate([np.arange(base, base + int(np.prod(shape))) for (m, _), (base, shape) in prog.grad_leaves.items()
                                if m not in blocks] or [np.zeros(0, np.int64)]).astype(np.int64)
        row = np.zeros(elems.size + 1, np.int64)
        col = np.zeros(0, np.int64)
        if elems.size:
            tabs = np.stack(_rest_gather(prog, elems), 1) if prog._jacobian_gather() else np.zeros((elems.size, 0), np.int64)
            row[1:] = np.cumsum((tabs >= 0).sum(1))
            col = tabs[tabs >= 0].astype(np.int64)        # row-major: per element, ascending multiplicity = ascending column
        layout['diag'] = (off, int(elems.size))
        layout['diag_elems'] = elems
        layout['size'] = off + int(elems.size)
        tabs = dict(mod=np.ascontiguousarray(np.asarray(mod, np.int64).reshape(-1, 8)), op=np.ascontiguousarray(np.asarray(op, np.int64).reshape(-1, 6)),
                    maps=np.ascontiguousarray(np.concatenate(maps or [np.zeros(0, np.int32)]).astype(np.int32)),
                    diag_pos=np.ascontiguousarray(elems), diag_row=row, diag_col=np.ascontiguousarray(col))
        return tabs, layout

    def _ensure_kfac_map(self):
        """Upload the KFAC tables on first use (dqmc_set_kfac_map), after the parameter map."""
        self._ensure_param_map()
        if not self._kfac_map_set:
            self.set_kfac_tables(*self._kfac_tables())

    def set_kfac_tables(self, tabs, layout):
        """Install explicit tables (the dict and layout of _kfac_tables) with dqmc_set_kfac_map: what _ensure_kfac_map does with
        the program's own tables; tests use it with tables of their own."""
        self._ensure_param_map()
        m = _lib.DqmcKfacMap()
        i64 = ctypes.c_int64
        m.n_modules, m.mod, m.n_ops, m.op = tabs['mod'].shape[0], _np_ptr(tabs['mod'], i64), tabs['op'].shape[0], _np_ptr(tabs['op'], i64)
        m.n_maps, m.maps = tabs['maps'].size, _np_ptr(tabs['maps'], ctypes.c_int32)
        m.n_diag, m.diag_pos, m.diag_row, m.diag_col = tabs['diag_pos'].size, _np_ptr(tabs['diag_pos'], i64), \
            _np_ptr(tabs['diag_row'], i64), _np_ptr(tabs['diag_col'], i64)
        self._check(self.lib.dqmc_set_kfac_map(self._ctx, ctypes.byref(m)))
        n = ctypes.c_size_t()
        self._check(self.lib.dqmc_kfac_state_size(self._ctx, ctypes.byref(n)))
        assert n.value == layout['size'], (n.value, layout['size'])
        self._kfac_layout, self._kfac_map_set = layout, True

    def kfac_state_layout(self):
        """The layout of the caller-owned state of kfac_direction (dqmc_kfac_state_size doubles): {'modules': {module:
        {'A': (offset, dim), 'G': (offset, dim)}} in Program.kfac_blocks order (row-major dim x dim matrices, the bias the last
        row of A), 'diag': (offset, n) the F of the elements outside the modules, 'diag_elems': their positions in theta,
        'size'}."""
        self._ensure_kfac_map()
        return self._kfac_layout

    def kfac_state(self):
        """A new state vector for kfac_direction (zeros; a call with first=True overwrites it)."""
        return torch.zeros(self.kfac_state_layout()['size'], dtype=torch.float64, device=self.device)

    def kfac_direction(self, grad_theta, factors_buf, rest, logpsi, sign, state, first, ema, damping, out=None):
        """The KFAC-preconditioned direction of loss.compute_energy_loss_and_kfac on the device (dqmc_kfac_direction):
        grad_theta float64 [n_params] (grad_to_params); factors_buf, rest, logpsi, sign as log_psi_kfac wrote them
        (factors_buf: the flat factor buffer); state: float64 [kfac_state_layout()['size']], updated in place (first: it is
        overwritten, not mixed).  Returns (delta [n_params], dot [1] = <delta, grad_theta>), float64 device tensors; `out`:
        preallocated (delta, dot).  Nothing waits for the host."""
        self._ensure_kfac_map()
        lay = self.program.kfac_layout()
        B = self._arg('logpsi', logpsi, self.dtype, (None,)).shape[0]
        self._arg('sign', sign, torch.int32, (B,))
        self._arg('rest', rest, self.dtype, (B, lay['n_rest']), optional=True)
        self._arg('factors_buf', factors_buf, torch.float64, (lay['n_factor_doubles'],))
        self._arg('state', state, torch.float64, (self._kfac_layout['size'],))
        delta, dot = out if out is not None else (torch.empty(self.program.n_params(), dtype=torch.float64, device=self.device),
                                                  torch.empty(1, dtype=torch.float64, device=self.device))
        self._thetas(grad_theta=grad_theta, delta=delta)
        self._arg('dot', dot, torch.float64, (1,))
        self._check(self.lib.dqmc_kfac_direction(self._ctx, grad_theta.data_ptr(), factors_buf.data_ptr(), _ptr(rest), logpsi.data_ptr(),
                                                 sign.data_ptr(), B, state.data_ptr(), int(bool(first)), float(ema), float(damping),
                                                 delta.data_ptr(), dot.data_ptr()))
        return delta, dot

    def kfac_apply(self, theta, delta, dot, lr, norm_constraint, norms=None):
        """theta += -lr min(1, sqrt(norm_constraint / (lr^2 dot))) delta on the device, then the re-pack (dqmc_kfac_apply);
        norms: optional float64 [4] receiving (param, direction, update) 2-norms and lr^2 dot."""
        self._thetas(norms, 4, theta=theta, delta=delta)
        self._arg('dot', dot, torch.float64, (1,))
        self._ensure_param_map()
        self._check(self.lib.dqmc_kfac_apply(self._ctx, theta.data_ptr(), delta.data_ptr(), dot.data_ptr(), float(lr),
                                             float(norm_constraint), _ptr(norms)))
        self.params_ahead, self._theta_ref = True, theta

    def debug_read_weights(self, which: int):
        """Raw bytes (np.uint8) of a weight buffer of the context (dqmc_debug_read_weights): 0 flat weights, 1 the sub-step
        kernel's tape, 2 the fused kernel's planes, 3 the float64 twin's flat weights, 4 the double copy of a float32 context's flat
        weights.  None if the context has no such buffer."""
        n = self.lib.dqmc_debug_read_weights(self._ctx, int(which), None, 0)
        if n == -4:         # DQMC_E_UNSUPPORTED
            return None
        if n < 0:
            self._check(n)
        out = np.empty(n, np.uint8)
        self._check(self.lib.dqmc_debug_read_weights(self._ctx, int(which), out.ctypes.data_as(ctypes.c_void_p), out.size))
        return out

    def graph_counters(self) -> dict:
        """{captures, replays} of the context's forward-Laplacian graphs (dqmc_graph_counters)."""
        return self._read(self.lib.dqmc_graph_counters, ctypes.c_int64, ('captures', 'replays'))

    # ---- loss assembly of multi-state training (dqmc_psi_ratio, dqmc_clip_rows, dqmc_loss_cotangents) ----
    def psi_ratio(self, log, sign):
        """ratio[S, S, B] from log|psi| and sign [S, S, B] (float64; element [i, j] = psi_i on the samples of state j) by the
        log shift of loss.compute_psi_ratio (dqmc_psi_ratio).  Nothing waits for the host."""
        S, _, B = self._arg('log', log, torch.float64, (None, None, None)).shape
        self._arg('log', log, torch.float64, (S, S, B))
        self._arg('sign', sign, torch.float64, (S, S, B))
        out = torch.empty_like(log)
        self._check(self.lib.dqmc_psi_ratio(self._ctx, log.data_ptr(), sign.data_ptr(), S, B, out.data_ptr()))
        return out

    def clip_rows(self, x, w=None, *, median_center=True, median_scale=False, clip_width=5.0, exclude_width=float('inf')):
        """Row-wise clip of x[n_rows, B] (float64) with each row's own centre (median or mean) and scale (mean or median absolute
        deviation) (dqmc_clip_rows).  Returns (x_clip [n_rows, B], mask bool [n_rows, B], row_stats [n_rows, 4] = centre,
        scale, mean_b(w x_clip), mask count).  A row with a non-finite element comes back non-finite."""
        n, B = self._arg('x', x, torch.float64, (None, None)).shape
        self._arg('w', w, torch.float64, (n, B), optional=True)
        out = torch.empty_like(x)
        mask = torch.empty(n, B, dtype=torch.uint8, device=self.device)
        stats = torch.empty(n, 4, dtype=torch.float64, device=self.device)
        self._check(self.lib.dqmc_clip_rows(self._ctx, x.data_ptr(), _ptr(w), n, B, int(bool(median_center)), int(bool(median_scale)),
                                            float(clip_width), float(exclude_width), out.data_ptr(), mask.data_ptr(), stats.data_ptr()))
        return out, mask.view(torch.bool), stats

    def loss_cotangents(self, e_clip, e_mask, e_stats, w=None, *, alpha=0.0, r_clip=None, r_mask=None, r_stats=None, scale=None,
                        rank=None, spin_kind=None, spin_penalty=0.0, spin=None, spin_mask=None, spin_stats=None, states=None):
        """The cotangents c[S, B] of log|psi_s| on the states' own samples from the clipped energies, optionally the clipped
        ratios and the spin rows (dqmc_loss_cotangents; formulas in include/dqmc.h).  spin_kind: None, 'squared' or 'raising'.
        Returns (c, k): k [n_states, B] the direct weights of the raising kind (else None).  Everything stays on the device."""
        S, B = self._arg('e_clip', e_clip, torch.float64, (None, None)).shape
        t = _lib.DqmcLossTerms()
        keep = []

        def ptr(name, x, shape, dtype=torch.float64):     # (the struct holds integers: `keep` holds the uint8 views)
            keep.append(self._arg(name, x, dtype, shape))
            return keep[-1].data_ptr()
        t.S, t.B = S, B
        t.w = ptr('w', w, (S, B)) if w is not None else None
        t.e_clip, t.e_mask, t.e_stats = e_clip.data_ptr(), ptr('e_mask', e_mask, (S, B), torch.uint8), ptr('e_stats', e_stats, (S, 4))
        t.alpha = float(alpha)
        if r_clip is not None:
            t.r_clip, t.r_mask = ptr('r_clip', r_clip, (S, S, B)), ptr('r_mask', r_mask, (S, S, B), torch.uint8)
            t.r_stats, t.scale, t.rank = ptr('r_stats', r_stats, (S * S, 4)), ptr('scale', scale, (S, S)), ptr('rank', rank, (S,), torch.int32)
        kinds = {None: 0, 'squared': 1, 'raising': 2}
        if spin_kind not in kinds:
            raise ValueError("spin_kind must be None, 'squared' or 'raising'")
        t.spin_kind, t.lam = kinds[spin_kind], float(spin_penalty)
        k = None
        if spin_kind is not None:
            states = list(range(S)) if states is None else [int(q) for q in states]
            n = len(states)
            arr = (ctypes.c_int32 * max(n, 1))(*states)
            t.states_host, t.n_states = arr, n
            t.spin = ptr('spin', spin, (n, B))
            if spin_kind == 'raising':
                t.spin_mask, t.spin_stats = ptr('spin_mask', spin_mask, (n, B), torch.uint8), ptr('spin_stats', spin_stats, (n, 4))
                k = torch.empty(n, B, dtype=torch.float64, device=self.device)
        c = torch.empty(S, B, dtype=torch.float64, device=self.device)
        self._check(self.lib.dqmc_loss_cotangents(self._ctx, ctypes.byref(t), c.data_ptr(), _ptr(k)))
        return c, k

    # ---- observables of the training loop (dqmc_oscillator_strength, dqmc_fd_displace, dqmc_fd_force) ----
    def oscillator_strength(self, r, psi_ratio, e_loc):
        """Oscillator strengths between S electronic states from r [S, B, N, 3] and e_loc [S, B] (the engine's dtype) and
        psi_ratio [S, S, B] (float64, as `psi_ratio` returns it): (os_mean [S, S], os_err [S, S], cd_mean [S, S, 3],
        cd_err [S, S, 3]), float64 device tensors (dqmc_oscillator_strength; formulas in include/dqmc.h).  The diagonal is
        os_mean 0, os_err NaN, as in the reference.  Two launches, nothing waits for the host."""
        r = self._arg('r', self._t(r), self.dtype, (None, None, self.N, 3))
        S, B = r.shape[:2]
        self._arg('psi_ratio', psi_ratio, torch.float64, (S, S, B))
        e_loc = self._arg('e_loc', self._t(e_loc), self.dtype, (S, B))
        os_mean, os_err = (torch.empty(S, S, dtype=torch.float64, device=self.device) for _ in range(2))
        cd_mean, cd_err = (torch.empty(S, S, 3, dtype=torch.float64, device=self.device) for _ in range(2))
        self._check(self.lib.dqmc_oscillator_strength(self._ctx, r.data_ptr(), psi_ratio.data_ptr(), e_loc.data_ptr(), S, B,
                                                      os_mean.data_ptr(), os_err.data_ptr(), cd_mean.data_ptr(), cd_err.data_ptr()))
        return os_mean, os_err, cd_mean, cd_err

    def oscillator_moments(self, S):
        """Test access (dqmc_debug_read -5; a host copy): the moments of the last oscillator_strength call between its two
        launches, (E [S], std_E [S], cd_std [S, S, 3]) as NumPy arrays."""
        out = np.empty(S * (2 + 3 * S), np.float64)
        self._check(self.lib.dqmc_debug_read(self._ctx, -5, _np_ptr(out), out.size))
        return out[:S], out[S:2 * S], out[2 * S:].reshape(S, S, 3)

    def fd_displace(self, r, R=None, h=1e-3):
        """The displaced copies of the finite-difference force (dqmc_fd_displace): (r_d [D, B, N, 3], R_d [D, n_nuc, 3]) in the
        engine's dtype, D = 3 n_nuc; displacement d = 3 n0 + j0 moves nucleus n0 by -h along j0 and every electron by +h times
        its softmax weight of that nucleus (computed in float64)."""
        r, R, B = self._walkers(r, R)
        D = 3 * self.hamil.n_nuc
        r_d = torch.empty(D, B, self.N, 3, dtype=self.dtype, device=self.device)
        R_d = torch.empty(D, self.hamil.n_nuc, 3, dtype=self.dtype, device=self.device)
        self._check(self.lib.dqmc_fd_displace(self._ctx, r.data_ptr(), R.data_ptr(), B, float(h), r_d.data_ptr(), R_d.data_ptr()))
        return r_d, R_d

    def fd_force(self, log_d, log_0, e_d, e_0, h):
        """F [B, n_nuc, 3] float64 = exp(2 (log_d - log_0)) (e_d - e_0) / h from log_d, e_d [D, B] and log_0, e_0 [B] in the
        engine's dtype (dqmc_fd_force)."""
        D = 3 * self.hamil.n_nuc
        B = self._arg('log_0', log_0, self.dtype, (None,)).shape[0]
        self._arg('log_d', log_d, self.dtype, (D, B))
        self._arg('e_d', e_d, self.dtype, (D, B))
        self._arg('e_0', e_0, self.dtype, (B,))
        F = torch.empty(B, self.hamil.n_nuc, 3, dtype=torch.float64, device=self.device)
        self._check(self.lib.dqmc_fd_force(self._ctx, log_d.data_ptr(), log_0.data_ptr(), e_d.data_ptr(), e_0.data_ptr(), B, float(h),
                                           F.data_ptr()))
        return F

    # ---- ansatz.apply ---------------------------------------------------
    def wf_eval(self, r, R=None):
        r, R, B = self._walkers(r, R)
        logpsi, sign = self._psi_out(B)
        self._check(self.lib.dqmc_wf_eval(self._ctx, r.data_ptr(), R.data_ptr(), B, logpsi.data_ptr(),
                                          sign.data_ptr()))
        return sign, logpsi

    # ---- jax.vjp of the batched log|psi| with respect to the parameters ----
    def log_psi_vjp(self, r, cot=None, R=None):
        """sum_b cot[b] d log|psi(r_b)| / d w over the flat weight buffer (loss/loss_function.py:59-75).
        Returns (sign, logpsi, grad_flat): grad_flat is float64 [n_weights] on the engine's device; map it onto the
        parameter tree with `self.program.unflatten_grad`.  cot None = all ones."""
        r, R, B = self._walkers(r, R)
        c = self._cot(cot, B)
        logpsi, sign = self._psi_out(B)
        grad = torch.empty(self.program.weights.size, dtype=torch.float64, device=self.device)
        self._check(self.lib.dqmc_log_psi_vjp(self._ctx, r.data_ptr(), R.data_ptr(), B, _ptr(c), grad.data_ptr(),
                                              logpsi.data_ptr(), sign.data_ptr()))
        return sign, logpsi, grad

    def log_psi_jacobian(self, r, R=None, out=None):
        """Per-walker rows J[b] = d log|psi(r_b)| / d w over the flat weight buffer (dqmc_log_psi_jacobian): the Jacobian that
        log_psi_vjp contracts with its cotangent.  Returns (sign, logpsi, J): J is [B, n_weights] on the engine's device, in the
        engine's dtype; map it onto the parameters with `self.program.unflatten_jacobian`.  `out`: a preallocated [B, ld]
        tensor (ld >= n_weights, unit column stride) that J is a view of; its columns >= n_weights are not touched."""
        r, R, B = self._walkers(r, R)
        nw = self.program.weights.size
        if out is None:
            out = torch.empty(B, nw, dtype=self.dtype, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.dim() != 2 or out.shape[0] != B or out.shape[1] < nw or out.dtype != self.dtype
              or out.device.type != self.device.type or out.stride(1) != 1 or out.stride(0) < nw):      # (strided rows: not _arg's case)
            raise DqmcError(f"'out' must be a [{B}, >= {nw}] {self.dtype} tensor on {self.device} with unit column stride")
        logpsi, sign = self._psi_out(B)
        self._check(self.lib.dqmc_log_psi_jacobian(self._ctx, r.data_ptr(), R.data_ptr(), B, out.data_ptr(),
                                                   out.stride(0), logpsi.data_ptr(), sign.data_ptr()))
        return sign, logpsi, out[:, :nw]

    def kfac_layout(self):
        """(n_linear, n_factor_doubles, n_rest) as the library computes them (dqmc_kfac_layout); Program.kfac_layout has the same."""
        n_lin, n_fac, n_rest = ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
        self._check(self.lib.dqmc_kfac_layout(self._ctx, ctypes.byref(n_lin), ctypes.byref(n_fac), ctypes.byref(n_rest)))
        return n_lin.value, n_fac.value, n_rest.value

    def log_psi_kfac(self, r, cot=None, R=None, rest=True, out=None):
        """The VJP of log_psi_vjp and the KFAC Kronecker factors of every LINEAR op in one reverse pass (dqmc_log_psi_kfac).
        Returns (sign, logpsi, grad, factors, rest): grad float64 [n_weights] as log_psi_vjp's; factors a list of per-op
        (A [d_A, d_A], G [ldw, ldw]) float64 tensors on the device, views of one buffer, in program order
        (Program.kfac_layout); rest [B, n_rest] in the engine's dtype, the per-walker partials of the weight entries no LINEAR
        op owns (columns Program.kfac_layout()['rest_index']), or None with rest=False.  `out`: optional preallocated
        (factor buffer, rest) tensors."""
        r, R, B = self._walkers(r, R)
        c = self._cot(cot, B)
        lay = self.program.kfac_layout()
        fac = out[0] if out is not None else torch.empty(lay['n_factor_doubles'], dtype=torch.float64, device=self.device)
        self._arg('out[0]', fac, torch.float64, (lay['n_factor_doubles'],))
        rst = None
        if rest:
            rst = out[1] if out is not None and out[1] is not None else torch.empty(B, lay['n_rest'], dtype=self.dtype, device=self.device)
            self._arg('out[1]', rst, self.dtype, (B, lay['n_rest']))
        logpsi, sign = self._psi_out(B)
        grad = torch.empty(self.program.weights.size, dtype=torch.float64, device=self.device)
        self._check(self.lib.dqmc_log_psi_kfac(self._ctx, r.data_ptr(), R.data_ptr(), B, _ptr(c), grad.data_ptr(), fac.data_ptr(),
                                               _ptr(rst), logpsi.data_ptr(), sign.data_ptr()))
        factors = [(fac[o['a_off']:o['a_off'] + o['d_a'] ** 2].view(o['d_a'], o['d_a']),
                    fac[o['g_off']:o['g_off'] + o['d_g'] ** 2].view(o['d_g'], o['d_g'])) for o in lay['ops']]
        return sign, logpsi, grad, factors, rst

    # ---- jax.grad of log|psi| with respect to the coordinates; force estimators ----
    def log_psi_grad_coords(self, r, R=None, want_r=True, want_R=True):
        """d log|psi(r_b)| / d r and d log|psi(r_b)| / d R per walker from the reverse pass (dqmc_log_psi_grad_coords).
        Returns (sign, logpsi, grad_r [B, N, 3] or None, grad_R [B, n_nuc, 3] or None) in the engine's dtype on its device.
        Walkers with sign 0 or a non-finite log|psi| get zero rows.  Programs with attention ops raise DqmcError (-4) unless
        option 'attention_reverse' is set to 1 (NeuralNetworkWaveFunction(..., attention_reverse=True)); programs with nuclear
        tokens need Engine(..., nuclear_coords=True), and their stream's part of grad_R is differentiated at the geometry the
        context was compiled for.  want_R=False never runs the stream's backward."""
        if not (want_r or want_R):
            raise ValueError('log_psi_grad_coords: want_r and want_R are both False')
        r, R, B = self._walkers(r, R)
        gr = torch.empty(B, self.N, 3, dtype=self.dtype, device=self.device) if want_r else None
        gR = torch.empty(B, self.hamil.n_nuc, 3, dtype=self.dtype, device=self.device) if want_R else None
        logpsi, sign = self._psi_out(B)
        self._check(self.lib.dqmc_log_psi_grad_coords(self._ctx, r.data_ptr(), R.data_ptr(), B, _ptr(gr), _ptr(gR),
                                                      logpsi.data_ptr(), sign.data_ptr()))
        return sign, logpsi, gr, gR

    def hf_force(self, estimator: str, r, R=None, grad_r=None, grad_R=None, e_loc=None, energy: float = 0.0):
        """Per-walker Hellmann-Feynman force of `estimator` (one of FORCE_ESTIMATORS; formulas at dqmc_hf_force in
        include/dqmc.h) as float64 [B, n_nuc, 3] on the device.  grad_r [B, N, 3] (the ZVQ family), grad_R [B, n_nuc, 3]
        ('ac_zb', 'ac_zvqzb') and e_loc [B] (the estimators with a ZB term) are device tensors in the engine's dtype."""
        if estimator not in FORCE_ESTIMATORS:
            raise ValueError(f'unknown force estimator {estimator!r}; one of {FORCE_ESTIMATORS}')
        r, R, B = self._walkers(r, R)
        self._arg('grad_r', grad_r, self.dtype, (B, self.N, 3), optional=True)
        self._arg('grad_R', grad_R, self.dtype, (B, self.hamil.n_nuc, 3), optional=True)
        self._arg('e_loc', e_loc, self.dtype, (B,), optional=True)
        force = torch.empty(B, self.hamil.n_nuc, 3, dtype=torch.float64, device=self.device)
        self._check(self.lib.dqmc_hf_force(self._ctx, FORCE_ESTIMATORS.index(estimator), r.data_ptr(), R.data_ptr(), B,
                                           _ptr(grad_r), _ptr(grad_R), _ptr(e_loc), float(energy), force.data_ptr()))
        return force

    def ecp_force(self, estimator: str, r, R=None, rng=None, ecp_phi=None, e_loc=None, energy: float = 0.0, rows='own',
                  return_parts=False):
        """Per-walker Hellmann-Feynman force of a Hamiltonian with a Gaussian-type ECP (dqmc_ecp_force; formulas in
        include/dqmc.h), float64 [B, n_nuc, 3] on the device: F_I = F_nuc,I - dV_loc/dR_I - G_I with G the gradient of the
        non-local term.  estimator: 'bare', or 'ac_zb' (bare - 2 (e_loc - energy) d log|psi| / dR_I; e_loc [B] in the engine's
        dtype).  `rng` / `ecp_phi` key the quadrature rotation exactly as in `local_energy`: the same seed or angles give the
        same vertices.  rows: 'own' keeps, for each non-local nucleus, only its own row of the ratio gradient (what the
        reference computes); 'all' keeps every row, the full dV_nl/dR.  return_parts: (force, parts) with parts [2, B, n_nuc, 3]
        = (F_nuc - dV_loc/dR, -G).  Walkers with sign 0 or a non-finite log|psi| get NaN rows.  Attention programs raise
        DqmcError (-4) unless option 'attention_reverse' is set to 1."""
        if estimator not in ('bare', 'ac_zb'):
            raise ValueError(f"unknown ECP force estimator {estimator!r}; one of ('bare', 'ac_zb')")
        if rows not in ('own', 'all'):
            raise ValueError(f"rows must be 'own' or 'all', not {rows!r}")
        r, R, B = self._walkers(r, R)
        if estimator == 'ac_zb' and e_loc is None:
            raise DqmcError("estimator 'ac_zb' needs e_loc")
        e_loc = self._arg('e_loc', e_loc, self.dtype, (B,)) if estimator == 'ac_zb' else None
        self._set_ecp_rotation(B, rng, ecp_phi)
        force = torch.empty(B, self.hamil.n_nuc, 3, dtype=torch.float64, device=self.device)
        parts = torch.empty(2, B, self.hamil.n_nuc, 3, dtype=torch.float64, device=self.device) if return_parts else None
        self._check(self.lib.dqmc_ecp_force(self._ctx, FORCE_ESTIMATORS.index(estimator), 1 if rows == 'all' else 0, r.data_ptr(),
                                            R.data_ptr(), B, _ptr(e_loc), float(energy), force.data_ptr(), _ptr(parts)))
        return (force, parts) if return_parts else force

    # ---- SCF-orbital pretraining: target, Slater matrices, their VJP, the fused loss step ----
    def set_pretrain_target(self, shells, mo_coeffs, confs, conf_coeffs):
        """Upload the (MC-)SCF target of this context (dqmc_set_pretrain_target).  shells: [(atom, (l, coeffs, zetas))] as
        GTOBasis.from_pyscf emits them; mo_coeffs [n_ao, n_mo]; confs [n_conf, N] orbital indices (up first); conf_coeffs
        [n_conf].  Malformed tables raise DqmcError (-1)."""
        atom = np.ascontiguousarray([a for a, _ in shells], np.int32)
        ls = np.ascontiguousarray([sh[0] for _, sh in shells], np.int32)
        cs = [np.asarray(sh[1], np.float64).reshape(-1) for _, sh in shells]
        zs = [np.asarray(sh[2], np.float64).reshape(-1) for _, sh in shells]
        if any(c.size != z.size for c, z in zip(cs, zs)):
            raise ValueError('every shell needs as many coefficients as exponents (one contraction per shell)')
        npr = np.ascontiguousarray([c.size for c in cs], np.int32)
        coeffs, zetas = np.ascontiguousarray(np.concatenate(cs)), np.ascontiguousarray(np.concatenate(zs))
        mo = np.ascontiguousarray(mo_coeffs, np.float64)
        confs = np.ascontiguousarray(confs, np.int32)
        cc = np.ascontiguousarray(conf_coeffs, np.float64).reshape(-1)
        if mo.ndim != 2 or confs.ndim != 2 or confs.shape[1] != self.N or cc.size != confs.shape[0]:
            raise ValueError(f'expected mo_coeffs [n_ao, n_mo], confs [n_conf, {self.N}], conf_coeffs [n_conf]')
        i32 = ctypes.c_int32
        self._check(self.lib.dqmc_set_pretrain_target(self._ctx, len(shells), _np_ptr(atom, i32), _np_ptr(ls, i32), _np_ptr(npr, i32),
                                                      _np_ptr(coeffs), _np_ptr(zetas), mo.shape[0], mo.shape[1], _np_ptr(mo),
                                                      confs.shape[0], _np_ptr(confs, i32), _np_ptr(cc)))
        self.pretrain_n_conf = confs.shape[0]

    def _orb_check(self, r, R):
        if not getattr(self.spec, 'full_determinant', True):
            raise DqmcError('only full-determinant programs expose their orbital matrices')
        return self._walkers(r, R)

    def pretrain_target(self, r, R=None):
        """The target Slater matrices [B, n_conf, N, N] (rows electrons, columns orbitals) of the uploaded table
        (dqmc_pretrain_target), on the device in the engine's dtype."""
        r, R, B = self._walkers(r, R)
        if self.pretrain_n_conf is None:
            raise DqmcError('pretrain_target: no target set (Engine.set_pretrain_target)')
        out = torch.empty(B, self.pretrain_n_conf, self.N, self.N, dtype=self.dtype, device=self.device)
        self._check(self.lib.dqmc_pretrain_target(self._ctx, r.data_ptr(), R.data_ptr(), B, out.data_ptr()))
        return out

    def orbitals(self, r, R=None):
        """The Slater matrices [B, K, N, N] of the value pass (dqmc_orbitals), on the device in the engine's dtype."""
        r, R, B = self._orb_check(r, R)
        out = torch.empty(B, self.spec.n_determinants, self.N, self.N, dtype=self.dtype, device=self.device)
        self._check(self.lib.dqmc_orbitals(self._ctx, r.data_ptr(), R.data_ptr(), B, out.data_ptr()))
        return out

    def orbitals_vjp(self, r, cot, R=None, want_orbitals=True):
        """sum_{b,k,i,mu} cot[b,k,i,mu] d A[b,k,i,mu] / d w over the flat weight buffer (dqmc_orbitals_vjp).  cot: [B, K, N, N].
        Returns (orbitals [B, K, N, N] or None, grad_flat float64 [n_weights]); map grad_flat onto the parameter tree with
        `self.program.unflatten_grad`.  Programs with attention ops raise DqmcError (-4) unless
        option 'attention_reverse' is set to 1 (NeuralNetworkWaveFunction(..., attention_reverse=True))."""
        r, R, B = self._orb_check(r, R)
        shape = (B, self.spec.n_determinants, self.N, self.N)
        c = self._arg('cot', self._t(cot), self.dtype, shape)
        orb = torch.empty(shape, dtype=self.dtype, device=self.device) if want_orbitals else None
        grad = torch.empty(self.program.weights.size, dtype=torch.float64, device=self.device)
        self._check(self.lib.dqmc_orbitals_vjp(self._ctx, r.data_ptr(), R.data_ptr(), B, c.data_ptr(), grad.data_ptr(),
                                               _ptr(orb)))
        return orb, grad

    def pretrain_loss_grad(self, r, R=None, n_total=None):
        """The fused pretraining step (dqmc_pretrain_loss_grad): returns (per_sample_loss float64 [B], grad_flat float64
        [n_weights]) with grad_flat = d (sum_b per_sample_loss[b] / n_total) / d w; n_total defaults to B."""
        r, R, B = self._orb_check(r, R)
        ps = torch.empty(B, dtype=torch.float64, device=self.device)
        grad = torch.empty(self.program.weights.size, dtype=torch.float64, device=self.device)
        self._check(self.lib.dqmc_pretrain_loss_grad(self._ctx, r.data_ptr(), R.data_ptr(), B,
                                                     float(B if n_total is None else n_total), grad.data_ptr(), ps.data_ptr()))
        return ps, grad

    def _set_ecp_rotation(self, B, rng, ecp_phi):
        """The quadrature rotation of the following call (dqmc_ecp_rotation): an int seed, or explicit angles [B, n_ecp_nl, N].
        Nothing to do without a non-local ECP channel."""
        if getattr(getattr(self.hamil, 'pot', None), 'nl_params', np.zeros(0)).size:
            if rng is None and ecp_phi is None:      # gaussian_type_ecp.py:183 `assert rng is not None`
                raise DqmcError('a Hamiltonian with a non-local ECP needs `rng` (the seed of the quadrature rotation)')
            if ecp_phi is None and not isinstance(rng, (int, np.integer)):
                raise DqmcError('`rng` must be an integer seed')
            self._ecp_phi = self._t(ecp_phi) if ecp_phi is not None else None      # keep alive during the call
            if self._ecp_phi is not None and self._ecp_phi.shape[0] != B:
                raise DqmcError('ecp_phi must have one row per walker')
            seed = int(rng) & (2 ** 64 - 1) if isinstance(rng, (int, np.integer)) else 0
            self._check(self.lib.dqmc_ecp_rotation(self._ctx, seed, _ptr(self._ecp_phi)))

    # ---- hamil.local_energy ---------------------------------------------
    def local_energy(self, phys_conf, rng=None, return_grad=False, ecp_phi=None, static_io=False):
        """`rng` (an int seed or None) keys the random quadrature rotation of the non-local ECP term
        (hamil.py:166, gaussian_type_ecp.py:221); `ecp_phi` [B, n_ecp_nl, N] overrides it with explicit
        angles (parity tests).  Both are ignored without an ECP.  `static_io`: the call reads the walkers from, and writes its
        results to, buffers the engine keeps per batch size (copies in and out), so that a training loop presents the same
        pointers at every step and the captured forward-Laplacian graph is replayed instead of re-captured."""
        if isinstance(phys_conf, PhysicalConfiguration):
            r, R = phys_conf.r, phys_conf.R
        else:
            r, R = phys_conf, None
        r, R, B = self._walkers(r, R)
        self._set_ecp_rotation(B, rng, ecp_phi)
        static_io = static_io and not return_grad
        if static_io:
            if B not in self._static_io:
                self._static_io[B] = (torch.empty(B, self.N, 3, dtype=self.dtype, device=self.device), torch.empty_like(R),
                                      torch.empty(B, dtype=self.dtype, device=self.device),
                                      torch.empty(6, B, dtype=self.dtype, device=self.device))
            r_in, R_in, e, st = self._static_io[B]
            r_in.copy_(r)
            if R is not self.R:          # (a sampler stacks a new R tensor per step: same values, another pointer)
                R_in.copy_(R)
                R = R_in
            r = r_in
        else:
            e = torch.empty(B, dtype=self.dtype, device=self.device)
            st = torch.empty(6, B, dtype=self.dtype, device=self.device)
        grad = torch.empty(B, 3 * self.N, dtype=self.dtype, device=self.device) if return_grad else None
        self._check(self.lib.dqmc_local_energy(self._ctx, r.data_ptr(), R.data_ptr(), B, e.data_ptr(),
                                               st.data_ptr(), _ptr(grad), None, None))
        if static_io:
            e, st = e.clone(), st.clone()
        stats = {k: st[i] for i, k in enumerate(STAT_KEYS)}
        return (e, stats, grad) if return_grad else (e, stats)

    def psi_and_grad(self, r, R=None):
        """(sign, log|psi|, grad log|psi| [B,N,3]) in one forward-Laplacian pass -- what the reference's
        LangevinSampler obtains with value_and_grad (electron_samplers.py:193-201).  No potential terms and
        no ECP quadrature run (dqmc_psi_grad)."""
        r, R, B = self._walkers(r, R)
        grad = torch.empty(B, 3 * self.N, dtype=self.dtype, device=self.device)
        logpsi, sign = self._psi_out(B)
        self._check(self.lib.dqmc_psi_grad(self._ctx, r.data_ptr(), R.data_ptr(), B, logpsi.data_ptr(),
                                           sign.data_ptr(), grad.data_ptr()))
        return sign, logpsi, grad.reshape(B, self.N, 3)

    # ---- sampler ----------------------------------------------------------
    def _check_state(self, state, keys, R):
        """The prologue of the sampler entry points: (B, the geometry tensor of the call, the device pointers of the tensors `keys`
        of the state, which the library updates in place)."""
        B = self._arg("state['r']", state['r'], self.dtype, (None, self.N, 3)).shape[0]
        want = {'r': (self.dtype, (B, self.N, 3)), 'force': (self.dtype, (B, self.N, 3)), 'log': (self.dtype, (B,)),
                'tau': (self.dtype, (1,)), 'sign': (torch.int32, (B,)), 'age': (torch.int32, (B,))}
        return B, self._R(R), [self._arg(f"state['{k}']", state[k], *want[k]).data_ptr() for k in keys]

    def _sampler_io(self, lead, noise, unif, return_accept):
        """What the sampler entry points share: (acc uint8 [*lead] or None, the host stats array, noise [*lead, N, 3] or None,
        unif [*lead] or None)."""
        acc = torch.empty(*lead, dtype=torch.uint8, device=self.device) if return_accept else None
        noise = self._arg('noise', self._t(noise), self.dtype, (*lead, self.N, 3)) if noise is not None else None
        unif = self._arg('unif', self._t(unif), self.dtype, lead) if unif is not None else None
        return acc, (ctypes.c_double * len(SAMPLER_STAT_KEYS))(), noise, unif

    @staticmethod
    def _sampler_result(stats, acc, want_stats=True):
        out = dict(zip(SAMPLER_STAT_KEYS, stats)) if want_stats else {}
        return out if acc is None else (out, acc)

    def _molz(self, charges):
        z = np.ascontiguousarray(charges, np.float64)
        if z.shape != (self.hamil.n_nuc,):
            raise DqmcError(f"'mol_charges' must have shape ({self.hamil.n_nuc},), got {z.shape}")
        return z, _np_ptr(z)

    def mcmc_steps(self, state: Dict[str, torch.Tensor], n_sub: int, *, max_age=None, target_acceptance=0.57,
                   seed: int = 0, noise=None, unif=None, R=None, want_stats=True, return_accept=False):
        """In-place Metropolis sub-steps on state {'r','log','sign','age','tau'} (device tensors)."""
        B, R, (r, log, sign, age, tau) = self._check_state(state, ('r', 'log', 'sign', 'age', 'tau'), R)
        acc, stats, noise, unif = self._sampler_io((n_sub, B), noise, unif, return_accept)
        self._check(self.lib.dqmc_mcmc_steps(
            self._ctx, r, log, sign, age, tau, R.data_ptr(), B, n_sub, -1 if max_age is None else int(max_age),
            -1.0 if target_acceptance is None else float(target_acceptance), int(seed), _ptr(noise), _ptr(unif), _ptr(acc),
            stats if want_stats else None))
        return self._sampler_result(stats, acc, want_stats)

    def langevin_update(self, r, tau, mol_charges, R=None):
        """LangevinSampler._update (electron_samplers.py:193-208): (sign, log|psi|, cleaned drift [B,N,3])."""
        r, R, B = self._walkers(r, R)
        tau = self._arg('tau', self._t(tau).reshape(-1), self.dtype, (1,))
        z, zp = self._molz(mol_charges)
        logpsi, sign = self._psi_out(B)
        force = torch.empty(B, self.N, 3, dtype=self.dtype, device=self.device)
        self._check(self.lib.dqmc_langevin_update(self._ctx, r.data_ptr(), R.data_ptr(), zp, B, tau.data_ptr(),
                                                  logpsi.data_ptr(), sign.data_ptr(), force.data_ptr()))
        return sign, logpsi, force

    def langevin_steps(self, state, n_sub, mol_charges, *, max_age=None, target_acceptance=0.57, seed=0, noise=None, unif=None,
                       R=None, want_stats=True, return_accept=False):
        """In-place Langevin sub-steps on state {'r','log','sign','age','tau','force'} (dqmc_langevin_steps)."""
        B, R, (r, log, sign, age, force, tau) = self._check_state(state, ('r', 'log', 'sign', 'age', 'force', 'tau'), R)
        acc, stats, noise, unif = self._sampler_io((n_sub, B), noise, unif, return_accept)
        z, zp = self._molz(mol_charges)
        self._check(self.lib.dqmc_langevin_steps(
            self._ctx, r, log, sign, age, force, tau, R.data_ptr(), zp, B, n_sub,
            -1 if max_age is None else int(max_age), -1.0 if target_acceptance is None else float(target_acceptance), int(seed),
            _ptr(noise), _ptr(unif), _ptr(acc), stats if want_stats else None))
        return self._sampler_result(stats, acc, want_stats)

    def exchange_step(self, state, up_idx, down_idx, unif, R=None, return_accept=False):
        """One opposite-spin exchange step, in place on state {'r','log','sign','age','tau'} (dqmc_exchange_step)."""
        B, R, (r, log, sign, age, tau) = self._check_state(state, ('r', 'log', 'sign', 'age', 'tau'), R)
        for name, idx, n in (('up_idx', up_idx, self.hamil.n_up), ('down_idx', down_idx, self.hamil.n_down)):
            host = idx if isinstance(idx, np.ndarray) else (idx if isinstance(idx, torch.Tensor) and idx.device.type == 'cpu' else None)
            if host is not None and len(host) and (int(host.min()) < 0 or int(host.max()) >= n):     # device tensors: clamped in the kernel
                raise DqmcError(f'{name} must lie in [0, {n})')
        up, dn = (self._arg(name, torch.as_tensor(idx, device=self.device).to(torch.int32).contiguous(), torch.int32, (B,))
                  for name, idx in (('up_idx', up_idx), ('down_idx', down_idx)))
        acc, stats, _, u = self._sampler_io((B,), None, unif, return_accept)
        self._check(self.lib.dqmc_exchange_step(self._ctx, r, log, sign, age, tau, R.data_ptr(), B,
                                                up.data_ptr(), dn.data_ptr(), u.data_ptr(), _ptr(acc), stats))
        return self._sampler_result(stats, acc)

    def energy_record(self, e_loc, w=None):
        B = self.check_walker_vector('e_loc', e_loc).shape[0]
        self._arg('w', w, self.dtype, (B,), optional=True)
        rec = (ctypes.c_double * 7)()
        self._check(self.lib.dqmc_energy_stats(self._ctx, e_loc.data_ptr(), _ptr(w), B, rec))
        return np.array(list(rec))

    def merge_energy_records(self, records: np.ndarray):
        records = np.ascontiguousarray(records, np.float64).reshape(-1, 7)
        out = (ctypes.c_double * 5)()
        self._check(self.lib.dqmc_merge_energy_stats(_np_ptr(records), records.shape[0], out))
        return dict(zip(('local_energy/mean', 'local_energy/std', 'local_energy/min', 'local_energy/max',
                         'local_energy/weighted_mean'), list(out)))

    # ---- debug / timing ---------------------------------------------------
    def debug_read(self, name_or_idx, B: int):
        TP = self.lib.dqmc_debug_lanes(self._ctx)
        if name_or_idx == 'logdet':
            shape, idx = (B, self.spec.n_determinants, TP), -1
        elif name_or_idx == 'sign_k':
            shape, idx = (B, self.spec.n_determinants), -2
        elif name_or_idx == 'kappa':      # conditioning record per walker (kernels_head.hip), last Laplacian-mode call
            shape, idx = (B,), -4
        else:
            idx = self.program.buf_names[name_or_idx] if isinstance(name_or_idx, str) else int(name_or_idx)
            rows, width = self.program.bufs[idx]
            shape = (B, rows, TP, width)
        out = np.empty(shape, np.float64)
        self._check(self.lib.dqmc_debug_read(self._ctx, idx, _np_ptr(out), out.size))
        return out

    def last_refined(self) -> int:
        """Walkers the last local-energy call re-evaluated in float64 (dqmc_last_refined)."""
        return int(self.lib.dqmc_last_refined(self._ctx))

    def refine_info(self) -> dict:
        """State of the float64 refinement after the last local-energy call (dqmc_refine_info)."""
        # ('error_per_score': the scale m of the exponential error model, float32 error = m x score x xi)
        out = self._read(self.lib.dqmc_refine_info, ctypes.c_double, ('mode', 'score_threshold', 'error_per_score', 'direct_f64_calls_left'))
        out['mode'], out['direct_f64_calls_left'] = int(out['mode']), int(out['direct_f64_calls_left'])
        return out

    def refine_counters(self) -> dict:
        """Running counts of the context (dqmc_refine_counters): local-energy calls, calls evaluated in float64 whole,
        calibration probes, walkers re-evaluated in float64."""
        return self._read(self.lib.dqmc_refine_counters, ctypes.c_int64, ('calls', 'direct_f64_calls', 'probe_calls', 'walkers_refined'))

    def substep_kernel(self) -> str:
        """Name of the plan-specialised sub-step kernel bound to this context's program (dqmc_substep_kernel), '' if none."""
        buf = ctypes.create_string_buffer(128)
        rc = self.lib.dqmc_substep_kernel(self._ctx, buf, 128)
        if rc < 0:
            self._check(rc)
        return buf.value.decode()

    def refine_scores(self, n: int) -> np.ndarray:
        """Error-predictor scores of the first n walkers of the last float32 forward-Laplacian pass (dqmc_refine_scores)."""
        out = np.empty(int(n), np.float64)
        self._check(self.lib.dqmc_refine_scores(self._ctx, _np_ptr(out), int(n)))
        return out

    def last_chunks(self) -> dict:
        """Walker chunks the last local-energy call was split into (dqmc_last_chunks): the context's own pass and its
        float64 twin's."""
        return self._read(self.lib.dqmc_last_chunks, ctypes.c_int, ('own', 'twin'))

    def ecp_counts(self) -> dict:
        """(nucleus, electron) pairs of the last mixed-precision ECP quadrature by class (dqmc_ecp_counts)."""
        return self._read(self.lib.dqmc_ecp_counts, ctypes.c_int64, ('f32', 'f64', 'dropped'))

    def set_option(self, name: str, value: int):
        self._check(self.lib.dqmc_set_option(self._ctx, name.encode(), int(value)))
        self._options[name] = int(value)      # (what the caller chose: apply(return_mos=True) restores it)
        if name == 'nuclear_params':          # (Program.kfac_blocks and the package's gates read it)
            self.nuclear_params = self.program.nuclear_params = bool(value)

    def get_option(self, name: str, default: int) -> int:
        """The value last set through set_option (the library has no getter), else `default`."""
        return self._options.get(name, default)

    def timing(self, enable=True):
        self._check(self.lib.dqmc_timing_enable(self._ctx, int(enable)))

    def timing_reset(self):
        self._check(self.lib.dqmc_timing_reset(self._ctx))

    def timing_report(self):
        buf = ctypes.create_string_buffer(1024)
        self._check(self.lib.dqmc_timing_names(self._ctx, buf, 1024))
        out = {}
        for nm in filter(None, buf.value.decode().split(',')):
            ms, n, fl = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
            self._check(self.lib.dqmc_timing_get(self._ctx, nm.encode(), ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)))
            ex = ctypes.c_double()
            self._check(self.lib.dqmc_timing_get_executed(self._ctx, nm.encode(), ctypes.byref(ex)))
            out[nm] = {'ms': ms.value, 'launches': n.value, 'flops': fl.value, 'flops_executed': ex.value}
        return out
