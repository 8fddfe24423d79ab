"""ctypes binding of libdqmc_hip.so (C ABI: include/dqmc.h).

There is no fallback: if the HIP library has not been built, `load()` raises.  Build it with
`python -c "import __graft_entry__ as g; g.build()"` (hipcc --offload-arch=gfx950).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_int, c_int32, c_int64, c_size_t, c_uint8, c_uint64, c_void_p

from .program import DqmcBuf, DqmcOp, DqmcSystem

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc')
LIB_PATH = os.path.join(CSRC, 'libdqmc_hip.so')


class DqmcLossTerms(ctypes.Structure):
    """dqmc_loss_terms of include/dqmc.h."""
    _fields_ = [('S', c_int), ('B', c_int), ('w', c_void_p), ('e_clip', c_void_p), ('e_mask', c_void_p), ('e_stats', c_void_p),
                ('alpha', c_double), ('r_clip', c_void_p), ('r_mask', c_void_p), ('r_stats', c_void_p), ('scale', c_void_p),
                ('rank', c_void_p), ('spin_kind', c_int), ('lam', c_double), ('spin', c_void_p), ('spin_mask', c_void_p),
                ('spin_stats', c_void_p), ('states_host', POINTER(c_int32)), ('n_states', c_int)]


class DqmcKfacMap(ctypes.Structure):
    """dqmc_kfac_map of include/dqmc.h."""
    _fields_ = [('n_modules', c_int), ('mod', POINTER(c_int64)), ('n_ops', c_int), ('op', POINTER(c_int64)), ('n_maps', c_size_t),
                ('maps', POINTER(c_int32)), ('n_diag', c_size_t), ('diag_pos', POINTER(c_int64)), ('diag_row', POINTER(c_int64)),
                ('diag_col', POINTER(c_int64))]


class DqmcNucLinear(ctypes.Structure):
    """dqmc_nuc_linear of include/dqmc.h."""
    _fields_ = [('w', c_int64), ('b', c_int64), ('n_in', c_int32), ('n_out', c_int32), ('act', c_int32), ('reserved', c_int32)]


class DqmcNucStream(ctypes.Structure):
    """dqmc_nuc_stream of include/dqmc.h."""
    _fields_ = [('n_nuc', c_int32), ('n_layers', c_int32), ('heads', c_int32), ('dim', c_int32), ('n_det', c_int32), ('n_env', c_int32),
                ('n_edge_lin', c_int32), ('n_embed_lin', c_int32), ('n_mlp_lin', c_int32), ('n_lin', c_int32),
                ('lin', POINTER(DqmcNucLinear)), ('zbias_up', c_int64), ('zbias_down', c_int64), ('nuc_types', POINTER(c_int32)),
                ('R', POINTER(c_double)), ('n_derived', c_int64), ('sc_row', POINTER(c_int64)), ('sc_col', POINTER(c_int32)),
                ('theta', POINTER(c_double))]


# every symbol include/dqmc.h declares: (name, restype, argtypes)
SIGNATURES = [
    ('dqmc_create', c_int, [POINTER(c_void_p), c_int, c_void_p, POINTER(DqmcSystem), POINTER(c_double),
                            POINTER(DqmcBuf), c_int, POINTER(DqmcOp), c_int, POINTER(c_double), c_size_t,
                            POINTER(c_int32), c_size_t]),
    ('dqmc_destroy', None, [c_void_p]),
    ('dqmc_last_error', c_char_p, []),
    ('dqmc_set_weights', c_int, [c_void_p, POINTER(c_double), c_size_t]),
    ('dqmc_set_param_map', c_int, [c_void_p, POINTER(c_int32), c_size_t, c_size_t]),
    ('dqmc_set_nuclear_stream', c_int, [c_void_p, POINTER(DqmcNucStream)]),
    ('dqmc_weights_from_params', c_int, [c_void_p, c_void_p]),
    ('dqmc_grad_to_params', c_int, [c_void_p, c_void_p, c_void_p]),
    ('dqmc_jacobian_to_params', c_int, [c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_void_p, c_void_p, c_size_t]),
    ('dqmc_adam_step', c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_double, c_double, c_double, c_double,
                               c_int64, c_void_p]),
    ('dqmc_apply_update', c_int, [c_void_p, c_void_p, c_void_p, c_double, c_void_p]),
    ('dqmc_set_kfac_map', c_int, [c_void_p, POINTER(DqmcKfacMap)]),
    ('dqmc_kfac_state_size', c_int, [c_void_p, POINTER(c_size_t)]),
    ('dqmc_kfac_direction', c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_double,
                                    c_double, c_void_p, c_void_p]),
    ('dqmc_kfac_apply', c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double, c_void_p]),
    ('dqmc_debug_read_weights', c_int, [c_void_p, c_int, c_void_p, c_size_t]),
    ('dqmc_debug_nuc_dx_time', c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    ('dqmc_graph_counters', c_int, [c_void_p, POINTER(c_int64)]),
    ('dqmc_psi_ratio', c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    ('dqmc_clip_rows', c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_double, c_double, c_void_p, c_void_p, c_void_p]),
    ('dqmc_loss_cotangents', c_int, [c_void_p, POINTER(DqmcLossTerms), c_void_p, c_void_p]),
    ('dqmc_oscillator_strength', c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    ('dqmc_fd_displace', c_int, [c_void_p, c_void_p, c_void_p, c_int, c_double, c_void_p, c_void_p]),
    ('dqmc_fd_force', c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_double, c_void_p]),
    ('dqmc_wf_eval', c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    ('dqmc_local_energy', c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ('dqmc_psi_grad', c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    ('dqmc_log_psi_vjp', c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    ('dqmc_log_psi_jacobian', c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    ('dqmc_kfac_layout', c_int, [c_void_p, POINTER(c_int), POINTER(c_size_t), POINTER(c_size_t)]),
    ('dqmc_log_psi_kfac', c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ('dqmc_log_psi_grad_coords', c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    ('dqmc_hf_force', c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_double, c_void_p]),
    ('dqmc_ecp_force', c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_double, c_void_p, c_void_p]),
    ('dqmc_set_pretrain_target', c_int, [c_void_p, c_int, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_double),
                                         POINTER(c_double), c_int, c_int, POINTER(c_double), c_int, POINTER(c_int32), POINTER(c_double)]),
    ('dqmc_pretrain_target', c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    ('dqmc_orbitals', c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    ('dqmc_orbitals_vjp', c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    ('dqmc_pretrain_loss_grad', c_int, [c_void_p, c_void_p, c_void_p, c_int, c_double, c_void_p, c_void_p]),
    ('dqmc_mcmc_steps', c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                c_int, c_double, c_uint64, c_void_p, c_void_p, c_void_p, POINTER(c_double)]),
    ('dqmc_langevin_update', c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_double), c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    ('dqmc_langevin_steps', c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_double),
                                    c_int, c_int, c_int, c_double, c_uint64, c_void_p, c_void_p, c_void_p, POINTER(c_double)]),
    ('dqmc_exchange_step', c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                   c_void_p, c_void_p, POINTER(c_double)]),
    ('dqmc_set_ecp', c_int, [c_void_p, c_int, POINTER(c_double), c_int, c_int, POINTER(c_double)]),
    ('dqmc_ecp_rotation', c_int, [c_void_p, c_uint64, c_void_p]),
    ('dqmc_set_pseudo_hamiltonian', c_int, [c_void_p, c_int, c_double, POINTER(c_double), POINTER(c_double), POINTER(c_int32)]),
    ('dqmc_energy_stats', c_int, [c_void_p, c_void_p, c_void_p, c_int, POINTER(c_double)]),
    ('dqmc_energy_stats_allgather', c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, POINTER(c_double)]),
    ('dqmc_merge_energy_stats', c_int, [POINTER(c_double), c_int, POINTER(c_double)]),
    ('dqmc_debug_read', c_int, [c_void_p, c_int, POINTER(c_double), c_size_t]),
    ('dqmc_debug_lanes', c_int, [c_void_p]),
    ('dqmc_last_refined', c_int, [c_void_p]),
    ('dqmc_refine_info', c_int, [c_void_p, POINTER(c_double)]),
    ('dqmc_last_chunks', c_int, [c_void_p, POINTER(c_int)]),
    ('dqmc_ecp_counts', c_int, [c_void_p, POINTER(c_int64)]),
    ('dqmc_refine_counters', c_int, [c_void_p, POINTER(c_int64)]),
    ('dqmc_substep_kernel', c_int, [c_void_p, c_char_p, c_size_t]),
    ('dqmc_refine_scores', c_int, [c_void_p, POINTER(c_double), c_int]),
    ('dqmc_set_option', c_int, [c_void_p, c_char_p, c_int]),
    ('dqmc_timing_enable', c_int, [c_void_p, c_int]),
    ('dqmc_timing_reset', c_int, [c_void_p]),
    ('dqmc_timing_get', c_int, [c_void_p, c_char_p, POINTER(c_double), POINTER(c_int64), POINTER(c_double)]),
    ('dqmc_timing_get_executed', c_int, [c_void_p, c_char_p, POINTER(c_double)]),
    ('dqmc_timing_names', c_int, [c_void_p, c_char_p, c_size_t]),
]


def bind(lib: ctypes.CDLL) -> ctypes.CDLL:
    """Attach argtypes/restype for every entry point; raises AttributeError if one is missing."""
    for name, restype, argtypes in SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    return lib


_cached = None


def load() -> ctypes.CDLL:
    global _cached
    if _cached is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} not found: the HIP library is not built. Run '
                '`python -c "import __graft_entry__ as g; g.build()"` (needs hipcc); there is no CPU fallback.')
        _cached = bind(ctypes.CDLL(LIB_PATH))
    return _cached
