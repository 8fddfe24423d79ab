"""The shapes between the ones every other test uses, through the SIMT emulation of the unmodified kernels: embedding widths,
two_particle_dim and head widths that are no multiple of the kernels' tiles (odd two_particle_dim; head widths 9, 10, 11, 18),
and electron counts on both sides of every kernel-selection boundary of the determinant and linear kernels.  Reference: the
float64 interpreter on the same walkers; no walker is left out of any check.  tests/test_gpu_shape_grid.py runs the same cases
on the device, with every electron count of the grid."""
import ctypes

import pytest
import torch

from shape_grid_util import (B64, F32_CASES, MLP_CASES, N_F32, N_F64, N_PSIFORMER, N_REVERSE, PSIFORMER_CASES,
                             TRANSPSIFORMER_CASES, chain_setup, chain_walkers, check_f32, check_f64, check_ill_conditioned,
                             check_metropolis_bit_exact,
                             check_psi_both_paths, check_value_determinants, check_vjp_and_coords, make_walkers, width_setup)
from simt_util import emu_lib

# Emulated subsets of N_F64 and N_F32 (the emulation and the interpreter both cost ~N^4; the largest sizes take 10 .. 20 s
# each): every boundary of the determinant kernels, and one size of each linear tile (64, 96, 176 and 192 lanes: 58 and 59
# share their tiles with 53 and 63).
N_F64_EMU = [n for n in N_F64 if n not in (58, 59)]
N_F32_EMU = [n for n in N_F32 if n <= 48]


@pytest.mark.parametrize('name,molname,d,e,k', MLP_CASES)
def test_emu_f64_pair_widths(name, molname, d, e, k):
    """FermiNet / PauliNet at embedding_dim d, two_particle_dim e: local energy, psi through both value paths, reverse pass."""
    spec, mol, h, tree, eng = width_setup(name, molname, d, e, k, torch.float64, 'cpu', emu_lib())
    r = make_walkers(mol, h.n_elec, B64)
    check_f64(eng, mol, r, 'cpu')
    check_psi_both_paths(eng, mol, r, 'cpu')
    check_vjp_and_coords(eng, spec, h, tree, r, 'cpu', tol=1e-9)


@pytest.mark.parametrize('molname,d,heads', PSIFORMER_CASES)
def test_emu_f64_head_widths(molname, d, heads):
    """Psiformer at head width d / heads with options attention_mfma 0, 1 and 2, then the reverse pass through attention."""
    spec, mol, h, tree, eng = width_setup('psiformer', molname, d, heads, 2, torch.float64, 'cpu', emu_lib())
    r = make_walkers(mol, h.n_elec, B64)
    for mfma in (0, 2, 1):
        eng.set_option('attention_mfma', mfma)
        check_f64(eng, mol, r, 'cpu')
        check_psi_both_paths(eng, mol, r, 'cpu')
    check_vjp_and_coords(eng, spec, h, tree, r, 'cpu', tol=1e-9)


@pytest.mark.parametrize('molname,d,heads', TRANSPSIFORMER_CASES)
def test_emu_f64_head_widths_nuclear_tokens(molname, d, heads):
    """TransPsiformer (constant nuclear key / value rows) at head widths 9 and 12: the forward checks."""
    spec, mol, h, tree, eng = width_setup('transpsiformer', molname, d, heads, 2, torch.float64, 'cpu', emu_lib())
    r = make_walkers(mol, h.n_elec, B64)
    check_f64(eng, mol, r, 'cpu')
    check_psi_both_paths(eng, mol, r, 'cpu')


@pytest.mark.parametrize('name,molname,d,second,k', F32_CASES)
def test_emu_f32_widths(name, molname, d, second, k):
    spec, mol, h, tree, eng = width_setup(name, molname, d, second, k, torch.float32, 'cpu', emu_lib())
    check_f32(eng, mol, spec, 'cpu')


def test_emu_metropolis_odd_pair_width_bit_exact():
    """Two Metropolis sub-steps of LiH / PauliNet at two_particle_dim 5 on given noise against oracle/sampling.py."""
    spec, mol, h, tree, eng = width_setup('paulinet', 'LiH', 16, 5, 2, torch.float64, 'cpu', emu_lib())
    check_metropolis_bit_exact(eng, spec, mol, h, tree, 'cpu')


@pytest.mark.parametrize('name,molname,d,second', [('paulinet', 'LiH', 16, 5), ('ferminet', 'LiH', 16, 7), ('psiformer', 'LiH', 18, 2)])
def test_emu_padding_columns_in_stale_memory(name, molname, d, second):
    """The emulation's device allocations are zero-filled, which hides a padding column nobody writes: a LINEAR op reads it
    against zero weight rows and gets 0 x 0.  With every new block filled with 0xFF bytes (NaN in both types, as the stale
    workspace of a real device can be) the aggregate padding of an odd two_particle_dim and the attention padding of an
    embedding_dim that is no multiple of 4 must still give the interpreter's numbers, in the Laplacian pass and in wf_eval one
    launch per op."""
    fill = ctypes.c_longlong.in_dll(emu_lib(), 'simt_alloc_fill')
    fill.value = 0xFF
    try:
        spec, mol, h, tree, eng = width_setup(name, molname, d, second, 2, torch.float64, 'cpu', emu_lib())
        r = make_walkers(mol, h.n_elec, B64)
        check_f64(eng, mol, r, 'cpu')
        check_psi_both_paths(eng, mol, r, 'cpu')
    finally:
        fill.value = 0


def test_emu_ill_conditioned_53_electrons():
    spec, mol, h, tree, eng = chain_setup('ferminet', 53, torch.float64, 'cpu', emu_lib())
    check_ill_conditioned(eng, mol, 53, 'cpu')


@pytest.mark.parametrize('n', N_F64_EMU)
def test_emu_f64_electron_counts(n):
    """Narrow FermiNet on the chain molecule: local energy with the MFMA determinant kernel where profitable (option
    slogdet_mfma 1), never (0) and from 9 electrons on (2); value determinants with the register and the LDS-resident LU."""
    spec, mol, h, tree, eng = chain_setup('ferminet', n, torch.float64, 'cpu', emu_lib())
    r = chain_walkers(eng, mol, n)
    check_f64(eng, mol, r, 'cpu', options=(1, 0, 2) if n > 8 else (1, 0))
    check_value_determinants(eng, mol, r, 'cpu')


@pytest.mark.parametrize('n', N_REVERSE)
def test_emu_reverse_pass_electron_counts(n):
    spec, mol, h, tree, eng = chain_setup('ferminet', n, torch.float64, 'cpu', emu_lib())
    check_vjp_and_coords(eng, spec, h, tree, chain_walkers(eng, mol, n), 'cpu', tol=1e-9)


@pytest.mark.parametrize('n', N_F32_EMU)
def test_emu_f32_electron_counts(n):
    spec, mol, h, tree, eng = chain_setup('ferminet', n, torch.float32, 'cpu', emu_lib())
    check_f32(eng, mol, spec, 'cpu')


@pytest.mark.parametrize('n', N_PSIFORMER)
def test_emu_f64_psiformer_key_tiles(n):
    """Psiformer at the key-tile boundaries of the MFMA attention kernels."""
    spec, mol, h, tree, eng = chain_setup('psiformer', n, torch.float64, 'cpu', emu_lib())
    check_f64(eng, mol, chain_walkers(eng, mol, n), 'cpu')
