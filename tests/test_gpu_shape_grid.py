"""The shapes between the ones every other test uses, on the MI355X: embedding widths, two_particle_dim and head widths that
are no multiple of the kernels' tiles, and the electron counts on both sides of every kernel-selection boundary of the
determinant and linear kernels (the cases of tests/shape_grid_util.py, all of them).  Reference: the float64 interpreter on the
same walkers.  Every case writes its deviations to shape_grid_report.json beside the other parity reports."""
import json
import os

import pytest
import torch

from test_gpu_parity import OUT          # the directory the parity reports go to
from shape_grid_util import (B64, F32_CASES, MLP_CASES, N_F32, N_F64, N_PSIFORMER, N_REVERSE, PSIFORMER_CASES,
                             TRANSPSIFORMER_CASES, chain_setup, chain_walkers, check_f32, check_f64, check_ill_conditioned,
                             check_metropolis_bit_exact,
                             check_psi_both_paths, check_value_determinants, check_vjp_and_coords, deviations, make_walkers,
                             width_setup)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def report(name, payload):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, 'shape_grid_report.json')
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[name] = payload
    json.dump(data, open(path, 'w'), indent=1)


@pytest.mark.parametrize('name,molname,d,e,k', MLP_CASES)
def test_f64_pair_widths(name, molname, d, e, k):
    """FermiNet / PauliNet at embedding_dim d, two_particle_dim e: local energy, psi through both value paths, reverse pass."""
    spec, mol, h, tree, eng = width_setup(name, molname, d, e, k, torch.float64, DEV)
    r = make_walkers(mol, h.n_elec, B64)
    dev = deviations(check_f64(eng, mol, r, DEV), eng, mol, r)
    dev['logpsi_abs'] = check_psi_both_paths(eng, mol, r, DEV)
    report(f'f64_{name}_{molname}_{d}_{e}_{k}', dev)
    check_vjp_and_coords(eng, spec, h, tree, r, DEV, tol=1e-9)


@pytest.mark.parametrize('molname,d,heads', PSIFORMER_CASES)
def test_f64_head_widths(molname, d, heads):
    """Psiformer at head width d / heads with options attention_mfma 0, 1 and 2, then the reverse pass through attention."""
    spec, mol, h, tree, eng = width_setup('psiformer', molname, d, heads, 2, torch.float64, DEV)
    r = make_walkers(mol, h.n_elec, B64)
    dev = {}
    for mfma in (0, 2, 1):
        eng.set_option('attention_mfma', mfma)
        dev[f'attention_mfma_{mfma}'] = deviations(check_f64(eng, mol, r, DEV), eng, mol, r)
        dev[f'attention_mfma_{mfma}']['logpsi_abs'] = check_psi_both_paths(eng, mol, r, DEV)
    report(f'f64_psiformer_{molname}_{d}_{heads}', dev)
    check_vjp_and_coords(eng, spec, h, tree, r, DEV, tol=1e-9)


@pytest.mark.parametrize('molname,d,heads', TRANSPSIFORMER_CASES)
def test_f64_head_widths_nuclear_tokens(molname, d, heads):
    """TransPsiformer (constant nuclear key / value rows) at head widths 9 and 12: the forward checks."""
    spec, mol, h, tree, eng = width_setup('transpsiformer', molname, d, heads, 2, torch.float64, DEV)
    r = make_walkers(mol, h.n_elec, B64)
    dev = deviations(check_f64(eng, mol, r, DEV), eng, mol, r)
    dev['logpsi_abs'] = check_psi_both_paths(eng, mol, r, DEV)
    report(f'f64_transpsiformer_{molname}_{d}_{heads}', dev)


@pytest.mark.parametrize('name,molname,d,second,k', F32_CASES)
def test_f32_widths(name, molname, d, second, k):
    spec, mol, h, tree, eng = width_setup(name, molname, d, second, k, torch.float32, DEV)
    report(f'f32_{name}_{molname}_{d}_{second}_{k}', {'err_over_bound': check_f32(eng, mol, spec, DEV)})


def test_metropolis_odd_pair_width_bit_exact():
    """Two Metropolis sub-steps of LiH / PauliNet at two_particle_dim 5 on given noise against oracle/sampling.py."""
    spec, mol, h, tree, eng = width_setup('paulinet', 'LiH', 16, 5, 2, torch.float64, DEV)
    check_metropolis_bit_exact(eng, spec, mol, h, tree, DEV)


@pytest.mark.parametrize('n', N_F64)
def test_f64_electron_counts(n):
    """Narrow FermiNet on the chain molecule: local energy with the MFMA determinant kernel where profitable (option
    slogdet_mfma 1), never (0) and from 9 electrons on (2); value determinants with the register and the LDS-resident LU."""
    spec, mol, h, tree, eng = chain_setup('ferminet', n, torch.float64, DEV)
    r = chain_walkers(eng, mol, n)
    dev = deviations(check_f64(eng, mol, r, DEV, options=(1, 0, 2) if n > 8 else (1, 0)), eng, mol, r)
    dev.update(check_value_determinants(eng, mol, r, DEV))
    report(f'f64_ferminet_chain_{n}', dev)


def test_f64_ill_conditioned_53_electrons():
    """The default-seed walkers at 53 electrons (cond(A) 2e7), which the grid above passes over: bound scaled by cond(A)."""
    spec, mol, h, tree, eng = chain_setup('ferminet', 53, torch.float64, DEV)
    report('f64_ferminet_chain_53_seed_1', check_ill_conditioned(eng, mol, 53, DEV))


@pytest.mark.parametrize('n', N_REVERSE)
def test_reverse_pass_electron_counts(n):
    spec, mol, h, tree, eng = chain_setup('ferminet', n, torch.float64, DEV)
    check_vjp_and_coords(eng, spec, h, tree, chain_walkers(eng, mol, n), DEV, tol=1e-9)


@pytest.mark.parametrize('n', N_F32)
def test_f32_electron_counts(n):
    spec, mol, h, tree, eng = chain_setup('ferminet', n, torch.float32, DEV)
    report(f'f32_ferminet_chain_{n}', {'err_over_bound': check_f32(eng, mol, spec, DEV)})


@pytest.mark.parametrize('n', N_PSIFORMER)
def test_f64_psiformer_key_tiles(n):
    """Psiformer at the key-tile boundaries of the MFMA attention kernels."""
    spec, mol, h, tree, eng = chain_setup('psiformer', n, torch.float64, DEV)
    r = chain_walkers(eng, mol, n)
    report(f'f64_psiformer_chain_{n}', deviations(check_f64(eng, mol, r, DEV), eng, mol, r))
