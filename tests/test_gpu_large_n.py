"""The electron counts between and beyond the benchmark systems' on the MI355X: 80- / 112- / 144- / 208-lane linear tiles, the
4 x 4-tile MFMA determinant kernel against the scalar one, float32 contexts at library defaults, the reverse pass at 64
electrons and one training step at 22.  Narrow ansatzes; a few seconds per test."""
import json
import os

import numpy as np
import pytest
import torch

from deepqmc_amd.fit import TrainState, fit_wf
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.optimizer import AdamOptimizer
from deepqmc_amd.sampling import MoleculeIdxSampler
from oracle import geom
from oracle.program_interp import Interp
from test_gpu_parity import OUT          # the directory the parity reports go to
from large_n_util import check_f32_pass_alone, check_f64, check_vjp_and_coords, make_walkers, molecule, narrow_spec, setup

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def report(name, payload):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, 'large_n_report.json')
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[name] = payload
    json.dump(data, open(path, 'w'), indent=1)


@pytest.mark.parametrize('name,n', [('ferminet', 22), ('ferminet', 32), ('ferminet', 43), ('ferminet', 45), ('ferminet', 49),
                                    ('ferminet', 64), ('psiformer', 22), ('psiformer', 49), ('psiformer', 64)])
def test_f64_local_energy(name, n):
    """The float64 assertions of test_gpu_parity.py::test_f64_every_buffer for three walkers, from 45 electrons on with the MFMA
    determinant kernel and with the scalar one; two identical calls are bit-identical."""
    spec, mol, h, tree, eng = setup(name, n, torch.float64, DEV)
    r = make_walkers(mol, n, 3)
    check_f64(eng, mol, r, DEV, options=(1, 0) if n >= 45 else (None,))
    rt = torch.as_tensor(r, device=DEV)
    e1, _, g1 = eng.local_energy(rt, return_grad=True)
    e1, g1 = e1.clone(), g1.clone()
    e2, _, g2 = eng.local_energy(rt, return_grad=True)
    assert torch.equal(e1, e2) and torch.equal(g1, g2)


@pytest.mark.parametrize('n', [49, 64])
def test_mfma_determinants_against_scalar(n):
    """k_slogdet_mfma64 against k_slogdet_dyn on the same orbitals: every lane of every determinant within 1e-9 relative of the
    scalar kernel's lane, with the absolute floor 1e-8 of the interpreter comparison (check_f64) for lanes that cancel; the
    same signs.  Prints the largest per-lane relative error and how many lanes needed the floor."""
    spec, mol, h, tree, eng = setup('ferminet', n, torch.float64, DEV)
    rt = torch.as_tensor(make_walkers(mol, n, 3), device=DEV)
    got = {}
    for opt in (1, 0):
        eng.set_option('slogdet_mfma', opt)
        eng.local_energy(rt)
        got[opt] = (eng.debug_read('logdet', 3).copy(), eng.debug_read('sign_k', 3).copy())
    T = 3 * n + 2
    mfma, scalar = got[1][0][..., :T], got[0][0][..., :T]
    diff = np.abs(mfma - scalar)
    rel = diff / np.maximum(np.abs(scalar), 1e-300)
    floor = (diff > 1e-9 * np.abs(scalar)) & (diff <= 1e-8 + 1e-9 * np.abs(scalar))
    print(f'N={n}: MFMA against scalar determinant lanes, largest per-lane relative error {rel.max():.2e} '
          f'(abs {diff.flat[rel.argmax()]:.2e} on a lane of {np.abs(scalar).flat[rel.argmax()]:.2e}), smallest |lane| {np.abs(scalar).min():.2e}, '
          f'{int(floor.sum())} of {rel.size} lanes needed the 1e-8 floor')
    report(f'mfma_vs_scalar_{n}', {'rel_err_max': float(rel.max()), 'lanes_on_floor': int(floor.sum()), 'lanes': int(rel.size)})
    np.testing.assert_array_equal(got[1][1], got[0][1])
    np.testing.assert_allclose(got[1][0], got[0][0], rtol=1e-9, atol=1e-8)


@pytest.mark.parametrize('n', [22, 36, 49, 64])
def test_f32_local_energy(n):
    """float32 contexts at library defaults (refinement on), 16 walkers: the assertions of test_gpu_parity.py::test_f32_local_energy."""
    B = 16
    spec, mol, h, tree, eng = setup('ferminet', n, torch.float32, DEV)
    r = make_walkers(mol, n, B).astype(np.float32)
    it = Interp(eng.program, mol.charges, geom.F32_EPS)
    ref = it.run(r.astype(np.float64), mol.coords.astype(np.float32).astype(np.float64), laplacian=True)
    e, stats, grad = eng.local_energy(torch.as_tensor(r, device=DEV), return_grad=True)
    n_refined = eng.last_refined()
    sign, logpsi = eng.wf_eval(torch.as_tensor(r, device=DEV))
    rel = np.abs(e.cpu().numpy() - ref['e_loc']) / np.maximum(1.0, np.abs(ref['e_loc']))
    lp = np.abs(logpsi.cpu().numpy() - ref['log'])
    K = spec.n_determinants
    A = it.bufs[eng.program.buf_names['orbitals']][:, :, 0, :n * n].reshape(B, K, n, n)
    cond = np.linalg.cond(A).max(1)
    report(f'f32_eloc_ferminet_{n}', {'B': B, 'n_refined': int(n_refined), 'rel_err_median': float(np.median(rel)),
                                      'rel_err_max': float(rel.max()), 'logpsi_abs_err_max': float(lp.max()),
                                      'cond_median': float(np.median(cond)), 'cond_max': float(cond.max()),
                                      'err_over_cond_eps_max': float((rel / (cond * 1.2e-7)).max())})
    print(f'N={n}: n_refined {n_refined}, rel err median {np.median(rel):.2e} max {rel.max():.2e}, cond median {np.median(cond):.2e}')
    np.testing.assert_array_equal(sign.cpu().numpy(), ref['sign'])       # bit-exact item
    assert np.all(np.isfinite(rel))
    assert np.median(rel) < 1e-5 or np.median(rel / (cond * 1.2e-7)) < 1.0
    if np.median(cond) < 1e4:
        assert np.quantile(rel, 0.9) < 1e-4
    assert (rel / (cond * 1.2e-7)).max() < 50.0
    assert np.median(lp) < (1e-5 if np.median(cond) < 1e4 else 1e-3)
    rel0 = check_f32_pass_alone(eng, it, spec, r, ref, DEV)
    report(f'f32_eloc_ferminet_{n}_refine_off', {'rel_err_median': float(np.median(rel0)), 'rel_err_max': float(rel0.max())})


def test_reverse_pass_64_electrons():
    spec, mol, h, tree, eng = setup('ferminet', 64, torch.float64, DEV)
    check_vjp_and_coords(eng, spec, h, tree, make_walkers(mol, 64, 3), DEV)


def test_fit_step_22_electrons():
    """One fit_wf step with Adam at N = 22 (float32, 64 walkers): finite loss, parameters changed."""
    from optimizer_util import training_setup
    h = MolecularHamiltonian(mol=molecule(22))
    wf, params, sampler, st = training_setup(h, narrow_spec('ferminet'), torch.float32, DEV, None, 1, 64, 2, seed=3)
    prog = wf.engine(params[0]).program
    start = prog.flatten_params(params[0]).copy()
    for _, state, _, stats in fit_wf(3, h, wf, AdamOptimizer(1e-3), MoleculeIdxSampler(0, 1, 1), sampler, range(1),
                                     TrainState(st, params, None), None):
        mean = float(stats['local_energy/mean'].mean())
        theta = state.opt[0]['theta'].cpu().numpy().copy()
    assert np.isfinite(mean), mean
    assert np.isfinite(theta).all() and not np.array_equal(theta, start)
    assert float(stats['opt/update_norm'][0]) > 0
