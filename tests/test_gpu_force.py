"""Coordinate gradients of log|psi| (dqmc_log_psi_grad_coords) and the Hellmann-Feynman force estimators (dqmc_hf_force) on
the MI355X: float64 against torch.autograd through the oracle, d log|psi| / d R against central finite differences of
wf_eval, float32 against float64, bit-identical repeats and chunks, and every estimator against a torch restatement of its
formula on inputs from the library."""
import numpy as np
import pytest
import torch

from deepqmc_amd import MolecularHamiltonian, Molecule, force
from deepqmc_amd.engine import Engine
from deepqmc_amd.params import init_params
from deepqmc_amd.sampling import synthetic_walkers
from deepqmc_amd.spec import ANSATZES
from deepqmc_amd.types import PhysicalConfiguration
from deepqmc_amd.wf import NeuralNetworkWaveFunction
from force_util import check_coords_against_oracle, restated_force, walker_errors
from oracle import geom

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('name,mol,B', [('paulinet', 'LiH', 256), ('ferminet', 'N2', 64)])
def test_grad_coords_match_oracle_autograd_gpu(name, mol, B):
    check_coords_against_oracle(name, mol, B, DEV, tol=1e-8)


def _setup(name='paulinet', mol='LiH', seed=7):
    h = MolecularHamiltonian(mol=Molecule.from_name(mol))
    spec = ANSATZES[name]()
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=seed, perturb_envelopes=0.1)
    return h, spec, tree


def test_grad_R_against_finite_differences():
    h, spec, tree = _setup()
    eng = Engine(spec, h, tree, dtype=torch.float64, device=DEV, norm_eps=geom.F32_EPS)
    r = torch.as_tensor(synthetic_walkers(h, 64, seed=5), device=DEV)
    _, _, _, gR = eng.log_psi_grad_coords(r)
    R0 = torch.as_tensor(h.mol.coords, dtype=torch.float64, device=DEV)
    fd = torch.zeros_like(gR)
    step = 1e-5
    for a in range(h.n_nuc):
        for x in range(3):
            Rp, Rm = R0.clone(), R0.clone()
            Rp[a, x] += step
            Rm[a, x] -= step
            fd[:, a, x] = (eng.wf_eval(r, Rp)[1] - eng.wf_eval(r, Rm)[1]) / (2 * step)
    err = walker_errors(gR.cpu().numpy(), fd.cpu().numpy())
    # measured: median 3e-10; a walker with an electron close to a nucleus carries the O(step^2) truncation error of the
    # difference (1.5e-5 for one of the 64), the oracle comparison above checks every walker at 1e-8
    assert np.median(err) < 1e-8 and np.quantile(err, 0.95) < 1e-6, (np.median(err), np.quantile(err, 0.95))


# float32 against float64 at 4096 LiH / PauliNet walkers, over the walkers whose float32 log|psi| is within 1e-5 of float64
# (away from a node of psi).  Measured normwise per-walker error on the MI355X: grad_r median 1.2e-6, 99th percentile 8.7e-6,
# max 1.1e-5; grad_R median 1.1e-6, 99th percentile 9.0e-6, max 1.3e-5.  Bounds: (median, 99th percentile), about 5x that.
F32_BOUNDS = {'grad_r': (5e-6, 5e-5), 'grad_R': (5e-6, 5e-5)}


def test_float32_against_float64():
    h, spec, tree = _setup()
    r = synthetic_walkers(h, 4096, seed=11)
    out = {}
    for dt in (torch.float64, torch.float32):
        eng = Engine(spec, h, tree, dtype=dt, device=DEV, norm_eps=geom.F32_EPS)
        out[dt] = [t.double().cpu() for t in eng.log_psi_grad_coords(torch.as_tensor(r, dtype=dt, device=DEV))]
        eng.close()
    good = ((out[torch.float32][1] - out[torch.float64][1]).abs() < 1e-5).numpy()
    assert good.mean() > 0.9
    for k, name in ((2, 'grad_r'), (3, 'grad_R')):
        err = walker_errors(out[torch.float32][k].numpy(), out[torch.float64][k].numpy())[good]
        med, q99 = np.median(err), np.quantile(err, 0.99)
        print(f'{name}: float32 vs float64 normwise per-walker error: median {med:.2e}, 99th percentile {q99:.2e}, max {err.max():.2e}')
        assert med < F32_BOUNDS[name][0] and q99 < F32_BOUNDS[name][1], (name, med, q99)


def test_repeats_and_chunks_are_bit_identical_gpu():
    h, spec, tree = _setup('ferminet', 'N2')
    eng = Engine(spec, h, tree, dtype=torch.float32, device=DEV)
    r = torch.as_tensor(synthetic_walkers(h, 4096, seed=2), dtype=torch.float32, device=DEV)
    out0 = eng.log_psi_grad_coords(r)
    out1 = eng.log_psi_grad_coords(r)
    assert all(torch.equal(a, b) for a, b in zip(out0, out1))
    assert eng.last_chunks()['own'] == 1
    eng.set_option('ws_budget_mb', 64)
    out2 = eng.log_psi_grad_coords(r)
    assert eng.last_chunks()['own'] > 1
    assert all(torch.equal(a, b) for a, b in zip(out0, out2))


def _inputs(wf, params, B, seed):
    h = wf.hamil
    r = torch.as_tensor(synthetic_walkers(h, B, seed=seed), dtype=wf.dtype, device=DEV)
    pc = PhysicalConfiguration(torch.as_tensor(h.mol.coords, dtype=wf.dtype, device=DEV), r, torch.zeros(B, dtype=torch.int64))
    e_loc, _ = h.local_energy(wf)(None, params, pc)
    return h, r, pc, e_loc, float(e_loc.double().mean())


def test_estimators_match_restated_formulas_gpu():
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    wf = NeuralNetworkWaveFunction(h, 'paulinet', dtype=torch.float32, device=DEV)
    params = wf.init(0, perturb_envelopes=0.1)
    h, r, pc, e_loc, energy = _inputs(wf, params, 4096, 3)
    eng = wf.engine(params)
    g_r = eng.psi_and_grad(r)[2]
    _, gr, gR = wf.log_psi_grad_coords(params, pc)
    R, Z = h.mol.coords.astype(np.float32), h.mol.charges
    for est in ('nuclear', 'bare', 'ac_zvq', 'ac_zvzbq', 'ac_zb', 'ac_zvqzb'):
        f = eng.hf_force(est, r, grad_r=g_r, grad_R=gR, e_loc=e_loc, energy=energy)
        assert f.dtype == torch.float64 and f.shape == (4096, h.n_nuc, 3) and f.device.type == 'cuda', est
        ref = restated_force(est, r, R, Z, grad_r=g_r, grad_R=gR, e_loc=e_loc, energy=energy)
        err = walker_errors(f.cpu().numpy(), ref.numpy())
        assert err.max() < 1e-10, (est, err.max())
    # the force.py surface on the same batch: the estimators without grad_r are the kernel's output exactly; the ZVQ family
    # takes grad_r from its own dqmc_psi_grad call (float32 with the float64 refinement of that call)
    assert torch.equal(force.evaluate_hf_force_bare(h, wf)(None, params, pc), eng.hf_force('bare', r))
    assert torch.equal(force.evaluate_hf_force_ac_zb(h, wf)(None, params, pc, e_loc, energy),
                       eng.hf_force('ac_zb', r, grad_R=gR, e_loc=e_loc, energy=energy))
    np.testing.assert_allclose(force.nuclear_force(R, pc, Z).cpu().numpy(), eng.hf_force('nuclear', r).cpu().numpy(), rtol=1e-12)
    for make, args in ((force.evaluate_hf_force_ac_zvq, ()), (force.evaluate_hf_force_ac_zvzbq, (e_loc, energy)),
                       (force.evaluate_hf_force_ac_zvqzb, (e_loc, energy))):
        f = make(h, wf)(params, pc, *args)
        ref = eng.hf_force(make(h, wf).estimator, r, grad_r=g_r, grad_R=gR, e_loc=e_loc, energy=energy)
        assert np.median(walker_errors(f.cpu().numpy(), ref.cpu().numpy())) < 1e-4, make.__name__
    a = force.antithetic_wrapper(force.evaluate_hf_force_ac_zvq(h, wf), wf, 0.5)(None, params, pc)
    assert a.shape == (4096, h.n_nuc, 3) and bool(torch.isfinite(a).all())


def test_ac_zvq_on_psiformer():
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    wf = NeuralNetworkWaveFunction(h, 'psiformer', dtype=torch.float32, device=DEV)
    params = wf.init(0)
    h, r, pc, e_loc, energy = _inputs(wf, params, 256, 8)
    eng = wf.engine(params)
    g_r = eng.psi_and_grad(r)[2]
    f = eng.hf_force('ac_zvq', r, grad_r=g_r)
    ref = restated_force('ac_zvq', r, h.mol.coords.astype(np.float32), h.mol.charges, grad_r=g_r)
    assert walker_errors(f.cpu().numpy(), ref.numpy()).max() < 1e-10
    for f2 in (force.evaluate_hf_force_ac_zvq(h, wf)(params, pc), force.evaluate_hf_force_ac_zvzbq(h, wf)(params, pc, e_loc, energy)):
        assert f2.shape == (256, h.n_nuc, 3) and bool(torch.isfinite(f2).all())
