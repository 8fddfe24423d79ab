"""SCF-orbital pretraining on the MI355X: the GTO target, the orbital VJP and the fused loss step in float64 against the
restatement and torch.autograd through the oracle, float32 against float64, and a short `pretrain` run with a real sampler."""
import numpy as np
import pytest
import torch

from deepqmc_amd import MolecularHamiltonian, Molecule
from deepqmc_amd.engine import Engine
from deepqmc_amd.params import init_params
from deepqmc_amd.pretrain import adam, pretrain
from deepqmc_amd.sampling import (DecorrSampler, MoleculeIdxSampler, MultiElectronicStateSampler, MultiNuclearGeometrySampler,
                                  synthetic_walkers)
from deepqmc_amd.spec import ANSATZES
from deepqmc_amd.wf import NeuralNetworkWaveFunction
from oracle import geom
from param_grad_util import leaf_errors
from pretrain_util import check_loss_grad, check_orbitals_vjp, check_target, make, synthetic_dataset, upload

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = [('paulinet', 'LiH', 256), ('ferminet', 'N2', 64)]


@pytest.mark.parametrize('name,mol,B', CASES)
@pytest.mark.parametrize('kind', ['hf', 'cas'])
def test_target_matches_restatement_gpu(name, mol, B, kind):
    h, spec, tree, eng, r = make(name, mol, B, DEV)
    check_target(eng, h, synthetic_dataset(h, kind, seed=1), r, rtol=1e-8)


@pytest.mark.parametrize('name,mol,B', CASES)
def test_orbitals_vjp_matches_oracle_autograd_gpu(name, mol, B):
    h, spec, tree, eng, r = make(name, mol, B, DEV)
    check_orbitals_vjp(eng, spec, h, tree, r, tol=1e-8)


@pytest.mark.parametrize('name,mol,B', CASES)
def test_pretrain_loss_grad_matches_restated_loss_gpu(name, mol, B):
    h, spec, tree, eng, r = make(name, mol, B, DEV)
    check_loss_grad(eng, spec, h, tree, r, synthetic_dataset(h, 'cas', seed=2), tol=1e-8, loss_rtol=1e-8, ps_rtol=1e-8)


def test_float32_against_float64():
    """Every one of the 4096 walkers is compared: there is no determinant inverse in this path, hence no near-node walkers to
    set aside.  Target: largest deviation relative to the largest entry (orbitals have zeros, so an entrywise ratio means
    nothing); per-sample losses: largest entrywise relative deviation; gradient: largest leaf-relative deviation."""
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = ANSATZES['paulinet']()
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=7, perturb_envelopes=0.1)
    ds = synthetic_dataset(h, 'cas', seed=3)
    B = 4096
    r = synthetic_walkers(h, B, seed=11)
    T, ps, g = {}, {}, {}
    for dt in (torch.float64, torch.float32):
        eng = Engine(spec, h, tree, dtype=dt, device=DEV, norm_eps=geom.F32_EPS)
        upload(eng, ds)
        rr = torch.as_tensor(r, dtype=dt, device=DEV)
        T[dt] = eng.pretrain_target(rr).double().cpu().numpy()
        p, gf = eng.pretrain_loss_grad(rr)
        ps[dt], g[dt] = p.cpu().numpy(), eng.program.unflatten_grad(gf)
        eng.close()
    e_t = float(np.abs(T[torch.float32] - T[torch.float64]).max() / np.abs(T[torch.float64]).max())
    e_p = float(np.max(np.abs(ps[torch.float32] - ps[torch.float64]) / ps[torch.float64]))
    err = leaf_errors(g[torch.float32], g[torch.float64])
    worst = max(err, key=err.get)
    print(f'float32 vs float64, LiH / PauliNet, {B} walkers: target {e_t:.2e}, per-sample losses {e_p:.2e}, '
          f'gradient {err[worst]:.2e} ({worst})')
    # Measured with the SIMT emulation of these kernels (tests/simt, the same sources compiled for the CPU; 4096 walkers,
    # float32 against float64): target 2.8e-7, per-sample losses 4.7e-7, gradient 1.3e-7 (256 walkers: 2.2e-7, 3.1e-7,
    # 1.4e-7).  NOT yet measured on the MI355X: no GPU run of this test has been made, so the figures above stand in for the
    # hardware ones until the line printed above has been read off a GPU run and entered here.  Each bound is 10 x the
    # measured value (one decade covers the spread between seeds and machines that the other float32 tests of this suite show).
    assert e_t < 2.8e-6, e_t
    assert e_p < 4.7e-6, e_p
    assert err[worst] < 1.3e-6, (worst, err[worst])


class _Recording:
    """Passes everything on to the sampler and keeps the state it was given and the electron positions it returned."""

    def __init__(self, sampler):
        self.sampler, self.seen, self.given = sampler, [], []

    def sample(self, rng, state, params, mol_idxs):
        self.given.append(state)
        state, pc, stats = self.sampler.sample(rng, state, params, mol_idxs)
        self.seen.append(pc.r.clone())
        return state, pc, stats

    def update(self, state, params):
        return self.sampler.update(state, params)


def test_pretrain_run_with_decorr_sampler():
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    wf = NeuralNetworkWaveFunction(h, 'paulinet', dtype=torch.float32, device=DEV)
    params = [wf.init(3, perturb_envelopes=0.1)]
    ds = synthetic_dataset(h, 'cas', seed=3)
    sampler = _Recording(MultiNuclearGeometrySampler(MultiElectronicStateSampler(DecorrSampler(h, wf, length=10), 1)))
    R = torch.as_tensor(np.asarray(h.mol.coords)[None], dtype=torch.float32, device=DEV)
    state = sampler.sampler.init(5, params, 512, R)
    losses = []
    for step, params, ps, mol_idxs in pretrain(1, h, wf, params, adam(3e-4), MoleculeIdxSampler(0, 1, 1), sampler, state, ds, None, range(20)):
        assert ps.shape == (1, 1, 512) and bool(torch.isfinite(ps).all()), step
        losses.append(float(ps.mean()))
    assert step == 19 and len(sampler.seen) == 20
    assert all(np.isfinite(np.asarray(v)).all() for lv in params[0].values() for v in lv.values())
    # the sampler state advanced: the first step started from the initial state, later ones did not, and the walkers moved
    assert sampler.given[0] is state and all(g is not state for g in sampler.given[1:])
    moved = [float((sampler.seen[k] - sampler.seen[k - 1]).abs().max()) for k in range(1, 20)]
    assert min(moved) > 0
    print('pretrain, LiH / PauliNet, float32, 512 walkers: loss', losses[0], '->', losses[-1])
