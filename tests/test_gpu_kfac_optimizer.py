"""The device-resident KFAC step on the MI355X: the blocked Cholesky solve at the real factor dimensions of the default specs,
the direction against the tree path at 256 walkers, determinism, and a float32 training run with KFACOptimizer whose
forward-Laplacian graph keeps being replayed."""
import numpy as np
import pytest
import torch

from deepqmc_amd import MolecularHamiltonian, Molecule
from deepqmc_amd.fit import TrainState, fit_wf
from deepqmc_amd.optimizer import KFACOptimizer
from deepqmc_amd.sampling import MoleculeIdxSampler, synthetic_walkers
from deepqmc_amd.spec import ANSATZES
from deepqmc_amd.wf import NeuralNetworkWaveFunction
from oracle import geom
from kfac_optimizer_util import (DAMPING, check_flat_against_tree, check_solve_against_kron, check_solve_residual, check_two_op_module,
                                 covered_shapes, synthetic_inputs)
from optimizer_util import make_pair, training_setup
from param_jacobian_util import jac_engine

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SMALL = dict(embedding_dim=32, n_interactions=1, n_determinants=2)


def test_solve_kernels_on_synthetic_factors_gpu():
    """Test 1 of the emulated suite on the hardware (dense Kronecker reference, 1e-10 per module), the two-op module, and two
    identical calls bit for bit."""
    *_, eng, _ = jac_engine('paulinet', 'LiH', 2, DEV, None, **SMALL)
    cov = covered_shapes(eng.program, eng.KFAC_PANEL)
    for key in ('one', 'off_panel', 'two_panels_and_rest', 'bias', 'no_bias'):
        assert cov[key], (key, cov)
    check_solve_against_kron(eng)
    x = synthetic_inputs(eng, 6, 3)
    n = eng.program.n_params()
    outs = []
    for _ in range(2):
        st = eng.kfac_state()
        eng.kfac_direction(x['g'], x['fac'], x['rest'], x['logpsi'], x['sign'], st, True, 0.95, DAMPING)
        buf_d = torch.full((n + 6,), float('nan'), dtype=torch.float64, device=DEV)
        buf_s = torch.full((4,), float('nan'), dtype=torch.float64, device=DEV)
        delta, dot = eng.kfac_direction(x['g'], x['fac'], x['rest'], x['logpsi'], x['sign'], st, False, 0.9, DAMPING, out=(buf_d[:n], buf_s[:1]))
        assert torch.isfinite(buf_d[:n]).all() and torch.isnan(buf_d[n:]).all() and torch.isnan(buf_s[1:]).all()
        outs.append((delta.clone(), dot.clone(), st.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    *_, eng2, _ = jac_engine('paulinet', 'LiH', 2, DEV, None, **SMALL)
    check_two_op_module(eng2)


@pytest.mark.parametrize('name,mol', [('paulinet', 'LiH'), ('ferminet', 'N2')])
def test_solve_residual_at_the_default_specs_gpu(name, mol):
    """The real 449- and 833-dimensional factors (synthetic SPD) in float64.  The dense Kronecker matrix is out of reach, so the
    check is the residual max|A_d delta G_d - g| / max|g|; it may be 10 x the residual torch's cholesky_solve pair leaves on the
    same inputs (the largest over the modules, for both)."""
    h, spec, tree, eng, _ = make_pair(name, mol, torch.float64, DEV)
    cov = covered_shapes(eng.program, eng.KFAC_PANEL)
    print(name, mol, 'factor dimensions', cov['dims'])
    assert max(cov['dims']) >= (800 if mol == 'N2' else 440)
    mine, ref, rows = check_solve_residual(eng)
    for r in rows:
        print(f'{r[0]:90s} {str(r[1]):12s} kernels {r[2]:.3e}  torch {r[3]:.3e}')
    print(f'{name} / {mol}: largest residual of the kernels {mine:.3e}, of torch.cholesky_solve {ref:.3e}')
    assert mine <= 10 * ref, (mine, ref)


def test_direction_against_the_tree_path_gpu():
    """Test 2 of the emulated suite at 256 walkers, float64, LiH / PauliNet at the default spec."""
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    wf = NeuralNetworkWaveFunction(h, ANSATZES['paulinet'](), dtype=torch.float64, device=DEV, norm_eps=geom.F32_EPS)
    trees = [wf.init(0, perturb_envelopes=0.1)]
    batch = lambda seed: torch.as_tensor(synthetic_walkers(h, 256, seed=seed), device=DEV)[None, None]
    check_flat_against_tree(h, wf, trees, batch(30), batch(77))


def test_kfac_training_run_replays_its_graph():
    """Twenty float32 steps of fit_wf with KFACOptimizer() at 4096 walkers on LiH / PauliNet: every E_loc mean is finite and
    the forward-Laplacian graph is captured at most twice and replayed ever after, as with the other device-resident
    optimisers."""
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = ANSATZES['paulinet']()
    wf, params, sampler, st = training_setup(h, spec, torch.float32, DEV, None, 1, 4096, 10, seed=3)
    means, norms = [], []
    for _, state, _, stats in fit_wf(3, h, wf, KFACOptimizer(), MoleculeIdxSampler(0, 1, 1), sampler, range(20),
                                     TrainState(st, params, None), None):
        means.append(float(stats['local_energy/mean'].mean()))
        norms.append([float(stats[k][0]) for k in ('opt/param_norm', 'opt/grad_norm', 'opt/update_norm', 'opt/scaled_grad_norm_sq')])
    assert len(means) == 20 and np.isfinite(means).all(), means
    assert np.isfinite(norms).all(), norms
    c = wf.engine(params[0]).graph_counters()
    print('E_loc mean', means[0], '->', means[-1], 'graph counters', c, 'last norms', norms[-1])
    assert c['captures'] <= 2 and c['replays'] > c['captures'], c
