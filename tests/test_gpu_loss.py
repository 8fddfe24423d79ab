"""The multi-state training loss on the MI355X: the assembly kernels against torch at walker counts below and beyond one pass of
a workgroup, the end-to-end loss and gradients at the default LiH / PauliNet spec, fit_wf with a loss function against the
host-path loop in float64, and a float32 two-state training run whose forward-Laplacian graphs keep being replayed."""
import math

import numpy as np
import pytest
import torch

from deepqmc_amd import MolecularHamiltonian, Molecule
from deepqmc_amd.fit import TrainState, fit_wf
from deepqmc_amd.loss import create_loss_fn
from deepqmc_amd.optimizer import AdamOptimizer
from deepqmc_amd.sampling import MoleculeIdxSampler
from deepqmc_amd.spec import ANSATZES
from loss_util import (check_clip_rows, check_clip_rows_nan, check_cotangents, check_end_to_end, check_fit_parity_loss,
                       check_fit_without_loss_fn, check_overlap_penalty_separates, check_psi_ratio, check_raising_gradient, lih_batch)
from optimizer_util import make_pair, training_setup

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def eng():
    return make_pair('paulinet', 'LiH', torch.float64, DEV)[3]


@pytest.mark.parametrize('n_rows', [1, 9])
@pytest.mark.parametrize('B', [65, 4097])
def test_clip_rows_matches_torch_sort_gpu(eng, B, n_rows):
    for median_center in (True, False):
        for median_scale in (True, False):
            for exclude_width in (1.0, math.inf):
                check_clip_rows(eng, B, n_rows, median_center, median_scale, exclude_width)
    check_clip_rows_nan(eng, B)


@pytest.mark.parametrize('B', [65, 4097])
@pytest.mark.parametrize('S', [1, 3])
def test_psi_ratio_matches_the_torch_ratio_gpu(eng, S, B):
    check_psi_ratio(eng, S, B)


@pytest.mark.parametrize('B', [65, 4097])
@pytest.mark.parametrize('S', [1, 2, 3])
def test_cotangents_match_autograd_of_the_restated_tangent_gpu(eng, S, B):
    for k, scale_overlap_by in enumerate((None, 'energy_gap', 'energy_std', 'max_gap_std')):
        for nan_ewm in (False, True):
            spin_kind = ('squared', 'raising')[(k + nan_ewm) % 2]
            states = None if S == 1 or k % 2 else list(range(S))[1:]
            check_cotangents(eng, S, B, scale_overlap_by, nan_ewm, 'energy' if k % 2 == 0 else None, spin_kind, states, seed=k)
    check_cotangents(eng, S, B, 'max_gap_std', False, 'energy', None, None, exclude=False)


@pytest.mark.parametrize('lam', [None, 1.0])
def test_loss_and_gradients_end_to_end_gpu(lam):
    """The default LiH / PauliNet spec in float64, two states of 256 walkers, alpha = 4 with max_gap_std, without and with the squared
    spin penalty: gradient tolerance 1e-8 leaf-relative, the value test_gpu_param_grad.py uses on the GPU."""
    h, spec, wf, params, pc, data = lih_batch(2, 256, DEV, None, small=False)
    check_end_to_end(h, wf, params, pc, data, lam, 1e-8)


def test_raising_penalty_gradient_gpu():
    """The raising kind's stacked-walker VJP (B (1 + n_up) walkers in one dqmc_log_psi_vjp call) on the device, against
    c . J(r) plus the direct term from the Jacobians of the swapped walkers; default spec, float64, two states of 64 walkers."""
    h, spec, wf, params, pc, data = lih_batch(2, 64, DEV, None, small=False)
    check_raising_gradient(h, wf, params, pc, data, 1e-8)


def test_fit_wf_without_a_loss_function_yields_what_it_yielded_gpu():
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    check_fit_without_loss_fn(h, ANSATZES['paulinet'](), torch.float64, DEV, None, 256, 3, 5e-3, 3)


def test_fit_wf_with_a_loss_function_matches_the_host_path_loop_gpu():
    """Float64, two states of 256 walkers, 10 Adam steps from the start of test_gpu_optimizer.py's parity run (seed 3, lr 5e-3)."""
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    check_fit_parity_loss(h, ANSATZES['paulinet'](), torch.float64, DEV, None, 256, 10, 5e-3, 3,
                          dict(alpha=4.0, scale_overlap_by='max_gap_std'))


def test_overlap_penalty_drives_nearby_states_apart_gpu():
    """Check 6's last part, on the GPU only (the emulation needs minutes for an evaluation set that resolves the estimate).
    Start: state 0 = wf.init(3), state 1 = the same tree with 0.02 x N(0, 1) added to every leaf (rng 4); default spec, float64.
    Ten Adam steps of fit_wf at 256 walkers per state and lr 1e-5, with alpha = 4 (max_gap_std) and with alpha = 0, same seeds.
    |overlap/pairwise/mean[0, 1]| on one fixed set of 8192 walkers per state (equilibrated under the start and reweighted by
    |psi_now / psi_start|^2, loss_util.fixed_set_overlap), seen on the MI355X:
        start 0.7509;  alpha = 4: 0.5916 (effective samples 6575 / 4805);  alpha = 0: 0.8359 (6575 / 5966).
    The learning rate is this small because ten steps at 1e-4 already move log|psi| of these untrained states by several units
    per walker (effective samples 68 of 8192), and without the reweighting the one-sided means of psi_i / psi_j on walkers that
    no longer follow |psi_j|^2 are dominated by a few outliers: the symmetrised estimate then jumps between 0 (signs differ)
    and values above 1 from step to step.  The same order was seen for seeds 3 and 5, noise 0.01 and 0.02, 256 and 2048
    training walkers and lr 3e-6 to 3e-5 (24 of 24 runs).  The estimate counts as resolved with at least 2048 effective samples
    per state: the ratios have variance below 1 / overlap^2 - 1 ~ 0.8, so each one-sided mean is then good to 0.02."""
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    out = check_overlap_penalty_separates(h, ANSATZES['paulinet'](), torch.float64, DEV, None, 256, 8192, 10, 1e-5, 3, 0.02)
    assert min(out['ess'][4.0].min(), out['ess'][0.0].min()) >= 8192 / 4, out['ess']
    assert out[4.0] < out[0.0], out


def test_two_state_training_run_replays_its_graphs():
    """20 float32 steps of fit_wf at S = 2 x 1024 walkers with alpha = 4: every loss and every overlap is finite, and the
    forward-Laplacian graph of each state's context is captured at most twice and replayed ever after."""
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = ANSATZES['paulinet']()
    wf, params, sampler, st = training_setup(h, spec, torch.float32, DEV, None, 2, 1024, 10, seed=3)
    opt = AdamOptimizer(1e-3, loss_fn=create_loss_fn(h, wf, alpha=4.0, scale_overlap_by='max_gap_std'))
    losses, overlaps = [], []
    for _, state, _, stats in fit_wf(3, h, wf, opt, MoleculeIdxSampler(0, 1, 1), sampler, range(20), TrainState(st, params, None), None):
        losses.append(float(stats['loss']))
        overlaps.append(stats['overlap/pairwise/mean'].cpu().numpy())
    print('loss', losses[0], '->', losses[-1], '|overlap[0,1]|', abs(overlaps[0][0, 0, 1]), '->', abs(overlaps[-1][0, 0, 1]))
    assert len(losses) == 20 and np.isfinite(losses).all() and np.isfinite(np.stack(overlaps)).all()
    for p in params:
        c = wf.engine(p).graph_counters()
        print('graph counters', c)
        assert c['captures'] <= 2 and c['replays'] > c['captures'], c
