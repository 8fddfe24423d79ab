"""The observable monitors on the MI355X: dqmc_oscillator_strength, dqmc_fd_displace and dqmc_fd_force against the NumPy
transcriptions at the shapes of the emulated tests, the finite-difference estimator end to end at 8 walkers, the monitors against
direct calls of their estimators, and fit_wf with monitors at 64 walkers per state (default LiH / PauliNet spec, float64)."""
import pytest
import torch

from deepqmc_amd import observable as obs
from loss_util import SMALL
from observable_util import (OS_SHAPES, check_fd_displace, check_fd_force, check_finite_difference_force, check_fit_with_monitors,
                             check_fit_without_monitors, check_monitor, check_oscillator_strength, monitor_batch)
from optimizer_util import make_pair

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def engines():
    """Small contexts: these entry points use the context's stream, dtype and particle counts only."""
    return {(mol, dtype): make_pair('paulinet', mol, dtype, DEV, **SMALL)[3] for mol in ('LiH', 'H2O') for dtype in (torch.float64, torch.float32)}


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('S,B', OS_SHAPES)
def test_oscillator_strength_matches_the_transcription_gpu(engines, S, B, dtype):
    check_oscillator_strength(engines['LiH', dtype], S, B)


@pytest.mark.parametrize('B', [1, 65])
@pytest.mark.parametrize('mol', ['LiH', 'H2O'])
def test_fd_displace_matches_numpy_gpu(engines, mol, B):
    check_fd_displace(engines[mol, torch.float64], engines[mol, torch.float32], B)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('B', [1, 65])
def test_fd_force_matches_numpy_gpu(engines, B, dtype):
    check_fd_force(engines['H2O', dtype], B)


def test_finite_difference_force_end_to_end_gpu():
    check_finite_difference_force(DEV, None)


def test_monitor_samples_are_the_direct_calls_gpu():
    """Default spec, float64, two states of 64 walkers: one monitor of each kind of signature."""
    batch = monitor_batch(DEV, None, B=64, small=False)
    for name in ('spin', 'hf_force_bare_anti', 'hf_force_ac_zvq', 'hf_force_ac_zb', 'hf_force_ac_zvqzb'):
        check_monitor(name, batch)
    hamil, wf, params, pc, psi, e_loc, ratios = batch
    out = obs.OscillatorStrengthMonitor(False, 1).finalize(hamil, wf)(0, 1, params, pc, psi, e_loc, ratios)
    assert torch.isfinite(out['oscillator_strength/mean']).all() and tuple(out['oscillator_strength/err'].shape) == (1, 2, 2)


def test_fit_wf_with_monitors_gpu():
    check_fit_with_monitors(DEV, None, torch.float64, 64, small=False)


def test_fit_wf_without_monitors_yields_what_it_yielded_gpu():
    check_fit_without_monitors(DEV, None, torch.float64, 64, small=False)
