"""TransPsiformer training (option "nuclear_reverse") on the MI355X: the checks of tests/test_nuclear_reverse_emu.py with the
HIP kernels -- the device fold against the host fold, the VJP of the four shape cases, the orbital mode, chunking and
determinism, freshness after a device step (the float32 context through its float64 twin), training parity, several states,
the checkpoint, and the gate."""
import pytest
import torch

import nuclear_reverse_util as U

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def test_gate():
    U.check_gate(DEV, None)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
def test_device_fold_equals_host_fold(dtype):
    U.check_fold_parity('LiH', DEV, None, dtype, n_interactions=2)


def test_device_fold_equals_host_fold_eight_nuclei():
    U.check_fold_parity('cyclobutadiene_square', DEV, None, torch.float64, n_interactions=2)


@pytest.mark.parametrize('case', list(U.CASES))
def test_vjp_matches_oracle_autograd(case):
    U.check_vjp_against_oracle(case, DEV, None)


def test_orbitals_vjp_and_pretraining_match_oracle_autograd():
    U.check_orbitals_and_pretraining(DEV, None)


def test_chunked_equals_unchunked_and_calls_are_bit_identical():
    U.check_chunking_and_determinism(DEV, None)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32-refined'])
def test_weights_are_fresh_after_a_device_step(dtype):
    U.check_fresh_after_device_step(DEV, None, dtype)


def test_adam_fit_matches_host_path():
    U.check_adam_fit_parity(DEV, None)


def test_two_states_loss_fn_flat_and_fit_step():
    U.check_two_states(DEV, None)


def test_checkpoint_round_trip(tmp_path):
    U.check_checkpoint(DEV, None, tmp_path)
