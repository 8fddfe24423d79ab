"""TransPsiformer training (option "nuclear_reverse") through the SIMT emulation of the kernels: the nuclear-token stream folded
on the device against the host fold, its backward and the attention backward with constant key / value rows against
torch.autograd of the float64 oracle, the orbital mode, chunking and determinism, freshness of every weight buffer after a device
step, training against the host path, several states, the checkpoint, and the gate.  Every test sets the flag, which neither
the library nor the package knew before."""
import pytest
import torch

import nuclear_reverse_util as U
from simt_util import emu_lib


def test_gate():
    U.check_gate('cpu', emu_lib())


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
def test_device_fold_equals_host_fold(dtype):
    U.check_fold_parity('LiH', 'cpu', emu_lib(), dtype, n_interactions=2)


def test_device_fold_equals_host_fold_eight_nuclei():
    U.check_fold_parity('cyclobutadiene_square', 'cpu', emu_lib(), torch.float64, n_interactions=2)


@pytest.mark.parametrize('case', list(U.CASES))
def test_vjp_matches_oracle_autograd(case):
    U.check_vjp_against_oracle(case, 'cpu', emu_lib())


def test_orbitals_vjp_and_pretraining_match_oracle_autograd():
    U.check_orbitals_and_pretraining('cpu', emu_lib())


def test_chunked_equals_unchunked_and_calls_are_bit_identical():
    U.check_chunking_and_determinism('cpu', emu_lib())


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32-refined'])
def test_weights_are_fresh_after_a_device_step(dtype):
    U.check_fresh_after_device_step('cpu', emu_lib(), dtype)


def test_adam_fit_matches_host_path():
    U.check_adam_fit_parity('cpu', emu_lib())


def test_two_states_loss_fn_flat_and_fit_step():
    U.check_two_states('cpu', emu_lib())


def test_checkpoint_round_trip(tmp_path):
    U.check_checkpoint('cpu', emu_lib(), tmp_path)
