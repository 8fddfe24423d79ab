"""The per-walker backward of the nuclear-token stream (option "nuclear_coords") through the SIMT emulation of the kernels:
d log|psi| / dr and d log|psi| / dR of the TransPsiformer against torch.autograd of the float64 oracle on the four shape cases,
row counts off the MFMA tile with chunked calls, want_R=False, an invalid walker, the gate, and the zero-bias force estimators
with their fit_wf monitors.  Every test sets the flag, which neither the library nor the package knew before."""
import pytest

import nuclear_coords_util as U
from simt_util import emu_lib


@pytest.mark.parametrize('case', list(U.CASES))
def test_grad_coords_match_oracle_autograd(case):
    U.check_against_oracle(case, 'cpu', emu_lib())


@pytest.mark.parametrize('case,B,budget_mb,min_chunks,unequal', [('LiH-2layers', 9, 1, 1, False), ('C4H4-2layers', 3, 1, 3, False),
                                                                 ('C4H4-2layers', 9, 2, 3, True)])
def test_row_tails_and_chunks(case, B, budget_mb, min_chunks, unequal):
    U.check_row_tails_and_chunks(case, B, 'cpu', emu_lib(), budget_mb, min_chunks, unequal)


def test_want_R_false_never_runs_the_stream_backward():
    U.check_want_R_false_skips_the_stream('cpu', emu_lib())


def test_invalid_walker_gets_zero_rows():
    U.check_invalid_walker('cpu', emu_lib())


def test_gate():
    U.check_gate('cpu', emu_lib())


def test_forces_match_restated_formulas_with_oracle_gradients():
    U.check_forces('cpu', emu_lib())


def test_fit_step_with_zero_bias_force_monitors():
    U.check_fit_with_force_monitors('cpu', emu_lib())
