"""The per-walker backward of the nuclear-token stream (option "nuclear_coords") on the MI355X: the checks of
tests/test_nuclear_coords_emu.py with the HIP kernels, and a float32 context against a float64 one."""
import pytest

import nuclear_coords_util as U

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('case', list(U.CASES))
def test_grad_coords_match_oracle_autograd(case):
    U.check_against_oracle(case, DEV, None)


@pytest.mark.parametrize('case,B,budget_mb,min_chunks,unequal', [('LiH-2layers', 9, 1, 1, False), ('C4H4-2layers', 3, 1, 3, False),
                                                                 ('C4H4-2layers', 9, 2, 3, True)])
def test_row_tails_and_chunks(case, B, budget_mb, min_chunks, unequal):
    U.check_row_tails_and_chunks(case, B, DEV, None, budget_mb, min_chunks, unequal)


def test_want_R_false_never_runs_the_stream_backward():
    U.check_want_R_false_skips_the_stream(DEV, None)


def test_invalid_walker_gets_zero_rows():
    U.check_invalid_walker(DEV, None)


def test_gate():
    U.check_gate(DEV, None)


def test_forces_match_restated_formulas_with_oracle_gradients():
    U.check_forces(DEV, None)


def test_fit_step_with_zero_bias_force_monitors():
    U.check_fit_with_force_monitors(DEV, None)


def test_float32_context_against_float64():
    """LiH with two layers, 256 float32-rounded walkers, a float32 context against a float64 one: median and 90th percentile
    of the normwise error per walker over all walkers.  The bounds are 5 x the values measured on the MI355X."""
    stats = U.f32_error_statistics(DEV, None)
    # measured: grad_R median 9.10e-07, 90th percentile 9.86e-06 (grad_r of the same call: 1.13e-06 and 1.06e-05)
    med, p90 = stats['grad_R']
    assert med < 4.6e-6 and p90 < 4.9e-5, stats
