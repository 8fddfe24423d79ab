"""The per-walker parameter partials of the nuclear-token stream (option "nuclear_params") on the MI355X: the checks of
tests/test_nuclear_params_emu.py with the HIP kernels, and a float32 context against a float64 one."""
import pytest

import nuclear_params_util as U
from deepqmc_amd.optimizer import KFACOptimizer, NaturalGradientOptimizer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('case', list(U.CASES))
def test_rows_match_oracle_autograd_and_transpose_the_vjp(case):
    U.check_rows_against_oracle(case, DEV, None)


def test_agrees_with_unflatten_jacobian_without_a_stream():
    U.check_no_stream_agreement(DEV, None)


@pytest.mark.parametrize('case,B,budget_mb,min_chunks,unequal,fold_chunks', U.CHUNK_CASES)
def test_row_tails_and_chunks(case, B, budget_mb, min_chunks, unequal, fold_chunks):
    U.check_row_tails_and_chunks(case, B, DEV, None, budget_mb, min_chunks, unequal, fold_chunks)


@pytest.mark.parametrize('case', list(U.CASES))
def test_kfac_direction_treats_the_stream_as_diagonal_elements(case):
    U.check_kfac_diagonal(case, DEV, None)


@pytest.mark.parametrize('make_opt', [lambda: NaturalGradientOptimizer(1e-2), lambda: KFACOptimizer(0.05)], ids=['natgrad', 'kfac'])
def test_three_fit_steps(make_opt):
    U.check_optimizer_steps(make_opt, DEV, None)


def test_natural_gradient_identity_and_the_kfac_paths():
    U.check_natgrad_identity(DEV, None)


def test_gate():
    U.check_gate(DEV, None)


def test_float32_context_against_float64():
    """LiH with two layers, 256 float32-rounded walkers, a float32 context against a float64 one: median and 90th percentile over
    the walkers of the normwise error of the row restricted to the stream's own leaves.  The bounds are 5 x the values measured
    on the MI355X."""
    med, p90 = U.f32_error_statistics(DEV, None)
    # measured: median 5.69e-07, 90th percentile 7.94e-06
    assert med < 2.9e-6 and p90 < 4.0e-5, (med, p90)
