"""The per-walker parameter partials of the nuclear-token stream (option "nuclear_params") through the SIMT emulation of the
kernels: the rows of dqmc_jacobian_to_params against torch.autograd of the float64 oracle on the four shape cases with the
transpose of the VJP, agreement with Program.unflatten_jacobian without a stream, row counts off the MFMA tile with chunked
calls and an invalid walker, the stream's diagonal elements of the KFAC direction, three fit_wf steps with
NaturalGradientOptimizer and KFACOptimizer, the natural-gradient identity, and the gate.  Every test sets the flag, which
neither the library nor the package knew before."""
import pytest

import nuclear_params_util as U
from deepqmc_amd.optimizer import KFACOptimizer, NaturalGradientOptimizer
from simt_util import emu_lib


@pytest.mark.parametrize('case', list(U.CASES))
def test_rows_match_oracle_autograd_and_transpose_the_vjp(case):
    U.check_rows_against_oracle(case, 'cpu', emu_lib())


def test_agrees_with_unflatten_jacobian_without_a_stream():
    U.check_no_stream_agreement('cpu', emu_lib())


@pytest.mark.parametrize('case,B,budget_mb,min_chunks,unequal,fold_chunks', U.CHUNK_CASES)
def test_row_tails_and_chunks(case, B, budget_mb, min_chunks, unequal, fold_chunks):
    U.check_row_tails_and_chunks(case, B, 'cpu', emu_lib(), budget_mb, min_chunks, unequal, fold_chunks)


@pytest.mark.parametrize('case', list(U.CASES))
def test_kfac_direction_treats_the_stream_as_diagonal_elements(case):
    U.check_kfac_diagonal(case, 'cpu', emu_lib())


@pytest.mark.parametrize('make_opt', [lambda: NaturalGradientOptimizer(1e-2), lambda: KFACOptimizer(0.05)], ids=['natgrad', 'kfac'])
def test_three_fit_steps(make_opt):
    U.check_optimizer_steps(make_opt, 'cpu', emu_lib())


def test_natural_gradient_identity_and_the_kfac_paths():
    U.check_natgrad_identity('cpu', emu_lib())


def test_gate():
    U.check_gate('cpu', emu_lib())
