"""Per-walker parameter Jacobian of log|psi| (dqmc_log_psi_jacobian) on the MI355X: float64 against the VJP and against
torch.autograd through the oracle, float32 against float64, bit-identical repeat and chunked calls, and the natural-gradient
identity on a full-size batch."""
import numpy as np
import pytest
import torch

from deepqmc_amd import MolecularHamiltonian, Molecule
from deepqmc_amd.engine import Engine
from deepqmc_amd.params import init_params
from deepqmc_amd.sampling import synthetic_walkers
from deepqmc_amd.spec import ANSATZES
from deepqmc_amd.wf import NeuralNetworkWaveFunction
from oracle import geom
from param_jacobian_util import check_natgrad, check_rows_against_oracle, check_transpose_of_vjp, jac_engine

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('name,mol,B', [('paulinet', 'LiH', 256), ('ferminet', 'N2', 64)])
def test_transpose_of_vjp_and_oracle_rows_gpu(name, mol, B):
    h, spec, tree, eng, r = jac_engine(name, mol, B, DEV)
    check_transpose_of_vjp(eng, r)
    check_rows_against_oracle(h, spec, tree, eng, r, [0, 1, B // 2, B - 1], tol=1e-8)


def _full(name='paulinet', mol='LiH', seed=7):
    h = MolecularHamiltonian(mol=Molecule.from_name(mol))
    spec = ANSATZES[name]()
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=seed, perturb_envelopes=0.1)
    return h, spec, tree


def test_float32_against_float64():
    h, spec, tree = _full()
    B = 4096
    r = synthetic_walkers(h, B, seed=11)
    J, logs = {}, {}
    for dt in (torch.float64, torch.float32):
        eng = Engine(spec, h, tree, dtype=dt, device=DEV, norm_eps=geom.F32_EPS)
        _, logs[dt], J[dt] = eng.log_psi_jacobian(torch.as_tensor(r, dtype=dt, device=DEV))
        eng.close()
    # rows of the walkers whose float32 log|psi| is within 1e-5 of float64 (away from a node of psi)
    good = (logs[torch.float32].double() - logs[torch.float64]).abs() < 1e-5
    assert int(good.sum()) > B // 2
    worst = 0.0
    for b0 in range(0, B, 512):                    # row by row relative error, in slices (J is 3.3 + 6.5 GB)
        j64 = J[torch.float64][b0:b0 + 512]
        d = (J[torch.float32][b0:b0 + 512].double() - j64).abs().amax(1) / j64.abs().amax(1)
        worst = max(worst, float(d[good[b0:b0 + 512]].max()))
    assert worst < 1e-4, worst


def test_repeat_and_chunked_calls_are_bit_identical_gpu():
    *_, eng, r = jac_engine('paulinet', 'LiH', 512, DEV)
    s0, l0, J0 = eng.log_psi_jacobian(r)
    s1, l1, J1 = eng.log_psi_jacobian(r)
    assert torch.equal(J0, J1) and torch.equal(l0, l1)
    assert eng.last_chunks()['own'] == 1
    eng.set_option('ws_budget_mb', 4)
    s2, l2, J2 = eng.log_psi_jacobian(r)
    assert eng.last_chunks()['own'] > 1
    assert torch.equal(s0, s2) and torch.equal(J0, J2)


def test_natgrad_identity_gpu():
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    wf = NeuralNetworkWaveFunction(h, 'paulinet', dtype=torch.float64, device=DEV, norm_eps=geom.F32_EPS)
    trees = [wf.init(0, perturb_envelopes=0.1)]
    r = torch.as_tensor(synthetic_walkers(h, 1024, seed=40), device=DEV)[None, None]
    check_natgrad(wf, trees, r, damping=1e-3)
