"""The opt-in reverse pass through attention (option "attention_reverse", kernel k_attention_bwd) on the MI355X: float64
gradients of narrow Psiformers and of the production head shape against torch.autograd of the oracle, float32 against float64,
a central finite difference, and the chunking, training and gate checks of tests/test_attention_reverse_emu.py on the device."""
import dataclasses

import numpy as np
import pytest
import torch

from attention_reverse_util import (check_adam_fit_parity, check_chunking_and_determinism, check_gate, check_kfac_step,
                                    check_loss_fn_flat, narrow_psiformer, psiformer_engine)
from deepqmc_amd import MolecularHamiltonian, Molecule
from deepqmc_amd.engine import Engine
from deepqmc_amd.params import init_params
from deepqmc_amd.sampling import synthetic_walkers
from deepqmc_amd.spec import ANSATZES, psiformer
from large_n_util import check_vjp_and_coords, make_walkers, setup
from oracle import geom
from param_grad_util import leaf_errors

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('molname', ['LiH', 'N2'])
def test_vjp_and_coords_match_oracle_autograd(molname):
    spec, h, tree, eng, r = psiformer_engine(molname, 3, DEV)
    check_vjp_and_coords(eng, spec, h, tree, r, DEV)


@pytest.mark.parametrize('n', [49, 64])
def test_vjp_and_coords_match_oracle_autograd_large_n(n):
    """49 electrons: one row in the last block of 16 query rows; 64: the largest LDS tile set of the float64 kernel."""
    spec, mol, h, tree, eng = setup('psiformer', n, torch.float64, DEV)
    eng.set_option('attention_reverse', 1)
    check_vjp_and_coords(eng, spec, h, tree, make_walkers(mol, n, 3), DEV)


def test_production_head_shape_matches_oracle_autograd():
    """Four heads of width 64 (embedding_dim 256), one layer, two determinants, N2, four walkers."""
    spec = dataclasses.replace(psiformer(), n_interactions=1, n_determinants=2)
    assert spec.embedding_dim == 256 and spec.num_heads == 4
    spec, h, tree, eng, r = psiformer_engine('N2', 4, DEV, spec=spec)
    check_vjp_and_coords(eng, spec, h, tree, r, DEV, tol=1e-9)


def _f32_off_node_error(name, B=1024):
    """The off-node figure of tests/test_gpu_param_grad.py::test_float32_against_float64 for LiH / `name` at defaults: the
    largest leaf-relative deviation of the float32 VJP from the float64 one, both contracted over the walkers whose float32
    log|psi| is within 1e-5 of float64.  Returns (figure, number of such walkers, the leaf of the figure)."""
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = ANSATZES[name]()
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=7, perturb_envelopes=0.1)
    r = synthetic_walkers(h, B, seed=11)
    cot = np.random.default_rng(0).normal(size=B) / B
    engs, logs = {}, {}
    for dt in (torch.float64, torch.float32):
        engs[dt] = Engine(spec, h, tree, dtype=dt, device=DEV, norm_eps=geom.F32_EPS)
        engs[dt].set_option('attention_reverse', 1)
        _, logs[dt] = engs[dt].wf_eval(torch.as_tensor(r, dtype=dt, device=DEV))
    good = ((logs[torch.float32].double() - logs[torch.float64]).abs() < 1e-5).cpu().numpy().astype(np.float64)
    out = {}
    for dt, eng in engs.items():
        _, _, g = eng.log_psi_vjp(torch.as_tensor(r, dtype=dt, device=DEV), torch.as_tensor(cot * good, dtype=dt, device=DEV))
        out[dt] = eng.program.unflatten_grad(g)
        eng.close()
    err = leaf_errors(out[torch.float32], out[torch.float64])
    worst = max(err, key=err.get)
    return err[worst], int(good.sum()), worst


def test_float32_against_float64():
    """LiH / Psiformer at defaults, 1024 walkers, against LiH / PauliNet measured the same way in the same run (the case
    tests/test_gpu_param_grad.py bounds at 1e-4): the Psiformer figure must stay within 10x of the PauliNet figure -- the
    network is deeper and has a softmax, and the check is there to catch a wrong kernel, not to model rounding.
    Measured on the MI355X: Psiformer 5.73e-06 over 770 walkers, PauliNet 9.57e-05 over 956 walkers (the
    reverse pass through attention)."""
    pf, n_pf, w_pf = _f32_off_node_error('psiformer')
    pn, n_pn, w_pn = _f32_off_node_error('paulinet')
    print(f'float32 vs float64 off the nodes, LiH, 1024 walkers: Psiformer {pf:.2e} ({n_pf} walkers, {w_pf}); '
          f'PauliNet {pn:.2e} ({n_pn} walkers, {w_pn})')
    assert n_pf > 512 and n_pn > 512
    assert pf < 10 * pn, (pf, pn)


def test_chunked_equals_unchunked_and_calls_are_bit_identical():
    spec, h, tree, eng, r = psiformer_engine('N2', 24, DEV)
    check_chunking_and_determinism(eng, torch.as_tensor(r, device=DEV))


def _tiny():
    return MolecularHamiltonian(mol=Molecule.from_name('LiH')), narrow_psiformer(embedding_dim=16, n_determinants=1)


def test_training_steps():
    h, spec = _tiny()
    check_adam_fit_parity(h, spec, DEV, None)
    check_kfac_step(h, spec, DEV, None)
    check_loss_fn_flat(h, spec, DEV, None)


def test_gate():
    check_gate(DEV, None)


def test_central_finite_difference():
    """sum_b cot_b log|psi| along a random unit direction through set_params + wf_eval, Richardson-extrapolated, against the
    VJP: the form and the 1e-7 bound of tests/test_gpu_param_grad.py::test_central_finite_difference, narrow Psiformer."""
    B = 32
    spec, h, tree, eng, r = psiformer_engine('LiH', B, DEV, seed=9)
    r = torch.as_tensor(r, device=DEV)
    cot = torch.as_tensor(np.random.default_rng(2).normal(size=B), device=DEV)
    _, _, g = eng.log_psi_vjp(r, cot)
    G = eng.program.unflatten_grad(g)
    rng = np.random.default_rng(3)
    v = {m: {k: rng.normal(size=np.shape(x)) for k, x in leaves.items()} for m, leaves in tree.items()}
    norm = np.sqrt(sum(float(np.sum(v[m][k] ** 2)) for m in v for k in v[m]))
    v = {m: {k: x / norm for k, x in leaves.items()} for m, leaves in v.items()}       # unit direction
    analytic = sum(float(np.sum(v[m][k] * G[m][k])) for m in G for k in G[m])

    def fd(eps):
        f = []
        for s in (1, -1):
            eng.set_params({m: {k: np.asarray(x) + s * eps * v[m][k] for k, x in leaves.items()} for m, leaves in tree.items()})
            f.append(float((cot * eng.wf_eval(r)[1]).sum()))
        return (f[0] - f[1]) / (2 * eps)
    eps = 1e-3
    richardson = (4 * fd(eps / 2) - fd(eps)) / 3          # central difference with its O(eps^2) term removed
    print(f'central difference {richardson:.12e}, VJP {analytic:.12e}')
    assert abs(richardson - analytic) < 1e-7 * max(1.0, abs(analytic)), (richardson, analytic)
