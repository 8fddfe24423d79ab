"""Parameter gradient of log|psi| (dqmc_log_psi_vjp) on the MI355X: the reference's own golden, float64 against
torch.autograd through the oracle, float32 against float64, a central finite difference through set_params + wf_eval,
and the energy-loss gradient against the same contraction formed by hand."""
import dataclasses

import numpy as np
import pytest
import torch

from deepqmc_amd import MolecularHamiltonian, Molecule
from deepqmc_amd.engine import Engine
from deepqmc_amd.loss import compute_energy_loss_and_grad, compute_local_energy, median_clip_and_mask
from deepqmc_amd.params import init_params
from deepqmc_amd.sampling import synthetic_walkers
from deepqmc_amd.spec import ANSATZES
from deepqmc_amd.wf import NeuralNetworkWaveFunction
from oracle import geom
from param_grad_util import check_against_oracle, check_grad_golden, leaf_errors, oracle_vjp

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def test_reference_grad_golden_on_gpu(kats):
    check_grad_golden(kats, DEV)


@pytest.mark.parametrize('name,mol,B', [('paulinet', 'LiH', 256), ('ferminet', 'N2', 64)])
def test_vjp_matches_oracle_autograd_gpu(name, mol, B):
    check_against_oracle(name, mol, B, DEV, tol=1e-8)


def _setup(name='paulinet', mol='LiH', seed=7):
    h = MolecularHamiltonian(mol=Molecule.from_name(mol))
    spec = ANSATZES[name]()
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=seed, perturb_envelopes=0.1)
    return h, spec, tree


def test_float32_against_float64():
    h, spec, tree = _setup()
    B = 4096
    r = synthetic_walkers(h, B, seed=11)
    cot = np.random.default_rng(0).normal(size=B) / B
    out, logs = {}, {}
    for dt in (torch.float64, torch.float32):
        eng = Engine(spec, h, tree, dtype=dt, device=DEV, norm_eps=geom.F32_EPS)
        rr = torch.as_tensor(r, dtype=dt, device=DEV)
        _, logs[dt], g = eng.log_psi_vjp(rr, torch.as_tensor(cot, dtype=dt, device=DEV))
        out[dt] = eng.program.unflatten_grad(g)
        # the same contraction over the walkers whose float32 log|psi| is within 1e-5 of float64 (away from a node of psi)
        if dt == torch.float32:
            good = ((logs[torch.float32].double() - logs[torch.float64]).abs() < 1e-5).cpu().numpy().astype(np.float64)
            _, _, g = eng.log_psi_vjp(rr, torch.as_tensor(cot * good, dtype=dt, device=DEV))
            out['f32_off_node'] = eng.program.unflatten_grad(g)
            off_node = good
        eng.close()
    err = leaf_errors(out[torch.float32], out[torch.float64])
    worst = max(err, key=err.get)
    eng = Engine(spec, h, tree, dtype=torch.float64, device=DEV, norm_eps=geom.F32_EPS)
    _, _, g = eng.log_psi_vjp(torch.as_tensor(r, device=DEV), torch.as_tensor(cot * off_node, device=DEV))
    err_off = leaf_errors(out['f32_off_node'], eng.program.unflatten_grad(g))
    worst_off = max(err_off, key=err_off.get)
    print(f'float32 vs float64, LiH / PauliNet, 4096 walkers: largest leaf-relative error {err[worst]:.2e} ({worst}); '
          f'{int(off_node.sum())} walkers off the nodes: {err_off[worst_off]:.2e}')
    # Measured on the MI355X: 7.2e-3 over all walkers -- the same with a same-sign cotangent and with the bf16-split forward
    # off ("linear_bf" 0) -- and 5.8e-6 over the 3735 (91 %) walkers whose float32 log|psi| is within 1e-5 of float64.  The
    # error is the float32 value path near a node of psi (log|psi| off by up to 1e-2 there; those walkers carry the
    # largest gradients, through A^-T), not the reverse pass.
    assert err_off[worst_off] < 1e-4, (worst_off, err_off[worst_off])
    assert err[worst] < 3e-2, (worst, err[worst])


def test_central_finite_difference():
    h, spec, tree = _setup(seed=9)
    B = 32
    r = torch.as_tensor(synthetic_walkers(h, B, seed=12), device=DEV)
    cot = torch.as_tensor(np.random.default_rng(2).normal(size=B), device=DEV)
    eng = Engine(spec, h, tree, dtype=torch.float64, device=DEV, norm_eps=geom.F32_EPS)
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
    assert abs(richardson - analytic) < 1e-7 * max(1.0, abs(analytic)), (richardson, analytic)


def test_energy_loss_gradient_matches_hand_contraction():
    """Two states of 1024 walkers: each state's gradient is its own contraction over the mask count of the whole [1, 2, B]
    batch (the reference's masked_mean over all axes)."""
    h, spec, tree = _setup(seed=4)
    trees = [tree, _setup(seed=5)[2]]
    wf = NeuralNetworkWaveFunction(h, spec, dtype=torch.float64, device=DEV, norm_eps=geom.F32_EPS)
    B = 1024
    r = torch.stack([torch.as_tensor(synthetic_walkers(h, B, seed=13 + s), device=DEV) for s in (0, 1)])[None]
    loss, grads, stats = compute_energy_loss_and_grad(None, h, wf, trees, r)
    e, _ = compute_local_energy(None, h, wf, trees, r)
    e = e[0].double()
    np.testing.assert_allclose(float(loss), float(e.mean()), rtol=1e-12)
    clipped = [median_clip_and_mask(e[s]) for s in (0, 1)]
    n_mask = sum(float(m.double().sum()) for _, m in clipped)
    for s, (ec, _) in enumerate(clipped):
        ref = oracle_vjp(spec, h, trees[s], r[0, s].cpu().numpy(), ((ec - ec.mean()) / n_mask).cpu().numpy(), geom.F32_EPS)
        err = leaf_errors(grads[s], ref)
        worst = max(err, key=err.get)
        assert err[worst] < 1e-8, (s, worst, err[worst])
