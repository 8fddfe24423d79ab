"""KFAC statistics of the reverse pass (dqmc_log_psi_kfac) on the MI355X: the factors against the oracle's recorded linear
calls in float64, float32 against float64, bit-identity with the VJP and between calls at 4096 walkers, the Jastrow
cross-check, and the cost of a call next to log_psi_vjp."""
import time

import numpy as np
import pytest
import torch

from deepqmc_amd import MolecularHamiltonian, Molecule
from deepqmc_amd.engine import Engine
from deepqmc_amd.params import OMNI, init_params
from deepqmc_amd.sampling import synthetic_walkers
from deepqmc_amd.spec import ANSATZES
from oracle import geom
from kfac_util import check_factors_against_oracle, rel_fro
from param_jacobian_util import jac_engine

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('name,mol,B', [('paulinet', 'LiH', 256), ('ferminet', 'N2', 64)])
def test_factors_match_oracle_gpu(name, mol, B):
    h, spec, tree, eng, r = jac_engine(name, mol, B, DEV)
    err_a, err_g = check_factors_against_oracle(h, spec, tree, eng, r, tol_a=1e-9, tol_g=1e-9)
    print(f'{name}/{mol}: max rel Frobenius A {max(err_a.values()):.2e}, G {max(err_g.values()):.2e}')


def _full_engine(dt, B=4096, seed=7):
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = ANSATZES['paulinet']()
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=seed, perturb_envelopes=0.1)
    eng = Engine(spec, h, tree, dtype=dt, device=DEV, norm_eps=geom.F32_EPS)
    return eng, torch.as_tensor(synthetic_walkers(h, B, seed=11), dtype=dt, device=DEV)


def test_float32_against_float64_gpu():
    out, logs = {}, {}
    for dt in (torch.float64, torch.float32):
        eng, r = _full_engine(dt)
        _, logs[dt], _, _, _ = eng.log_psi_kfac(r, rest=False)
        out[dt] = (eng, r)
    good = (logs[torch.float32].double() - logs[torch.float64]).abs() < 1e-5
    assert int(good.sum()) > 2048
    idx = torch.nonzero(good)[:, 0]
    fac = {}
    for dt, (eng, r) in out.items():
        _, _, _, fac[dt], _ = eng.log_psi_kfac(r[idx].contiguous(), rest=False)
        eng.close()
    worst = 0.0
    for (a32, g32), (a64, g64) in zip(fac[torch.float32], fac[torch.float64]):
        worst = max(worst, rel_fro(a32.cpu(), a64.cpu()), rel_fro(g32.cpu(), g64.cpu()))
    print(f'float32 vs float64 factors, {int(good.sum())} walkers: max rel Frobenius {worst:.3e}')
    assert worst < 1e-4, worst


def test_bit_identity_and_jastrow_float32_gpu():
    eng, r = _full_engine(torch.float32)
    s, l, g, fac, rest = eng.log_psi_kfac(r)
    _, _, g0 = eng.log_psi_vjp(r)
    assert torch.equal(g, g0)
    s1, l1, g1, fac1, rest1 = eng.log_psi_kfac(r)
    assert torch.equal(g, g1) and torch.equal(rest, rest1)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(fac, fac1))
    lay = eng.program.kfac_layout()
    q = next(k for k, o in enumerate(lay['ops']) if o['module'] == f'{OMNI}/~/Jastrow/~/mlp/linear_0')
    o = lay['ops'][q]
    i = eng.program.ops[o['op']].i
    _, _, J = eng.log_psi_jacobian(r[:1024].contiguous())
    _, _, _, fq, _ = eng.log_psi_kfac(r[:1024].contiguous(), rest=False)
    eng.set_option('fused', 0)
    eng.wf_eval(r[:1024].contiguous())
    x = torch.as_tensor(eng.debug_read('x_sum', 1024)).reshape(1024, -1)[:, :o['d_a']].to(DEV)
    jw = J[:, i[22]:i[22] + o['d_a'] * o['d_g']].reshape(1024, o['d_a'], o['d_g']).double()
    jb = torch.einsum('bk,bkn->bn', x, jw) / (x * x).sum(1, keepdim=True)
    err = rel_fro(fq[q][1].cpu(), (jb.T @ jb).cpu())
    print(f'Jastrow G against the Jacobian (float32): {err:.2e}')
    assert err < 1e-4


def test_cost_against_vjp_gpu():
    eng, r = _full_engine(torch.float32)
    def timed(fn, n=10):
        fn(); torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n * 1e3
    t_vjp = timed(lambda: eng.log_psi_vjp(r))
    t_kfac = timed(lambda: eng.log_psi_kfac(r))
    print(f'LiH / PauliNet float32 4096 walkers: log_psi_vjp {t_vjp:.2f} ms, log_psi_kfac {t_kfac:.2f} ms, ratio {t_kfac / t_vjp:.2f}')
    assert t_kfac < 3.0 * t_vjp
