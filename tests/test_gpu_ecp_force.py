"""Hellmann-Feynman forces of Gaussian-type ECP Hamiltonians (dqmc_ecp_force, deepqmc_amd/ecp_force.py) on the MI355X:
float64 against torch.autograd of the oracle's potentials (both row modes), the full gradient against central differences of
the library's own V_loc + V_nl, bit-identical repeats and chunks in float32, float32 against float64, and the makers with the
antithetic wrapper."""
import numpy as np
import pytest
import torch

from deepqmc_amd import ecp_force, force
from deepqmc_amd.spec import ANSATZES
from deepqmc_amd.types import PhysicalConfiguration
from ecp_force_util import fd_grad_potential, make_system, oracle_parts_cached
from force_util import restated_force, walker_errors

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _t(x, dtype=torch.float64):
    return torch.as_tensor(x, dtype=dtype, device=DEV)


@pytest.mark.parametrize('rows', ['own', 'all'])
@pytest.mark.parametrize('system', ['b', 'c'])
def test_parts_match_oracle_autograd_gpu(system, rows):
    B = 4
    h, wf, params, r, phi = make_system(system, B, DEV)
    f, parts = wf.engine(params).ecp_force('bare', _t(r), ecp_phi=_t(phi), rows=rows, return_parts=True)
    assert f.device.type == 'cuda' and f.dtype == torch.float64
    ref0, ref1 = oracle_parts_cached(system, B, rows)
    e0, e1 = walker_errors(parts[0].cpu().numpy(), ref0), walker_errors(parts[1].cpu().numpy(), ref1)
    print(f'{system} {rows}: parts[0] error {e0.max():.2e}, parts[1] error {e1.max():.2e}')
    assert e1.max() < 1e-8, e1
    assert e0.max() < 1e-10, e0
    tot = (parts[0] + parts[1]).cpu().numpy()
    assert np.all(np.abs(f.cpu().numpy() - tot) <= np.spacing(np.abs(tot)))
    if system == 'c' and rows == 'own':
        assert torch.all(parts[1][:, 0] == 0)


def test_all_rows_against_finite_differences_gpu():
    B = 67                                         # not a multiple of the wave size
    h, wf, params, r, phi = make_system('b', B, DEV, spec=ANSATZES['paulinet']())
    eng = wf.engine(params)
    f = eng.ecp_force('bare', _t(r), ecp_phi=_t(phi), rows='all')
    grad_v = restated_force('nuclear', r, h.mol.coords, h.ns_valence).numpy() - f.cpu().numpy()      # dV_loc/dR + dV_nl/dR
    err = walker_errors(grad_v, fd_grad_potential(eng, h, r, phi, step=1e-5))
    print(f'all rows vs central differences: median {np.median(err):.2e}, 95th percentile {np.quantile(err, 0.95):.2e}, max {err.max():.2e}')
    assert np.median(err) < 1e-8 and np.quantile(err, 0.95) < 1e-6, (np.median(err), np.quantile(err, 0.95))


def test_repeats_and_chunks_are_bit_identical_gpu():
    B = 257
    h, wf, params, r, phi = make_system('b', B, DEV, dtype=torch.float32)
    eng = wf.engine(params)
    rt, ph = _t(r, torch.float32), _t(phi, torch.float32)
    for rows in ('own', 'all'):
        eng.set_option('ecp_max_cfg', 1 << 16)
        out0 = eng.ecp_force('bare', rt, ecp_phi=ph, rows=rows, return_parts=True)
        assert eng.last_chunks()['own'] == 1
        out1 = eng.ecp_force('bare', rt, ecp_phi=ph, rows=rows, return_parts=True)
        assert all(torch.equal(a, b) for a, b in zip(out0, out1))
        eng.set_option('ecp_max_cfg', 96 * 100)      # 96 quadrature configurations per walker: chunks of 100, 100, 57 walkers
        out2 = eng.ecp_force('bare', rt, ecp_phi=ph, rows=rows, return_parts=True)
        assert eng.last_chunks()['own'] == 3
        assert all(torch.equal(a, b) for a, b in zip(out0, out2))
        assert torch.all(torch.isfinite(out0[0]))


# float32 against float64 at 1024 LiH / PauliNet walkers, two-centre tables, same walkers and angles, over the walkers whose
# float32 log|psi| is within 1e-5 of float64 (away from a node of psi).  Parameters and walkers are drawn as
# test_gpu_force.py::test_float32_against_float64 draws them (parameter seed 7, walker seed 11): 91.8 % of the walkers pass
# that filter (with parameter seed 0 and walker seed 5 it was 89.8 %, and the errors 1.9e-6 / 2.0e-5: the share sits at 0.9).
# Measured normwise per-walker error on the MI355X, rows='own': parts[1] median 1.49e-6, 99th percentile 1.72e-5, max 1.1e-4;
# force median 1.65e-6, 99th percentile 1.82e-5, max 4.4e-5 (over all 1024 walkers: median 1.9e-6, 99th percentile 1.7e-4,
# max 2.1e-2, a walker near a node).  Bounds: (median, 99th percentile), about 5x that.
F32_BOUNDS = {'parts[1]': (7.5e-6, 8.5e-5), 'force': (8e-6, 9e-5)}


def test_float32_against_float64():
    B = 1024
    out = {}
    for dt in (torch.float64, torch.float32):
        h, wf, params, r, phi = make_system('b', B, DEV, dtype=dt, spec=ANSATZES['paulinet'](), seed=11, param_seed=7)
        # (the float32 context sees the float32-rounded walkers and angles; the float64 one is given exactly those)
        r32, phi32 = r.astype(np.float32), phi.astype(np.float32)
        eng = wf.engine(params)
        f, parts = eng.ecp_force('bare', _t(r32, dt), ecp_phi=_t(phi32, dt), rows='own', return_parts=True)
        # log|psi| of the walkers by the value pass the force call runs (the reverse pass's, op by op)
        logpsi = eng.log_psi_grad_coords(_t(r32, dt), want_r=False)[1]
        out[dt] = (logpsi.double().cpu().numpy(), parts[1].cpu().numpy(), f.cpu().numpy())
        wf.release()
    good = np.abs(out[torch.float32][0] - out[torch.float64][0]) < 1e-5
    print(f'walkers whose float32 log|psi| is within 1e-5 of float64: {good.mean():.4f}')
    assert good.mean() > 0.9, good.mean()
    for k, name in ((1, 'parts[1]'), (2, 'force')):
        err = walker_errors(out[torch.float32][k], out[torch.float64][k])[good]
        med, q99 = np.median(err), np.quantile(err, 0.99)
        print(f'{name}: float32 vs float64 normwise per-walker error: median {med:.2e}, 99th percentile {q99:.2e}, max {err.max():.2e}')
        assert med < F32_BOUNDS[name][0] and q99 < F32_BOUNDS[name][1], (name, med, q99)


def test_makers_and_antithetic_wrapper_gpu():
    B = 64
    h, wf, params, r, phi = make_system('a', B, DEV, dtype=torch.float32)
    rt = _t(r, torch.float32)
    pc = PhysicalConfiguration(_t(h.mol.coords, torch.float32), rt, torch.zeros(B, dtype=torch.int64))
    bare = ecp_force.evaluate_hf_force_bare(h, wf)
    for f in (bare(3, params, pc), force.antithetic_wrapper(bare, wf, 1.0)(3, params, pc),
              ecp_force.grad_nonloc_potential(h, wf)(3, params, pc)):
        assert f.shape == (B, 2, 3) and f.dtype == torch.float64 and f.device.type == 'cuda'
        assert torch.all(torch.isfinite(f))
    e_loc, _ = h.local_energy(wf)(3, params, pc)
    zb = ecp_force.evaluate_hf_force_ac_zb(h, wf)(3, params, pc, e_loc, float(e_loc.double().mean()))
    assert zb.shape == (B, 2, 3) and torch.all(torch.isfinite(zb))
