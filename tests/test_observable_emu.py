"""The observable monitors through the SIMT emulation of the kernels: dqmc_oscillator_strength, dqmc_fd_displace and dqmc_fd_force
against NumPy transcriptions of their formulas, the finite-difference estimator end to end, every monitor against a direct call
of what it is built on, fit_wf with and without `observable_monitors`."""
import numpy as np
import pytest
import torch

from deepqmc_amd import observable as obs
from deepqmc_amd.engine import DqmcError
from ecp_force_util import make_system
from loss_util import SMALL
from observable_util import (ALL_NAMES, F64, OS_SHAPES, check_fd_displace, check_fd_force, check_finite_difference_force,
                             check_fit_with_monitors, check_fit_without_monitors, check_monitor, check_oscillator_strength,
                             monitor_batch)
from optimizer_util import make_pair
from simt_util import emu_lib


@pytest.fixture(scope='module')
def engines():
    """{(molecule, dtype): Engine}: small PauliNet contexts of LiH and of H2O (three nuclei) in both dtypes."""
    return {(mol, dtype): make_pair('paulinet', mol, dtype, 'cpu', emu_lib(), **SMALL)[3]
            for mol in ('LiH', 'H2O') for dtype in (torch.float64, torch.float32)}


@pytest.fixture(scope='module')
def batch():
    return monitor_batch('cpu', emu_lib())


# ---- 1. dqmc_oscillator_strength
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('S,B', OS_SHAPES)
def test_oscillator_strength_matches_the_transcription(engines, S, B, dtype):
    check_oscillator_strength(engines['LiH', dtype], S, B)


def test_oscillator_strength_rejects_wrong_arguments(engines):
    eng = engines['LiH', torch.float64]
    r, ratio, e = torch.zeros(2, 5, 4, 3, dtype=F64), torch.ones(2, 2, 5, dtype=F64), torch.zeros(2, 5, dtype=F64)
    with pytest.raises(DqmcError, match="'psi_ratio'"):
        eng.oscillator_strength(r, ratio.float(), e)
    with pytest.raises(DqmcError, match="'psi_ratio'"):
        eng.oscillator_strength(r, ratio[:, :, :4].contiguous(), e)
    with pytest.raises(DqmcError, match="'e_loc'"):
        eng.oscillator_strength(r, ratio, e[:1])
    with pytest.raises(DqmcError, match="'r'"):
        eng.oscillator_strength(r[:, :, :3], ratio, e)
    with pytest.raises(DqmcError, match='number of states'):
        eng.oscillator_strength(torch.zeros(33, 1, 4, 3, dtype=F64), torch.ones(33, 33, 1, dtype=F64), torch.zeros(33, 1, dtype=F64))


# ---- 2. dqmc_fd_displace
@pytest.mark.parametrize('B', [1, 65])
@pytest.mark.parametrize('mol', ['LiH', 'H2O'])
def test_fd_displace_matches_numpy(engines, mol, B):
    check_fd_displace(engines[mol, torch.float64], engines[mol, torch.float32], B)


# ---- 3. dqmc_fd_force
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('B', [1, 65])
def test_fd_force_matches_numpy(engines, B, dtype):
    check_fd_force(engines['H2O', dtype], B)
    eng = engines['LiH', dtype]
    with pytest.raises(DqmcError, match="'log_d'"):
        eng.fd_force(torch.zeros(5, B, dtype=dtype), torch.zeros(B, dtype=dtype), torch.zeros(6, B, dtype=dtype), torch.zeros(B, dtype=dtype), 1e-3)
    with pytest.raises(DqmcError, match='step size'):
        eng.fd_force(torch.zeros(6, B, dtype=dtype), torch.zeros(B, dtype=dtype), torch.zeros(6, B, dtype=dtype), torch.zeros(B, dtype=dtype), 0.0)


# ---- 4. evaluate_finite_difference_force
def test_finite_difference_force_end_to_end():
    check_finite_difference_force('cpu', emu_lib())


# ---- 5. monitors
@pytest.mark.parametrize('name', ALL_NAMES)
def test_monitor_from_name_round_trips(name):
    m = obs.observable_monitor_from_name(name)
    assert isinstance(m, obs.ObservableMonitor) and m.name == name and m.save_samples is True and m.period == 1


def test_unknown_and_unbuilt_names():
    with pytest.raises(ValueError, match='Unknown observable monitor'):
        obs.observable_monitor_from_name('no_such_monitor')
    for name in ('hf_force_ac_zv', 'hf_force_ac_zvzb'):
        with pytest.raises(NotImplementedError, match='ZV term'):
            obs.observable_monitor_from_name(name)
    (m,) = obs.default_observable_monitors()
    assert isinstance(m, obs.WaveFunctionMonitor) and m.save_samples and m.period == 1


@pytest.mark.parametrize('name', ['spin', 'hf_force_bare', 'hf_force_bare_anti', 'hf_force_ac_zvq', 'hf_force_ac_zvq_anti',
                                  'hf_force_ac_zvzbq', 'hf_force_ac_zb', 'hf_force_ac_zvqzb', 'finite_difference_force'])
def test_monitor_samples_are_the_direct_calls(batch, name):
    stats = check_monitor(name, batch)
    assert torch.isfinite(stats[f'{name}/mean']).all()


def test_the_monitors_without_an_estimator(batch):
    hamil, wf, params, pc, psi, e_loc, ratios = batch
    call = lambda m: m.finalize(hamil, wf)(0, 1, params, pc, psi, e_loc, ratios)
    S, B = pc.r.shape[1:3]
    e64 = e_loc.double()
    out = call(obs.EnergyMonitor(True, 1))
    assert set(out) == {'local_energy/mean', 'local_energy/std', 'local_energy/min', 'local_energy/max', 'local_energy/samples'}
    want = {'mean': e64.mean(dim=-1), 'std': e64.std(dim=-1, unbiased=False), 'min': e64.amin(dim=-1), 'max': e64.amax(dim=-1), 'samples': e64}
    for key, v in want.items():                      # (what fit_wf computes: test_fit_wf_with_monitors compares the yielded ones)
        assert torch.equal(out[f'local_energy/{key}'], v), key
    out = call(obs.ElectronPositionMonitor(True, 1))
    assert set(out) == {'r/samples'} and torch.equal(out['r/samples'], pc.r.double())
    out = call(obs.NuclearPositionMonitor(True, 1))
    assert set(out) == {'R/samples'} and tuple(out['R/samples'].shape) == (1, S, hamil.n_nuc, 3)
    assert torch.equal(out['R/samples'][0, 1], torch.as_tensor(pc.R[0]).double())
    out = call(obs.WaveFunctionMonitor(True, 1))
    assert set(out) == {'psi/samples'} and torch.equal(out['psi/samples']['log'], psi.log.double())
    assert torch.equal(out['psi/samples']['sign'], psi.sign.double()) and tuple(psi.log.shape) == (1, S, B)
    out = call(obs.PsiRatioMonitor(True, 1))
    assert set(out) == {'psi_ratio/samples'} and torch.equal(out['psi_ratio/samples'], ratios)
    for m in (obs.ElectronPositionMonitor(False, 1), obs.PsiRatioMonitor(False, 1), obs.WaveFunctionMonitor(True, 3)):
        assert m.finalize(hamil, wf)(1 if m.period == 3 else 0, 1, params, pc, psi, e_loc, ratios) == {}
    out = call(obs.OscillatorStrengthMonitor(True, 1))
    assert set(out) == {'oscillator_strength/mean', 'oscillator_strength/err'} and tuple(out['oscillator_strength/mean'].shape) == (1, S, S)
    os_mean, os_err, _, _ = wf.engine(params[0], pc.R[0]).oscillator_strength(pc.r[0], ratios[0].contiguous(), e_loc[0])
    assert torch.equal(out['oscillator_strength/mean'][0], os_mean)
    assert torch.equal(torch.nan_to_num(out['oscillator_strength/err'][0], nan=-1.0), torch.nan_to_num(os_err, nan=-1.0))
    with pytest.raises(ValueError, match='psi ratios'):
        obs.OscillatorStrengthMonitor(False, 1).finalize(hamil, wf)(0, 1, params, pc, psi, e_loc, None)
    with pytest.raises(RuntimeError, match='finalize'):
        obs.OscillatorStrengthMonitor(False, 1)(0, 1, params, pc, psi, e_loc, ratios)


def test_oscillator_strength_monitor_is_single_process(batch, monkeypatch):
    import torch.distributed as dist
    hamil, wf, params, pc, psi, e_loc, ratios = batch
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda *a: 2)
    with pytest.raises(NotImplementedError, match='single process'):
        obs.OscillatorStrengthMonitor(False, 1).finalize(hamil, wf)(0, 1, params, pc, psi, e_loc, ratios)


def test_ecp_hamiltonians_are_routed_and_refused():
    """Gaussian-type ECP (system 'b': both nuclei, N = 4): the bare and ZB monitors give what deepqmc_amd.ecp_force gives, the ZVQ
    family refuses the Hamiltonian in finalize."""
    h, wf, p, r, _ = make_system('b', 2, 'cpu', emu_lib())
    params = [p, wf.init(1, perturb_envelopes=0.1)]
    r = torch.as_tensor(np.stack([r, r[::-1].copy()]))[None]
    from deepqmc_amd.types import PhysicalConfiguration, Psi
    pc = PhysicalConfiguration(torch.as_tensor(np.asarray(h.mol.coords))[None], r, None)
    e_loc = torch.stack([wf.engine(params[s]).local_energy(r[0, s].contiguous(), rng=11)[0] for s in range(2)])[None]
    psi = Psi(torch.ones(1, 2, 2), torch.zeros(1, 2, 2))
    batch = (h, wf, params, pc, psi, e_loc, None)
    for name in ('hf_force_bare', 'hf_force_ac_zb', 'hf_force_bare_anti'):
        check_monitor(name, batch)
    for cls in (obs.ACZVQForceMonitor, obs.ACZVQForceAntiMonitor, obs.ACZVZBQForceMonitor, obs.ACZVQZBForceMonitor):
        with pytest.raises(NotImplementedError, match='effective core potential'):
            cls(False, 1).finalize(h, wf)


# ---- 6. fit_wf
def test_fit_wf_with_monitors():
    check_fit_with_monitors('cpu', emu_lib(), torch.float64, 16)


def test_fit_wf_without_monitors_yields_what_it_yielded():
    check_fit_without_monitors('cpu', emu_lib(), torch.float64, 16)
