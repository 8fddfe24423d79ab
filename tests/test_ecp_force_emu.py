"""Hellmann-Feynman forces of Gaussian-type ECP Hamiltonians (dqmc_ecp_force, deepqmc_amd/ecp_force.py) through the SIMT
emulation of the kernels, float64: both row modes against torch.autograd of the oracle's local and non-local potential, the
full gradient against finite differences of the library's own V_loc + V_nl, the zero-bias estimator, the Python surface,
zero tables, chunking / determinism / invalid walkers, and the refusals."""
import numpy as np
import pytest
import torch

from deepqmc_amd import ecp_force, force
from deepqmc_amd.engine import DqmcError, Engine
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.params import init_params
from deepqmc_amd.sampling import synthetic_walkers
from deepqmc_amd.types import PhysicalConfiguration
from deepqmc_amd.wf import NeuralNetworkWaveFunction
from ecp_force_util import SMALL, TWO_CENTRE, fd_grad_potential, make_hamil, make_system, oracle_parts_cached
from force_util import mirror, restated_force, walker_errors
from oracle import geom
from param_grad_util import small_spec
from simt_util import emu_lib

T = torch.as_tensor


def _one_ulp(got, ref):
    return bool(np.all(np.abs(got - ref) <= np.spacing(np.abs(ref))))


@pytest.mark.parametrize('rows', ['own', 'all'])
@pytest.mark.parametrize('system,B', [('a', 2), ('b', 1), ('c', 1)])
def test_parts_match_oracle_autograd(system, B, rows):
    h, wf, params, r, phi = make_system(system, B, 'cpu', emu_lib())
    f, parts = wf.engine(params).ecp_force('bare', T(r), ecp_phi=T(phi), rows=rows, return_parts=True)
    assert f.dtype == torch.float64 and f.shape == (B, h.n_nuc, 3) and parts.shape == (2, B, h.n_nuc, 3)
    ref0, ref1 = oracle_parts_cached(system, B, rows)
    e0, e1 = walker_errors(parts[0].numpy(), ref0), walker_errors(parts[1].numpy(), ref1)
    print(f'{system} {rows}: parts[0] error {e0.max():.2e}, parts[1] error {e1.max():.2e}')
    assert e1.max() < 1e-8, e1
    assert e0.max() < 1e-10, e0
    assert _one_ulp(f.numpy(), (parts[0] + parts[1]).numpy())
    if system == 'c':
        assert list(h.pot.nuc_with_nl_pot) == [1]
        if rows == 'own':
            assert torch.all(parts[1][:, 0] == 0)          # Li has no non-local channel: its own row is empty
        assert float(parts[1][:, 1].abs().max()) > 1e-3    # ... and H's row sits at row 1, not at row j = 0
    if system == 'b' and rows == 'all':                    # the two modes differ where a test can see it
        own = oracle_parts_cached(system, B, 'own')[1]
        assert np.abs(own[:, 1] - ref1[:, 1]).max() > 0.1


def test_all_rows_against_finite_differences_of_the_potential():
    B = 4
    h, wf, params, r, phi = make_system('b', B, 'cpu', emu_lib())
    eng = wf.engine(params)
    f = eng.ecp_force('bare', T(r), ecp_phi=T(phi), rows='all')
    grad_v = restated_force('nuclear', r, h.mol.coords, h.ns_valence).numpy() - f.numpy()      # dV_loc/dR + dV_nl/dR
    fd = fd_grad_potential(eng, h, r, phi, step=1e-5)
    err = walker_errors(grad_v, fd)
    print(f'all rows vs central differences: median {np.median(err):.2e}, 95th percentile {np.quantile(err, 0.95):.2e}')
    assert np.median(err) < 1e-8 and np.quantile(err, 0.95) < 1e-6, err


def test_ac_zb_adds_the_zero_bias_term():
    B = 3
    h, wf, params, r, phi = make_system('b', B, 'cpu', emu_lib())
    eng = wf.engine(params)
    rt, ph = T(r), T(phi)
    e_loc, _ = eng.local_energy(rt, ecp_phi=ph)
    energy = float(e_loc.mean())
    gR = eng.log_psi_grad_coords(rt, want_r=False)[3]
    for rows in ('own', 'all'):
        bare = eng.ecp_force('bare', rt, ecp_phi=ph, rows=rows)
        zb = eng.ecp_force('ac_zb', rt, ecp_phi=ph, e_loc=e_loc, energy=energy, rows=rows)
        ref = bare - 2 * (e_loc - energy)[:, None, None] * gR
        assert walker_errors(zb.numpy(), ref.numpy()).max() < 1e-10
    assert float((zb - bare).abs().max()) > 1e-6


def test_python_surface():
    B = 3
    h, wf, params, r, phi = make_system('b', B, 'cpu', emu_lib())
    eng = wf.engine(params)
    rt, ph = T(r), T(phi)
    pc = PhysicalConfiguration(T(h.mol.coords), rt, torch.zeros(B, dtype=torch.int64))
    for rows in ('own', 'all'):
        f, parts = eng.ecp_force('bare', rt, ecp_phi=ph, rows=rows, return_parts=True)
        assert torch.equal(ecp_force.grad_nonloc_potential(h, wf, rows)(None, params, pc, ecp_phi=ph), -parts[1])
        assert torch.equal(ecp_force.evaluate_hf_force_bare(h, wf, rows)(None, params, pc, ecp_phi=ph), f)
    # an int seed instead of explicit angles: finite, the same from call to call, the same through every entry
    f7, p7 = eng.ecp_force('bare', rt, rng=7, return_parts=True)
    assert torch.all(torch.isfinite(f7)) and torch.equal(f7, eng.ecp_force('bare', rt, rng=7))
    assert not torch.equal(f7, eng.ecp_force('bare', rt, rng=8))
    assert torch.equal(ecp_force.evaluate_hf_force_bare(h, wf)(7, params, pc), f7)
    assert torch.equal(ecp_force.evaluate_hf_force_bare(h, wf)(7, params, rt), f7)
    assert torch.equal(ecp_force.grad_nonloc_potential(h, wf)(7, params, pc), -p7[1])
    assert torch.equal(h.pot.grad_nonloc_potential(wf, 7, pc, params), -p7[1])
    e_loc, _ = eng.local_energy(rt, rng=7)
    zb = ecp_force.evaluate_hf_force_ac_zb(h, wf)
    assert (zb.takes_rng, zb.needs_energy, zb.estimator) == (True, True, 'ac_zb')
    assert torch.equal(zb(7, params, pc, e_loc, 0.25), eng.ecp_force('ac_zb', rt, rng=7, e_loc=e_loc, energy=0.25))
    # dV_loc/dR: the first part without the nuclear repulsion force
    dloc = ecp_force.grad_local_potential(h, wf)(params, pc)
    ref = restated_force('nuclear', r, h.mol.coords, h.ns_valence) - p7[0]
    assert walker_errors(dloc.numpy(), ref.numpy()).max() < 1e-13
    with pytest.raises(DqmcError, match='needs `rng`'):
        eng.ecp_force('bare', rt)


def test_antithetic_wrapper_matches_restatement():
    B, r_cut, seed = 3, 1.0, 11
    h, wf, params, r, phi = make_system('b', B, 'cpu', emu_lib(), seed=4)
    R = h.mol.coords
    r_ = mirror(r, R, r_cut)
    assert not np.array_equal(r_, r)
    log, log_ = wf(params, T(r)).log, wf(params, T(r_)).log
    w_ = 1 / (1 + torch.exp(-2 * (log_ - log)))
    bare = ecp_force.evaluate_hf_force_bare(h, wf)
    assert (bare.takes_rng, bare.needs_energy, bare.estimator) == (True, False, 'bare')
    pc = PhysicalConfiguration(T(R), T(r), torch.zeros(B, dtype=torch.int64))
    got = force.antithetic_wrapper(bare, wf, r_cut)(seed, params, pc)
    eng = wf.engine(params)
    f, f_ = eng.ecp_force('bare', T(r), rng=seed), eng.ecp_force('bare', T(r_), rng=seed)
    ref = (1 - w_)[:, None, None] * f + w_[:, None, None] * f_
    assert walker_errors(got.numpy(), ref.numpy()).max() < 1e-10
    with pytest.raises(ValueError, match='local energy'):
        force.antithetic_wrapper(ecp_force.evaluate_hf_force_ac_zb(h, wf), wf, r_cut)


def test_zero_tables():
    B = 2
    loc_li, loc_h = TWO_CENTRE['Li'][1][0], TWO_CENTRE['H'][1][0]
    zero_loc = lambda a: [-1, [[], [[a, 0.0]], [[a, 0.0]], [[a, 0.0]]]]
    # non-local coefficients zero under non-zero exponents: the quadrature runs and every term vanishes
    tabs = {'Li': [0, [loc_li, [0, [[], [], [[1.3, 0.0]]]]]], 'H': [0, [loc_h, [0, [[], [], [[0.7, 0.0]]]]]]}
    h, wf, params, r, phi = make_system('b', B, 'cpu', emu_lib(), tables=tabs)
    assert len(h.pot.nuc_with_nl_pot) == 2
    eng = wf.engine(params)
    f, parts = eng.ecp_force('bare', T(r), ecp_phi=T(phi), return_parts=True)
    assert torch.all(parts[1] == 0) and torch.equal(f, parts[0])
    # a non-local table of zeros: a local-only ECP, no reverse pass
    tabs = {'Li': [0, [loc_li, [0, [[], [], [[0.0, 0.0]]]]]], 'H': [0, [loc_h, [0, [[], [], [[0.0, 0.0]]]]]]}
    h, wf, params, r, phi = make_system('b', B, 'cpu', emu_lib(), tables=tabs)
    assert len(h.pot.nuc_with_nl_pot) == 0 and h.pot.loc_params.any()
    eng = wf.engine(params)
    f0, parts = eng.ecp_force('bare', T(r), rng=1, return_parts=True)
    assert torch.all(parts[1] == 0) and torch.equal(f0, parts[0]) and torch.equal(f0, f)
    assert walker_errors(f0.numpy(), eng.hf_force('bare', T(r)).numpy()).min() > 1e-3      # the local terms are there
    # ... unless the zero-bias term asks for the walkers' own d log|psi| / dR
    e_loc, _ = eng.local_energy(T(r), rng=1)
    zb = eng.ecp_force('ac_zb', T(r), rng=1, e_loc=e_loc, energy=0.5)
    ref = f0 - 2 * (e_loc - 0.5)[:, None, None] * eng.log_psi_grad_coords(T(r), want_r=False)[3]
    assert walker_errors(zb.numpy(), ref.numpy()).max() < 1e-12
    # all local coefficients zero as well: the all-electron bare force of the same context
    for nl_exp in (0.0, 0.9):
        tabs = {'Li': [0, [zero_loc(5.4), [0, [[], [], [[nl_exp, 0.0]]]]]], 'H': [0, [zero_loc(21.2), [0, [[], [], [[nl_exp, 0.0]]]]]]}
        h, wf, params, r, phi = make_system('b', B, 'cpu', emu_lib(), tables=tabs)
        eng = wf.engine(params)
        f, parts = eng.ecp_force('bare', T(r), rng=1, return_parts=True)
        assert torch.all(parts[1] == 0)
        assert walker_errors(f.numpy(), eng.hf_force('bare', T(r)).numpy()).max() < 1e-12


def test_chunks_repeats_and_invalid_walkers():
    B = 10
    h, wf, params, r, phi = make_system('b', B, 'cpu', emu_lib())
    eng = wf.engine(params)
    rt, ph = T(r), T(phi)
    for rows in ('own', 'all'):
        eng.set_option('ecp_max_cfg', 1 << 16)
        out0 = eng.ecp_force('bare', rt, ecp_phi=ph, rows=rows, return_parts=True)
        assert eng.last_chunks()['own'] == 1
        out1 = eng.ecp_force('bare', rt, ecp_phi=ph, rows=rows, return_parts=True)
        assert all(torch.equal(a, b) for a, b in zip(out0, out1))
        eng.set_option('ecp_max_cfg', 300)          # 96 quadrature configurations per walker: chunks of 3, 3, 3, 1 walkers
        out2 = eng.ecp_force('bare', rt, ecp_phi=ph, rows=rows, return_parts=True)
        assert eng.last_chunks()['own'] == 4
        assert all(torch.equal(a, b) for a, b in zip(out0, out2))
        bad = rt.clone()
        bad[4, 1, 2] = float('nan')
        fb, pb = eng.ecp_force('bare', bad, ecp_phi=ph, rows=rows, return_parts=True)
        assert torch.all(torch.isnan(fb[4])) and torch.all(torch.isnan(pb[1][4]))
        keep = [b for b in range(B) if b != 4]
        assert torch.equal(fb[keep], out0[0][keep]) and torch.equal(pb[:, keep], out0[1][:, keep])


def test_refusals():
    from test_pseudo_hamiltonian import synthetic_tables
    mol = Molecule.from_name('LiH')
    spec = small_spec('paulinet', **SMALL)
    mk = lambda h: NeuralNetworkWaveFunction(h, spec, dtype=torch.float64, device='cpu', lib=emu_lib(), norm_eps=geom.F32_EPS)
    h_ph = MolecularHamiltonian(mol=mol, ecp_type='PH', ecp_mask=[True, False], ph_tables=synthetic_tables())
    h_ae = MolecularHamiltonian(mol=mol)
    for h in (h_ph, h_ae):
        wf = mk(h)
        for make in (ecp_force.evaluate_hf_force_bare, ecp_force.evaluate_hf_force_ac_zb, ecp_force.grad_nonloc_potential,
                     ecp_force.grad_local_potential):
            with pytest.raises(NotImplementedError, match='pseudo-Hamiltonian' if h is h_ph else 'deepqmc_amd.force'):
                make(h, wf)
        # the library itself refuses too
        r = T(synthetic_walkers(h, 2, seed=0))
        with pytest.raises(DqmcError, match='dqmc error -1'):
            wf.engine(wf.init(0)).ecp_force('bare', r, rng=1)
    h = make_hamil('a')
    spec_pf = small_spec('psiformer', n_interactions=1, n_determinants=2)
    tree = init_params(spec_pf, h.n_up, h.n_down, h.n_nuc, seed=0)
    eng = Engine(spec_pf, h, tree, dtype=torch.float64, device='cpu', lib=emu_lib(), norm_eps=geom.F32_EPS)
    r = T(synthetic_walkers(h, 2, seed=0))
    with pytest.raises(DqmcError, match='dqmc error -4'):
        eng.ecp_force('bare', r, rng=1)
    h, wf, params, r, phi = make_system('a', 2, 'cpu', emu_lib())
    eng = wf.engine(params)
    with pytest.raises(DqmcError, match='e_loc'):
        eng.ecp_force('ac_zb', T(r), ecp_phi=T(phi))
    with pytest.raises(ValueError, match='unknown ECP force estimator'):
        eng.ecp_force('ac_zvq', T(r), ecp_phi=T(phi))
    with pytest.raises(ValueError, match='rows'):
        eng.ecp_force('bare', T(r), ecp_phi=T(phi), rows='some')
