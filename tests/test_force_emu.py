"""Coordinate gradients of log|psi| (dqmc_log_psi_grad_coords) and the Hellmann-Feynman force estimators (dqmc_hf_force,
deepqmc_amd/force.py) through the SIMT emulation of the kernels: oracle autograd, the reference's quantum-force golden,
translation invariance, agreement with dqmc_psi_grad, determinism and chunking, invalid walkers, unsupported programs, and
every estimator against a torch restatement of its formula."""
import numpy as np
import pytest
import torch

from deepqmc_amd import force
from deepqmc_amd.engine import DqmcError, Engine
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.params import init_params
from deepqmc_amd.sampling import synthetic_walkers
from deepqmc_amd.types import PhysicalConfiguration
from deepqmc_amd.wf import NeuralNetworkWaveFunction
from force_util import check_coords_against_oracle, mirror, restated_force, setup, walker_errors
from oracle import geom
from param_grad_util import small_spec
from ref_ansatz_util import reference_test_engine
from simt_util import emu_lib

SMALL = dict(embedding_dim=32, n_interactions=1, n_determinants=2)


@pytest.mark.parametrize('name,mol,B', [('paulinet', 'LiH', 4), ('ferminet', 'N2', 2)])
def test_grad_coords_match_oracle_autograd(name, mol, B):
    check_coords_against_oracle(name, mol, B, 'cpu', emu_lib(), tol=1e-9, **SMALL)


def test_reference_quantum_force_golden(kats):
    h, P, tree, eng = reference_test_engine('cpu', lib=emu_lib(), norm_eps=geom.F64_EPS)
    r = torch.as_tensor(kats['lih_edges_ne'][0][None], dtype=torch.float64)
    sign, log, gr, gR = eng.log_psi_grad_coords(r)
    assert int(sign[0]) == int(kats['wf_psi_sign'])
    np.testing.assert_allclose(gr[0].numpy().reshape(-1), kats['wf_quantum_force'], rtol=0, atol=2e-6)
    # translation invariance of the reference ansatz (its 'ne' edges carry the nuclear dependence)
    np.testing.assert_allclose(gR[0].numpy().sum(0), -gr[0].numpy().sum(0), rtol=0, atol=1e-12)


def test_translation_invariance_and_psi_grad_agreement():
    h, spec, tree, eng, r = setup('paulinet', 'LiH', 6, 'cpu', emu_lib(), **SMALL)
    r = torch.as_tensor(r)
    sign, log, gr, gR = eng.log_psi_grad_coords(r)
    tot = gr.sum(1) + gR.sum(1)
    assert float(tot.abs().max()) < 1e-12 * max(1.0, float(gr.abs().max())), tot
    s2, l2, g2 = eng.psi_and_grad(r)
    assert torch.equal(s2, sign)
    assert walker_errors(gr.numpy(), g2.numpy()).max() < 1e-12
    np.testing.assert_allclose(log.numpy(), l2.numpy(), rtol=0, atol=1e-12)


def test_repeats_and_chunks_are_bit_identical():
    h, spec, tree, eng, r = setup('paulinet', 'LiH', 80, 'cpu', emu_lib(), **SMALL)
    r = torch.as_tensor(r)
    out0 = eng.log_psi_grad_coords(r)
    out1 = eng.log_psi_grad_coords(r)
    assert all(torch.equal(a, b) for a, b in zip(out0, out1))
    assert eng.last_chunks()['own'] == 1
    eng.set_option('ws_budget_mb', 1)
    out2 = eng.log_psi_grad_coords(r)
    assert eng.last_chunks()['own'] > 1
    assert all(torch.equal(a, b) for a, b in zip(out0, out2))
    # one output alone: the same values
    _, _, gr, none = eng.log_psi_grad_coords(r, want_R=False)
    assert none is None and torch.equal(gr, out0[2])


def test_invalid_walkers_get_zero_rows():
    h, spec, tree, eng, r = setup('paulinet', 'LiH', 4, 'cpu', emu_lib(), **SMALL)
    r = torch.as_tensor(r)
    bad = r.clone()
    bad[1, 0, 0] = float('nan')
    sign, log, gr, gR = eng.log_psi_grad_coords(bad)
    assert not np.isfinite(float(log[1])) or int(sign[1]) == 0
    assert torch.all(gr[1] == 0) and torch.all(gR[1] == 0)
    _, _, gr0, gR0 = eng.log_psi_grad_coords(r)
    keep = [0, 2, 3]
    assert torch.equal(gr[keep], gr0[keep]) and torch.equal(gR[keep], gR0[keep])


def test_attention_programs_are_unsupported():
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    spec = small_spec('psiformer', n_interactions=1, n_determinants=2)
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=0)
    eng = Engine(spec, h, tree, dtype=torch.float64, device='cpu', lib=emu_lib(), norm_eps=geom.F32_EPS)
    with pytest.raises(DqmcError, match='dqmc error -4'):
        eng.log_psi_grad_coords(torch.as_tensor(synthetic_walkers(h, 2, seed=0)))


def _wf(B=6, seed=9):
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'))
    wf = NeuralNetworkWaveFunction(h, small_spec('paulinet', **SMALL), dtype=torch.float64, device='cpu', lib=emu_lib(),
                                   norm_eps=geom.F32_EPS)
    params = wf.init(seed, perturb_envelopes=0.1)
    r = torch.as_tensor(synthetic_walkers(h, B, seed=seed))
    return h, wf, params, r


def test_estimators_match_restated_formulas():
    h, wf, params, r = _wf()
    pc = PhysicalConfiguration(torch.as_tensor(h.mol.coords), r, torch.zeros(r.shape[0], dtype=torch.int64))
    eng = wf.engine(params)
    _, _, g_r = eng.psi_and_grad(r)
    psi, gr, gR = wf.log_psi_grad_coords(params, pc)
    assert torch.equal(psi.sign, wf(params, r).sign)
    e_loc, _ = h.local_energy(wf)(None, params, r)
    energy = float(e_loc.mean())
    R, Z = h.mol.coords, h.mol.charges
    got = {
        'nuclear': force.nuclear_force(R, pc, Z),
        'bare': force.evaluate_hf_force_bare(h, wf)(None, params, pc),
        'ac_zvq': force.evaluate_hf_force_ac_zvq(h, wf)(params, pc),
        'ac_zvzbq': force.evaluate_hf_force_ac_zvzbq(h, wf)(params, pc, e_loc, energy),
        'ac_zb': force.evaluate_hf_force_ac_zb(h, wf)(None, params, pc, e_loc, energy),
        'ac_zvqzb': force.evaluate_hf_force_ac_zvqzb(h, wf)(params, pc, e_loc, energy),
    }
    for est, f in got.items():
        assert f.dtype == torch.float64 and f.shape == (r.shape[0], h.n_nuc, 3), est
        ref = restated_force(est, r, R, Z, grad_r=g_r, grad_R=gR, e_loc=e_loc, energy=energy)
        assert walker_errors(f.numpy(), ref.numpy()).max() < 1e-10, est
        if est != 'nuclear':            # the kernel's own estimator code gives the same
            eng_f = eng.hf_force(est, r, grad_r=g_r, grad_R=gR, e_loc=e_loc, energy=energy)
            assert torch.equal(eng_f, f), est
    np.testing.assert_array_equal(eng.hf_force('nuclear', r).numpy(), got['nuclear'].numpy())
    np.testing.assert_allclose(force.make_grad_nuc_log_wf(wf)(params, pc).numpy(), gR.numpy(), rtol=0, atol=0)
    q = force.Q(r, R, Z)
    d = r[:, None] - torch.as_tensor(R)[None, :, None]
    np.testing.assert_allclose(q.numpy(), (torch.as_tensor(Z)[None, :, None] * (d / d.norm(dim=-1, keepdim=True)).sum(2)).numpy(),
                               rtol=1e-14, atol=1e-14)
    # an estimator that needs an input it was not given is refused
    with pytest.raises(DqmcError, match='needs grad_R'):
        eng.hf_force('ac_zb', r, e_loc=e_loc, energy=energy)


def test_antithetic_wrapper_matches_restatement():
    h, wf, params, r = _wf(B=5, seed=4)
    r_cut = 1.0
    R, Z = h.mol.coords, h.mol.charges
    r_ = torch.as_tensor(mirror(r.numpy(), R, r_cut))
    assert not torch.equal(r_, r)
    log, log_ = wf(params, r).log, wf(params, r_).log
    w_ = 1 / (1 + torch.exp(-2 * (log_ - log)))
    eng = wf.engine(params)
    for name, make in (('bare', force.evaluate_hf_force_bare), ('ac_zvq', force.evaluate_hf_force_ac_zvq)):
        pc = PhysicalConfiguration(torch.as_tensor(R), r, torch.zeros(r.shape[0], dtype=torch.int64))
        got = force.antithetic_wrapper(make(h, wf), wf, r_cut)(None, params, pc)
        assert torch.equal(got, force.antithetic_wrapper(make(h, wf), wf, r_cut)(None, params, r))
        f = restated_force(name, r, R, Z, grad_r=eng.psi_and_grad(r)[2])
        f_ = restated_force(name, r_, R, Z, grad_r=eng.psi_and_grad(r_)[2])
        ref = (1 - w_)[:, None, None] * f + w_[:, None, None] * f_
        assert walker_errors(got.numpy(), ref.numpy()).max() < 1e-10, name
    with pytest.raises(ValueError, match='local energy'):
        force.antithetic_wrapper(force.evaluate_hf_force_ac_zb(h, wf), wf, r_cut)


def test_ecp_hamiltonians_are_refused():
    from test_ecp import TABLES
    h = MolecularHamiltonian(mol=Molecule.from_name('LiH'), ecp_type='synthetic', ecp_tables=TABLES)
    wf = NeuralNetworkWaveFunction(h, small_spec('paulinet', **SMALL), dtype=torch.float64, device='cpu', lib=emu_lib(),
                                   norm_eps=geom.F32_EPS)
    for make in (force.evaluate_hf_force_bare, force.evaluate_hf_force_ac_zvq, force.evaluate_hf_force_ac_zvzbq,
                 force.evaluate_hf_force_ac_zb, force.evaluate_hf_force_ac_zvqzb):
        with pytest.raises(NotImplementedError, match='effective core potential'):
            make(h, wf)
    # d log|psi| / d R itself does not depend on the Hamiltonian
    params = wf.init(0, perturb_envelopes=0.1)
    r = torch.as_tensor(synthetic_walkers(h, 2, seed=1))
    g = force.make_grad_nuc_log_wf(wf)(params, r)
    assert g.shape == (2, h.n_nuc, 3) and torch.all(torch.isfinite(g))
