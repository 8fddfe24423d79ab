"""Cases and shared checks of the shape-grid tests (tests/test_shape_grid_emu.py, tests/test_gpu_shape_grid.py): the widths,
head widths and electron counts BETWEEN the shapes every other test uses -- embedding widths that are no multiple of 16, odd
and non-multiple-of-4 two_particle_dim and head widths, and the electron counts on both sides of every kernel-selection
boundary (16/17, 32/33, 44/45, 48/49 of the determinant kernels; the 64-, 96-, 176- and 192-lane linear tiles).  The reference
is always oracle.program_interp.Interp in float64 on the same walkers, through the checks of large_n_util."""
import dataclasses

import numpy as np
import torch

from deepqmc_amd.engine import Engine
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.params import init_params
from deepqmc_amd.spec import ferminet, paulinet, psiformer, transpsiformer
from oracle import geom
from oracle.program_interp import Interp
from large_n_util import (check_f32_pass_alone, check_f64, check_vjp_and_coords, interp_reference, line, make_walkers,
                          narrow_spec)

B64, B32 = 3, 4       # walkers of a float64 / a float32 case

# ---------------------------------------------------------------- A. width grid
# (ansatz, molecule, embedding_dim, two_particle_dim, n_determinants); two interactions, so that the second layer reads
# two_particle_dim-wide pair features.  The last four pairs are the odd two_particle_dim ones.
PAIR_WIDTHS = [(17, 8), (18, 6), (33, 8), (36, 20), (100, 12), (16, 5), (16, 7), (32, 9), (65, 33)]
_MOLS, _DETS = ['LiH', 'C', 'N2'], [1, 3, 5, 7, 17]
MLP_CASES = [(name, _MOLS[(k + a) % 3], d, e, _DETS[(k + 2 * a) % 5])
             for a, name in enumerate(['ferminet', 'paulinet']) for k, (d, e) in enumerate(PAIR_WIDTHS)]
# (molecule, embedding_dim, num_heads): head widths 9, 10, 11, 18 (no multiple of 4), then 12, 12, 20, 36, 128; the last two
# have an embedding_dim that is no multiple of 4 (head widths 9 and 5), so the attention output has padding columns
PSIFORMER_CASES = [('LiH', 36, 4), ('C', 40, 4), ('N2', 44, 4), ('LiH', 36, 2),
                   ('C', 24, 2), ('N2', 36, 3), ('LiH', 80, 4), ('C', 36, 1), ('LiH', 256, 2), ('LiH', 18, 2), ('C', 10, 2)]
TRANSPSIFORMER_CASES = [('LiH', 36, 4), ('LiH', 48, 4)]
# float32 subset: (ansatz, molecule, embedding_dim, two_particle_dim or num_heads, n_determinants); odd pair widths for both
# message-passing ansatzes, head widths 9 and 18, and one right case of each kind
F32_CASES = [('ferminet', 'LiH', 16, 5, 2), ('paulinet', 'C', 32, 9, 3), ('ferminet', 'N2', 33, 8, 2), ('paulinet', 'LiH', 18, 6, 5),
             ('psiformer', 'LiH', 36, 4, 2), ('psiformer', 'C', 36, 2, 3), ('psiformer', 'N2', 24, 2, 2),
             ('psiformer', 'LiH', 18, 2, 2)]

# ---------------------------------------------------------------- B. electron-count grid
N_F64 = [5, 8, 9, 16, 17, 20, 27, 31, 33, 44, 47, 48, 53, 58, 59, 63]
N_REVERSE = [17, 33, 44, 48, 63]
N_F32 = [17, 20, 31, 33, 48, 58, 63]
N_PSIFORMER = [17, 33, 48]


def chain_molecule(n):
    """n electrons on a chain of nuclei of charge at most 9, 2.4 bohr apart: n // 9 fluorine-like nuclei and one of the
    remaining charge; spin n % 2."""
    charges = [9] * (n // 9) + ([n % 9] if n % 9 else [])
    coords, charges = line(charges, 2.4)
    return Molecule(coords=coords, charges=charges, charge=0, spin=n % 2)


def width_spec(name, mol, embedding_dim, second, n_determinants):
    """`second`: two_particle_dim of the message-passing ansatzes, num_heads of the attention ones."""
    if name in ('ferminet', 'paulinet'):
        return dataclasses.replace({'ferminet': ferminet, 'paulinet': paulinet}[name](), embedding_dim=embedding_dim,
                                   two_particle_dim=second, n_interactions=2, n_determinants=n_determinants)
    base = transpsiformer(mol.charges) if name == 'transpsiformer' else psiformer()
    return dataclasses.replace(base, embedding_dim=embedding_dim, num_heads=second, n_interactions=1, n_determinants=n_determinants)


def make_engine(spec, mol, dtype, device, lib=None):
    """(h, tree, eng) as large_n_util.setup makes them, for any spec and molecule."""
    h = MolecularHamiltonian(mol=mol)
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=3, perturb_envelopes=0.3)
    eng = Engine(spec, h, tree, dtype=dtype, device=device, lib=lib, norm_eps=geom.F32_EPS)
    if spec.layer_kind == 'attention' and not spec.nuclei_tokens:
        eng.set_option('attention_reverse', 1)
    return h, tree, eng


def width_setup(name, molname, embedding_dim, second, n_determinants, dtype, device, lib=None):
    mol = Molecule.from_name(molname)
    spec = width_spec(name, mol, embedding_dim, second, n_determinants)
    return (spec, mol) + make_engine(spec, mol, dtype, device, lib)


def chain_setup(name, n, dtype, device, lib=None):
    mol = chain_molecule(n)
    spec = narrow_spec(name)
    h, tree, eng = make_engine(spec, mol, dtype, device, lib)
    assert h.n_elec == n and eng.N == n
    return spec, mol, h, tree, eng


def chain_walkers(eng, mol, n, B=B64, cond_max=1e6):
    """The float64 walkers of an electron-count case: make_walkers with the first seed (1, 2, ...) for which every Slater
    matrix of the INTERPRETER has cond(A) < 1e6.  The derivative lanes of log|det A| carry the float64 round-off of the
    orbitals amplified by cond(A) in any implementation, the interpreter's LAPACK inverse included: at cond(A) = 4.5e6 that
    alone is the 1e-9 of check_f64, so a walker beyond it tests the conditioning and not the kernel (random-init determinants
    of 50 electrons reach 2e7; the rule looks at the reference only, never at the engine's answer)."""
    it = Interp(eng.program, mol.charges, geom.F32_EPS)
    for seed in range(1, 9):
        r = make_walkers(mol, n, B, seed=seed)
        it.run(r, mol.coords, laplacian=False)
        A = it.bufs[eng.program.buf_names['orbitals']][:, :, 0, :n * n].reshape(B, eng.spec.n_determinants, n, n)
        if np.linalg.cond(A).max() < cond_max:
            return r
    raise AssertionError(f'N={n}: no seed below 9 gives {B} walkers with cond(A) < {cond_max:g}')


def check_ill_conditioned(eng, mol, n, device, B=B64):
    """The walkers chain_walkers passes over (make_walkers' default seed, whatever cond(A) is -- 2e7 at 53 electrons), so that a
    pivoting fault of a determinant kernel cannot hide behind the selection: sign_k exact, and E_loc and E_kin of every walker
    within 50 cond(A) eps_f64 of the interpreter, relative to max(1, |value|) -- the form and constant of the float32 bound of
    test_gpu_parity.py::test_f32_local_energy with the float64 epsilon 2.2e-16 -- under options slogdet_mfma 1, 0 and 2.
    Returns the err / bound ratios and cond(A)."""
    r = make_walkers(mol, n, B)
    ref, _, sign_k = interp_reference(eng, mol, r)[:3]
    it = Interp(eng.program, mol.charges, geom.F32_EPS)
    it.run(r, mol.coords, laplacian=False)
    A = it.bufs[eng.program.buf_names['orbitals']][:, :, 0, :n * n].reshape(B, eng.spec.n_determinants, n, n)
    cond = np.linalg.cond(A).max(1)
    bound = 50 * cond * 2.2e-16
    out = {'cond_max': float(cond.max())}
    for opt in (1, 0, 2):
        eng.set_option('slogdet_mfma', opt)
        e, stats = eng.local_energy(torch.as_tensor(r, device=device))
        np.testing.assert_array_equal(eng.debug_read('sign_k', B), sign_k)
        for key, got, want in (('e_loc', e.cpu().numpy(), ref['e_loc']), ('e_kin', stats['hamil/E_kin'].cpu().numpy(), ref['stats'][1])):
            rel = np.abs(got - want) / np.maximum(1.0, np.abs(want))
            print(f'N={n} slogdet_mfma={opt} {key}: rel err {rel.max():.2e}, err / bound {(rel / bound).max():.2e}')
            out[f'{key}_rel_{opt}'] = float(rel.max())
            out[f'{key}_over_bound_{opt}'] = float((rel / bound).max())
            assert np.all(rel < bound), (opt, key, rel, bound)
    eng.set_option('slogdet_mfma', 1)
    return out


def deviations(out, eng, mol, r):
    """Largest deviations of what check_f64 returned ({option: (E_loc, logdet lanes)}) from the interpreter."""
    ref, logdet = interp_reference(eng, mol, r)[:2]
    return {f'slogdet_mfma_{opt}': {'e_loc_rel': float(np.abs(e / ref['e_loc'] - 1).max()), 'logdet_abs': float(np.abs(ld - logdet).max())}
            for opt, (e, ld) in out.items()}


def check_psi_both_paths(eng, mol, r, device):
    """wf_eval through the fused value kernel (option fused 1) and one launch per op (0): signs exact, log|psi| to 1e-11.
    Returns the largest deviation per path."""
    val = interp_reference(eng, mol, r)[3]
    dev = {}
    for fused in (1, 0):
        eng.set_option('fused', fused)
        sign, logpsi = eng.wf_eval(torch.as_tensor(r, device=device))
        err = np.abs(logpsi.cpu().numpy() - val['log'])
        print(f'N={r.shape[1]} {eng.spec.name} fused={fused}: log|psi| abs {err.max():.2e}')
        np.testing.assert_array_equal(sign.cpu().numpy(), val['sign'], err_msg=f'fused {fused}')
        np.testing.assert_allclose(logpsi.cpu().numpy(), val['log'], rtol=1e-11, atol=1e-11, err_msg=f'fused {fused}')
        dev[f'fused_{fused}'] = float(err.max())
    eng.set_option('fused', 1)
    return dev


def check_value_determinants(eng, mol, r, device):
    """wf_eval one launch per op with the register LU (option slogdet_mfma 1) and the LDS-resident LU (3), as
    test_large_n_emu.py::test_emu_value_determinants: sign_k exact, logdet and log|psi| to 1e-10."""
    B = r.shape[0]
    _, _, _, val, logdet, sign_k = interp_reference(eng, mol, r)
    eng.set_option('fused', 0)
    dev = {}
    for opt in (1, 3):
        eng.set_option('slogdet_mfma', opt)
        sign, logpsi = eng.wf_eval(torch.as_tensor(r, device=device))
        got = eng.debug_read('logdet', B)
        dev[f'value_logdet_abs_{opt}'] = float(np.abs(got - logdet).max())
        np.testing.assert_array_equal(eng.debug_read('sign_k', B), sign_k)
        np.testing.assert_allclose(got, logdet, rtol=1e-10, atol=1e-10)
        np.testing.assert_array_equal(sign.cpu().numpy(), val['sign'])
        np.testing.assert_allclose(logpsi.cpu().numpy(), val['log'], rtol=1e-10, atol=1e-10)
    eng.set_option('slogdet_mfma', 1)
    eng.set_option('fused', 1)
    return dev


def check_f32(eng, mol, spec, device):
    """The float32 checks of a case, on B32 walkers: psi signs equal to the float64 interpreter's and
    |log|psi| - ref| < 50 cond(A) 1.2e-7 (the constant of test_gpu_parity.py::test_f32_local_energy) through the fused value
    kernel and one launch per op, then large_n_util.check_f32_pass_alone.  Returns the err / bound ratios."""
    n = eng.N
    r32 = make_walkers(mol, n, B32).astype(np.float32)
    it = Interp(eng.program, mol.charges, geom.F32_EPS)
    ref = it.run(r32.astype(np.float64), mol.coords.astype(np.float32).astype(np.float64), laplacian=True)
    A = it.bufs[eng.program.buf_names['orbitals']][:, :, 0, :n * n].reshape(B32, spec.n_determinants, n, n)
    cond = np.linalg.cond(A).max(1)
    bound = 50 * cond * 1.2e-7
    ratios = {}
    for fused in (1, 0):
        eng.set_option('fused', fused)
        sign, logpsi = eng.wf_eval(torch.as_tensor(r32, device=device))
        err = np.abs(logpsi.cpu().numpy() - ref['log'])
        ratios[f'logpsi_fused_{fused}'] = float((err / bound).max())
        print(f'N={n} {spec.name} fused={fused}: float32 log|psi| err {err.max():.2e}, err / bound {(err / bound).max():.2e}')
        np.testing.assert_array_equal(sign.cpu().numpy(), ref['sign'], err_msg=f'fused {fused}')
        assert np.all(err < bound), (fused, err, bound)
    eng.set_option('fused', 1)
    rel = check_f32_pass_alone(eng, it, spec, r32, ref, device)
    ratios['e_loc_refine_0'] = float((rel / bound).max())
    return ratios


def check_metropolis_bit_exact(eng, spec, mol, h, tree, device, B=B64, n_sub=2):
    """Metropolis sub-steps on given noise against oracle/sampling.py, as
    test_large_n_emu.py::test_emu_metropolis_49_electrons_bit_exact: accept bits (at least one set), ages, tau, positions, log|psi|."""
    from oracle import sampling as osamp
    from oracle import wf as owf
    n = h.n_elec
    r0 = make_walkers(mol, n, B)
    val = interp_reference(eng, mol, r0)[3]           # the start state is the interpreter's, so a wrong psi cannot hide in it
    sign0 = torch.as_tensor(val['sign'], dtype=torch.int32, device=device)
    log0 = torch.as_tensor(val['log'], dtype=torch.float64, device=device)
    rng = np.random.default_rng(3)
    noise, unif = rng.standard_normal((n_sub, B, n, 3)), rng.random((n_sub, B))
    st = {'r': torch.as_tensor(r0, device=device).clone(), 'log': log0.clone(), 'sign': sign0.clone(),
          'age': torch.zeros(B, dtype=torch.int32, device=device), 'tau': torch.full((1,), 0.3, dtype=torch.float64, device=device)}
    stats, acc = eng.mcmc_steps(st, n_sub, noise=noise, unif=unif, return_accept=True)
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    ost = {'r': T(r0), 'sign': T(sign0.cpu().numpy()), 'log': T(log0.cpu().numpy()), 'age': torch.zeros(B, dtype=torch.int64), 'tau': 0.3}
    ost, ostats, oacc = osamp.decorr_sample(owf.to_torch(tree), spec, ost, T(mol.coords), h.n_up, geom.F32_EPS, T(noise), T(unif))
    assert np.isfinite(st['log'].cpu().numpy()).all() and oacc.numpy().any()
    np.testing.assert_array_equal(acc.cpu().numpy().astype(bool), oacc.numpy())
    np.testing.assert_array_equal(st['age'].cpu().numpy(), ost['age'].numpy())
    np.testing.assert_allclose(float(st['tau'][0]), float(ost['tau']), rtol=1e-14)
    np.testing.assert_allclose(st['r'].cpu().numpy(), ost['r'].numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(st['log'].cpu().numpy(), ost['log'].numpy(), rtol=1e-11, atol=1e-11)
    return int(oacc.numpy().sum())


__all__ = ['B64', 'B32', 'MLP_CASES', 'PSIFORMER_CASES', 'TRANSPSIFORMER_CASES', 'F32_CASES', 'N_F64', 'N_REVERSE', 'N_F32',
           'N_PSIFORMER', 'chain_setup', 'chain_walkers', 'check_ill_conditioned', 'width_setup', 'deviations', 'check_psi_both_paths', 'check_value_determinants',
           'check_f32', 'check_metropolis_bit_exact', 'check_f64', 'check_vjp_and_coords', 'make_walkers']
