"""Local energy, psi, Metropolis sub-steps and the reverse pass for the electron counts between and beyond the benchmark
systems', through the SIMT emulation of the unmodified kernels: the 80- / 112- / 144- / 208-lane linear tiles, the determinant
kernels of 45 .. 64 electrons (4 x 4-tile MFMA form, dynamic-LDS scalar form, 64-wide register LU, dynamic-LDS inverse of
the reverse pass) and the creation gate at 64.  Narrow ansatzes, 2 walkers; no walker is left out of any check."""
import numpy as np
import pytest
import torch

from deepqmc_amd.engine import DqmcError
from oracle import geom
from oracle.program_interp import Interp
from large_n_util import check_f32_pass_alone, check_f64, check_vjp_and_coords, interp_reference, make_walkers, molecule, setup
from simt_util import emu_lib

B = 2


@pytest.mark.parametrize('n', [45, 64])
def test_creation_succeeds_past_44(n):
    spec, mol, h, tree, eng = setup('ferminet', n, torch.float64, 'cpu', emu_lib())
    assert eng.N == n


def test_creation_refuses_65_electrons():
    with pytest.raises(DqmcError, match=r'^dqmc error -1: malformed op #\d+ kind 9$'):
        setup('ferminet', 65, torch.float64, 'cpu', emu_lib())


@pytest.mark.parametrize('name,n', [('ferminet', 22), ('ferminet', 32), ('ferminet', 43), ('ferminet', 45), ('ferminet', 49),
                                    ('ferminet', 64), ('psiformer', 22), ('psiformer', 49), ('psiformer', 64)])
def test_emu_f64_local_energy(name, n):
    """local_energy(return_grad=True) and wf_eval against the interpreter; from 45 electrons on with the MFMA determinant
    kernel (option slogdet_mfma 1) and the scalar one (0)."""
    spec, mol, h, tree, eng = setup(name, n, torch.float64, 'cpu', emu_lib())
    r = make_walkers(mol, n, B)
    check_f64(eng, mol, r, 'cpu', options=(1, 0) if n >= 45 else (None,))


@pytest.mark.parametrize('n', [45, 49, 64])
def test_emu_value_determinants(n):
    """wf_eval with the 64-wide register LU (option 1) and the LDS-resident LU (option 3): signs exact, log 1e-10."""
    spec, mol, h, tree, eng = setup('ferminet', n, torch.float64, 'cpu', emu_lib())
    eng.set_option('fused', 0)
    r = make_walkers(mol, n, B)
    _, _, _, val, logdet, sign_k = interp_reference(eng, mol, r)
    for opt in (1, 3):
        eng.set_option('slogdet_mfma', opt)
        sign, logpsi = eng.wf_eval(torch.as_tensor(r))
        np.testing.assert_array_equal(eng.debug_read('sign_k', B), sign_k)
        np.testing.assert_allclose(eng.debug_read('logdet', B), logdet, rtol=1e-10, atol=1e-10)
        np.testing.assert_array_equal(sign.numpy(), val['sign'])
        np.testing.assert_allclose(logpsi.numpy(), val['log'], rtol=1e-10, atol=1e-10)


def test_emu_metropolis_49_electrons_bit_exact():
    """Two Metropolis sub-steps at N = 49 on given noise against oracle/sampling.py: accept bits, ages, tau, positions."""
    from oracle import sampling as osamp
    from oracle import wf as owf
    n = 49
    spec, mol, h, tree, eng = setup('ferminet', n, torch.float64, 'cpu', emu_lib())
    r0 = make_walkers(mol, n, B)
    sign0, log0 = eng.wf_eval(torch.as_tensor(r0))
    n_sub = 2
    rng = np.random.default_rng(3)
    noise, unif = rng.standard_normal((n_sub, B, n, 3)), rng.random((n_sub, B))
    st = {'r': torch.as_tensor(r0).clone(), 'log': log0.clone(), 'sign': sign0.clone(),
          'age': torch.zeros(B, dtype=torch.int32), 'tau': torch.full((1,), 0.05, dtype=torch.float64)}
    stats, acc = eng.mcmc_steps(st, n_sub, noise=noise, unif=unif, return_accept=True)
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    ost = {'r': T(r0), 'sign': T(sign0.numpy()), 'log': T(log0.numpy()), 'age': torch.zeros(B, dtype=torch.int64), 'tau': 0.05}
    ost, ostats, oacc = osamp.decorr_sample(owf.to_torch(tree), spec, ost, T(mol.coords), h.n_up, geom.F32_EPS, T(noise), T(unif))
    np.testing.assert_array_equal(acc.numpy().astype(bool), oacc.numpy())
    np.testing.assert_array_equal(st['age'].numpy(), ost['age'].numpy())
    np.testing.assert_allclose(float(st['tau'][0]), float(ost['tau']), rtol=1e-14)
    np.testing.assert_allclose(st['r'].numpy(), ost['r'].numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(st['log'].numpy(), ost['log'].numpy(), rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize('n', [49, 64])
def test_emu_reverse_pass(n):
    """log_psi_vjp and log_psi_grad_coords past the old 44-electron cap of the reverse pass's inverse."""
    spec, mol, h, tree, eng = setup('ferminet', n, torch.float64, 'cpu', emu_lib())
    check_vjp_and_coords(eng, spec, h, tree, make_walkers(mol, n, B), 'cpu')


@pytest.mark.parametrize('n', [22, 49])
def test_emu_f32_local_energy(n):
    """float32 FermiNet: E_loc finite, psi signs equal to the float64 interpreter's."""
    spec, mol, h, tree, eng = setup('ferminet', n, torch.float32, 'cpu', emu_lib())
    r32 = make_walkers(mol, n, B).astype(np.float32)
    it = Interp(eng.program, mol.charges, geom.F32_EPS)
    ref = it.run(r32.astype(np.float64), mol.coords.astype(np.float32).astype(np.float64), laplacian=True)
    e, stats = eng.local_energy(torch.as_tensor(r32))
    assert np.all(np.isfinite(e.numpy()))
    print(f'N={n}: float32 E_loc rel err {np.abs(e.numpy() / ref["e_loc"] - 1).max():.2e}')
    sign, logpsi = eng.wf_eval(torch.as_tensor(r32))
    np.testing.assert_array_equal(sign.numpy(), ref['sign'])
    check_f32_pass_alone(eng, it, spec, r32, ref, 'cpu')


@pytest.mark.parametrize('n', [36, 43])
def test_emu_f32_value_path_first_unit_on_the_bf16_pipe(n):
    """float32 wf_eval through the fused value kernel at 36 and 43 electrons (one walker per tile: the node layers have fewer
    row blocks than the workgroup has waves, so a wave's first unit is a bf16-pipe unit): signs equal to the float64
    interpreter's for every walker, and log|psi| within 50 cond(A) eps_f32 of it (the constant of
    test_gpu_parity.py::test_f32_local_energy; with the first weight group of such a unit read as three copies of its first
    bf16 plane the error was 8 .. 21 and half the signs were wrong); the staged path (option fused 0) agrees."""
    Bv = 4
    spec, mol, h, tree, eng = setup('ferminet', n, torch.float32, 'cpu', emu_lib())
    r32 = make_walkers(mol, n, Bv).astype(np.float32)
    it = Interp(eng.program, mol.charges, geom.F32_EPS)
    ref = it.run(r32.astype(np.float64), mol.coords.astype(np.float32).astype(np.float64), laplacian=False)
    A = it.bufs[eng.program.buf_names['orbitals']][:, :, 0, :n * n].reshape(Bv, spec.n_determinants, n, n)
    bound = 50 * np.linalg.cond(A).max(1) * 1.2e-7
    for fused in (1, 0):
        eng.set_option('fused', fused)
        sign, logpsi = eng.wf_eval(torch.as_tensor(r32))
        err = np.abs(logpsi.numpy() - ref['log'])
        print(f'N={n} fused={fused}: log|psi| err {err.max():.2e}, bound {bound.min():.2e}')
        np.testing.assert_array_equal(sign.numpy(), ref['sign'])
        assert np.all(err < bound), (err, bound)
