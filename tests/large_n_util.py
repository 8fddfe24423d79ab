"""Systems and shared checks of the large-N tests (tests/test_large_n_emu.py, tests/test_gpu_large_n.py): molecules whose
electron counts need the lane counts and determinant kernels beyond the benchmark systems' -- 80 / 112 / 144 lanes (22, 32, 43
electrons), 3 x 3 tiles past the old cap (45), the first 4 x 4 size with one row in the last tile (49), full tiles and 208
lanes (64), and the first size that is refused (65)."""
import dataclasses

import numpy as np
import torch

from deepqmc_amd.engine import Engine
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.params import init_params
from deepqmc_amd.spec import ferminet, psiformer
from oracle import geom
from oracle.program_interp import Interp
from test_program_interp import make_walkers


def ring(z, n, bond=2.6):
    """n nuclei of charge z on a regular polygon, neighbours `bond` bohr apart."""
    rad = bond / (2 * np.sin(np.pi / n))
    phi = 2 * np.pi * np.arange(n) / n
    return np.stack([rad * np.cos(phi), rad * np.sin(phi), np.zeros(n)], 1), [z] * n


def line(charges, bond):
    n = len(charges)
    return np.stack([np.zeros(n), np.zeros(n), bond * (np.arange(n) - (n - 1) / 2)], 1), list(charges)


# N: (coords, charges), spin
SYSTEMS = {
    22: (line([8, 6, 8], 2.2), 0),          # CO2-like: 80 lanes
    32: (line([16, 16], 3.6), 0),           # S2-like: 112 lanes
    36: (ring(6, 6), 0),                    # C6 ring: 112 lanes, the upper end
    43: (line([15, 14, 14], 3.8), 1),       # 144 lanes, below the old determinant cap
    45: (ring(9, 5), 1),                    # F5 ring, 23 up / 22 down: first past the old cap, 3 x 3 tiles, odd
    49: (ring(7, 7), 1),                    # N7 ring, 25 / 24: first 4 x 4 size, one row in the last tile
    64: (ring(8, 8), 0),                    # O8 ring, 32 / 32: full tiles, 208 lanes
    65: ((np.concatenate([ring(8, 8)[0], [[0.0, 0.0, 2.0]]]), [8] * 8 + [1]), 1),    # refused
}


def molecule(n):
    (coords, charges), spin = SYSTEMS[n]
    return Molecule(coords=coords, charges=charges, charge=0, spin=spin)


def narrow_spec(name):
    if name == 'ferminet':
        return dataclasses.replace(ferminet(), embedding_dim=16, n_interactions=1, n_determinants=2)
    return dataclasses.replace(psiformer(), embedding_dim=32, n_interactions=1, n_determinants=2)


def setup(name, n, dtype, device, lib=None):
    mol = molecule(n)
    spec = narrow_spec(name)
    h = MolecularHamiltonian(mol=mol)
    assert h.n_elec == n
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=3, perturb_envelopes=0.3)
    eng = Engine(spec, h, tree, dtype=dtype, device=device, lib=lib, norm_eps=geom.F32_EPS)
    return spec, mol, h, tree, eng


def interp_reference(eng, mol, r, cache={}):
    """Interpreter results (Laplacian mode and value-only) for the engine's program on the float64 walkers r of make_walkers,
    computed once per (spec, weights, walkers) and left unchanged."""
    key = (repr(eng.spec), r.shape, hash(np.ascontiguousarray(r).tobytes()), hash(eng.program.weights.tobytes()))
    if key not in cache:
        it = Interp(eng.program, mol.charges, geom.F32_EPS)
        ref = it.run(r, mol.coords, laplacian=True)
        logdet, sign_k = it.logdet.copy(), it.sign_k.copy()
        val = it.run(r, mol.coords, laplacian=False)
        cache[key] = (ref, logdet, sign_k, val, it.logdet.copy(), it.sign_k.copy())
    return cache[key]


def check_f64(eng, mol, r, device, options=(None,)):
    """The float64 assertions of tests/test_gpu_parity.py::test_f64_every_buffer on every walker: sign_k exact, logdet lanes
    1e-8, E_loc rtol 1e-9 / atol 1e-8, gradient 1e-9, log|psi| 1e-11 -- once per value of option slogdet_mfma."""
    B = r.shape[0]
    ref, logdet, sign_k, val, _, _ = interp_reference(eng, mol, r)
    rt = torch.as_tensor(r, device=device)
    out = {}
    for opt in options:
        if opt is not None:
            eng.set_option('slogdet_mfma', opt)
        e, stats, grad = eng.local_energy(rt, return_grad=True)
        got_ld = eng.debug_read('logdet', B)
        print(f'N={r.shape[1]} {eng.spec.name} slogdet_mfma={opt}: E_loc rel {np.abs(e.cpu().numpy() / ref["e_loc"] - 1).max():.2e}, '
              f'logdet lanes abs {np.abs(got_ld - logdet).max():.2e}, grad abs {np.abs(grad.cpu().numpy() - ref["grad"]).max():.2e}')
        np.testing.assert_array_equal(eng.debug_read('sign_k', B), sign_k)
        np.testing.assert_allclose(got_ld, logdet, rtol=1e-8, atol=1e-8)
        np.testing.assert_allclose(e.cpu().numpy(), ref['e_loc'], rtol=1e-9, atol=1e-8)
        np.testing.assert_allclose(grad.cpu().numpy(), ref['grad'], rtol=1e-9, atol=1e-9)
        for k, key in enumerate(['hamil/V_el', 'hamil/E_kin', 'hamil/V_loc', 'hamil/V_nl', 'hamil/lap', 'hamil/quantum_force']):
            np.testing.assert_allclose(stats[key].cpu().numpy(), ref['stats'][k], rtol=1e-9, atol=1e-8)
        out[opt] = (e.cpu().numpy(), got_ld)
    if options != (None,):
        eng.set_option('slogdet_mfma', 1)
    sign, logpsi = eng.wf_eval(rt)
    np.testing.assert_array_equal(sign.cpu().numpy(), val['sign'])
    np.testing.assert_allclose(logpsi.cpu().numpy(), val['log'], rtol=1e-11, atol=1e-11)
    return out


def check_f32_pass_alone(eng, it, spec, r32, ref, device):
    """At these batch sizes a float32 context at defaults hands every walker to its float64 twin, so E_loc at defaults says
    nothing about the float32 tiles.  With option refine 0 the float32 pass answers alone: every E_loc finite and within
    50 cond(A) eps_f32 of the float64 interpreter, relative to max(1, |E_loc|) -- the outlier bound of
    tests/test_gpu_parity.py::test_f32_local_energy, applied to every walker."""
    B, n = r32.shape[0], r32.shape[1]
    eng.set_option('refine', 0)
    e, _ = eng.local_energy(torch.as_tensor(r32, device=device))
    eng.set_option('refine', 1)
    A = it.bufs[eng.program.buf_names['orbitals']][:, :, 0, :n * n].reshape(B, spec.n_determinants, n, n)
    cond = np.linalg.cond(A).max(1)
    rel = np.abs(e.cpu().numpy() - ref['e_loc']) / np.maximum(1.0, np.abs(ref['e_loc']))
    print(f'N={n}: float32 pass alone (refine 0): rel err median {np.median(rel):.2e} max {rel.max():.2e}, '
          f'over cond eps max {(rel / (cond * 1.2e-7)).max():.2e}')
    assert np.all(np.isfinite(rel))
    assert (rel / (cond * 1.2e-7)).max() < 50.0
    return rel


def check_vjp_and_coords(eng, spec, h, tree, r, device, tol=1e-9):
    """log_psi_vjp against torch.autograd of the oracle (largest deviation of every leaf relative to the leaf's norm) and
    log_psi_grad_coords against autograd with respect to r and R (normwise per walker), both below tol."""
    from force_util import oracle_grad_coords, walker_errors
    from param_grad_util import leaf_errors, oracle_vjp
    B = r.shape[0]
    cot = np.random.default_rng(3).normal(size=B)
    rt = torch.as_tensor(r, device=device)
    _, _, g = eng.log_psi_vjp(rt, torch.as_tensor(cot, device=device))
    err = leaf_errors(eng.program.unflatten_grad(g), oracle_vjp(spec, h, tree, r, cot, geom.F32_EPS))
    worst = max(err, key=err.get)
    sign, log, gr, gR = eng.log_psi_grad_coords(rt)
    ref_r, ref_R = oracle_grad_coords(spec, h, tree, r, geom.F32_EPS)
    er, eR = walker_errors(gr.cpu().numpy(), ref_r), walker_errors(gR.cpu().numpy(), ref_R)
    print(f'N={r.shape[1]}: vjp worst leaf {worst} {err[worst]:.2e}, d/dr {er.max():.2e}, d/dR {eR.max():.2e}')
    assert err[worst] < tol, (worst, err[worst])
    assert er.max() < tol and eR.max() < tol, (er.max(), eR.max())


__all__ = ['SYSTEMS', 'molecule', 'narrow_spec', 'setup', 'check_f64', 'check_vjp_and_coords', 'interp_reference', 'make_walkers']
