"""Parity tests proper: the HIP path on a real MI355X, through the C ABI, against the oracle.

Oracle = NumPy forward-Laplacian interpreter (oracle/program_interp.py, itself checked against
torch autograd in tests/test_program_interp.py) and the torch Metropolis restatement
(oracle/sampling.py).  Tolerances: float64 build 1e-9 (arithmetic reordering only); float32
build -- the reference's production dtype -- 1e-5 relative on E_loc in the median and 1e-4 at
the 99th percentile (north star: "within 1e-5 Ha relative"; f32 round-off of the O(10^2)
Laplacian/|grad|^2 cancellation sets the tail).  psi signs, accept bits and ages: bit-exact.
"""
import json
import os

import numpy as np
import pytest
import torch

from deepqmc_amd.engine import Engine
from deepqmc_amd.hamil import MolecularHamiltonian
from deepqmc_amd.molecule import Molecule
from deepqmc_amd.params import init_params
from deepqmc_amd.sampling import synthetic_walkers
from deepqmc_amd.spec import ferminet, paulinet, psiformer, transpsiformer
from oracle import geom, sampling as osamp
from oracle import wf as owf
from oracle.program_interp import Interp

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gpurun_out')


def setup(spec_fn, molname, dtype, seed=5):
    mol = Molecule.from_name(molname)
    spec = spec_fn(mol.charges) if spec_fn is transpsiformer else spec_fn()
    h = MolecularHamiltonian(mol=mol)
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=seed, perturb_envelopes=0.1)
    eng = Engine(spec, h, tree, dtype=dtype, device=DEV, norm_eps=geom.F32_EPS)
    it = Interp(eng.program, mol.charges, geom.F32_EPS)
    return spec, mol, h, tree, eng, it


def report(name, payload):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, 'parity_report.json')
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[name] = payload
    json.dump(data, open(path, 'w'), indent=1)


@pytest.mark.parametrize('spec_fn,molname,B', [(paulinet, 'LiH', 8), (ferminet, 'LiH', 5), (paulinet, 'Be', 4), (ferminet, 'N2', 3),
                                               (paulinet, 'H2', 5), (paulinet, 'C', 3),
                                               (psiformer, 'LiH', 4), (psiformer, 'N2', 2), (transpsiformer, 'LiH', 4),
                                               (transpsiformer, 'cyclobutadiene_square', 1)])
def test_f64_every_buffer(spec_fn, molname, B):
    spec, mol, h, tree, eng, it = setup(spec_fn, molname, torch.float64)
    r = synthetic_walkers(h, B, seed=3)
    ref = it.run(r, mol.coords, laplacian=True)
    from buffers_util import check_every_buffer
    (e, stats, grad), worst = check_every_buffer(eng, it, B, lambda: eng.local_energy(torch.as_tensor(r, device=DEV), return_grad=True))
    np.testing.assert_array_equal(eng.debug_read('sign_k', B), it.sign_k)
    np.testing.assert_allclose(eng.debug_read('logdet', B), it.logdet, rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(e.cpu().numpy(), ref['e_loc'], rtol=1e-9, atol=1e-8)
    np.testing.assert_allclose(grad.cpu().numpy(), ref['grad'], rtol=1e-9, atol=1e-9)
    for k, key in enumerate(['hamil/V_el', 'hamil/E_kin', 'hamil/V_loc', 'hamil/V_nl', 'hamil/lap', 'hamil/quantum_force']):
        np.testing.assert_allclose(stats[key].cpu().numpy(), ref['stats'][k], rtol=1e-9, atol=1e-8)
    val = it.run(r, mol.coords, laplacian=False)
    sign, logpsi = eng.wf_eval(torch.as_tensor(r, device=DEV))
    np.testing.assert_array_equal(sign.cpu().numpy(), val['sign'])
    np.testing.assert_allclose(logpsi.cpu().numpy(), val['log'], rtol=1e-11, atol=1e-11)
    report(f'f64_buffers_{spec.name}_{molname}', {'max_abs_err': max(worst.values())})


@pytest.mark.parametrize('spec_fn,molname,B', [(paulinet, 'LiH', 256), (ferminet, 'N2', 16), (psiformer, 'LiH', 32),
                                               (transpsiformer, 'LiH', 32), (transpsiformer, 'cyclobutadiene_square', 3)])
def test_f32_local_energy(spec_fn, molname, B, lih_walker):
    spec, mol, h, tree, eng, it = setup(spec_fn, molname, torch.float32)
    r = synthetic_walkers(h, B, seed=11).astype(np.float32)
    if molname == 'LiH':
        r[0] = lih_walker.astype(np.float32)     # the reference's canonical (near-coalescence) test walker
    ref = it.run(r.astype(np.float64), mol.coords.astype(np.float32).astype(np.float64), laplacian=True)
    e, stats, grad = eng.local_energy(torch.as_tensor(r, device=DEV), return_grad=True)
    sign, logpsi = eng.wf_eval(torch.as_tensor(r, device=DEV))
    np.testing.assert_array_equal(sign.cpu().numpy(), ref['sign'])       # bit-exact item
    rel = np.abs(e.cpu().numpy() - ref['e_loc']) / np.maximum(1.0, np.abs(ref['e_loc']))
    lp = np.abs(logpsi.cpu().numpy() - ref['log'])
    # conditioning of the Slater matrices: f32 round-off of the orbitals is amplified by cond(A)
    N, K = h.n_elec, spec.n_determinants
    A = it.bufs[eng.program.buf_names['orbitals']][:, :, 0, :N * N].reshape(B, K, N, N)
    cond = np.linalg.cond(A).max(1)
    well = cond < 1e3
    report(f'f32_eloc_{spec.name}_{molname}', {
        'B': B, 'rel_err_median': float(np.median(rel)), 'rel_err_p90': float(np.quantile(rel, 0.9)),
        'rel_err_p99': float(np.quantile(rel, 0.99)), 'rel_err_max': float(rel.max()),
        'logpsi_abs_err_median': float(np.median(lp)), 'logpsi_abs_err_max': float(lp.max()),
        'cond_median': float(np.median(cond)), 'cond_max': float(cond.max()), 'n_well_conditioned': int(well.sum()),
        'rel_err_max_well_conditioned': float(rel[well].max()) if well.any() else None,
        'err_over_cond_eps_max': float((rel / (cond * 1.2e-7)).max())})
    assert np.all(np.isfinite(rel))
    # north-star tolerance for the bulk of the walkers; where the random-init Slater matrices are ill conditioned
    # (C4H4: cond ~ 1e6) the f32 round-off of the orbitals is amplified by cond(A) in ANY implementation, so the
    # bound there is relative to cond * eps_f32
    assert np.median(rel) < 1e-5 or np.median(rel / (cond * 1.2e-7)) < 1.0
    if np.median(cond) < 1e4:                         # (N2/FermiNet at random init: median cond ~ 1e5)
        assert np.quantile(rel, 0.9) < 1e-4
    # outliers are ill-conditioned determinants of the random-init ansatz: error <= C * cond * eps_f32
    assert (rel / (cond * 1.2e-7)).max() < 50.0
    assert np.median(lp) < (1e-5 if np.median(cond) < 1e4 else 1e-3)


def test_golden_local_potential(kats, lih_walker):
    """Reference golden (tests/test_potential, LiH, ecp None): V_loc = -93.0144804569 at the
    canonical walker, through the HIP path's hamil/V_loc stat."""
    spec, mol, h, tree, eng, it = setup(paulinet, 'LiH', torch.float64)
    e, stats = eng.local_energy(torch.as_tensor(lih_walker[None], device=DEV))
    np.testing.assert_allclose(float(stats['hamil/V_loc'][0]), float(kats['lih_potential_local_potential']), rtol=1e-7)


def test_metropolis_bit_exact_f64():
    """Same noise in, same accept bits / ages / positions out (float64 build)."""
    spec, mol, h, tree, eng, it = setup(paulinet, 'LiH', torch.float64)
    B, n_sub = 64, 6
    rng = np.random.default_rng(0)
    r0 = synthetic_walkers(h, B, seed=2)
    noise = rng.standard_normal((n_sub, B, h.n_elec, 3))
    unif = rng.random((n_sub, B))
    sign0, log0 = eng.wf_eval(torch.as_tensor(r0, device=DEV))
    st = {'r': torch.as_tensor(r0, device=DEV).clone(), 'log': log0.clone(), 'sign': sign0.clone(),
          'age': torch.zeros(B, dtype=torch.int32, device=DEV), 'tau': torch.full((1,), 0.3, dtype=torch.float64, device=DEV)}
    stats, acc = eng.mcmc_steps(st, n_sub, max_age=3, target_acceptance=0.57, noise=noise, unif=unif, return_accept=True)
    p = owf.to_torch(tree)
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    ost = {'r': T(r0), 'sign': T(sign0.cpu().numpy()), 'log': T(log0.cpu().numpy()),
           'age': torch.zeros(B, dtype=torch.int64), 'tau': 0.3}
    ost, ostats, oacc = osamp.decorr_sample(p, spec, ost, T(mol.coords), h.n_up, geom.F32_EPS, T(noise), T(unif),
                                            max_age=3, target_acceptance=0.57)
    np.testing.assert_array_equal(acc.cpu().numpy().astype(bool), oacc.numpy())
    np.testing.assert_array_equal(st['age'].cpu().numpy(), ost['age'].numpy())
    np.testing.assert_allclose(st['r'].cpu().numpy(), ost['r'].numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(float(st['tau'][0]), ost['tau'], rtol=1e-12)
    for k in ostats:
        np.testing.assert_allclose(stats[k], ostats[k], rtol=1e-9, atol=1e-9, err_msg=k)


def test_device_rng_and_sampler_f32():
    """Device Philox noise: N(0,1)/U[0,1) moments, acceptance in range, psi stays consistent."""
    spec, mol, h, tree, eng, it = setup(paulinet, 'LiH', torch.float32)
    B = 4096
    r0 = synthetic_walkers(h, B, seed=2).astype(np.float32)
    sign0, log0 = eng.wf_eval(torch.as_tensor(r0, device=DEV))
    st = {'r': torch.as_tensor(r0, device=DEV).clone(), 'log': log0.clone(), 'sign': sign0.clone(),
          'age': torch.zeros(B, dtype=torch.int32, device=DEV), 'tau': torch.full((1,), 0.2, dtype=torch.float32, device=DEV)}
    stats = eng.mcmc_steps(st, 10, seed=123)
    assert 0.05 < stats['sampling/acceptance'] < 0.99
    s2, l2 = eng.wf_eval(st['r'])
    np.testing.assert_array_equal(s2.cpu().numpy(), st['sign'].cpu().numpy())
    np.testing.assert_allclose(l2.cpu().numpy(), st['log'].cpu().numpy(), rtol=1e-5, atol=1e-5)
    moved = (st['r'].cpu().numpy() - r0).reshape(B, -1)
    assert np.abs(moved).max() > 0


def test_bf16_pipe_sub_steps_against_f32_mfma_and_float64():
    """The Metropolis hot loop at BASELINE size with its float32 layers on the bf16 matrix pipe (option 'fused_bf' 1, the
    default: three-piece split, six bf16 MFMAs per block) and with v_mfma_f32_16x16x4_f32 (0): log|psi| of 4096 walkers
    against the float64 engine must be in the same accuracy class (median, 99th percentile), signs bit-exact for every walker
    whose float64 |psi| is not at a node, and a sampler run from the same state and noise must agree in its accept
    decisions except where the float32 ratio sits within round-off of the uniform number."""
    spec, mol, h, tree, eng, it = setup(paulinet, 'LiH', torch.float32)
    e64 = Engine(spec, h, tree, dtype=torch.float64, device=DEV, norm_eps=geom.F32_EPS)
    B = 4096
    r0 = synthetic_walkers(h, B, seed=11).astype(np.float32)
    s64, l64 = e64.wf_eval(torch.as_tensor(r0.astype(np.float64), device=DEV))
    l64 = l64.cpu().numpy()
    err, acc = {}, {}
    gen = torch.Generator(device='cpu').manual_seed(5)
    noise = torch.randn(6, B, h.n_elec, 3, generator=gen).to(DEV)
    unif = torch.rand(6, B, generator=gen).to(DEV)
    try:
        for bf in (0, 1):
            eng.set_option('fused_bf', bf)
            s, l = eng.wf_eval(torch.as_tensor(r0, device=DEV))
            np.testing.assert_array_equal(s.cpu().numpy(), s64.cpu().numpy())
            err[bf] = np.abs(l.cpu().numpy().astype(np.float64) - l64)
            st = {'r': torch.as_tensor(r0, device=DEV).clone(), 'log': l.clone(), 'sign': s.clone(),
                  'age': torch.zeros(B, dtype=torch.int32, device=DEV), 'tau': torch.full((1,), 0.2, dtype=torch.float32, device=DEV)}
            out = eng.mcmc_steps(st, 6, seed=3, noise=noise, unif=unif, return_accept=True, target_acceptance=None)
            acc[bf] = out[1].cpu().numpy() if isinstance(out, tuple) else None
    finally:
        eng.set_option('fused_bf', 1)
    assert np.median(err[0]) < 5e-6 and np.median(err[1]) < 3 * np.median(err[0]) + 2e-7, (np.median(err[0]), np.median(err[1]))
    assert np.quantile(err[1], 0.99) < 3 * np.quantile(err[0], 0.99) + 1e-5, (np.quantile(err[0], 0.99), np.quantile(err[1], 0.99))
    if acc[0] is not None:
        # the first sub-step starts from identical state: its decisions differ only for ratios within float32 round-off of u
        assert (acc[0][0] != acc[1][0]).mean() < 2e-3


def test_captured_pass_replays_bit_exactly():
    """Option 'pass_graph' (default 1): the forward-Laplacian pass of a batch size is launched eagerly once, captured into a
    hipGraph on its second call and replayed afterwards -- the float32 pass and the float64 twin's pass over the flagged
    walkers (count rounded up to a multiple of 64, the surplus rows not written back).  Every call must give bit-identical
    local energies to the eager launches ('pass_graph' 0), for the same walkers and for walkers that change between calls,
    and the count of refined walkers must be the flagged count, not the padded one."""
    spec, mol, h, tree, eng, it = setup(paulinet, 'LiH', torch.float32)
    B = 1536
    rs = [torch.as_tensor(synthetic_walkers(h, B, seed=20 + k).astype(np.float32), device=DEV) for k in range(3)]
    seq = [0, 0, 0, 1, 2, 1, 0, 2]
    out = {}
    for mode in (0, 1):
        eng.set_option('pass_graph', mode)
        eng.set_option('refine_probe', 0)              # (fixed threshold: both runs flag the same walkers)
        res, ref = [], []
        for k in seq:
            e, _ = eng.local_energy(rs[k])
            res.append(e.clone()); ref.append(eng.last_refined())
        out[mode] = (res, ref)
    eng.set_option('pass_graph', 1)
    for a, b in zip(out[0][0], out[1][0]):
        assert torch.equal(a, b)
    assert out[0][1] == out[1][1] and min(out[1][1]) > 0 and max(out[1][1]) < B // 2
    for k, e in zip(seq, out[1][0]):                   # the same walkers give the same energies whenever they come back
        assert torch.equal(e, out[1][0][seq.index(k)])


def test_workspace_growth_keeps_answers_and_graphs():
    """A context whose workspace, flag list and score buffer grow between calls (64 -> 128 walkers) and are then used below
    their capacity (64 again): every local energy equals that of a fresh context which only ever saw that batch size, and
    the last call is a graph replay.  64 walkers is the smallest batch the graph path accepts."""
    spec, mol, h, tree, eng, it = setup(paulinet, 'LiH', torch.float32)
    eng.set_option('refine_probe', 0)                  # (fixed threshold: every context flags the same walkers)
    rs = {B: torch.as_tensor(synthetic_walkers(h, B, seed=30 + B).astype(np.float32), device=DEV) for B in (64, 128)}
    want = {}
    for B, r in rs.items():
        fresh = setup(paulinet, 'LiH', torch.float32)[4]
        fresh.set_option('refine_probe', 0)
        want[B] = fresh.local_energy(r)[0].clone()
        fresh.close()
    replays = 0
    for B in (64, 128, 64):
        for _ in range(3):
            replays = eng.graph_counters()['replays']
            e, _ = eng.local_energy(rs[B])
            assert torch.equal(e, want[B]), B
    assert eng.graph_counters()['replays'] > replays


def test_full_size_properties():
    """BASELINE size (4096 walkers): determinism, batch-split invariance, and fermionic
    antisymmetry (swapping two same-spin electrons flips the sign, keeps log|psi| and E_loc)."""
    spec, mol, h, tree, eng, it = setup(paulinet, 'LiH', torch.float32)
    B = 4096
    r = torch.as_tensor(synthetic_walkers(h, B, seed=9).astype(np.float32), device=DEV)
    e1, _ = eng.local_energy(r)
    e2, _ = eng.local_energy(r)
    assert torch.equal(e1, e2)
    ea, _ = eng.local_energy(r[:1000].contiguous())
    eb, _ = eng.local_energy(r[1000:].contiguous())
    assert torch.equal(torch.cat([ea, eb]), e1)
    perm = [1, 0, 2, 3]                      # swap the two spin-up electrons
    rs = r[:, perm].contiguous()
    s1, l1 = eng.wf_eval(r)
    s2, l2 = eng.wf_eval(rs)
    assert torch.equal(s1, -s2)
    dl = (l1 - l2).abs().cpu().numpy()               # f32: outliers are ill-conditioned determinants
    assert np.median(dl) < 1e-5 and np.quantile(dl, 0.99) < 1e-3
    es, _ = eng.local_energy(rs)
    rel = (es - e1).abs() / e1.abs().clamp(min=1.0)
    assert float(rel.median()) < 1e-5
    rec = eng.energy_record(e1)
    x = e1.double().cpu().numpy()
    np.testing.assert_allclose(rec, [B, B, x.sum(), x.sum(), ((x - x.mean()) ** 2).sum(), x.min(), x.max()], rtol=1e-9)
    merged = eng.merge_energy_records(np.stack([eng.energy_record(e1[:1024].contiguous()), eng.energy_record(e1[1024:].contiguous())]))
    np.testing.assert_allclose(merged['local_energy/mean'], x.mean(), rtol=1e-10)
    np.testing.assert_allclose(merged['local_energy/std'], x.std(), rtol=1e-9)


ECP_TABLES = {     # synthetic coefficients in pyscf's ECP format (pyscf's tables are not available offline)
    'Li': [0, [[-1, [[], [[5.4104, 1.0]], [[4.6015, -4.6015]], [[2.7052, 5.4104]]]],
               [0, [[], [], [[1.3302, 6.7529], [0.9, -0.8]]]],
               [1, [[], [], [[1.25, 0.45]]]]]],
}


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_ecp_local_energy(dtype):
    """Gaussian-type ECP on Li (local r^-1/r^0/r^1 terms + s and p non-local channels): V_loc, V_nl and E_loc
    from the HIP path (12 N value-only psi evaluations per walker through the fused kernel) against
    oracle/ecp.py on the same walkers and rotation angles; then the Philox-keyed rotation path."""
    from oracle import ecp as oecp, physics
    spec = paulinet()
    mol = Molecule.from_name('LiH')
    h = MolecularHamiltonian(mol=mol, ecp_type='synthetic', ecp_tables=ECP_TABLES)
    tree = init_params(spec, h.n_up, h.n_down, h.n_nuc, seed=5, perturb_envelopes=0.1)
    eng = Engine(spec, h, tree, dtype=dtype, device=DEV, norm_eps=geom.F32_EPS)
    B, N = 6, h.n_elec
    r = synthetic_walkers(h, B, seed=3)
    phi = np.random.default_rng(1).uniform(0, np.pi / 5, (B, 1, N))
    e, stats = eng.local_energy(torch.as_tensor(r, dtype=dtype, device=DEV), ecp_phi=torch.as_tensor(phi, dtype=dtype, device=DEV))
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    R, p, zv = T(mol.coords), owf.to_torch(tree), T(h.ns_valence)
    rt = T(r)
    e_ref, st_ref, _ = physics.batch_local_energy(p, spec, rt, R, zv, h.n_up, geom.F32_EPS)
    psi = lambda rr: physics.batch_wave_function(p, spec, rr, R, h.n_up, geom.F32_EPS)
    tol = 1e-9 if dtype == torch.float64 else 2e-4
    worst = 0.0
    for b in range(B):
        v_loc = float(oecp.local_potential(rt[b], R, zv, T(h.pot.loc_params), h.ecp_mask))
        v_nl = float(oecp.nonloc_potential(rt[b], R, T(h.pot.nl_params), psi, T(phi[b])))
        np.testing.assert_allclose(float(stats['hamil/V_loc'][b]), v_loc, rtol=10 * tol)
        np.testing.assert_allclose(float(stats['hamil/V_nl'][b]), v_nl, rtol=50 * tol, atol=10 * tol)
        e_b = float(e_ref[b]) - float(st_ref['hamil/V_loc'][b]) + v_loc + v_nl
        worst = max(worst, abs(float(e[b]) - e_b) / max(1.0, abs(e_b)))
    assert worst < (1e-8 if dtype == torch.float64 else 5e-4), worst
    # device-drawn rotations: finite, reproducible per seed, different across seeds, chunking-invariant
    rd = torch.as_tensor(synthetic_walkers(h, 64, seed=9), dtype=dtype, device=DEV)
    e1, s1 = eng.local_energy(rd, rng=11)
    e2, s2 = eng.local_energy(rd, rng=11)
    e3, s3 = eng.local_energy(rd, rng=12)
    assert torch.isfinite(s1['hamil/V_nl']).all() and torch.equal(s1['hamil/V_nl'], s2['hamil/V_nl'])
    assert not torch.equal(s1['hamil/V_nl'], s3['hamil/V_nl'])
    eng.set_option('ecp_max_cfg', 7 * N * 12)          # 7 walkers per quadrature batch -> 10 chunks
    e4, s4 = eng.local_energy(rd, rng=11)
    assert torch.equal(s4['hamil/V_nl'], s1['hamil/V_nl']) and torch.equal(e4, e1)
    report(f'ecp_{"f64" if dtype == torch.float64 else "f32"}', {'worst_rel_eloc': worst})


@pytest.mark.parametrize('spec_fn,molname', [(transpsiformer, 'cyclobutadiene_square'), (psiformer, 'benzene')])
def test_attention_mfma_vs_scalar_f32(spec_fn, molname):
    """The MFMA attention kernel (f32, N > 16; kernel_attention_mfma.hip) against the scalar attention kernel on
    the first layer's attention output (identical inputs: every lane incl. the Laplacian lane, 28 / 42 electrons,
    with and without nuclear-token keys) and on log|psi| of the whole ansatz."""
    spec, mol, h, tree, eng, it = setup(spec_fn, molname, torch.float32)
    B = 2
    r = torch.as_tensor(synthetic_walkers(h, B, seed=4).astype(np.float32), device=DEV)
    eng.set_option('fused', 0)
    res = {}
    for flag in (2, 0):
        eng.set_option('attention_mfma', flag)
        e, _ = eng.local_energy(r)
        att = eng.debug_read('l0/att', B)
        sign, logpsi = eng.wf_eval(r)
        res[flag] = (att, logpsi.cpu().numpy(), sign.cpu().numpy(), e.cpu().numpy())
    a, b = res[2][0], res[0][0]
    scale = np.abs(b).max(axis=(0, 1, 3), keepdims=True) + 1e-30          # per lane: derivative lanes have their own magnitude
    err = float((np.abs(a - b) / scale).max())
    assert np.isfinite(a).all() and err < 2e-5, err
    np.testing.assert_array_equal(res[2][2], res[0][2])
    np.testing.assert_allclose(res[2][1], res[0][1], rtol=5e-5, atol=2e-4)     # f32 round-off through 4 layers + 42x42 determinants
    report(f'attention_mfma_{molname}', {'l0_att_max_rel_err_per_lane': err,
                                         'logpsi_max_abs_diff': float(np.abs(res[2][1] - res[0][1]).max())})


