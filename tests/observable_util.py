"""Checks of the observable monitors (deepqmc_amd/observable.py), the oscillator strengths (dqmc_oscillator_strength), the
finite-difference force (dqmc_fd_displace, dqmc_fd_force, force.evaluate_finite_difference_force) and fit_wf's
`observable_monitors`, shared by the emulated CPU tests and the GPU tests.

The expected values of the three entry points are NumPy float64 transcriptions of the formulas in include/dqmc.h (reference
observable.py:556-605 and force.py:550-606), written here."""
import numpy as np
import pytest
import torch

from deepqmc_amd import observable as obs
from deepqmc_amd import ecp_force, force
from deepqmc_amd.fit import TrainState, fit_wf
from deepqmc_amd.loss import create_loss_fn
from deepqmc_amd.optimizer import AdamOptimizer
from deepqmc_amd.physics import evaluate_spin
from deepqmc_amd.sampling import MoleculeIdxSampler
from deepqmc_amd.types import PhysicalConfiguration, Psi
from loss_util import lih
from optimizer_util import training_setup
from oracle import geom
from oracle.program_interp import Interp

F64 = torch.float64
EPS = 2.0 ** -52
ALL_NAMES = ('r', 'R', 'psi', 'local_energy', 'psi_ratio', 'spin', 'hf_force_bare', 'hf_force_bare_anti', 'hf_force_ac_zvq',
             'hf_force_ac_zvq_anti', 'hf_force_ac_zvzbq', 'hf_force_ac_zb', 'hf_force_ac_zvqzb', 'finite_difference_force',
             'oscillator_strength')
OS_SHAPES = [(S, B) for S in (2, 3) for B in (1, 2, 63, 64, 65, 300)]


# ---------------------------------------------------------------- 1. oscillator strengths
def ref_oscillator_strength(r, ratio, e):
    """observable.py:556-605 in NumPy float64, one process: r [S, B, N, 3], ratio [S, S, B], e [S, B] ->
    dict(E, std_E, cd_mean, cd_std, cd_err, ex, ds, os_mean, os_err, abs_cd [S, S, 3] = sum_b |cd|, abs_e [S] = sum_b |e|)."""
    r, ratio, e = (np.asarray(x, np.float64) for x in (r, ratio, e))
    B = e.shape[-1]
    d = np.zeros(r.shape[:2] + (3,))
    for n in range(r.shape[2]):                       # (the electrons in ascending order, as the kernel adds them)
        d = d + r[:, :, n]
    d = -d
    cd = d[None] * ratio[..., None]                   # [S, S, B, 3]
    E, std_E = e.mean(-1), e.std(-1)
    err_E = std_E / np.sqrt(float(B))
    ex = E[None, :] - E[:, None]
    ex_err = np.sqrt(err_E[None, :] ** 2 + err_E[:, None] ** 2)
    cd_mean, cd_std = cd.mean(-2), cd.std(-2)
    cd_err = cd_std / np.sqrt(float(B))
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = cd_err / cd_mean
        ds_vec = cd_mean * cd_mean.swapaxes(0, 1)
        ds_err_vec = np.abs(ds_vec) * np.sqrt(rel ** 2 + rel.swapaxes(0, 1) ** 2)
        ds = ds_vec.sum(-1)
        ds_err = np.sqrt((ds_err_vec ** 2).sum(-1))
        os_mean = (2 / 3) * ex * ds
        os_err = (2 / 3) * np.abs(os_mean) * np.sqrt((ex_err / ex) ** 2 + (ds_err / ds) ** 2)
    return dict(E=E, std_E=std_E, cd_mean=cd_mean, cd_std=cd_std, cd_err=cd_err, ex=ex, ds=ds, os_mean=os_mean, os_err=os_err,
                abs_cd=np.abs(cd).sum(-2), abs_e=np.abs(e).sum(-1))


def os_inputs(S, B, dtype, seed, N=4):
    """Walkers, ratios (diagonal: ones) and local energies of S states with distinct mean energies; r and e carry the values of
    `dtype` exactly."""
    g = torch.Generator().manual_seed(seed)
    r = (1.5 * torch.randn(S, B, N, 3, generator=g, dtype=F64)).to(dtype)
    ratio = 0.3 * torch.randn(S, S, B, generator=g, dtype=F64) + 0.2
    for s in range(S):
        ratio[s, s] = 1.0
    e = (-8.0 + 0.3 * torch.arange(S, dtype=F64)[:, None] + 0.2 * torch.randn(S, B, generator=g, dtype=F64)).to(dtype)
    return r, ratio, e


def os_qualifies(ref):
    """The entries whose oscillator strength is well conditioned by its INPUTS: |ds| and |ex| above 1e-3 of their largest entry
    (both are differences / sums that can cancel; where they do not, the moments' errors below carry over to os at ~1e3 x B eps)."""
    S = ref['ex'].shape[0]
    off = ~np.eye(S, dtype=bool)
    return off & (np.abs(ref['ds']) > 1e-3 * np.abs(ref['ds'][off]).max()) & (np.abs(ref['ex']) > 1e-3 * np.abs(ref['ex']).max())


def os_seed(S, B, dtype):
    """The first seed at which every off-diagonal entry qualifies (a property of the inputs alone)."""
    for seed in range(100 * S + B, 100 * S + B + 50):
        r, ratio, e = os_inputs(S, B, dtype, seed)
        if os_qualifies(ref_oscillator_strength(r.numpy(), ratio.numpy(), e.numpy()))[~np.eye(S, dtype=bool)].all():
            return seed
    raise AssertionError('no seed found')


def check_oscillator_strength(eng, S, B):
    """dqmc_oscillator_strength of a context of either dtype against the transcription.

    Moments: a sum of B terms in any fixed order is within (B - 1) u sum|x| of the exact one (u = 2^-53), the products and the
    division add 2 u, and the transcription's own pairwise sum ~ log2(B) u: together below (B + 2) 2^-52 sum_b |x_b|.  The means
    are held to that bound divided by B (what it says about sum / B); the standard deviations, which are below max|x| <= sum|x|
    and relatively good to ~ (B + 3) u, to the bound itself.  B = 1 and the diagonal of the ratios leave no freedom: equal.
    os_mean / os_err: rtol 1e-10 on every off-diagonal entry (all qualify at the seed used; none is skipped); the diagonal is
    os_mean == 0, os_err NaN.  Two calls are bit-equal."""
    seed = os_seed(S, B, eng.dtype)
    r, ratio, e = os_inputs(S, B, eng.dtype, seed)
    ref = ref_oscillator_strength(r.numpy(), ratio.numpy(), e.numpy())
    dev = eng.device
    args = (r.to(dev), ratio.to(dev).contiguous(), e.to(dev))
    out = eng.oscillator_strength(*args)
    E, std_E, cd_std = eng.oscillator_moments(S)
    out2 = eng.oscillator_strength(*args)
    for a, b in zip(out, out2):
        assert torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all() and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    os_mean, os_err, cd_mean, cd_err = (o.cpu().numpy() for o in out)
    tol_cd, tol_e = (B + 2) * EPS * ref['abs_cd'], (B + 2) * EPS * ref['abs_e']
    dev_ = {'cd_mean': np.abs(cd_mean - ref['cd_mean']) / np.maximum(tol_cd / B, 1e-300), 'cd_std': np.abs(cd_std - ref['cd_std']) / np.maximum(tol_cd, 1e-300),
            'E': np.abs(E - ref['E']) / (tol_e / B), 'std_E': np.abs(std_E - ref['std_E']) / tol_e}
    print(f'S={S} B={B} {eng.dtype} seed {seed}: largest deviation in units of its bound: ' + ', '.join(f'{k} {v.max():.3f}' for k, v in dev_.items()))
    for k, v in dev_.items():
        assert (v <= 1.0).all(), (k, v.max())
    np.testing.assert_array_equal(cd_err, cd_std / np.sqrt(float(B)))
    off = ~np.eye(S, dtype=bool)
    ok = os_qualifies(ref)
    assert ok[off].all(), 'an off-diagonal entry would be skipped'
    rel = lambda a, b: np.abs(a - b)[off] / np.maximum(np.abs(b)[off], 1e-300)
    print(f'    os_mean rel {rel(os_mean, ref["os_mean"]).max():.2e}, os_err rel {rel(os_err, ref["os_err"]).max():.2e}')
    np.testing.assert_allclose(os_mean[off], ref['os_mean'][off], rtol=1e-10, atol=0)
    np.testing.assert_allclose(os_err[off], ref['os_err'][off], rtol=1e-10, atol=0)
    assert (np.diagonal(os_mean) == 0).all() and np.isnan(np.diagonal(os_err)).all()
    assert np.isfinite(os_mean).all() and np.isfinite(os_err[off]).all()


# ---------------------------------------------------------------- 2. / 3. finite-difference force: displacements and quotient
def ref_fd_displace(r, R, h):
    """force.py:584-594 in NumPy float64: r [B, N, 3], R [n_nuc, 3] -> (r_d [D, B, N, 3], R_d [D, n_nuc, 3]), D = 3 n_nuc."""
    r, R = np.asarray(r, np.float64), np.asarray(R, np.float64)
    n_nuc = R.shape[0]
    dist = np.sqrt(((R[None, :, None, :] - r[:, None, :, :]) ** 2).sum(-1))          # [B, n_nuc, N]
    w = np.exp(-dist) / np.exp(-dist).sum(1, keepdims=True)
    r_d, R_d = np.repeat(r[None], 3 * n_nuc, 0), np.repeat(R[None], 3 * n_nuc, 0)
    for n0 in range(n_nuc):
        for j0 in range(3):
            R_d[3 * n0 + j0, n0, j0] -= h
            r_d[3 * n0 + j0, :, :, j0] += h * w[:, n0, :]
    return r_d, R_d


def fd_walkers(eng, B, seed=2):
    """Walkers and a geometry whose values are float32 numbers (so both dtypes see the same inputs), as float64 NumPy arrays."""
    from deepqmc_amd.sampling import synthetic_walkers
    r = synthetic_walkers(eng.hamil, B, seed=seed).astype(np.float32).astype(np.float64)
    R = np.asarray(eng.hamil.mol.coords, np.float64).astype(np.float32).astype(np.float64)
    return r, R


def check_fd_displace(eng64, eng32, B, h=1e-3):
    """float64 context: |r_d - ref| <= 4 x 2^-52 (|r| + h) (w <= 1 is good to a few ulp of exp, sqrt and the division, and enters
    times h; the sum r + h w rounds once), R_d exact.  float32 context on the same inputs: the float64 result rounded once."""
    r, R = fd_walkers(eng64, B)
    ref_r, ref_R = ref_fd_displace(r, R, h)
    r_d, R_d = eng64.fd_displace(torch.as_tensor(r, device=eng64.device), torch.as_tensor(R, device=eng64.device), h)
    D = 3 * R.shape[0]
    assert tuple(r_d.shape) == (D,) + r.shape and tuple(R_d.shape) == (D,) + R.shape and r_d.dtype == F64
    err = np.abs(r_d.cpu().numpy() - ref_r) / (4 * EPS * (np.abs(r)[None] + h))
    print(f'fd_displace n_nuc={R.shape[0]} B={B}: largest |delta r_d| in units of the bound {err.max():.3f}')
    assert (err <= 1.0).all()
    assert float(np.abs(r_d.cpu().numpy() - r[None]).max()) > 0.1 * h        # (it did displace)
    np.testing.assert_array_equal(R_d.cpu().numpy(), ref_R)
    r32, R32 = eng32.fd_displace(torch.as_tensor(r, dtype=torch.float32, device=eng32.device),
                                 torch.as_tensor(R, dtype=torch.float32, device=eng32.device), h)
    assert r32.dtype == torch.float32
    assert torch.equal(r32.cpu(), r_d.cpu().float()) and torch.equal(R32.cpu(), R_d.cpu().float())


def check_fd_force(eng, B, h=1e-3, seed=0):
    """dqmc_fd_force on random inputs against NumPy: rtol 2^-50 (1 + 2 |log_d - log_0|) -- the rounding of the difference of the
    logs enters exp times 2 |delta log|, exp itself, the energy difference, the division and the product an ulp each."""
    D = 3 * eng.hamil.n_nuc
    g = torch.Generator().manual_seed(seed + B)
    log_0, e_0 = 3.0 * torch.randn(B, generator=g, dtype=F64), -8.0 + torch.randn(B, generator=g, dtype=F64)
    log_d, e_d = log_0 + 0.5 * torch.randn(D, B, generator=g, dtype=F64), e_0 + 0.3 * torch.randn(D, B, generator=g, dtype=F64)
    a = [x.to(eng.dtype) for x in (log_d, log_0, e_d, e_0)]
    F = eng.fd_force(*(x.to(eng.device) for x in a), h).cpu().numpy()
    ld, l0, ed, e0 = (x.double().numpy() for x in a)
    ref = (np.exp(2 * (ld - l0)) * ((ed - e0) / h)).T.reshape(B, eng.hamil.n_nuc, 3)
    rtol = (2.0 ** -50 * (1 + 2 * np.abs(ld - l0))).T.reshape(ref.shape)
    err = np.abs(F - ref) / (rtol * np.abs(ref))
    print(f'fd_force B={B} {eng.dtype}: largest deviation in units of the bound {err.max():.3f}')
    assert F.dtype == np.float64 and (err <= 1.0).all()


# ---------------------------------------------------------------- 4. the estimator end to end
def check_finite_difference_force(device, lib, B=8, h=1e-3, d_oracle=4):
    """LiH / small PauliNet, float64: F is fd_force of the engine's own wf_eval / local_energy at the returned (r_d, R_d), bit for
    bit; log_d and e_d of displacement `d_oracle` agree with the forward-Laplacian interpreter at the displaced walkers and
    geometry to rtol = atol = 1e-9, the tolerance of tests/test_kernels_emu.py::test_emu_f64_buffers_and_energy for E_loc."""
    h_, spec = lih()
    wf, params, sampler, st = training_setup(h_, spec, F64, device, lib, 1, B, 3, 3)
    _, pc, _ = sampler.sample(7, st, params, MoleculeIdxSampler(0, 1, 1).sample())
    p, r = params[0], pc.r[0, 0].contiguous()
    pcs = PhysicalConfiguration(pc.R[0], r, None)
    eng = wf.engine(p, pc.R[0])
    e_loc, _ = eng.local_energy(pcs, rng=5)
    f = force.evaluate_finite_difference_force(h_, wf, h)
    F, (r_d, R_d, log_d, e_d) = f(5, p, pcs, e_loc, None, return_parts=True)
    assert tuple(F.shape) == (B, h_.n_nuc, 3) and F.dtype == F64 and torch.isfinite(F).all()
    assert torch.equal(F, f(5, p, pcs, e_loc, float(e_loc.mean())))
    D = 3 * h_.n_nuc
    logs = torch.stack([eng.wf_eval(r_d[d], R_d[d])[1] for d in range(D)])
    es = torch.stack([eng.local_energy(PhysicalConfiguration(R_d[d], r_d[d], None), rng=5)[0] for d in range(D)])
    assert torch.equal(logs, log_d) and torch.equal(es, e_d)
    assert torch.equal(F, eng.fd_force(logs, eng.wf_eval(r, pc.R[0])[1], es, e_loc, h))
    ref = Interp(eng.program, h_.mol.charges, geom.F32_EPS).run(r_d[d_oracle].cpu().numpy(), R_d[d_oracle].cpu().numpy(), laplacian=True)
    np.testing.assert_allclose(log_d[d_oracle].cpu().numpy(), ref['log'], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(e_d[d_oracle].cpu().numpy(), ref['e_loc'], rtol=1e-9, atol=1e-9)
    return F


# ---------------------------------------------------------------- 5. monitors
def monitor_batch(device, lib, S=2, B=8, dtype=F64, small=True, seed=3):
    """(hamil, wf, params, phys_conf [1, S, B, N, 3], psi [1, S, B], e_loc [1, S, B], ratios [1, S, S, B]) of S LiH / PauliNet
    states, from one sampled batch and the value side of the multi-state loss."""
    h, spec = lih(small)
    wf, params, sampler, st = training_setup(h, spec, dtype, device, lib, S, B, 3, seed)
    st, pc, _ = sampler.sample(7, st, params, MoleculeIdxSampler(0, 1, 1).sample())
    nan = torch.full((1, S), float('nan'), dtype=F64, device=pc.r.device)
    v = create_loss_fn(h, wf, alpha=4.0).evaluate(5, params, (pc, None, {'energy_ewm': nan, 'std_ewm': nan}))
    psi = Psi(torch.stack([s['psi'].sign for s in st['elec'][0]])[None], torch.stack([s['psi'].log for s in st['elec'][0]])[None])
    return h, wf, params, pc, psi, v['e_loc'], v['psi_ratio']


def direct_samples(name, hamil, wf, params, pc, e_loc, cutoff=0.3, h=1e-3, rng=11, float_energy=False):
    """[1, S, B, ...] from direct calls of the estimator behind monitor `name`, state by state.  float_energy: the batch energy as a
    host float, the way a caller outside the loop passes it (bit-identical in float64)."""
    ecp = hamil.pot is not None
    mod = ecp_force if ecp else force
    rows = []
    for s in range(pc.r.shape[1]):
        c = PhysicalConfiguration(pc.R[0], pc.r[0, s].contiguous(), None)
        e = e_loc[0, s]
        en = float(e.double().mean()) if float_energy else e.double().mean()
        p = params[s]
        rows.append({
            'spin': lambda: evaluate_spin(hamil, wf)(p, c),
            'hf_force_bare': lambda: mod.evaluate_hf_force_bare(hamil, wf)(rng, p, c),
            'hf_force_bare_anti': lambda: force.antithetic_wrapper(mod.evaluate_hf_force_bare(hamil, wf), wf, cutoff)(rng, p, c),
            'hf_force_ac_zvq': lambda: force.evaluate_hf_force_ac_zvq(hamil, wf)(p, c),
            'hf_force_ac_zvq_anti': lambda: force.antithetic_wrapper(force.evaluate_hf_force_ac_zvq(hamil, wf), wf, cutoff)(rng, p, c),
            'hf_force_ac_zvzbq': lambda: force.evaluate_hf_force_ac_zvzbq(hamil, wf)(p, c, e, en),
            'hf_force_ac_zb': lambda: mod.evaluate_hf_force_ac_zb(hamil, wf)(rng, p, c, e, en),
            'hf_force_ac_zvqzb': lambda: force.evaluate_hf_force_ac_zvqzb(hamil, wf)(p, c, e, en),
            'finite_difference_force': lambda: force.evaluate_finite_difference_force(hamil, wf, h)(rng, p, c, e, en),
        }[name]())
    return torch.stack(rows)[None]


def check_monitor(name, batch, float_energy=True):
    """One monitor by name: samples bit-equal to the direct calls, mean / std over the walker axis, the period and the samples
    switch."""
    hamil, wf, params, pc, psi, e_loc, ratios = batch
    m = obs.observable_monitor_from_name(name)
    assert m.name == name and m.save_samples and m.period == 1
    with pytest.raises(RuntimeError, match='finalize'):
        m(0, 11, params, pc, psi, e_loc, ratios)
    assert m.finalize(hamil, wf) is m
    stats = m(0, 11, params, pc, psi, e_loc, ratios)
    samples = stats[f'{name}/samples']
    S, B = pc.r.shape[1:3]
    assert samples.dtype == F64 and tuple(samples.shape[:3]) == (1, S, B)
    want = direct_samples(name, hamil, wf, params, pc, e_loc)
    assert torch.equal(samples, want), float((samples - want).abs().max())
    if float_energy and m.requires_energy:
        assert torch.equal(samples, direct_samples(name, hamil, wf, params, pc, e_loc, float_energy=True))
    assert torch.equal(stats[f'{name}/mean'], samples.mean(2)) and torch.equal(stats[f'{name}/std'], samples.std(2, unbiased=False))
    assert tuple(stats[f'{name}/mean'].shape[:2]) == (1, S)
    m.period = 3
    assert m(1, 11, params, pc, psi, e_loc, ratios) == {} and m(2, 11, params, pc, psi, e_loc, ratios) == {}
    assert set(m(3, 11, params, pc, psi, e_loc, ratios)) == set(stats)
    m.save_samples = False
    assert set(m(0, 11, params, pc, psi, e_loc, ratios)) == {f'{name}/mean', f'{name}/std'}
    return stats


# ---------------------------------------------------------------- 6. fit_wf
def fit_setup(device, lib, dtype, n_walkers, small=True, seed=3):
    h, spec = lih(small)
    wf, params, sampler, st = training_setup(h, spec, dtype, device, lib, 2, n_walkers, 3, seed)
    opt = AdamOptimizer(2e-2, loss_fn=create_loss_fn(h, wf, alpha=4.0, scale_overlap_by='max_gap_std'))
    return h, wf, params, sampler, st, opt


def check_fit_with_monitors(device, lib, dtype, n_walkers, small=True, steps=3, seed=3):
    """Three steps of fit_wf at S = 2 with AdamOptimizer and a loss function (the device path: no sync in between) and the
    monitors below.  Per step: the monitors' keys are in the stats; oscillator_strength/mean is Engine.oscillator_strength of
    the yielded phys_conf, E_loc and ratios; spin/mean is evaluate_spin on the same phys_conf AFTER wf.sync_params brought the
    trees up to date (a monitor that read the stale leaves would differ); without monitors the key set is that of the unchanged
    call."""
    h, wf, params, sampler, st, opt = fit_setup(device, lib, dtype, n_walkers, small, seed)
    seen = {}
    orig_step = opt.step

    def step(rng, params_, opt_state, batch):
        out = orig_step(rng, params_, opt_state, batch)
        seen['pc'], seen['e_loc'], seen['ratios'] = batch[0], out[2], out[3]
        return out
    opt.step = step
    monitors = [obs.SpinMonitor(False, 1), obs.OscillatorStrengthMonitor(False, 1), obs.EnergyMonitor(True, 1),
                obs.WaveFunctionMonitor(True, 2), obs.ACZVQForceMonitor(True, 1)]
    mis = MoleculeIdxSampler(0, 1, 1)
    n = 0
    for k, state, _, stats in fit_wf(seed, h, wf, opt, mis, sampler, range(steps), TrainState(st, params, None), None,
                                     observable_monitors=monitors):
        n += 1
        for key in ('spin/mean', 'spin/std', 'oscillator_strength/mean', 'oscillator_strength/err', 'local_energy/samples',
                    'hf_force_ac_zvq/mean', 'hf_force_ac_zvq/samples', 'loss', 'energy/ewm'):
            assert key in stats, key
        assert ('psi/samples' in stats) == (k % 2 == 0)
        samples, rest = obs.split_samples(stats)
        assert all(key.endswith('/samples') for key in samples) and not any(key.endswith('/samples') for key in rest)
        assert set(samples) | set(rest) == set(stats) and 'local_energy/samples' in samples
        assert any(wf.params_stale(p) for p in state.params)            # (the device path: the trees are behind)
        pc, e_loc, ratios = seen['pc'], seen['e_loc'], seen['ratios']
        assert tuple(stats['oscillator_strength/mean'].shape) == (1, 2, 2)
        os_mean = wf.engine(state.params[0], pc.R[0]).oscillator_strength(pc.r[0], ratios[0].contiguous(), e_loc[0])[0]
        assert torch.equal(stats['oscillator_strength/mean'][0], os_mean)
        assert torch.isfinite(stats['oscillator_strength/mean']).all()
        e64 = e_loc.double()
        assert torch.equal(stats['local_energy/mean'], e64.mean(-1)) and torch.equal(stats['local_energy/samples'], e64)
        if 'psi/samples' in stats:          # the sampler's refreshed psi: that of the updated parameters at the step's walkers
            for s in range(2):
                sign, log = wf.engine(state.params[s], pc.R[0]).wf_eval(pc.r[0, s].contiguous(), pc.R[0])
                assert torch.equal(stats['psi/samples']['log'][0, s], log.double()) and torch.equal(stats['psi/samples']['sign'][0, s], sign.double())
        spin_monitor = stats['spin/mean'].clone()
        for p in state.params:
            wf.sync_params(p)
        assert not any(wf.params_stale(p) for p in state.params)
        spin = torch.stack([evaluate_spin(h, wf)(state.params[s], PhysicalConfiguration(pc.R[0], pc.r[0, s].contiguous(), None)) for s in range(2)])
        assert torch.equal(spin_monitor[0], spin.mean(-1)), (spin_monitor, spin.mean(-1))
    assert n == steps
    return stats


def check_fit_without_monitors(device, lib, dtype, n_walkers, small=True, steps=2, seed=3):
    """observable_monitors=None (and []): the keys and the values of the call without the argument."""
    runs = []
    for kw in ({}, {'observable_monitors': None}, {'observable_monitors': []}):
        h, wf, params, sampler, st, opt = fit_setup(device, lib, dtype, n_walkers, small, seed)
        runs.append([stats for _, _, _, stats in fit_wf(seed, h, wf, opt, MoleculeIdxSampler(0, 1, 1), sampler, range(steps),
                                                        TrainState(st, params, None), None, **kw)])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.keys() == b.keys()
            for key in a:
                assert torch.equal(torch.as_tensor(a[key]), torch.as_tensor(b[key])), key
