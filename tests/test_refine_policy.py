"""The host-only policy of the float64 refinement (deepqmc_amd/csrc/refine_policy.h): the threshold calibration against
the same formulas in NumPy, the direct-mode state machine against the sequence test_facade_emu.py documents.  The header is
driven by a stand-alone program (refine_policy_main.cpp, built with the address and undefined-behaviour sanitizers): nothing
is loaded into Python."""
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'deepqmc_amd', 'csrc')
TARGET, MISS = 1e-5, 1e-8            # the library's defaults: "refine_target_e7" 100, "refine_miss_e9" 10
LN2, LN10 = 0.6931471805599453, 2.302585092994046


@pytest.fixture(scope='module')
def policy(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('refine_policy') / 'refine_policy_main')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', CSRC,
                    os.path.join(HERE, 'refine_policy_main.cpp'), '-o', exe], check=True)

    def run(text):
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        return out.stdout.split('\n')[:-1]
    return run


def fmt(xs):
    return ' '.join(float(x).hex() for x in np.asarray(xs, dtype=np.float64).ravel())      # ('nan' / 'inf' as strtod reads them)


def calib_case(rel, s_score, score, B, m, thr):
    return f'calib {len(rel)} {B} {fmt([TARGET, MISS, m, thr])}\n{fmt(np.stack([rel, s_score], -1))}\n{fmt(score)}\n'


def calibrate_np(rel, s_score, score, B, m, thr):
    """refine_calibrate in NumPy; also the least relative distance of a running miss sum from MISS (inf: no sum)."""
    ok = np.isfinite(rel) & np.isfinite(s_score) & (s_score > 0)
    cs = np.sort(rel[ok] / s_score[ok])
    if cs.size < 2:
        return m, thr, math.inf
    q50, q90 = cs[int(0.5 * (cs.size - 1) + 0.5)], cs[int(0.9 * (cs.size - 1) + 0.5)]
    m_now = max(q50 / LN2, q90 / LN10, 1e-14)
    m = math.sqrt(m * m_now) if m > 0 else m_now
    ss = np.sort(score[np.isfinite(score) & (score > 0)])
    acc, new, margin = 0.0, 1.0, math.inf
    for s in ss:
        acc += np.exp(-TARGET / (m * s)) / B
        margin = min(margin, abs(acc - MISS) / MISS)
        if acc > MISS:
            break
        new = s
    if ss.size and acc <= MISS:
        new = 1e9
    return m, min(max(new, 1.0), 1e9), margin


def within_ulp(a, b, n):
    return abs(a - b) <= n * np.spacing(abs(b))


@pytest.mark.parametrize('m_true', [1.3e-8, 5.6e-8])            # the scales engine.hip quotes (LiH / PauliNet, LiH / Psiformer)
@pytest.mark.parametrize('B,n_sample', [(256, 256), (20, 3)])
@pytest.mark.parametrize('m_prev', [0.0, 2e-8])                 # first probe; a later one (geometric smoothing)
def test_calibration_matches_numpy(policy, m_true, B, n_sample, m_prev):
    rng = np.random.default_rng([B, int(m_true * 1e10), 7])
    score = 10.0 ** rng.uniform(0.0, 4.0, B)
    err = m_true * score * rng.exponential(1.0, B)
    pick = np.arange(n_sample) * B // n_sample                  # the strided sample of a probe call
    m, thr, margin = calibrate_np(err[pick], score[pick], score, B, m_prev, 200.0)
    # libm's exp against NumPy's cannot flip the chosen score: no running miss sum lies within 1e-3 (relative) of the budget
    assert margin > 1e-3, margin
    got_m, got_thr = (float.fromhex(x) for x in policy(calib_case(err[pick], score[pick], score, B, m_prev, 200.0))[0].split())
    assert got_thr == thr and (thr in score or thr in (1.0, 1e9))
    assert 1.0 < thr < 1e9                                        # (these cases cut inside the batch)
    assert within_ulp(got_m, m, 4), (got_m, m)                    # two IEEE divisions, a max and a sqrt
    if n_sample == B:                                             # (a sample of 256 measures the scale it was drawn with)
        assert 0.7 * m_true < (got_m if m_prev == 0 else got_m ** 2 / m_prev) < 1.4 * m_true


def test_calibration_degenerate_cases(policy):
    rng = np.random.default_rng(3)
    score = 10.0 ** rng.uniform(0.0, 4.0, 32)
    err = 1.3e-8 * score * rng.exponential(1.0, 32)
    nan, inf = math.nan, math.inf
    cases = [
        # fewer than two usable samples: (m, threshold) unchanged
        (np.array([]), np.array([]), score, 5e-8, 321.0),
        (err[:1], score[:1], score, 5e-8, 321.0),
        (np.array([nan, err[1], inf, err[3]]), np.array([score[0], score[1], score[2], -1.0]), score, 0.0, 77.0),
        # all scores tiny: the whole batch may stay in float32
        (err[:8] * 1e-6, score[:8] * 1e-6, score * 1e-6, 0.0, 200.0),
        # the first score is over the miss budget by itself
        (err[:8] * 1e3, score[:8] * 1e3, score * 1e3 + 1e6, 0.0, 200.0),
    ]
    out = policy(''.join(calib_case(r, s, sc, 32, m, t) for r, s, sc, m, t in cases))
    got = [tuple(float.fromhex(x) for x in line.split()) for line in out]
    assert got[0] == (5e-8, 321.0) and got[1] == (5e-8, 321.0) and got[2] == (0.0, 77.0)
    assert got[3][1] == 1e9 and got[4][1] == 1.0
    for (r, s, sc, m, t), g in zip(cases, got):
        m_np, thr_np, _ = calibrate_np(r, s, sc, 32, m, t)
        assert g[1] == thr_np and within_ulp(g[0], m_np, 4)


def test_direct_mode_state_machine(policy):
    def replay(params, B, n_above):
        out = policy(f'direct {params}\n' + ''.join(f'call {n} {B}\n' for n in n_above))
        return [tuple(int(x) for x in line.split()) for line in out]
    # the sequence of test_direct_mode_hysteresis_counters_and_scores: B = 20, lines 60 % / 45 %, a stay of 1 call, no back-off;
    # 50 % stays mixed, 75 % enters, (a direct call), 50 % coming from the direct mode stays there, (a direct call), 40 % leaves
    assert replay('0.6 0.45 1 0', 20, [10, 15, 10, 10, 10, 8]) == [(0, 0), (1, 1), (1, 0), (1, 1), (1, 0), (0, 0)]
    # back-off 2: every look that confirms the direct mode doubles the stay, twice at most
    seq, stays = [], [1, 2, 4, 4]
    for s in stays:
        seq += [(1, s)] + [(1, s - 1 - k) for k in range(s)]
    assert replay('0.6 0.45 1 2', 20, [15] * len(seq)) == seq
    # batches below 16 walkers never go direct
    assert replay('0.6 0.45 1 2', 15, [15, 15, 0, 15]) == [(0, 0)] * 4
