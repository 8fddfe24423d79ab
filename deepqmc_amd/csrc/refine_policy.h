// refine_policy.h -- the decisions of the float64 refinement that are arithmetic on the host alone: the self-calibration of
// the score threshold and the whole-batch float64 ("direct") mode with its hysteresis.  Plain C++: no HIP, nothing of Engine
// (engine_refine.inl gathers the inputs and acts on the answers; tests/refine_policy_main.cpp drives this header by itself).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace dqmc {

// One walker of a probe call's calibration sample: its relative float32 error against the float64 twin and its score.
struct RefineSample { double rel_err, score; };

// Re-derives the scale m of the exponential error model err = m x score x xi (engine.hip, above refine_thresh) and the score
// threshold from a probe call's sample and the B scores of its batch.  m is the previous estimate on entry (0: none yet);
// with fewer than two usable samples both stay as they are.
inline void refine_calibrate(const std::vector<RefineSample>& sample, const double* score, int B, double refine_target,
                             double refine_miss, double& m, double& thresh) {
  std::vector<double> cs;
  for (const RefineSample& s : sample)
    if (std::isfinite(s.rel_err) && std::isfinite(s.score) && s.score > 0) cs.push_back(s.rel_err / s.score);
  if (cs.size() < 2) return;
  // two robust estimates of m from the sample's quantiles, the larger one
  std::sort(cs.begin(), cs.end());
  const double q50 = cs[(size_t)(0.5 * (cs.size() - 1) + 0.5)], q90 = cs[(size_t)(0.9 * (cs.size() - 1) + 0.5)];
  const double m_now = std::fmax(std::fmax(q50 / 0.6931471805599453, q90 / 2.302585092994046), 1e-14);
  m = m > 0 ? std::sqrt(m * m_now) : m_now;         // geometric smoothing over the probes
  // the largest threshold whose kept walkers (scores of THIS batch, ascending) miss the tolerance at an expected
  // rate <= refine_miss:  (1 / B) sum_{s_i <= thr} exp(-tol / (m s_i)) <= refine_miss
  std::vector<double> ss;
  for (int b = 0; b < B; ++b) if (std::isfinite(score[b]) && score[b] > 0) ss.push_back(score[b]);
  std::sort(ss.begin(), ss.end());
  double acc = 0.0, thr = 1.0;
  for (size_t k = 0; k < ss.size(); ++k) {
    acc += std::exp(-refine_target / (m * ss[k])) / (double)B;
    if (acc > refine_miss) break;
    thr = ss[k];
  }
  if (!ss.empty() && acc <= refine_miss) thr = 1e9;           // (the whole batch may stay in float32)
  thresh = std::fmin(std::fmax(thr, 1.0), 1e9);
}

// Whole-batch float64 ("direct") mode, with hysteresis: a context ENTERS it when more than `enter` of a batch
// lies above the threshold (the float32 pass would mostly be wasted: f32(B) + f64(p B) costs more than f64(B) from
// p ~ 0.6 on, the float64 pass being ~2.5-3 x the float32 one per walker), runs 15 calls there, then looks again with a
// float32 pass and LEAVES only if the flagged fraction has fallen below `exit`.  One draw near a single
// 50 % line used to flip the mode -- and the cost of a benzene step between 166 and 207 ms -- from run to run.
struct DirectMode {
  double enter = 0.60, exit = 0.45;   // options "refine_direct_pct", "refine_direct_exit_pct"
  int calls = 15;                // calls a context stays in the direct mode before it looks again (option "refine_direct_calls")
  int backoff = 4;               // every look that CONFIRMS the direct mode doubles the stay, at most this many times (15, 30, ... 240 calls:
                                 // the float32 pass of such a look is thrown away -- 1/16 of ~0.4 of a benzene / C4H4 E_loc call at a fixed stay);
                                 // option "refine_direct_backoff"
  int streak = 0;                // consecutive confirmations
  bool was_direct = false;       // the last mode decision was "direct"
  int calls_left = 0;            // > 0: most walkers were flagged last time -> the next calls go to float64 directly

  // A float32 look found n_above of B walkers above the threshold: more than the line of the mode the context is in (and a
  // batch of 16 walkers or more) sends the batch to float64 whole, this call and the following stay() ones.
  bool decide(long n_above, int B) {
    const double lim = was_direct ? exit : enter;
    const bool yes = B >= 16 && (double)n_above > lim * (double)B;
    streak = (yes && was_direct) ? streak + 1 : 0;
    was_direct = yes;
    if (yes) calls_left = stay();
    return yes;
  }
  // a call begins: true while calls of a stay are left (this one is taken off them and needs no float32 look)
  bool take_call() {
    if (calls_left <= 0) return false;
    --calls_left;
    return true;
  }
  // calls the context now stays in the direct mode: doubled by every look that confirmed it (backoff)
  int stay() const {
    const int sh = streak < backoff ? streak : backoff;
    const long n = (long)calls << (sh < 16 ? sh : 16);
    return n > 1000000 ? 1000000 : (int)n;
  }
};

}  // namespace dqmc
