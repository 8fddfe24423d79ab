// Stand-alone driver of deepqmc_amd/csrc/refine_policy.h for tests/test_refine_policy.py: reads cases from stdin, prints one
// result line per case (doubles as hex floats: exact).
//   calib <n_samples> <B> <target> <miss> <m> <thresh>  then n_samples pairs (rel_err score), then B scores
//       -> "<m> <thresh>"
//   direct <enter> <exit> <calls> <backoff>             a fresh state machine with these parameters   -> nothing
//   call <n_above> <B>                                   one local-energy call: a direct call of a stay, or a look that decides
//       -> "<direct 0/1> <calls_left>"
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "refine_policy.h"

static double rd() {      // (strtod: reads nan / inf as well)
  std::string s;
  std::cin >> s;
  return std::strtod(s.c_str(), nullptr);
}

int main() {
  dqmc::DirectMode dm;
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "calib") {
      const int ns = (int)rd(), B = (int)rd();
      const double target = rd(), miss = rd();
      double m = rd(), thresh = rd();
      std::vector<dqmc::RefineSample> sample((size_t)ns);
      for (auto& s : sample) { s.rel_err = rd(); s.score = rd(); }
      std::vector<double> score((size_t)B);
      for (auto& s : score) s = rd();
      dqmc::refine_calibrate(sample, score.data(), B, target, miss, m, thresh);
      std::printf("%a %a\n", m, thresh);
    } else if (cmd == "direct") {
      dm = dqmc::DirectMode();
      dm.enter = rd(); dm.exit = rd(); dm.calls = (int)rd(); dm.backoff = (int)rd();
    } else if (cmd == "call") {
      const long n_above = (long)rd();
      const int B = (int)rd();
      const bool direct = dm.take_call() || dm.decide(n_above, B);
      std::printf("%d %d\n", direct ? 1 : 0, dm.calls_left);
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
