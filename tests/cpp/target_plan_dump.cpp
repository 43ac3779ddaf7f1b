// Host-side dump of mgard_amd/csrc/target_plan.hpp for tests/test_target_plan_cpu.py: no HIP, a plain
// C++ compiler builds it. Commands on stdin, one per line, doubles as hexadecimal floating-point literals:
//   search <tol_min> <tol_max> <rounds> <t1> <t2> <t3>
//       target_search against the stub "meets(tol) = tol <= t1 || (t2 <= tol && tol <= t3)" (a monotone
//       curve: t2 > t3). Prints: end (0 found, 1 nothing_meets, 2 bad_argument), tol, coarser, candidates,
//       then every tolerance the search evaluated, in order.
//   meets <metric> <target> <n> <nonfinite> <max_abs_err> <argmax> <sum_sq_err> <ref_min> <ref_max>
//         <ref_abs_max> <ref_sum_sq>
//       Prints target_achieved and target_meets (1 / 0).
//   refusal <total>       prints 1 if mgh_quantize_roundtrip refuses an array of that many elements, else 0
//   metric <int>          prints target_metric_valid
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "target_plan.hpp"

int main() {
  using namespace mgh;
  char line[1024];
  while (std::fgets(line, sizeof line, stdin)) {
    char cmd[32] = {0};
    int used = 0;
    if (std::sscanf(line, "%31s%n", cmd, &used) != 1) continue;
    const char *rest = line + used;
    if (!std::strcmp(cmd, "search")) {
      double tol_min, tol_max, t1, t2, t3;
      int rounds;
      if (std::sscanf(rest, "%la %la %d %la %la %la", &tol_min, &tol_max, &rounds, &t1, &t2, &t3) != 6) return 2;
      std::vector<double> seen;
      const TargetResult r = target_search(tol_min, tol_max, rounds, [&](double tol) {
        seen.push_back(tol);
        return tol <= t1 || (t2 <= tol && tol <= t3);
      });
      std::printf("%d %a %a %d", (int)r.end, r.tol, r.coarser, r.candidates);
      for (double t : seen) std::printf(" %a", t);
      std::printf("\n");
    } else if (!std::strcmp(cmd, "meets")) {
      int metric;
      double target;
      mgh_error_stats s{};
      if (std::sscanf(rest, "%d %la %" SCNu64 " %" SCNu64 " %la %" SCNu64 " %la %la %la %la %la", &metric, &target, &s.n,
                      &s.nonfinite, &s.max_abs_err, &s.argmax, &s.sum_sq_err, &s.ref_min, &s.ref_max, &s.ref_abs_max,
                      &s.ref_sum_sq) != 11)
        return 2;
      std::printf("%a %d\n", target_achieved(s, (TargetMetric)metric), target_meets(s, (TargetMetric)metric, target) ? 1 : 0);
    } else if (!std::strcmp(cmd, "refusal")) {
      uint64_t total;
      if (std::sscanf(rest, "%" SCNu64, &total) != 1) return 2;
      std::printf("%d\n", qround_refusal(total) ? 1 : 0);
    } else if (!std::strcmp(cmd, "metric")) {
      std::printf("%d\n", target_metric_valid(std::atoi(rest)) ? 1 : 0);
    } else {
      return 2;
    }
  }
  return 0;
}
