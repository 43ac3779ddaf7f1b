// Answers questions about mgard_amd/csrc/size_plan.hpp read from stdin, one per line
// (tests/test_size_plan_cpu.py). Doubles travel as C99 hexadecimal literals, so nothing is rounded.
//   record n dict chunk total_bits noutlier with_sync       -> min max
//   container metadata_bytes n elem record_min record_max   -> min max raw
//   sync lossless dict chunk total_bits n sync_env          -> 0 | 1
//   split dict K                                            -> tolerances of every launch
//   refuse total ntol dict                                  -> 0 | 1
//   search tol_min tol_max rounds nint lo hi [lo hi ...]    -> end tol finer index evaluations
//     (the stub: a tolerance fits when it lies in one of the closed intervals)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "size_plan.hpp"

using namespace mgh;

static double hexd(const std::string &t) { return std::strtod(t.c_str(), nullptr); }

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "record") {
      uint64_t n, dict, chunk, bits, nout;
      int sync;
      in >> n >> dict >> chunk >> bits >> nout >> sync;
      const ByteBracket b = record_bytes_bracket(n, dict, chunk, bits, nout, sync != 0);
      std::printf("%llu %llu\n", (unsigned long long)b.min, (unsigned long long)b.max);
    } else if (cmd == "container") {
      uint64_t meta, n, elem;
      ByteBracket r;
      in >> meta >> n >> elem >> r.min >> r.max;
      const ContainerBracket c = container_bytes_bracket(meta, n, elem, r);
      std::printf("%llu %llu %d\n", (unsigned long long)c.min, (unsigned long long)c.max, c.raw);
    } else if (cmd == "sync") {
      int lossless;
      uint64_t dict, chunk, bits, n;
      long env;
      in >> lossless >> dict >> chunk >> bits >> n >> env;
      std::printf("%d\n", record_has_sync(lossless, dict, chunk, bits, n, env) ? 1 : 0);
    } else if (cmd == "split") {
      uint64_t dict;
      int K;
      in >> dict >> K;
      for (int left = K; left > 0;) {
        const int kk = qhist_per_launch(dict, left);
        if (kk < 1) break;
        std::printf("%d ", kk);
        left -= kk;
      }
      std::printf("\n");
    } else if (cmd == "refuse") {
      uint64_t total, dict;
      int ntol;
      in >> total >> ntol >> dict;
      std::printf("%d\n", qhist_refusal(total, ntol, dict) ? 1 : 0);
    } else if (cmd == "search") {
      std::string a, b;
      int rounds, nint;
      in >> a >> b >> rounds >> nint;
      std::vector<double> iv(2 * (size_t)nint);
      for (double &x : iv) {
        std::string t;
        in >> t;
        x = hexd(t);
      }
      int evals = 0;
      auto fits = [&](double tol) {
        evals++;
        for (int k = 0; k < nint; k++)
          if (tol >= iv[2 * k] && tol <= iv[2 * k + 1]) return true;
        return false;
      };
      const SearchResult r = budget_search(hexd(a), hexd(b), rounds, fits);
      std::printf("%s %a %a %d %d\n",
                  r.end == SearchEnd::found ? "found" : r.end == SearchEnd::nothing_fits ? "nothing" : "bad", r.tol,
                  r.finer, r.index, evals);
    } else {
      std::fprintf(stderr, "unknown command: %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
