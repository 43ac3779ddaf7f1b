// Prints what mgard_amd/csrc/prolong_window_plan.hpp plans (tests/test_prolong_window_cpu.py). No HIP.
// stdin, one query per line:  D L level  shape[0][0..D) ... shape[L][0..D)  lo[0..D)  ext[0..D)
// stdout, one line per query: the chain, (L - level + 1) * 2 * D integers, or "bad".
// A line "plan n_r n_c n_f a_r a_c a_f b_r b_c b_f tall_ok" prints the launch plan of one window step.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "prolong_window_plan.hpp"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    if (line.rfind("plan", 0) == 0) {
      std::string word;
      uint32_t n[3];
      int64_t a[3], b[3];
      int tall = 0;
      in >> word >> n[0] >> n[1] >> n[2] >> a[0] >> a[1] >> a[2] >> b[0] >> b[1] >> b[2] >> tall;
      const mgh::ProlongWinPlan w = mgh::prolong_window_plan(n, a, b, tall != 0);
      std::printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", w.p.TC, w.p.TF, w.p.gxm, w.p.ntile, w.p.rch, w.p.nchunk, w.J0[0],
                  w.J0[1], w.J0[2], w.nJ[0], w.nJ[1], w.nJ[2]);
      continue;
    }
    int D = 0, L = 0, level = 0;
    if (!(in >> D >> L >> level)) continue;
    std::vector<std::vector<uint64_t>> shape(L + 1, std::vector<uint64_t>(D));
    for (auto &s : shape)
      for (auto &e : s) in >> e;
    std::vector<uint64_t> lo(D), ext(D);
    for (auto &e : lo) in >> e;
    for (auto &e : ext) in >> e;
    std::vector<int64_t> out;
    if (!in || !mgh::prolong_window_chain(shape, level, lo.data(), ext.data(), out)) {
      std::puts("bad");
      continue;
    }
    std::string text;
    for (size_t i = 0; i < out.size(); i++) text += (i ? " " : "") + std::to_string(out[i]);
    std::puts(text.c_str());
  }
  return 0;
}
