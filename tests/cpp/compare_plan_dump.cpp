// Stand-alone driver of mgard_amd/csrc/compare_plan.hpp for tests/test_compare_cpu.py: built with the
// host compiler against the header alone (no HIP). One command per line on stdin:
//   plan N ESZ                      -> "plan groups slab unit cap", then "slab b lo hi" for the first,
//                                      the second and the last two slabs
//   merge f32|f64 FILE_A FILE_B N ORDER K CUT_1 .. CUT_K
//                                   -> the arrays cut at the K positions; every part reduced on its own
//                                      by the plain loop below (argmax local to the part), the parts
//                                      folded with merge() -- ORDER fwd: ascending, rev: descending --
//                                      -> "stats ..." and "derived ..."
//   derive N NONFINITE MAX ARGMAX SSE RMIN RMAX RAMAX RSS   -> "derived ..."
// Floating-point values travel as C99 hex floats, so nothing is lost in print.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "compare_plan.hpp"

using namespace mgh;

// the statistics of one part, as mgh_error_stats defines them
template <typename T> mgh_error_stats reduce_part(const T *a, const T *b, uint64_t n) {
  mgh_error_stats s{};
  s.n = n;
  bool any = false;
  for (uint64_t i = 0; i < n; i++) {
    const T d = a[i] - b[i];
    if (!std::isfinite(d)) {
      s.nonfinite++;
      continue;
    }
    const double e = (double)std::fabs(d), x = (double)a[i];
    if (!any || e > s.max_abs_err) {
      s.max_abs_err = e;
      s.argmax = i;
    }
    s.sum_sq_err += e * e;
    s.ref_sum_sq += x * x;
    if (!any || x < s.ref_min) s.ref_min = x;
    if (!any || x > s.ref_max) s.ref_max = x;
    if (!any || std::fabs(x) > s.ref_abs_max) s.ref_abs_max = std::fabs(x);
    any = true;
  }
  return s;
}

template <typename T> std::vector<T> read_all(const std::string &path, uint64_t n) {
  std::vector<T> v(n);
  std::ifstream f(path, std::ios::binary);
  f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(n * sizeof(T)));
  if (!f && n) {
    std::fprintf(stderr, "short read of %s\n", path.c_str());
    std::exit(2);
  }
  return v;
}

void print_stats(const mgh_error_stats &s) {
  std::printf("stats %" PRIu64 " %" PRIu64 " %a %" PRIu64 " %a %a %a %a %a\n", s.n, s.nonfinite, s.max_abs_err, s.argmax,
              s.sum_sq_err, s.ref_min, s.ref_max, s.ref_abs_max, s.ref_sum_sq);
}
void print_derived(const mgh_error_stats &s) {
  std::printf("derived %a %a %a %a %a\n", mse(s), rmse(s), l2_error(s, true), l2_error(s, false), psnr(s));
}

template <typename T>
void run_merge(const std::string &fa, const std::string &fb, uint64_t n, bool rev, const std::vector<uint64_t> &cuts) {
  const std::vector<T> a = read_all<T>(fa, n), b = read_all<T>(fb, n);
  std::vector<uint64_t> edge{0};
  for (uint64_t c : cuts) edge.push_back(c);
  edge.push_back(n);
  mgh_error_stats total{};
  const size_t parts = edge.size() - 1;
  for (size_t k = 0; k < parts; k++) {
    const size_t p = rev ? parts - 1 - k : k;
    merge(total, reduce_part<T>(a.data() + edge[p], b.data() + edge[p], edge[p + 1] - edge[p]), edge[p]);
  }
  print_stats(total);
  print_derived(total);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "plan") {
      uint64_t n = 0;
      size_t esz = 0;
      in >> n >> esz;
      const ComparePlan p = compare_plan(n, esz);
      std::printf("plan %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", p.groups, p.slab, p.unit, kCompareMaxGroups);
      for (uint64_t b = 0; b < p.groups; b++) {
        if (b >= 2 && b + 2 < p.groups) continue;
        const uint64_t lo = b * p.slab, hi = lo + p.slab < n ? lo + p.slab : n;
        std::printf("slab %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", b, lo, hi);
      }
    } else if (cmd == "merge") {
      std::string ty, fa, fb, order;
      uint64_t n = 0, k = 0;
      in >> ty >> fa >> fb >> n >> order >> k;
      std::vector<uint64_t> cuts(k);
      for (auto &c : cuts) in >> c;
      if (ty == "f32") run_merge<float>(fa, fb, n, order == "rev", cuts);
      else run_merge<double>(fa, fb, n, order == "rev", cuts);
    } else if (cmd == "derive") {
      mgh_error_stats s{};
      std::string f[7];
      in >> s.n >> s.nonfinite >> f[0] >> s.argmax >> f[1] >> f[2] >> f[3] >> f[4] >> f[5];
      s.max_abs_err = std::strtod(f[0].c_str(), nullptr);
      s.sum_sq_err = std::strtod(f[1].c_str(), nullptr);
      s.ref_min = std::strtod(f[2].c_str(), nullptr);
      s.ref_max = std::strtod(f[3].c_str(), nullptr);
      s.ref_abs_max = std::strtod(f[4].c_str(), nullptr);
      s.ref_sum_sq = std::strtod(f[5].c_str(), nullptr);
      print_derived(s);
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
