// Compression to a measured error target (mgh_achieved_errors, mgh_compress_target; DESIGN.md
// section 8): which figure of an mgh_error_stats a target is held against, when it is met, and the
// search for the largest tolerance that meets it. Host-only and free of HIP: a plain C++ compiler
// builds it and the CPU suite pins it (tests/test_target_plan_cpu.py).
#pragma once
#include <cmath>
#include <cstdint>

#include "compare_plan.hpp"

namespace mgh {

// what mgh_quantize_roundtrip refuses (nullptr: nothing): its kernel divides a 32-bit linear index,
// like k_quantize_histograms's
inline const char *qround_refusal(uint64_t total) {
  if (total == 0 || total >= ((uint64_t)1 << 32)) return "quantize_roundtrip: 1 .. 2^32 - 1 elements (32-bit index arithmetic)";
  return nullptr;
}

constexpr int kTargetMaxTols = 64;    // mgh_achieved_errors: tolerances per call
constexpr int kTargetMaxRounds = 16;  // mgh_compress_target: rounds of the search

// (the values of mgh_target_metric, include/mgard_hip_compress.h)
enum class TargetMetric { max_abs = 0, rmse = 1, psnr = 2 };

inline bool target_metric_valid(int metric) { return metric >= 0 && metric <= 2; }

// The figure of the statistics the metric names (the derived ones are compare_plan.hpp's).
inline double target_achieved(const mgh_error_stats &s, TargetMetric metric) {
  switch (metric) {
  case TargetMetric::max_abs: return s.max_abs_err;
  case TargetMetric::rmse: return rmse(s);
  case TargetMetric::psnr: return psnr(s);
  }
  return std::nan("");
}

// An error must not exceed its target, a PSNR must reach it. A result with non-finite positions
// meets nothing (mgh_verify reports within = 0 there), nor does a figure that is NaN.
inline bool target_meets(const mgh_error_stats &s, TargetMetric metric, double target) {
  if (s.nonfinite > 0) return false;
  const double got = target_achieved(s, metric);
  if (std::isnan(got)) return false;
  return metric == TargetMetric::psnr ? got >= target : got <= target;
}

// ---- the search ------------------------------------------------------------------------------------
// The largest tolerance in [tol_min, tol_max] that meets the target, on a logarithmic grid: tol_max if
// it meets it; else tol_min must, and the bracket [a, b] -- a meets, b does not -- is halved (in log)
// `rounds` times at m = sqrt(a) * sqrt(b): sqrt and one multiply are exact IEEE operations, the
// construction of budget_search (size_plan.hpp), so any restatement in double precision walks the same
// values. a always meets the target BY MEASUREMENT, so an error curve that is not monotone costs
// compression at worst, never the target.
enum class TargetEnd { found, nothing_meets, bad_argument };
struct TargetResult {
  TargetEnd end = TargetEnd::bad_argument;
  double tol = 0;      // found: the tolerance to use (it meets the target)
  double coarser = 0;  // found after rounds: the bracket's other end (it does not meet the target); else 0
  int candidates = 0;  // evaluations of `meets`
};
// meets(tol) -> bool
template <typename Meets> TargetResult target_search(double tol_min, double tol_max, int rounds, Meets &&meets) {
  TargetResult r;
  if (!(tol_min > 0) || !(tol_min <= tol_max) || !std::isfinite(tol_max) || rounds < 1 || rounds > kTargetMaxRounds)
    return r;
  r.candidates = 1;
  if (meets(tol_max)) {
    r.end = TargetEnd::found;
    r.tol = tol_max;
    return r;
  }
  r.candidates = 2;
  if (!meets(tol_min)) {
    r.end = TargetEnd::nothing_meets;
    return r;
  }
  double a = tol_min, b = tol_max;
  for (int round = 0; round < rounds; round++) {
    const double m = std::sqrt(a) * std::sqrt(b);
    r.candidates++;
    if (meets(m)) a = m;
    else b = m;
  }
  r.end = TargetEnd::found;
  r.tol = a;
  r.coarser = b;
  return r;
}

}  // namespace mgh
