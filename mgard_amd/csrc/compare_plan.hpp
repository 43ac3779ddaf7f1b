// Error statistics of two arrays (mgh_compare, mgh_verify): how the elements are dealt to the
// workgroups of the reduction kernel, how two partial results become one, and the figures derived
// from a result. Host-only and free of HIP, so that all three can be compiled by a plain C++
// compiler and pinned by the CPU suite (tests/test_compare_cpu.py). merge() is the ONE statement of
// the tie rule of `argmax`: the second kernel stage (kernels_compare.hpp: k_compare_final), the
// staging loop of host arrays (capi.hip) and mgh_verify's fold over the subdomains (highlevel.hip)
// all go through it.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

#include "../../include/mgard_hip.h"

#if defined(__HIPCC__)
#define MGH_CMP_HD __host__ __device__
#else
#define MGH_CMP_HD
#endif

namespace mgh {

// 16-byte loads by 256 lanes: the unit the slabs are made of
constexpr uint64_t kCompareVecBytes = 16;
constexpr uint64_t kCompareThreads = 256;
// Most workgroups of one launch. A CONSTANT, not the compute units of the device: the slabs, and
// with them the order of every addition, are then the same on every box. 2048 = 256 compute units
// x 8 workgroups of 256 threads, one full round of resident workgroups on the MI355X.
constexpr uint64_t kCompareMaxGroups = 2048;

struct ComparePlan {
  uint64_t groups = 0;  // workgroups; workgroup b reduces [b * slab, min(n, (b + 1) * slab))
  uint64_t slab = 0;    // elements of a slab: a multiple of unit
  uint64_t unit = 0;    // elements 256 lanes load at once: (16 / esz) * 256
};

inline ComparePlan compare_plan(uint64_t n, size_t esz) {
  ComparePlan p;
  p.unit = kCompareVecBytes / (uint64_t)esz * kCompareThreads;
  p.slab = p.unit;
  if (n == 0) return p;
  const uint64_t per = (n - 1) / kCompareMaxGroups + 1;  // elements a workgroup must take at least
  p.slab = ((per - 1) / p.unit + 1) * p.unit;
  p.groups = (n - 1) / p.slab + 1;
  return p;
}

// mgh_compare_masked_: a wave holds `left` (1 .. 64) consecutive positions of a row against the mask bits
// p, p + 1, ... They begin in word p / 64 at bit p % 64; the NEXT word is read only where they reach it, so
// the last word of a mask is never stepped over.
MGH_CMP_HD inline bool compare_mask_second_word(uint64_t p, uint32_t left) { return (p & 63) + left > 64; }

// positions that take part in the maxima and sums
MGH_CMP_HD inline uint64_t compare_finite(const mgh_error_stats &s) { return s.n - s.nonfinite; }

// Folds `part` into `into`. `part` covers positions whose flat indices are index_offset further on
// than part.argmax says. Counters and sums add (part is added TO into: the sums depend on the order
// of the calls, so every caller folds in ascending order of its parts). Extremes: of the two; a part
// without a finite position carries none. max_abs_err: the larger, and on a tie the LOWER global
// index -- whichever order the parts come in.
MGH_CMP_HD inline void merge(mgh_error_stats &into, const mgh_error_stats &part, uint64_t index_offset) {
  const bool have = compare_finite(into) > 0, add = compare_finite(part) > 0;
  into.n += part.n;
  into.nonfinite += part.nonfinite;
  if (!add) return;
  const uint64_t at = part.argmax + index_offset;
  if (!have) {
    into.max_abs_err = part.max_abs_err;
    into.argmax = at;
    into.ref_min = part.ref_min;
    into.ref_max = part.ref_max;
    into.ref_abs_max = part.ref_abs_max;
    into.sum_sq_err += part.sum_sq_err;  // (into's sums are 0: the order is still the callers')
    into.ref_sum_sq += part.ref_sum_sq;
    return;
  }
  if (part.max_abs_err > into.max_abs_err || (part.max_abs_err == into.max_abs_err && at < into.argmax)) {
    into.max_abs_err = part.max_abs_err;
    into.argmax = at;
  }
  into.sum_sq_err += part.sum_sq_err;
  into.ref_sum_sq += part.ref_sum_sq;
  if (part.ref_min < into.ref_min) into.ref_min = part.ref_min;
  if (part.ref_max > into.ref_max) into.ref_max = part.ref_max;
  if (part.ref_abs_max > into.ref_abs_max) into.ref_abs_max = part.ref_abs_max;
}

// ---- figures derived from a result (reference include/mgard-x/Utilities/ErrorCalculator.h:99-121;
// the divisor is the number of positions that took part, so non-finite ones do not dilute it).
// Without a finite position the mean is taken over nothing: 0, not 0 / 0.
inline double mse(const mgh_error_stats &s) {
  const uint64_t m = compare_finite(s);
  return m ? s.sum_sq_err / (double)m : 0.0;
}
inline double rmse(const mgh_error_stats &s) { return std::sqrt(mse(s)); }
inline double l2_error(const mgh_error_stats &s, bool normalize) {
  return normalize ? std::sqrt(mse(s)) : std::sqrt(s.sum_sq_err);
}
// 20 log10(range of the reference / rmse); +inf for a zero error (also when the range is zero)
inline double psnr(const mgh_error_stats &s) {
  const double r = rmse(s);
  if (r == 0) return std::numeric_limits<double>::infinity();
  return 20.0 * std::log10((s.ref_max - s.ref_min) / r);
}

}  // namespace mgh
