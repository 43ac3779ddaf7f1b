// mgard_hip_errors.hpp -- the figures of the reference's error calculator
// (include/mgard-x/Utilities/ErrorCalculator.h: L_inf_norm, L_2_norm, L_inf_error, L_2_error, MSE,
// PSNR) from ONE pass of mgh_compare (mgard_hip.h) over the arrays, which may lie in host or in
// device memory. compress_x_hip.hpp (namespace mgard_x, the reference's signatures) and
// compress_hip.hpp (namespace mgard_hip) wrap these. What the reference's loops define, restated:
//   * differences and absolute values are taken in T, then widened to double; squares are summed
//     in double;
//   * a norm that comes out 0 is replaced by DBL_EPSILON (L_2_norm replaces the SUM of squares
//     before the root, so the L2 norm of a zero array is sqrt(epsilon), or sqrt(epsilon / n));
//   * a REL error is the ABS error divided by the norm of the original;
//   * MSE divides by n;
//   * PSNR's range is max - min of the original with the maximum STARTING AT 0 and the minimum
//     starting at DBL_MAX: range = max(ref_max, 0) - ref_min, so for an all-negative array it is
//     -ref_min and not ref_max - ref_min. (mgh_error_stats' own psnr uses ref_max - ref_min.)
// One difference: a position whose difference is not finite is left out of every figure here
// (mgh_error_stats::nonfinite counts them), where the reference lets a NaN poison its sums and
// ignores it in its maxima. A failed call (no device, bad pointer) yields NaN.
#ifndef MGARD_HIP_ERRORS_HPP
#define MGARD_HIP_ERRORS_HPP

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <type_traits>
#include <vector>

#include "mgard_hip.h"

namespace mgard_hip_errors {

template <typename T> constexpr int dtype_of() {
  static_assert(std::is_same<T, float>::value || std::is_same<T, double>::value, "float or double");
  return std::is_same<T, double>::value ? MGH_DOUBLE : MGH_FLOAT;
}
// statistics of the n elements of a against b as a 1-D array; false: the call failed
template <typename T> bool stats(size_t n, const T *a, const T *b, mgh_error_stats &out, int device = 0) {
  const uint64_t shape[1] = {(uint64_t)n};
  return mgh_compare(1, dtype_of<T>(), shape, a, nullptr, b, nullptr, &out, device, nullptr) == MGH_SUCCESS;
}
inline size_t count(const std::vector<uint64_t> &shape) {
  size_t n = 1;
  for (uint64_t e : shape) n *= (size_t)e;
  return n;
}
inline double nan() { return std::numeric_limits<double>::quiet_NaN(); }
inline double l2_of(double sum_sq, size_t n, bool normalize_coordinates) {
  if (sum_sq == 0) sum_sq = DBL_EPSILON;
  return normalize_coordinates ? std::sqrt(sum_sq / (double)n) : std::sqrt(sum_sq);
}

template <typename T> double L_inf_norm(size_t n, const T *data, int device = 0) {
  mgh_error_stats s;
  if (!stats(n, data, data, s, device)) return nan();
  return s.ref_abs_max == 0 ? DBL_EPSILON : s.ref_abs_max;
}
template <typename T> double L_2_norm(size_t n, const T *data, bool normalize_coordinates, int device = 0) {
  mgh_error_stats s;
  if (!stats(n, data, data, s, device)) return nan();
  return l2_of(s.ref_sum_sq, n, normalize_coordinates);
}
template <typename T> double L_inf_error(size_t n, const T *original, const T *decompressed, bool rel, int device = 0) {
  mgh_error_stats s;
  if (!stats(n, original, decompressed, s, device)) return nan();
  return rel ? s.max_abs_err / (s.ref_abs_max == 0 ? DBL_EPSILON : s.ref_abs_max) : s.max_abs_err;
}
template <typename T>
double L_2_error(size_t n, const T *original, const T *decompressed, bool rel, bool normalize_coordinates, int device = 0) {
  mgh_error_stats s;
  if (!stats(n, original, decompressed, s, device)) return nan();
  const double err = l2_of(s.sum_sq_err, n, normalize_coordinates);
  return rel ? err / l2_of(s.ref_sum_sq, n, normalize_coordinates) : err;
}
template <typename T> double MSE(size_t n, const T *original, const T *decompressed, int device = 0) {
  mgh_error_stats s;
  if (!stats(n, original, decompressed, s, device)) return nan();
  return s.sum_sq_err / (double)n;
}
template <typename T> double PSNR(size_t n, const T *original, const T *decompressed, int device = 0) {
  mgh_error_stats s;
  if (!stats(n, original, decompressed, s, device)) return nan();
  // (the reference's maximum starts at 0, its minimum at DBL_MAX)
  const double range = std::max(s.ref_max, 0.0) - std::min(s.ref_min, DBL_MAX);
  return 20 * std::log10(range / std::sqrt(s.sum_sq_err / (double)n));
}

}  // namespace mgard_hip_errors

#endif  // MGARD_HIP_ERRORS_HPP
