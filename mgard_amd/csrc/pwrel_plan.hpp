// Pointwise relative error bound (mgh_compress_pwrel and its readers): |x' - x| <= eps |x| at
// every element, by compressing y = log2|x| under an ABS, s = inf bound delta. This header holds the classification
// of an element, the tolerance delta with its derivation, and the trailer of such a buffer. Host-only and free of
// HIP: a plain C++ compiler builds it and the CPU suite pins it (tests/test_pwrel_plan_cpu.py); the kernels of
// kernels_pwrel.hpp use the classification through MGH_MASK_HD.
//
// CLASSES of an element x of type T against floor_eff = max(abs_floor, smallest normal of T) (abs_floor >= 0 is the
// caller's; a denormal cannot carry a relative bound and is always below the floor; the comparison is made in
// double, where |x| is exact):
//   nonfinite  NaN or +-Inf                      mask bit 1, flag bit 1            decodes to a quiet NaN
//   zeroed     |x| < floor_eff                   mask bit 1, flag bit 0            decodes to +0.0
//   valid      everything else                   mask bit 0, flag bit = sign of x  decodes to +-exp2(y')
// Two bitmaps in the layout of mask_words() are enough: a masked position whose flag bit is set was non-finite.
// NaN and +-Inf are not told apart after the round trip, and a small negative value (-0.0 included) decodes to +0.0.
//
// THE TOLERANCE delta = log2(1 + eps) - E1 - 1.5 E2. The transform is evaluated in DOUBLE for both data types:
//   forward   y  = (T)log2((double)|x|)          inverse   x' = +-(T)exp2((double)y')
// With L the exact log2|x| and |y' - y| <= delta (the ABS, s = inf guarantee of the container of y):
//   |y - L| <= E1 = ulp_T(ybound), ybound the largest |y| of a valid element: the device log2 of a double is within
//      1 ulp of a double (HIP Programming Guide, "HIP math API", double-precision table: log2, maximum error 1 ulp),
//      and rounding to T adds half an ulp of T; for T = double nothing is rounded. ulp_T(y) <= ulp_T(ybound).
//   x' = 2^{y'} (1 + r), |r| <= E2 = 2^-23 (float), 2^-52 (double): the device exp2 of a double is within 1 ulp
//      (same table: exp2, maximum error 1 ulp), i.e. within 2^-52 relative, and rounding to float adds 2^-24.
// So x' / x <= 2^{delta + E1} (1 + E2) <= 2^{delta + E1 + 1.5 E2} = 1 + eps, because log2(1 + E2) <= E2 / ln 2
// < 1.5 E2: the upper side, which binds. The lower side, x' / x >= 2^{-(delta + E1)} (1 - E2) >= 1 / (1 + eps)
// >= 1 - eps, follows for eps < 1 (1 - E2 >= 2^{-1.5 E2}). E1 and E2 are derived margins, not measured ones; the
// smallest delta the container is trusted with (below) is MEASURED.
// The inverse clamps |x'| to [smallest normal, largest finite] of T: a valid |x| lies in that range, so the clamp
// moves x' towards x and keeps the bound.
// delta is evaluated in double and rounded DOWN: log2(1 + eps) is log1p(eps) / ln 2 shrunk by 2^-50 relative (more
// than the two roundings and the 1 ulp of log1p can add), and the result of the two subtractions is stepped down
// two doubles.
//
// THE ROUNDING OF THE CONTAINER. |y' - y| <= delta is the container's guarantee in exact arithmetic. It decomposes,
// quantizes, dequantizes and recomposes y in T, and that rounding is not in the derivation above: the round trip
// without a quantizer already moves y by 1 to 3 ulp_T(ybound), and at a delta of a few ulps the error EXCEEDS delta.
// There is no derivation of how much, so it was measured, on the CPU oracle (oracle.Hierarchy, which
// tests/test_gpu_parity.py pins the GPU transform to bit for bit; tests/pwrel_model.py: oracle_y_errors), on
// 2026-10-21: delta = m ulp_T(ybound) for every m in 1..64 and 72, 80, 96, 112, 128, 160, 192, 224, 256; float and
// double; an all-valid smooth field and an all-valid field of magnitudes 10^U(-30, 30) / 10^U(-300, 300); shapes
// 1000, 100001, 17x130, 513x513, 34x33x32, 65^3, 129^3, 5x6x7x9, 17^4, 5^5. excess = (max |y' - y| - delta) / ulp:
//   m* = 24    the smallest m from which no case has an excess > 0 at any larger probed m. The last breach is
//              double, 10^U, 5x6x7x9 at m = 23 (+6.25); the other cases stop between m = 1 (smooth 1-D, 2-D) and
//              m = 19 (5^5). The largest excess anywhere is +19 ulp (double, 10^U, 5x6x7x9, m = 1 and 3); float: +18.
//   e* = -2.0  the largest excess at any probed m >= m* (m = 27): not positive, so delta takes NO allowance for the
//              container's rounding (K_alloc = 0: delta stays log2(1 + eps) - E1 - 1.5 E2). At m = 64 it is -43.
//   K_min = 64 = 2 m* rounded up to a power of two; the factor 2 because the table is a sample, not a proof.
// tests/test_pwrel_rounding_cpu.py has the per-case table and repeats the measurement at the threshold. On the GPU
// (tests/test_gpu_pwrel.py) a container that quantizes gives the oracle's max |y' - y| to the bit, the breach at 1 and
// 2 ulps included; a container that would be larger than the array is stored as it is (y' = y), which at a delta of
// 64 ulps is every double field and every float field not smooth to about 12 bits -- the rough and tiny cases that
// set m* among them. The rule does not count on that: it bounds what the container may be asked for.
// REFUSALS. Where delta < kPwrelMinUlps ulp_T(ybound), or delta < 0.5 log2(1 + eps), the data type cannot carry
// eps at this field's dynamic range and the call is refused: a looser bound is never delivered silently. The first
// rule is the stricter one unless E1 < E2 / 42 (|y| below 1/32). Float: eps below about 3.5e-4 with 64 <= |y| < 128
// (6.9e-4 where the largest finite value puts |y| at 128; 5.5e-6 with 1 <= |y| < 2). Double: below about 5.2e-12
// with 512 <= |y| < 1024.
//
// A buffer:   [masked buffer of y, M bytes][flag record, S bytes][56-byte footer]
// The first M bytes are what mgh_compress_masked writes for y with the mask nonfinite | zeroed, restore_value 0 (its
// own first C bytes: an ordinary container of the filled y). The footer, little-endian, found from the END:
//   u64 M | u64 S | u64 n_flag | f64 eps | f64 abs_floor | u32 kind | u32 crc32(record) | u64 "MGHPWRL1"
// kind and the record's encoding are the mask record's (mask_plan.hpp): 0 the packed flag words, 1 their bytes in one
// record of the lossless stage where that is smaller, 2 no flag bit is set (S = 0).
// NOT BUILT: reduced-resolution, preview and progressive readers of such buffers; ladders, budgets, targets and
// layers; _multi and _dist; telling NaN from Inf, or -0.0 from +0.0.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>

#include "mask_plan.hpp"

namespace mgh {

constexpr uint64_t kPwrelMagic = 0x314c52575048474dull;  // "MGHPWRL1"
constexpr size_t kPwrelFooterBytes = 56;

// ---- classification ------------------------------------------------------------------------------------------
constexpr int kPwrelValid = 0, kPwrelZeroed = 1, kPwrelNonfinite = 2;

MGH_MASK_HD inline double pwrel_floor_eff(bool is_double, double abs_floor) {
  const double tiny = is_double ? 2.2250738585072014e-308 : 1.1754943508222875e-38;  // smallest normals
  return abs_floor > tiny ? abs_floor : tiny;
}

// x as a double (exact for both data types)
MGH_MASK_HD inline int pwrel_classify(double x, double floor_eff) {
  const double a = x < 0 ? -x : x;
  if (!(a <= 1.7976931348623157e308)) return kPwrelNonfinite;  // NaN, +-Inf
  return a < floor_eff ? kPwrelZeroed : kPwrelValid;
}

// ---- tolerance -----------------------------------------------------------------------------------------------
// the distance from |v| to the next larger number of T
inline double pwrel_ulp(bool is_double, double v) {
  v = std::fabs(v);
  if (is_double) return std::nextafter(v, std::numeric_limits<double>::infinity()) - v;
  const float f = (float)v;
  return (double)std::nextafter(f, std::numeric_limits<float>::infinity()) - (double)f;
}

inline double pwrel_e2(bool is_double) { return is_double ? 0x1p-52 : 0x1p-23; }

// K_min: the smallest delta handed to the container, in ulp_T(ybound) (measured: the header's comment)
constexpr double kPwrelMinUlps = 64.0;

// log2(1 + eps), not above the exact value
inline double pwrel_log2_1p(double eps) { return std::log1p(eps) / 0.6931471805599453 * (1.0 - 0x1p-50); }

// delta for a field whose valid elements have |y| <= ybound; ybound < 0: no valid element (delta = log2(1 + eps)).
// nullptr, or the refusal's message (MGH_ERR_INVALID_ARGUMENT).
inline const char *pwrel_abs_tolerance(bool is_double, double eps, double ybound, double *delta) {
  if (!std::isfinite(eps) || !(eps > 0.0 && eps < 1.0)) return "pwrel: eps must be finite with 0 < eps < 1";
  if (std::isnan(ybound) || std::isinf(ybound)) return "pwrel: ybound is not finite";
  const double L = pwrel_log2_1p(eps);
  if (ybound < 0) {
    *delta = L;
    return nullptr;
  }
  const double u = pwrel_ulp(is_double, ybound);
  double d = L - u - 1.5 * pwrel_e2(is_double);
  d = std::nextafter(std::nextafter(d, -std::numeric_limits<double>::infinity()), -std::numeric_limits<double>::infinity());
  if (d < kPwrelMinUlps * u || d < 0.5 * L)
    return "pwrel: the data type cannot carry this eps at the field's dynamic range (the rounding of log2|x| and of "
           "exp2 would take more than half of log2(1 + eps)): use a larger eps, or float64 data";
  *delta = d;
  return nullptr;
}

// ---- footer --------------------------------------------------------------------------------------------------
struct PwrelFooter {
  uint64_t masked = 0, record = 0, n_flag = 0;  // M, S, flag bits set
  double eps = 0, abs_floor = 0;
  uint32_t kind = kMaskNone, crc = 0;
};

inline uint64_t pwrel_double_bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return b;
}
inline double pwrel_bits_double(uint64_t b) {
  double v;
  std::memcpy(&v, &b, 8);
  return v;
}

inline void pwrel_footer_serialize(const PwrelFooter &f, uint8_t out[kPwrelFooterBytes]) {
  mask_put_le(out, f.masked, 8);
  mask_put_le(out + 8, f.record, 8);
  mask_put_le(out + 16, f.n_flag, 8);
  mask_put_le(out + 24, pwrel_double_bits(f.eps), 8);
  mask_put_le(out + 32, pwrel_double_bits(f.abs_floor), 8);
  mask_put_le(out + 40, f.kind, 4);
  mask_put_le(out + 44, f.crc, 4);
  mask_put_le(out + 48, kPwrelMagic, 8);
}

// tail: the LAST min(size, 56) bytes of a buffer of `size` bytes. Is it a pointwise-relative buffer's?
inline bool pwrel_footer_present(const uint8_t *tail, uint64_t size) {
  return size >= kPwrelFooterBytes && mask_get_le(tail + 48, 8) == kPwrelMagic;
}

// The footer of a buffer that has the magic, and what can be checked without the container's header.
inline const char *pwrel_footer_parse(const uint8_t *tail, uint64_t size, PwrelFooter &f) {
  if (!pwrel_footer_present(tail, size)) return "pwrel footer: no magic";
  f.masked = mask_get_le(tail, 8);
  f.record = mask_get_le(tail + 8, 8);
  f.n_flag = mask_get_le(tail + 16, 8);
  f.eps = pwrel_bits_double(mask_get_le(tail + 24, 8));
  f.abs_floor = pwrel_bits_double(mask_get_le(tail + 32, 8));
  f.kind = (uint32_t)mask_get_le(tail + 40, 4);
  f.crc = (uint32_t)mask_get_le(tail + 44, 4);
  const uint64_t body = size - kPwrelFooterBytes;
  if (f.masked > body || f.record != body - f.masked) return "pwrel footer: masked buffer + record + footer is not the buffer";
  if (f.masked < kMaskFooterBytes + 1) return "pwrel footer: no masked buffer";
  if (f.kind > kMaskNone) return "pwrel footer: unknown kind";
  if (f.kind == kMaskNone && (f.record != 0 || f.n_flag != 0)) return "pwrel footer: kind 2 with a record or flag bits";
  if (f.kind != kMaskNone && (f.record == 0 || f.n_flag == 0)) return "pwrel footer: a record kind without a record or flag bits";
  if (!std::isfinite(f.eps) || !(f.eps > 0.0 && f.eps < 1.0)) return "pwrel footer: eps outside (0, 1)";
  if (!std::isfinite(f.abs_floor) || f.abs_floor < 0.0) return "pwrel footer: abs_floor is negative or not finite";
  return nullptr;
}

// ... and what the header of the container adds: n, the elements of the array it holds.
inline const char *pwrel_footer_check_n(const PwrelFooter &f, uint64_t n) {
  if (f.n_flag > n) return "pwrel footer: more flag bits than the array has elements";
  if (f.kind == kMaskPacked && f.record != mask_packed_bytes(n)) return "pwrel footer: kind 0 record is not 8 ceil(n / 64) bytes";
  if (f.kind == kMaskCoded && f.record >= mask_packed_bytes(n)) return "pwrel footer: kind 1 record is not smaller than kind 0";
  return nullptr;
}

inline const char *pwrel_record_check_crc(const PwrelFooter &f, const uint8_t *record) {
  return fmt::crc32(record, (size_t)f.record) == f.crc ? nullptr : "pwrel flag record: CRC32 mismatch";
}

} // namespace mgh
