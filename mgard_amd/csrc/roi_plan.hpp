// Region of interest (mgh_compress_roi and its readers): a tighter POINTWISE bound inside boxes
// of an array, made in the spatial domain as a refinement of an ordinary container. This header holds the rules of the
// boxes, the tolerance of a box's residual with its derivation, and the table and footer of such a buffer. Host-only
// and free of HIP: a plain C++ compiler builds it and the CPU suite pins it (tests/test_roi_plan_cpu.py).
//
// THE SCHEME. x is compressed once at the base tolerance (C0, written by mgh_compress itself: byte for byte its
// container, up to the order of the outlier pairs, which differs between two mgh_compress calls too), decoded on
// the device (b), and for every box i the dense residual r_i = fl_T(x[box_i] - b[box_i]) is compressed on its own: ABS,
// s = inf, shape ext_i, no coordinates, at tolres_i. The reader decodes C0, decodes every r_i' and adds it into the
// box in place: x'' = fl_T(b + r_i'). The multilevel transform cannot give a local bound from locally finer
// quantisation -- the correction solves are global, coarse-region error leaks into the box -- so the bound is made
// here, where it is a statement about one element.
//
// THE BOUND. A = tol (ABS) or tol * norm of C0's header (REL), the rule of mgh_verify; A_i = tol_i times the same
// factor. With u(v) the distance from |v| to the next larger number of T, R_i = max |r_i| and M_i = max |x| over the box:
//   |x'' - x| <= |r_i' - r_i| + u(R_i) / 2 + u(M_i + A_i) / 2
// The first term is the residual container's guarantee, the second the rounding of the subtraction in the writer
// (|r_i| <= R_i, and a rounded result is within half the spacing of its binade), the third the rounding of the
// addition in the reader (|b + r_i'| <= |x| + A_i <= M_i + A_i). So
//   tolres_i = A_i - u(R_i) / 2 - u(M_i + A_i) / 2, evaluated in double and stepped down one double.
// u of a float argument is taken at the argument rounded UP to float, so it is never the finer binade's.
// REFUSALS (MGH_ERR_INVALID_ARGUMENT, a looser bound is never delivered silently): tolres_i < A_i / 2 -- the two
// roundings would take more than half of the bound -- or tolres_i < kPwrelMinUlps u(R_i): the smallest ABS, s = inf
// tolerance the container path holds on this arithmetic is 64 ulps of the largest magnitude it is given, MEASURED on
// the CPU oracle (pwrel_plan.hpp, "THE ROUNDING OF THE CONTAINER", has the measurement; it is reused here, not
// re-derived: the residual container is the same path with R_i in the place of ybound).
// R_i = 0: the base is exact in the box (x - b rounds to zero only where it is zero). Nothing is stored for the box:
// an empty record, size = 0, which the reader skips; tolres_i is recorded as A_i.
//
// A buffer:   [C0, C bytes][C_0] ... [C_{nbox-1}][box table, 120 nbox bytes][40-byte footer]
// A table entry, little-endian:
//   u64 lo[5] | u64 ext[5] (right-aligned, leading 0 / 1) | f64 tol_i | f64 tolres_i | u64 offset | u64 size |
//   u32 crc32(C_i) | u32 pad (0)
// offset: of C_i from the start of the buffer. The records lie back to back behind C0 in the order of the table.
// The footer, found from the END:
//   u64 C | u64 nbox | u64 table_bytes | u32 crc32(table) | u32 pad (0) | u64 "MGHROI01"
// The magic stands where the masked and the pointwise-relative footers have theirs (the last 8 bytes), so each of the
// three is "no footer" to the other two. The parser works on host copies whose length it is told, checks every size
// and offset against the buffer before it is used, and returns the message of an MGH_ERR_FORMAT, nullptr when all is
// well.
// NOT BUILT: masked or pointwise-relative arrays with boxes; overlapping boxes; boxes of previews and of reduced
// resolutions; decoding one box without decoding the base.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "pwrel_plan.hpp"

namespace mgh {

constexpr uint64_t kRoiMagic = 0x3130494f5248474dull;  // "MGHROI01"
constexpr size_t kRoiFooterBytes = 40;
constexpr size_t kRoiEntryBytes = 120;
constexpr int kRoiMaxBoxes = 16;
constexpr int kRoiMaxDim = 5;  // (MGH_MAX_DIM)

// A box: lo and ext right-aligned (leading 0 / 1), its tolerance, and what the writer adds.
struct RoiBox {
  uint64_t lo[kRoiMaxDim] = {0, 0, 0, 0, 0}, ext[kRoiMaxDim] = {1, 1, 1, 1, 1};
  double tol = 0, tolres = 0;
  uint64_t offset = 0, size = 0;
  uint32_t crc = 0;
};

struct RoiFooter {
  uint64_t container = 0, nbox = 0, table_bytes = 0;
  uint32_t crc = 0;
};

// ---- the boxes -----------------------------------------------------------------------------------------------
// lo, ext of D entries -> right-aligned
inline RoiBox roi_box(int D, const uint64_t *lo, const uint64_t *ext, double tol) {
  RoiBox b;
  for (int d = 0; d < D; d++) {
    b.lo[kRoiMaxDim - D + d] = lo[d];
    b.ext[kRoiMaxDim - D + d] = ext[d];
  }
  b.tol = tol;
  return b;
}

inline uint64_t roi_box_elems(const RoiBox &b) {
  uint64_t n = 1;
  for (int k = 0; k < kRoiMaxDim; k++) n *= b.ext[k];
  return n;
}

// Every rule of the call but the footprint. shape: D entries; boxes: right-aligned (roi_box). nullptr, or the
// refusal's message (MGH_ERR_INVALID_ARGUMENT).
inline const char *roi_check_boxes(int D, const uint64_t *shape, double tol, double s, int64_t nbox, const RoiBox *boxes) {
  if (D < 1 || D > kRoiMaxDim) return "compress_roi: D must be 1 .. 5";
  if (!(std::isinf(s) && s > 0))
    return "compress_roi: s must be infinite (any other s bounds a norm, not a point)";
  if (!std::isfinite(tol) || !(tol > 0)) return "compress_roi: tol must be positive and finite";
  uint64_t n = 1;
  for (int d = 0; d < D; d++) {
    if (shape[d] == 0 || shape[d] > 0xffffffffull || n * shape[d] > 0xffffffffull)
      return "compress_roi: the array must have 1 .. 2^32 - 1 elements";
    n *= shape[d];
  }
  if (nbox < 1 || nbox > kRoiMaxBoxes) return "compress_roi: nbox must be in 1 .. 16";
  const int k0 = kRoiMaxDim - D;
  for (int64_t i = 0; i < nbox; i++) {
    const RoiBox &b = boxes[i];
    for (int d = 0; d < D; d++) {
      if (b.lo[k0 + d] >= shape[d] || b.ext[k0 + d] > shape[d] - b.lo[k0 + d]) return "compress_roi: a box leaves the array";
      if (b.ext[k0 + d] < 3) return "compress_roi: every extent of a box must be at least 3 (the hierarchy's minimum)";
    }
    if (!(b.tol > 0) || !(b.tol < tol)) return "compress_roi: every box needs 0 < tol_i < tol";
  }
  for (int64_t i = 0; i < nbox; i++)
    for (int64_t j = i + 1; j < nbox; j++) {
      bool meet = true;
      for (int d = k0; d < kRoiMaxDim; d++)
        meet = meet && boxes[i].lo[d] < boxes[j].lo[d] + boxes[j].ext[d] && boxes[j].lo[d] < boxes[i].lo[d] + boxes[i].ext[d];
      if (meet) return "compress_roi: the boxes must be pairwise disjoint";
    }
  return nullptr;
}

// The array on the device (a host original's upload) and the decoded base b beside it.
inline const char *roi_check_footprint(uint64_t array_bytes, uint64_t max_memory_footprint) {
  if (array_bytes > max_memory_footprint / 2)
    return "compress_roi: the array and its decoded base do not fit max_memory_footprint (arrays with boxes are not "
           "streamed in parts)";
  return nullptr;
}

// ---- tolerance -----------------------------------------------------------------------------------------------
// the distance from |v| to the next larger number of T, |v| rounded up to T first
inline double roi_ulp(bool is_double, double v) {
  v = std::fabs(v);
  if (is_double) return std::nextafter(v, std::numeric_limits<double>::infinity()) - v;
  float f = (float)v;
  if ((double)f < v) f = std::nextafter(f, std::numeric_limits<float>::infinity());
  return (double)std::nextafter(f, std::numeric_limits<float>::infinity()) - (double)f;
}

// tolres of a box with absolute bound A, R = max |r| and M = max |x| over it. nullptr, or the refusal's message
// (MGH_ERR_INVALID_ARGUMENT). R = 0: nothing is stored, *tolres = A.
inline const char *roi_tolres(bool is_double, double A, double R, double M, double *tolres) {
  if (!std::isfinite(A) || !(A > 0)) return "roi: the box's absolute bound must be positive and finite";
  if (!std::isfinite(R) || R < 0 || !std::isfinite(M) || M < 0) return "roi: the box's statistics are not finite";
  if (R == 0) {
    *tolres = A;
    return nullptr;
  }
  const double uR = roi_ulp(is_double, R), uX = roi_ulp(is_double, M + A);
  double t = A - 0.5 * uR - 0.5 * uX;
  t = std::nextafter(t, -std::numeric_limits<double>::infinity());
  if (!(t >= 0.5 * A) || !(t >= kPwrelMinUlps * uR))
    return "roi: the data type cannot carry this tol_i at the box's magnitudes (the rounding of x - b and of b + r would "
           "take more than half of the bound, or the residual's tolerance falls below 64 ulps of the largest residual): "
           "use a larger tol_i, a tighter tol, or float64 data";
  *tolres = t;
  return nullptr;
}

// ---- table and footer ----------------------------------------------------------------------------------------
inline void roi_entry_serialize(const RoiBox &b, uint8_t out[kRoiEntryBytes]) {
  for (int k = 0; k < kRoiMaxDim; k++) {
    mask_put_le(out + 8 * k, b.lo[k], 8);
    mask_put_le(out + 40 + 8 * k, b.ext[k], 8);
  }
  mask_put_le(out + 80, pwrel_double_bits(b.tol), 8);
  mask_put_le(out + 88, pwrel_double_bits(b.tolres), 8);
  mask_put_le(out + 96, b.offset, 8);
  mask_put_le(out + 104, b.size, 8);
  mask_put_le(out + 112, b.crc, 4);
  mask_put_le(out + 116, 0, 4);
}

// table and footer behind `container` bytes of C0 and the records, whose offsets and sizes the boxes carry
inline std::vector<uint8_t> roi_trailer_serialize(uint64_t container, const std::vector<RoiBox> &boxes) {
  std::vector<uint8_t> out(boxes.size() * kRoiEntryBytes + kRoiFooterBytes);
  for (size_t i = 0; i < boxes.size(); i++) roi_entry_serialize(boxes[i], out.data() + i * kRoiEntryBytes);
  const size_t tb = boxes.size() * kRoiEntryBytes;
  uint8_t *f = out.data() + tb;
  mask_put_le(f, container, 8);
  mask_put_le(f + 8, boxes.size(), 8);
  mask_put_le(f + 16, tb, 8);
  mask_put_le(f + 24, fmt::crc32(out.data(), tb), 4);
  mask_put_le(f + 28, 0, 4);
  mask_put_le(f + 32, kRoiMagic, 8);
  return out;
}

// tail: the LAST min(size, 40) bytes of a buffer of `size` bytes. Is it a buffer with boxes?
inline bool roi_footer_present(const uint8_t *tail, uint64_t size) {
  return size >= kRoiFooterBytes && mask_get_le(tail + 32, 8) == kRoiMagic;
}

// The footer of a buffer that has the magic: where the table lies is known and inside the buffer afterwards.
inline const char *roi_footer_parse(const uint8_t *tail, uint64_t size, RoiFooter &f) {
  if (!roi_footer_present(tail, size)) return "roi footer: no magic";
  f.container = mask_get_le(tail, 8);
  f.nbox = mask_get_le(tail + 8, 8);
  f.table_bytes = mask_get_le(tail + 16, 8);
  f.crc = (uint32_t)mask_get_le(tail + 24, 4);
  if (mask_get_le(tail + 28, 4) != 0) return "roi footer: the padding is not zero";
  if (f.nbox < 1 || f.nbox > (uint64_t)kRoiMaxBoxes) return "roi footer: nbox outside 1 .. 16";
  if (f.table_bytes != f.nbox * kRoiEntryBytes) return "roi footer: the table is not 120 nbox bytes";
  const uint64_t body = size - kRoiFooterBytes;
  if (f.table_bytes > body) return "roi footer: the table is larger than the buffer";
  if (f.container == 0) return "roi footer: no container";
  if (f.container > body - f.table_bytes) return "roi footer: container + table + footer is larger than the buffer";
  return nullptr;
}

// The table (f.table_bytes bytes, which lie at size - 40 - f.table_bytes) of a buffer of `size` bytes.
inline const char *roi_table_parse(const RoiFooter &f, const uint8_t *table, uint64_t size, std::vector<RoiBox> &boxes) {
  if (fmt::crc32(table, (size_t)f.table_bytes) != f.crc) return "roi table: CRC32 mismatch";
  const uint64_t end = size - kRoiFooterBytes - f.table_bytes;  // the records are [container, end)
  boxes.assign((size_t)f.nbox, RoiBox());
  uint64_t at = f.container;
  for (size_t i = 0; i < boxes.size(); i++) {
    const uint8_t *e = table + i * kRoiEntryBytes;
    RoiBox &b = boxes[i];
    for (int k = 0; k < kRoiMaxDim; k++) {
      b.lo[k] = mask_get_le(e + 8 * k, 8);
      b.ext[k] = mask_get_le(e + 40 + 8 * k, 8);
      if (b.ext[k] == 0 || b.ext[k] > 0xffffffffull || b.lo[k] > 0xffffffffull) return "roi table: a box of no or of 2^32 elements";
    }
    b.tol = pwrel_bits_double(mask_get_le(e + 80, 8));
    b.tolres = pwrel_bits_double(mask_get_le(e + 88, 8));
    b.offset = mask_get_le(e + 96, 8);
    b.size = mask_get_le(e + 104, 8);
    b.crc = (uint32_t)mask_get_le(e + 112, 4);
    if (mask_get_le(e + 116, 4) != 0) return "roi table: the padding is not zero";
    if (!std::isfinite(b.tol) || !(b.tol > 0) || !std::isfinite(b.tolres) || !(b.tolres > 0)) return "roi table: a tolerance is not positive and finite";
    if (b.offset != at) return "roi table: the records do not lie back to back behind the container";
    if (b.size > end - at) return "roi table: a record leaves the buffer";
    at += b.size;
  }
  if (at != end) return "roi table: container + records + table + footer is not the buffer";
  return nullptr;
}

// ... and what the header of the container adds: the shape of the array (D entries).
inline const char *roi_table_check_shape(const std::vector<RoiBox> &boxes, int D, const uint64_t *shape) {
  if (D < 1 || D > kRoiMaxDim) return "roi table: dimension";
  const int k0 = kRoiMaxDim - D;
  for (const RoiBox &b : boxes) {
    for (int k = 0; k < k0; k++)
      if (b.lo[k] != 0 || b.ext[k] != 1) return "roi table: a box has more dimensions than the array";
    for (int d = 0; d < D; d++)
      if (b.lo[k0 + d] >= shape[d] || b.ext[k0 + d] > shape[d] - b.lo[k0 + d]) return "roi table: a box leaves the array";
  }
  return nullptr;
}

inline const char *roi_record_check_crc(const RoiBox &b, const uint8_t *record) {
  return fmt::crc32(record, (size_t)b.size) == b.crc ? nullptr : "roi record: CRC32 mismatch";
}

} // namespace mgh
