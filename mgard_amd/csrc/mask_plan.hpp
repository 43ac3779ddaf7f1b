// Missing-value masks (mgh_mask_*, mgh_compress_masked): the trailer behind the
// container of a masked array, the choice of the mask record's kind, the constant of an all-masked
// segment and the segment geometry of the fill. Host-only and free of HIP: a plain C++ compiler builds
// it and the CPU suite pins it (tests/test_mask_plan_cpu.py); the kernels of kernels_mask.hpp use the
// geometry through MGH_MASK_HD.
//
// A masked buffer:   [ordinary container, C bytes][mask record, R bytes][48-byte footer]
// The footer, little-endian, is found from the END of the buffer:
//   u64 C | u64 R | u64 n_masked | u64 restore_bits | u32 kind | u32 crc32(record) | u64 "MGHMASK1"
// restore_bits: the bits of (T)restore_value, zero-extended. kind:
//   0  the packed mask as it is: ceil(n / 64) u64, bit i % 64 of word i / 64 set when flat element i is
//      masked, the unused high bits of the last word zero. R = 8 ceil(n / 64).
//   1  the bytes of those words as 16-bit symbols of dictionary 256 in one record of the lossless stage
//      (Huffman, or Huffman_Zstd, as the container's header says). Stored only where smaller than kind 0.
//   2  no element is masked. R = 0.
// The parser works on host copies whose length it is told. A refusal is MGH_ERR_FORMAT: the functions
// return the message, nullptr when all is well.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "format.hpp"
#include "huffman_record.hpp"

#ifdef __HIPCC__
#define MGH_MASK_HD __host__ __device__
#else
#define MGH_MASK_HD
#endif

namespace mgh {

constexpr uint64_t kMaskMagic = 0x314b53414d48474dull;  // "MGHMASK1"
constexpr size_t kMaskFooterBytes = 48;
constexpr uint32_t kMaskPacked = 0, kMaskCoded = 1, kMaskNone = 2;
constexpr uint64_t kMaskDict = 256;  // a byte of the packed mask is a symbol

struct MaskFooter {
  uint64_t container = 0, record = 0, n_masked = 0, restore_bits = 0;
  uint32_t kind = kMaskNone, crc = 0;
};

inline uint64_t mask_words(uint64_t n) { return (n + 63) / 64; }
inline uint64_t mask_packed_bytes(uint64_t n) { return 8 * mask_words(n); }

inline void mask_put_le(uint8_t *p, uint64_t v, int bytes) {
  for (int i = 0; i < bytes; i++) p[i] = (uint8_t)(v >> (8 * i));
}
inline uint64_t mask_get_le(const uint8_t *p, int bytes) {
  uint64_t v = 0;
  for (int i = 0; i < bytes; i++) v |= (uint64_t)p[i] << (8 * i);
  return v;
}

inline void mask_footer_serialize(const MaskFooter &f, uint8_t out[kMaskFooterBytes]) {
  mask_put_le(out, f.container, 8);
  mask_put_le(out + 8, f.record, 8);
  mask_put_le(out + 16, f.n_masked, 8);
  mask_put_le(out + 24, f.restore_bits, 8);
  mask_put_le(out + 32, f.kind, 4);
  mask_put_le(out + 36, f.crc, 4);
  mask_put_le(out + 40, kMaskMagic, 8);
}

// tail: the LAST min(size, 48) bytes of a buffer of `size` bytes. Is it a masked buffer's?
inline bool mask_footer_present(const uint8_t *tail, uint64_t size) {
  return size >= kMaskFooterBytes && mask_get_le(tail + 40, 8) == kMaskMagic;
}

// The footer of a buffer that has the magic, and what can be checked without the container's header.
inline const char *mask_footer_parse(const uint8_t *tail, uint64_t size, MaskFooter &f) {
  if (!mask_footer_present(tail, size)) return "mask footer: no magic";
  f.container = mask_get_le(tail, 8);
  f.record = mask_get_le(tail + 8, 8);
  f.n_masked = mask_get_le(tail + 16, 8);
  f.restore_bits = mask_get_le(tail + 24, 8);
  f.kind = (uint32_t)mask_get_le(tail + 32, 4);
  f.crc = (uint32_t)mask_get_le(tail + 36, 4);
  const uint64_t body = size - kMaskFooterBytes;
  if (f.container > body || f.record != body - f.container) return "mask footer: container + record + footer is not the buffer";
  if (f.container == 0) return "mask footer: no container";
  if (f.kind > kMaskNone) return "mask footer: unknown kind";
  if (f.kind == kMaskNone && (f.record != 0 || f.n_masked != 0)) return "mask footer: kind 2 with a record or masked elements";
  if (f.kind != kMaskNone && (f.record == 0 || f.n_masked == 0)) return "mask footer: a record kind without a record or masked elements";
  return nullptr;
}

// ... and what the header of the container adds: n, the elements of the array it holds.
inline const char *mask_footer_check_n(const MaskFooter &f, uint64_t n, bool is_double) {
  if (f.n_masked > n) return "mask footer: more masked elements than the array has";
  if (f.kind == kMaskPacked && f.record != mask_packed_bytes(n)) return "mask footer: kind 0 record is not 8 ceil(n / 64) bytes";
  if (f.kind == kMaskCoded && f.record >= mask_packed_bytes(n)) return "mask footer: kind 1 record is not smaller than kind 0";
  if (!is_double && (f.restore_bits >> 32)) return "mask footer: restore bits wider than the data type";
  return nullptr;
}

inline const char *mask_record_check_crc(const MaskFooter &f, const uint8_t *record) {
  return fmt::crc32(record, (size_t)f.record) == f.crc ? nullptr : "mask record: CRC32 mismatch";
}

// Can the lossless stage code the mask's bytes as 16-bit symbols with this chunk (the single-pass encoder)?
inline bool mask_record_codable(uint64_t chunk) {
  return chunk >= 1 && chunk <= ((uint64_t)1 << 24) && lossless_sym16_ok(kMaskDict, chunk);
}

// The kind the writer stores: coded only where that is smaller. coded_bytes: the lossless record's size, 0 when
// there is none (not codable, or the encoder gave up).
inline uint32_t mask_record_kind(uint64_t n, uint64_t n_masked, uint64_t coded_bytes) {
  if (n_masked == 0) return kMaskNone;
  return coded_bytes != 0 && coded_bytes < mask_packed_bytes(n) ? kMaskCoded : kMaskPacked;
}

// The value of a masked element whose segment has no valid element: midway between the extremes of the valid
// elements, in double (two exact halvings and one rounding: nothing a contraction could change). 0 for an
// all-masked array, whose vmin = vmax = 0.
inline double mask_fill_constant(double vmin, double vmax) { return 0.5 * vmin + 0.5 * vmax; }

// The bits of (T)value, zero-extended, and back (a float NaN keeps its payload through both casts).
inline uint64_t mask_value_bits(bool is_double, double value) {
  if (is_double) {
    uint64_t b;
    std::memcpy(&b, &value, 8);
    return b;
  }
  const float v = (float)value;
  uint32_t b;
  std::memcpy(&b, &v, 4);
  return b;
}
inline double mask_bits_value(bool is_double, uint64_t bits) {
  if (is_double) {
    double v;
    std::memcpy(&v, &bits, 8);
    return v;
  }
  const uint32_t b = (uint32_t)bits;
  float v;
  std::memcpy(&v, &b, 4);
  return (double)v;
}

// ---- segment geometry of the fill -------------------------------------------------------------------------
// Rows run along the last (fastest) dimension, of length nf; every row is cut into segments
// [k 1024, min((k + 1) 1024, nf)), restarting at every row. A segment is filled from itself alone.
constexpr uint64_t kMaskSegment = 1024;
constexpr int kMaskSegmentWords = (int)(kMaskSegment / 64);  // aligned 64-bit words of a segment; it touches one more of the array's

struct MaskSegments {
  uint64_t nf = 0, rows = 0, per_row = 0, total = 0;
};

inline MaskSegments mask_segments(int D, const uint64_t *shape) {
  MaskSegments g;
  g.nf = shape[D - 1];
  g.rows = 1;
  for (int d = 0; d + 1 < D; d++) g.rows *= shape[d];
  g.per_row = (g.nf + kMaskSegment - 1) / kMaskSegment;
  g.total = g.rows * g.per_row;
  return g;
}

// Segment `seg` (row-major: row, then position in the row): flat index of its first element and its length.
MGH_MASK_HD inline void mask_segment(const MaskSegments &g, uint64_t seg, uint64_t &start, uint64_t &len) {
  const uint64_t row = seg / g.per_row, k = seg % g.per_row;
  start = row * g.nf + k * kMaskSegment;
  len = g.nf - k * kMaskSegment < kMaskSegment ? g.nf - k * kMaskSegment : kMaskSegment;
}

// Where the segment lies in the packed words: its first word, the bit of that word its first element has, and
// the words it touches (at most 17: a segment need not start on a word when nf % 64 != 0).
MGH_MASK_HD inline void mask_segment_words(uint64_t start, uint64_t len, uint64_t &first_word, int &shift, int &nwords) {
  first_word = start >> 6;
  shift = (int)(start & 63);
  nwords = (int)(((uint64_t)shift + len + 63) / 64);
}

// ---- sampling a packed mask (mgh_mask_sample_) ---------------------------------------------------------------
// Output element e of a dense array of `out_shape` is set when the element of the source array at the
// coordinates (idx_0[i_0], ..., idx_{D-1}[i_{D-1}]) is set: a level or coarsened grid through its node lists, a
// window through lo + i. Every count here is below 2^32 (the limit of the mgh_mask_* calls), so the arithmetic
// is 32-bit; the kernel (kernels_mask.hpp: k_mask_sample) and tests/cpp/mask_sample_dump.cpp share it.
constexpr int kMaskMaxDim = 5;  // (MGH_MAX_DIM)

// coordinates of flat element e of a dense row-major array of `ext`
MGH_MASK_HD inline void mask_unravel(int D, const uint32_t *ext, uint32_t e, uint32_t *coord) {
  for (int d = D - 1; d > 0; d--) {
    const uint32_t q = e / ext[d];
    coord[d] = e - q * ext[d];
    e = q;
  }
  coord[0] = e;
}

// flat index of `coord` in a dense row-major array of `shape`; false (and nothing to read) when a coordinate
// lies outside it
MGH_MASK_HD inline bool mask_flat_index(int D, const uint32_t *shape, const uint32_t *coord, uint64_t &flat) {
  uint64_t f = 0;
  bool inside = true;
  for (int d = 0; d < D; d++) {
    inside = inside && coord[d] < shape[d];
    f = f * shape[d] + coord[d];
  }
  flat = f;
  return inside;
}

// the source bit of output element e: lists[d] == nullptr is the identity list
MGH_MASK_HD inline bool mask_sample_source(int D, const uint32_t *shape, const uint32_t *out_shape,
                                           const uint32_t *const *lists, uint32_t e, uint64_t &flat) {
  uint32_t c[kMaskMaxDim];
  mask_unravel(D, out_shape, e, c);
  for (int d = 0; d < D; d++)
    if (lists[d]) c[d] = lists[d][c[d]];
  return mask_flat_index(D, shape, c, flat);
}

// ---- the same source bit, walked by rows (mgh_pwrel_inverse_sampled_) ------------------------------------------
// A row of the dense output runs along its last (fastest) dimension: out_shape[D - 1] elements, and
// prod(out_shape[0 .. D - 2]) rows. The row is unravelled ONCE -- the only divisions -- into the part of the flat
// source index its slow coordinates give, already multiplied by shape[D - 1]; an element of the row then costs one
// list entry, one comparison and one addition. The kernel k_pwrel_inverse_sampled (kernels_pwrel.hpp) and
// tests/cpp/mask_row_walk_dump.cpp share it; the CPU suite holds it against mask_sample_source.
struct MaskRow {
  uint64_t base = 0;    // flat source index of the row's element with source coordinate 0 in the last dimension
  bool inside = false;  // every slow coordinate lies inside the source
};

MGH_MASK_HD inline uint32_t mask_row_count(int D, const uint32_t *out_shape) {
  uint32_t rows = 1;
  for (int d = 0; d + 1 < D; d++) rows *= out_shape[d];
  return rows;
}

MGH_MASK_HD inline MaskRow mask_row_begin(int D, const uint32_t *shape, const uint32_t *out_shape,
                                          const uint32_t *const *lists, uint32_t row) {
  MaskRow r;
  uint32_t c[kMaskMaxDim];
  c[0] = 0;  // (D == 1: the one row has no slow coordinate)
  for (int d = D - 2; d > 0; d--) {
    const uint32_t q = row / out_shape[d];
    c[d] = row - q * out_shape[d];
    row = q;
  }
  if (D > 1) c[0] = row;
  r.inside = true;
  for (int d = 0; d + 1 < D; d++) {
    const uint32_t s = lists[d] ? lists[d][c[d]] : c[d];
    r.inside = r.inside && s < shape[d];
    r.base = r.base * shape[d] + s;
  }
  r.base *= shape[D - 1];
  return r;
}

// the source bit of element j of that row: false (and nothing to read) when a coordinate lies outside the source
MGH_MASK_HD inline bool mask_row_source(const MaskRow &r, uint32_t shape_last, const uint32_t *list_last, uint32_t j,
                                        uint64_t &flat) {
  const uint32_t s = list_last ? list_last[j] : j;
  flat = r.base + s;
  return r.inside && s < shape_last;
}

} // namespace mgh
