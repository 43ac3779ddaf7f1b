// The serialized Huffman record (huffman.hpp describes the format): where its members lie, what a
// reader may believe of one, which chunks and code units a prefix or a range of it needs, and which
// decoder takes it. Host-only and free of HIP, so that a plain C++ compiler builds it and the CPU
// suite pins it (tests/test_huffman_record_cpu.py) -- this is the code that reads bytes nobody vouches
// for. The parser works on host copies whose length it is told and never follows a pointer into the
// record's own (possibly device) memory; what is fetched, and when, is the caller's business
// (highlevel.hip: lossless_decompress). A refused record is MGH_ERR_FORMAT: the functions return the
// message, nullptr when all is well.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>

namespace mgh {

namespace huff {
// launch geometry the layout and the plan share with the kernels of huffman.hpp
constexpr int kSyncLanes = 64;  // synchronisation points per chunk = lanes of the decoder's wave
constexpr int kParWaves = 16;
constexpr int kParBatch = 32;  // symbols a lane decodes between two write-outs
constexpr int kEncRun = 40;      // symbols per thread the single-pass encoder keeps in registers (default chunk: 20480 = 40 x 512)
constexpr int kEncThreads = 512;  // threads of an encoder workgroup (two workgroups per CU with 32-bit code entries)
constexpr size_t kRingLdsCap = 150 * 1024;  // dynamic LDS a ring decoder's launch asks for at most
constexpr size_t kRingWaveLds = 8 * 64 * 8 + 64 * 17 * 2;  // of which per wave: code-unit ring + write-out staging (decode_ring_lds)
constexpr int kRingMinWaves = 8;  // waves of a ring decoder's workgroup when the table leaves no room for 16
} // namespace huff

// ---- offsets with natural alignment (Huffman.hpp:163-239) ---------------------------------------
inline size_t align_up(size_t off, size_t a) { return (off + a - 1) / a * a; }

struct PayloadLayout {
  size_t primary_count = 0, huffmeta = 0, decodebook_size = 0, decodebook = 0, ddata_size = 0,
         ddata = 0, outlier_count = 0, outlier_idx = 0, outliers = 0, total = 0;
  // Behind the reference's payload (its reader stops at the outlier lists), optional: the decoder's
  // synchronisation points (huffman.hpp: k_encode_chain), [u64 kSyncTag][u32 x 64 per chunk]. The
  // section's size is 8 (mod 16) while the outlier lists' is 0: a reader that knows the record's
  // size and where the lists start sees from the remainder whether it is there.
  size_t sync_tag = 0, sync = 0;
  static constexpr uint64_t kSyncTag = 0x31434e595348474dull;  // "MGHSYNC1"
  static size_t sync_bytes(size_t nchunk) { return 8 + 4 * (size_t)huff::kSyncLanes * nchunk; }
  // offsets of: primary_count, dict_size, chunk_size, huffmeta_size are fixed (0, 8, 12, 16)
  void compute(size_t nchunk, size_t dict, size_t units, size_t noutlier, bool with_sync = false) {
    size_t off = 0;
    primary_count = off; off += 8;
    off += 4;  // dict_size (int)
    off += 4;  // chunk_size (int)
    off = align_up(off, 8); off += 8;  // huffmeta_size
    huffmeta = off; off += 8 * 2 * nchunk;
    decodebook_size = off; off += 8;
    decodebook = off; off += 8 * (2 * 64) + 8 * dict;
    off = align_up(off, 8);
    ddata_size = off; off += 8;
    off = align_up(off, 8);
    ddata = off; off += 8 * units;
    outlier_count = off; off += 8;
    outlier_idx = off; off += 8 * noutlier;
    outliers = off; off += 8 * noutlier;
    sync_tag = sync = 0;
    if (with_sync) {
      sync_tag = off; off += 8;
      sync = off; off += 4 * (size_t)huff::kSyncLanes * nchunk;
    }
    total = off;
  }
};

// The single-pass encoder stages code table and symbols of a chunk in LDS.
inline bool lossless_sym16_ok(uint64_t dict, uint64_t chunk) {
  return dict <= 65536 && dict * 8 + chunk * 2 <= 140 * 1024;
}

// ---- reading a record ----------------------------------------------------------------------------
// What a decode call wants of the record; the defaults mean all of it.
// n_prefix < n: only the chunks that hold the first n_prefix integers. first > 0: the chunks in front
// of the one that holds integer `first` are left out as well. q_cap: elements the output holds (the
// record's own chunk length decides what is written; one that needs more is refused). n_prefix == 0:
// nothing is decoded.
struct DecodeRange {
  uint64_t n_prefix = ~(uint64_t)0, q_cap = ~(uint64_t)0, first = 0;
};

// MGH_HUFF_* developer switches as the caller read them (this header asks no environment)
struct DecodeSwitches {
  bool serial = false, par = false;  // MGH_HUFF_SERIAL_DECODE, MGH_HUFF_PAR_DECODE: cross-checks
  bool sync_decode = true;           // MGH_HUFF_SYNC_DECODE = 0: decode without the synchronisation points
  long pair = 1;                     // MGH_HUFF_PAIR (decode_plan)
  static constexpr long kNotSet = std::numeric_limits<long>::min();
  long tb = kNotSet;                 // MGH_HUFF_TB: bits of the decoders' first-level tables (any value is clamped)
};

struct RecordPlan {
  // record_fixed(): the fixed header, and the chunks [cf, ndec) a call decodes -- the output's first
  // element is integer cf * chunk, n_dec the integers in front of chunk ndec
  int32_t dict = 0, chunk = 0;
  size_t nchunk = 0;
  PayloadLayout L;  // (units and outliers taken as 0: the offsets up to ddata)
  size_t ndec = 0, cf = 0, n_dec = 0;
  size_t tb0 = 0, tb_cnt = 0;  // chunk-table entries on the device: those of the range, or the whole table
  // record_plan(): everything behind the chunk table
  uint64_t dbsize = 0, units = 0, ocount = 0;
  size_t o_oc = 0, o_oidx = 0, o_oval = 0, o_sync = 0;  // outlier count, lists, synchronisation entries (behind the tag)
  bool has_sync = false;
  size_t units_lo = 0, units_need = 0;  // code units [first one of chunk cf, end of chunk ndec - 1)
  int book_max_len = 0;                 // longest code of the decodebook
};

// code units of a chunk of `bits` bits (written so that no bit count wraps)
inline uint64_t chunk_units(uint64_t bits) { return bits / 64 + (bits % 64 != 0); }

// head[0 .. head_len): the leading bytes of a record of psize bytes, 24 of them unless the record
// is shorter. n: integers the record has to hold. keep: the whole chunk table goes to the device.
inline const char *record_fixed(const uint8_t *head, size_t head_len, uint64_t psize, uint64_t n,
                                const DecodeRange &r, bool keep, RecordPlan &R) {
  if (head_len < 24) return "Huffman record truncated";
  uint64_t primary = 0, huffmeta_size = 0;
  std::memcpy(&primary, head, 8);
  std::memcpy(&R.dict, head + 8, 4);
  std::memcpy(&R.chunk, head + 12, 4);
  std::memcpy(&huffmeta_size, head + 16, 8);
  if (primary != n || R.dict <= 0 || R.dict > 16384 || R.chunk <= 0 ||
      huffmeta_size != 2 * ((n - 1) / (uint64_t)R.chunk + 1))
    return "Huffman record: header does not match the subdomain";
  const uint64_t chunk = (uint64_t)R.chunk;
  R.nchunk = huffmeta_size / 2;
  R.ndec = r.n_prefix == 0 ? 0 : std::min<size_t>(R.nchunk, (size_t)((std::min<uint64_t>(r.n_prefix, n) - 1) / chunk + 1));
  R.cf = (size_t)(r.first / chunk);
  R.n_dec = (size_t)std::min<uint64_t>(n, (uint64_t)R.ndec * chunk);
  if (R.ndec && R.n_dec - R.cf * chunk > r.q_cap) return "Huffman record: chunk length does not match the header";
  R.tb0 = keep ? 0 : R.cf;
  R.tb_cnt = keep ? R.nchunk : R.ndec - R.cf;
  R.L.compute(R.nchunk, (size_t)R.dict, 0, 0);
  if (R.L.ddata > psize) return "Huffman record truncated";
  return nullptr;
}

// head[0 .. head_len): host copy of the record up to its code units (R.L.ddata bytes). host_rec: the
// whole record (psize bytes) where it lies in host memory, else nullptr -- then the outlier count
// follows from the record's size, and the tag of the synchronisation section is left to whoever can
// read it (highlevel.hip: k_record_pieces).
inline const char *record_plan(const uint8_t *head, size_t head_len, const uint8_t *host_rec, uint64_t psize,
                               const DecodeSwitches &sw, RecordPlan &R) {
  const PayloadLayout &L = R.L;
  if (head_len < L.ddata || psize < L.ddata) return "Huffman record truncated";
  std::memcpy(&R.dbsize, head + L.decodebook_size, 8);
  if (R.dbsize != 8 * 128 + 8 * (uint64_t)R.dict) return "Huffman record: decodebook size";
  std::memcpy(&R.units, head + L.ddata_size, 8);
  const uint64_t units = R.units;
  if (units > (psize - L.ddata) / 8) return "Huffman record truncated";
  R.o_oc = L.ddata + 8 * units;
  if (psize - R.o_oc < 8) return "Huffman record truncated";
  // Behind the outlier lists: nothing, or the synchronisation points of the decoder (PayloadLayout;
  // 8 mod 16 bytes where the lists are 0 mod 16).
  const size_t sync_bytes = PayloadLayout::sync_bytes(R.nchunk);
  const size_t rem = psize - R.o_oc - 8;
  R.has_sync = rem % 16 == 8 && rem >= sync_bytes;
  if (!host_rec) {
    // the record ends with the two outlier arrays (and that section): their length follows from
    // the record size (saves a synchronous 8-byte copy from the device)
    if (rem % 16 != 0 && !R.has_sync) return "Huffman record: outlier lists";
    R.ocount = (rem - (R.has_sync ? sync_bytes : 0)) / 16;
  } else {
    std::memcpy(&R.ocount, host_rec + R.o_oc, 8);
    if (R.has_sync && (R.ocount > (rem - sync_bytes) / 16 || rem - 16 * R.ocount != sync_bytes)) R.has_sync = false;
  }
  if (R.ocount > rem / 16) return "Huffman record truncated";
  R.o_oidx = R.o_oc + 8;
  R.o_oval = R.o_oidx + 8 * R.ocount;
  R.o_sync = R.o_oval + 8 * R.ocount + 8;
  if (R.has_sync && host_rec) {
    uint64_t tag = 0;
    std::memcpy(&tag, host_rec + R.o_sync - 8, 8);
    if (tag != PayloadLayout::kSyncTag) R.has_sync = false;
  }
  if (!sw.sync_decode) R.has_sync = false;
  // the chunk entries must stay inside the unit array (they index it in the decoder)
  uint64_t bits_k = 0, ent_k = 0;
  R.units_need = 0;
  R.units_lo = R.cf ? units : 0;
  for (size_t k = 0; k < R.nchunk; k++) {
    std::memcpy(&bits_k, head + L.huffmeta + 8 * k, 8);
    std::memcpy(&ent_k, head + L.huffmeta + 8 * (R.nchunk + k), 8);
    if (ent_k > units || chunk_units(bits_k) > units - ent_k) return "Huffman record: chunk outside the code stream";
    if (k < R.ndec) R.units_need = std::max<size_t>(R.units_need, ent_k + chunk_units(bits_k));
    if (R.cf && k >= R.cf && k < R.ndec) R.units_lo = std::min<size_t>(R.units_lo, ent_k);
  }
  if (R.ndec == R.nchunk) R.units_need = units;
  R.units_lo = std::min(R.units_lo, R.units_need);
  // (unused lengths carry first = 2^64-1)
  R.book_max_len = 0;
  for (int l = 1; l < 64; l++) {
    uint64_t first_l = 0;
    std::memcpy(&first_l, head + L.decodebook + 8 * l, 8);
    if (first_l != ~(uint64_t)0) R.book_max_len = l;
  }
  return nullptr;
}

// ---- choosing the decoder ------------------------------------------------------------------------
enum class DecodeKind { none, ring, par, serial };
struct DecodePlan {
  DecodeKind kind = DecodeKind::none;
  bool sync = false;  // ring: the launches read the record's synchronisation points
  bool pair = false;  // ring: k_decode_sync and its pair table instead of k_decode_ring
  int tb = 0;         // par, serial: bits of the prefix table
  int rtb = 0;        // ring: bits of the root table
  size_t lds = 0;     // par, serial: dynamic LDS (the ring decoder's follows from its table)
};

inline DecodePlan decode_plan(const RecordPlan &R, uint64_t n, const DecodeSwitches &sw) {
  DecodePlan D;
  const size_t chunk = (size_t)R.chunk, dict = (size_t)R.dict;
  // (the ring decoder keeps more than 32 bits in its bit buffer: codes of up to 32 bits)
  if (!sw.serial && !sw.par && chunk >= 1024 && chunk <= (1u << 24) && dict <= 65536 && R.book_max_len <= 32) {
    // parallel decoding inside the chunks: two-level table from the decodebook, code units through
    // per-lane LDS rings
    D.kind = DecodeKind::ring;
    D.rtb = (int)std::max<long>(8, std::min<long>(14, sw.tb != DecodeSwitches::kNotSet ? sw.tb : 12));
    D.sync = R.has_sync && chunk <= 65535;
    // Records with synchronisation points and SHORT codes: the decoder that takes two codes per
    // root-table slot where both fit its 12 bits (k_decode_sync). 512^3 f32, int64 output, same box:
    // 5.7 bits per symbol 0.79 against 0.85 ms with k_decode_ring's single-symbol steps; 7.4 bits 0.98
    // against 0.87, 9.1 bits (the benchmark's field at 1e-3) 0.97 against 0.79 -- pairs no longer fit
    // and the wider entries only cost. MGH_HUFF_PAIR: 0 never, 1 up to 6.5 bits per symbol (default),
    // 2 whenever the record has the points (cross-check).
    // The pair table's root alone is 8 << rtb bytes and has to fit beside the rings of the smallest workgroup:
    // 13 bits at most. MGH_HUFF_TB=14 decodes with single-symbol steps (its launch with pairs asked for
    // 178 KiB of LDS and failed).
    const bool pair_fits = ((size_t)8 << D.rtb) + huff::kRingMinWaves * huff::kRingWaveLds <= huff::kRingLdsCap;
    D.pair = D.sync && pair_fits && (sw.pair == 2 || (sw.pair == 1 && (double)R.units * 64.0 <= 6.5 * (double)n));
    return D;
  }
  if (R.ndec <= R.cf) return D;  // (nothing to decode)
  // prefix table as large as LDS allows next to the 16-bit keys (15 bits for dict = 8192)
  int tb = 15;
  const size_t lds_keys = (dict * 2 + 7) / 8 * 8 + 16 * 64 * 8;
  while (tb > 8 && ((size_t)4 << tb) + lds_keys > 154 * 1024) tb--;
  if (sw.tb != DecodeSwitches::kNotSet) tb = (int)std::max<long>(8, std::min<long>(tb, sw.tb));
  if (!sw.serial && chunk >= 1024) {
    // parallel decoding inside the chunks (one wave per chunk): 14-bit prefix table at most, so that
    // the write-out staging (4 KiB per wave) fits beside it
    const size_t lds_par = (dict + 3) / 4 * 8 + (size_t)huff::kParWaves * 64 * huff::kParBatch * 2;
    while (tb > 8 && ((size_t)4 << tb) + lds_par > 150 * 1024) tb--;
    D.kind = DecodeKind::par;
    D.lds = ((size_t)4 << tb) + lds_par;
  } else {
    D.kind = DecodeKind::serial;
    D.lds = ((size_t)4 << tb) + lds_keys;
  }
  D.tb = tb;
  return D;
}

// A caller whose output holds 16-bit symbols can be served by the ring decoder alone (k_decode_ring and
// k_decode_sync have a uint16_t instantiation; the cross-check decoders write int64 values): what such
// a caller is told about any other plan, nullptr when the plan is the ring decoder's.
inline const char *sym16_refusal(const DecodePlan &D) {
  return D.kind == DecodeKind::ring ? nullptr : "lossless: 16-bit symbols need the ring decoder for this record";
}

// A record whose code units arrive in pieces: with units [0, have) of the record on the device (all
// the call needs, on the last piece), chunks [c_done, return value) can be decoded -- a chunk counts
// when its units and the one unit the decoder peeks at behind them have landed.
inline size_t chunks_landed(const RecordPlan &R, const uint64_t *h_bits, const uint64_t *h_ent, size_t c_done,
                            uint64_t have, bool last_piece) {
  if (last_piece) return R.ndec;
  size_t c_hi = c_done;
  while (c_hi < R.ndec && h_ent[c_hi] + chunk_units(h_bits[c_hi]) + 1 <= have) c_hi++;
  return c_hi;
}

} // namespace mgh
