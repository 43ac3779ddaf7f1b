// What a tolerance will cost in bytes, from the histogram of its symbols alone, and the search for
// the tolerance of a byte budget (mgh_estimate_sizes, mgh_compress_budget).
// Host-only and free of HIP: a plain C++ compiler builds it and the CPU suite pins it
// (tests/test_size_plan_cpu.py).
//
// A Huffman record's size is PayloadLayout::total, a function of the chunk count, the dictionary, the
// outlier count and the number of 64-bit code units. The units are the sum over the chunks of
// chunk_units(bits of the chunk): the histogram gives the sum of the bits (Codebook::total_bits) but
// not how they fall into chunks, and every chunk rounds up to a whole unit on its own. Hence
//   ceil(total_bits / 64)  <=  units  <=  floor(total_bits / 64) + nchunk
// (each chunk adds at most one unit to its bits / 64, and the fractions that make a chunk round up
// sum to less than nchunk), and a bracket of the record that is at most 8 bytes a chunk wide.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/mgard_hip_compress.h"
#include "huffman_record.hpp"

namespace mgh {

// The record carries the decoder's synchronisation points (PayloadLayout): with the single-pass
// encoder, chunks of the size it keeps in registers, and streams of 4 bits per symbol or more
// -- 256 bytes per chunk are 1.1 % of a chunk of 20 480 nine-bit codes, and the short codes of
// a low-entropy stream re-synchronise within a symbol or two anyway. sync_env: MGH_HUFF_SYNC (0: never).
inline bool record_has_sync(int lossless, uint64_t dict, uint64_t chunk, uint64_t total_bits, uint64_t n,
                            long sync_env) {
  return lossless == MGH_LOSSLESS_HUFFMAN && lossless_sym16_ok(dict, chunk) && chunk >= 1024 &&
         chunk <= (uint64_t)huff::kEncRun * huff::kEncThreads && sync_env != 0 && total_bits >= 4 * n;
}

struct ByteBracket {
  uint64_t min = 0, max = 0;
};

inline uint64_t record_chunks(uint64_t n, uint64_t chunk) { return (n - 1) / chunk + 1; }

// Bytes of the record of n symbols whose codes take total_bits bits: PayloadLayout::total at the
// two ends of the unit count. max - min <= 8 * nchunk.
inline ByteBracket record_bytes_bracket(uint64_t n, uint64_t dict, uint64_t chunk, uint64_t total_bits,
                                        uint64_t noutlier, bool with_sync) {
  const uint64_t nchunk = record_chunks(n, chunk);
  PayloadLayout L;
  ByteBracket b;
  L.compute((size_t)nchunk, (size_t)dict, (size_t)chunk_units(total_bits), (size_t)noutlier, with_sync);
  b.min = L.total;
  L.compute((size_t)nchunk, (size_t)dict, (size_t)(total_bits / 64 + nchunk), (size_t)noutlier, with_sync);
  b.max = L.total;
  return b;
}

// Bytes of the container of ONE subdomain: header, the record's size prefix, and the record -- or
// the subdomain itself where the record is not smaller. raw: 1 both ends of the bracket are raw, 0
// neither is, -1 they disagree. (A record of exactly n * elem bytes counts as raw, as a reader takes a
// record of that size -- GPUPipelines.hpp:414-417; the bytes are the same either way.)
struct ContainerBracket {
  uint64_t min = 0, max = 0;
  int raw = 0;
};
inline ContainerBracket container_bytes_bracket(uint64_t metadata_bytes, uint64_t n, uint64_t elem,
                                                const ByteBracket &record) {
  const uint64_t dense = n * elem;
  ContainerBracket c;
  c.min = metadata_bytes + 8 + std::min(record.min, dense);
  c.max = metadata_bytes + 8 + std::min(record.max, dense);
  const bool raw_lo = record.min >= dense, raw_hi = record.max >= dense;
  c.raw = raw_lo && raw_hi ? 1 : !raw_lo && !raw_hi ? 0 : -1;
  return c;
}

// ---- histogram launches ----------------------------------------------------------------------------
// k_quantize_histograms keeps one histogram of `dict` 32-bit counters per tolerance in LDS: as many
// tolerances per launch as 128 KB hold (dict = 16384: two, 8192: four), never more than 8 (the
// kernel keeps an outlier counter per tolerance in registers).
constexpr uint64_t kQhistLdsBytes = 128 * 1024;
constexpr int kQhistMaxPerLaunch = 8;
constexpr int kQhistMaxTols = 64;
// what mgh_quantize_histograms refuses (nullptr: nothing). The counters are 32-bit like huff::k_histogram's.
inline const char *qhist_refusal(uint64_t total, int ntol, uint64_t dict) {
  if (total == 0 || total >= ((uint64_t)1 << 32)) return "quantize_histograms: 1 .. 2^32 - 1 elements (32-bit counters)";
  if (ntol < 1 || ntol > kQhistMaxTols) return "quantize_histograms: ntol must be in 1..64";
  if (dict < 2 || dict > 16384) return "quantize_histograms: dict_size must be in 2..16384";
  return nullptr;
}
inline int qhist_per_launch(uint64_t dict, int k_left) {
  const uint64_t fit = dict ? kQhistLdsBytes / (4 * dict) : 0;
  return (int)std::min<uint64_t>({(uint64_t)std::max(k_left, 0), fit, (uint64_t)kQhistMaxPerLaunch});
}

// k_quantize_symbols keeps one histogram in LDS, 64 KB at the largest dictionary; the symbols are 16 bits
// wide and the dictionary is centred on dict / 2, so an odd one is refused. (nullptr: nothing refused)
constexpr uint64_t kQsymLdsBytes = 64 * 1024;
inline const char *qsym_refusal(uint64_t total, uint64_t dict) {
  if (total == 0 || total >= ((uint64_t)1 << 32)) return "quantize_symbols: 1 .. 2^32 - 1 elements (32-bit index arithmetic and counters)";
  if (dict < 2 || dict > 16384 || (dict & 1)) return "quantize_symbols: dict_size must be even and in 2..16384";
  return nullptr;
}

// ---- the search ------------------------------------------------------------------------------------
// The largest accuracy (smallest tolerance) in [tol_min, tol_max] that fits, on a logarithmic grid:
// tol_min if it fits; else a bracket [a, b], a does not fit, b fits, narrowed `rounds` times to a
// quarter (in log) by its three log-quartiles, which the caller prices in one pass (`fits3`). Every
// candidate is a product of two square roots of earlier candidates: sqrt and one multiply are exact
// IEEE operations, so any restatement in double precision walks the same values. b always fits, so a
// size curve that is not monotone costs accuracy at worst, never the budget.
enum class SearchEnd { found, nothing_fits, bad_argument };
struct SearchResult {
  SearchEnd end = SearchEnd::bad_argument;
  double tol = 0;   // found: the tolerance to use (it fits)
  double finer = 0; // found after rounds: the next finer candidate of the last round (it does not fit); else 0
  int index = -1;   // found: what `tol` was -- 0 tol_min, 1 tol_max, 2 + k: candidate m(k+1) of the last round that moved b
};
inline void log_quartiles(double a, double b, double m[3]) {
  m[1] = std::sqrt(a) * std::sqrt(b);
  m[0] = std::sqrt(a) * std::sqrt(m[1]);
  m[2] = std::sqrt(m[1]) * std::sqrt(b);
}
// fits1(tol) -> bool; fits3(const double m[3], bool out[3])
template <typename Fits1, typename Fits3>
SearchResult budget_search(double tol_min, double tol_max, int rounds, Fits1 &&fits1, Fits3 &&fits3) {
  SearchResult r;
  if (!(tol_min > 0) || !(tol_min <= tol_max) || !std::isfinite(tol_max) || rounds < 1 || rounds > 8) return r;
  if (fits1(tol_min)) {
    r.end = SearchEnd::found;
    r.tol = tol_min;
    r.index = 0;
    return r;
  }
  if (!fits1(tol_max)) {
    r.end = SearchEnd::nothing_fits;
    return r;
  }
  double a = tol_min, b = tol_max;
  r.index = 1;
  r.finer = a;
  for (int round = 0; round < rounds; round++) {
    double m[3];
    bool ok[3] = {false, false, false};
    log_quartiles(a, b, m);
    fits3(m, ok);
    // b: the smallest of m1 < m2 < m3 < b that fits, a: its predecessor
    int k = 0;
    while (k < 3 && !ok[k]) k++;
    if (k < 3) {
      b = m[k];
      r.index = 2 + k;
    }
    if (k > 0) a = m[k - 1];
    r.finer = a;
  }
  r.end = SearchEnd::found;
  r.tol = b;
  return r;
}
template <typename Fits1> SearchResult budget_search(double tol_min, double tol_max, int rounds, Fits1 &&fits1) {
  return budget_search(tol_min, tol_max, rounds, fits1, [&](const double m[3], bool ok[3]) {
    for (int k = 0; k < 3; k++) ok[k] = fits1(m[k]);
  });
}

}  // namespace mgh
