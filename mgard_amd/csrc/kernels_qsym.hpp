// A coefficient array to what the lossless stage reads, in one pass (mgh_quantize_symbols; the second
// entry into the high-level writer): 16-bit symbols, the outlier list and,
// optionally, the histogram of the symbols. And the two kernels of the precision layers (DESIGN.md
// sections 4 and 8), where tier k of a layer set stores the quantized residual the tiers before it left in
// the COEFFICIENTS: that quantizer with one more output (writer, mgh_quantize_symbols_residual) and the
// dequantizer that adds to what is there (reader, mgh_dequantize_add).
//
// For every element the symbol kernels compute what k_quantize computes with prep_huffman = 1 --
// quantize_one() itself with the level's reciprocal quantizer and the level's volume, plus dict / 2 --
// and store it as uint16_t when it lies in [0, dict); else they store symbol 0 and append (linear
// index, that int64) to the outlier list, as k_quantize does (append_outliers, kernels_qwalk.hpp).
//
// HIST: the stored symbols are counted in bins privatised in LDS (dict <= 16384: 64 KB); a workgroup
// ends with one global atomic per used bin, like huff::k_histogram, which this replaces. An outlier
// counts in bin 0, the symbol stored for it. The centre symbol dict / 2 -- most of a smooth field --
// is counted in a register and reaches its bin once per wave.
//
// RES (k_quantize_symbols_residual): in addition, per element,
//     r_out = r - (qz[level] * vol_d[level]) * (T)q
// with q the exact int64 BEFORE the dictionary shift (for an outlier: the value that travels through the
// list, never the symbol 0 stored in its place) and the subtrahend k_dequantize's own expression on
// k_dequantize's own two tables: four tables in LDS (QTab) instead of the quantizer's two. Multiply,
// multiply and subtract are three IEEE operations (the build has -ffp-contract=off). A thread reads its
// vector before it writes it and no thread touches another's, so r_out == v (in place) is allowed; the
// two pointers are therefore not __restrict__.
//
// The walk is the level cursor's (kernels_qwalk.hpp) over groups of one 16-byte vector. A group is loaded
// as one vector where the pointer is 16-byte aligned and the group is whole, element by element otherwise
// (a misaligned view, the tail); its symbols leave as one plain vector store (8 bytes per 4 floats), and
// its residuals as one, on the same terms.
//
// k_dequantize_add is k_dequantize on int64 integers whose outliers are written back already
// (k_outlier_restore), as a pure stream (stream_levels) with its two tables in LDS. FIRST stores
// k_dequantize's value (it is not added to zero: -0.0 stays -0.0); otherwise acc = acc + that value, one
// IEEE add. 8 + esz bytes read (2 esz with the accumulator) and esz written per element, no atomics.
//
// The same two for the layers in LEVEL ORDER (reorder = 1 records; further down): k_quantize_residual_int64,
// the symbol body with int64 output for the writer, and k_dequantize_add_linear, the reader's stream over a
// window of the level-linearised array.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_qwalk.hpp"

namespace mgh {

constexpr int kQsThreads = 256;

template <typename T, bool HIST, bool RES, typename SYM = uint16_t>
__device__ __forceinline__ void quantize_symbols_body(const QuantMeta &m, size_t total, const T *v,
                                                      const int *__restrict__ marks, const T *__restrict__ tab, int nlev,
                                                      int dict, SYM *__restrict__ sym, unsigned *__restrict__ freq,
                                                      unsigned long long *outlier_count, uint64_t *__restrict__ outlier_idx,
                                                      int64_t *__restrict__ outlier_val, unsigned long long outlier_cap,
                                                      T *r_out /* RES only */) {
  extern __shared__ unsigned qs_bins[];  // [dict], HIST only
  __shared__ T s_tab[RES ? 4 : 2][kMaxLevels];
  if (HIST)
    for (int i = threadIdx.x; i < dict; i += kQsThreads) qs_bins[i] = 0;
  stage_tables<kQsThreads>(tab, nlev, s_tab);
  __syncthreads();

  const int64_t half = (int64_t)dict / 2;
  constexpr int VN = Vec16<T>::N;
  typedef T NV __attribute__((ext_vector_type(VN)));
  typedef SYM SV __attribute__((ext_vector_type(VN)));
  const bool vec_in = aligned16(v);
  const bool vec_out = (reinterpret_cast<uintptr_t>(sym) & (sizeof(SV) - 1)) == 0;
  const bool vec_res = RES && aligned16(r_out);
  const size_t ngroup = (total + VN - 1) / VN;
  LevelCursor cur(m, marks);
  unsigned centre = 0;  // HIST: symbols dict / 2 this thread has seen
  // (uniform trip count per workgroup: the barriers of append_outliers are reached by every thread)
  const size_t stride = (size_t)gridDim.x * kQsThreads;
  for (size_t gb = (size_t)blockIdx.x * kQsThreads; gb < ngroup; gb += stride) {
    const size_t g = gb + threadIdx.x;
    const size_t lin0 = g * VN;
    const int cnt = g < ngroup ? (int)(total - lin0 < (size_t)VN ? total - lin0 : (size_t)VN) : 0;
    const bool whole = cnt == VN;
    NV x;
#pragma unroll
    for (int u = 0; u < VN; u++) x[u] = (T)0;
    if (whole && vec_in) {
      x = reinterpret_cast<const NV *>(v)[g];
    } else {
#pragma unroll
      for (int u = 0; u < VN; u++)
        if (u < cnt) x[u] = v[lin0 + u];
    }
    int64_t qd[VN];
    bool outl[VN];
    NV res;
    unsigned mine = 0;
    if (cnt > 0) cur.seek((uint32_t)lin0);
#pragma unroll
    for (int u = 0; u < VN; u++) {
      qd[u] = 0;
      outl[u] = false;
      res[u] = (T)0;
      if (u < cnt) {
        const int level = cur.next(u + 1 < cnt);
        const int64_t q = quantize_one(x[u], s_tab[kTabRqz][level], m.calc_vol ? s_tab[kTabQvol][level] : (T)1);
        if constexpr (RES) {
          const T volume = m.calc_vol ? s_tab[kTabDvol][level] : (T)1;
          const T back = (s_tab[kTabQz][level] * volume) * (T)q;  // (k_dequantize's value of this integer)
          res[u] = x[u] - back;
        }
        qd[u] = q + half;
        outl[u] = !(qd[u] >= 0 && qd[u] < (int64_t)dict);
        mine += outl[u] ? 1u : 0u;
      }
    }
    if constexpr (RES) {
      if (whole && vec_res) {
        reinterpret_cast<NV *>(r_out)[g] = res;
      } else {
#pragma unroll
        for (int u = 0; u < VN; u++)
          if (u < cnt) r_out[lin0 + u] = res[u];
      }
    }
    append_outliers<kQsThreads>(mine, outl, qd, lin0, outlier_count, outlier_idx, outlier_val, outlier_cap);
    SV s;
#pragma unroll
    for (int u = 0; u < VN; u++) {
      s[u] = (SYM)qd[u];
      if (HIST && u < cnt) {
        if (qd[u] == half) centre++;
        else atomicAdd(&qs_bins[(int)qd[u]], 1u);
      }
    }
    if (whole && vec_out) {
      reinterpret_cast<SV *>(sym)[g] = s;
    } else {
#pragma unroll
      for (int u = 0; u < VN; u++)
        if (u < cnt) sym[lin0 + u] = s[u];
    }
  }
  if (HIST) flush_bins<kQsThreads>(qs_bins, dict, centre, (int)half, freq);
}

template <typename T, bool HIST>
__global__ void __launch_bounds__(kQsThreads)
k_quantize_symbols(QuantMeta m, size_t total, const T *__restrict__ v, const int *__restrict__ marks,
                   const T *__restrict__ tab /* [2][nlev]: reciprocal quantizers, volumes */, int nlev, int dict,
                   uint16_t *__restrict__ sym, unsigned *__restrict__ freq /* [dict], HIST only */,
                   unsigned long long *outlier_count, uint64_t *__restrict__ outlier_idx,
                   int64_t *__restrict__ outlier_val, unsigned long long outlier_cap) {
  quantize_symbols_body<T, HIST, false>(m, total, v, marks, tab, nlev, dict, sym, freq, outlier_count, outlier_idx,
                                        outlier_val, outlier_cap, nullptr);
}

template <typename T, bool HIST>
__global__ void __launch_bounds__(kQsThreads)
k_quantize_symbols_residual(QuantMeta m, size_t total, const T *v, const int *__restrict__ marks,
                            const T *__restrict__ tab /* [4][nlev]: QTab */, int nlev, int dict,
                            uint16_t *__restrict__ sym, unsigned *__restrict__ freq /* [dict], HIST only */,
                            unsigned long long *outlier_count, uint64_t *__restrict__ outlier_idx,
                            int64_t *__restrict__ outlier_val, unsigned long long outlier_cap, T *r_out) {
  quantize_symbols_body<T, HIST, true>(m, total, v, marks, tab, nlev, dict, sym, freq, outlier_count, outlier_idx,
                                       outlier_val, outlier_cap, r_out);
}

// SYM = int64_t (mgh_quantize_residual_linear, the writer of a level-ordered layer): the same pass with
// the integers stored as mgh_quantize(prep_huffman = 1) stores them -- the shifted value, 0 for an outlier
// -- in array order; the launcher linearises them and the list's indices behind it (k_level_linearize,
// k_linearize_indices).
template <typename T>
__global__ void __launch_bounds__(kQsThreads)
k_quantize_residual_int64(QuantMeta m, size_t total, const T *v, const int *__restrict__ marks,
                          const T *__restrict__ tab /* [4][nlev]: QTab */, int nlev, int dict, int64_t *__restrict__ q,
                          unsigned long long *outlier_count, uint64_t *__restrict__ outlier_idx,
                          int64_t *__restrict__ outlier_val, unsigned long long outlier_cap, T *r_out) {
  quantize_symbols_body<T, false, true, int64_t>(m, total, v, marks, tab, nlev, dict, q, nullptr, outlier_count,
                                                 outlier_idx, outlier_val, outlier_cap, r_out);
}

constexpr int kQaThreads = 256;

template <typename T, bool FIRST>
__global__ void __launch_bounds__(kQaThreads)
k_dequantize_add(QuantMeta m, size_t total, const int64_t *__restrict__ q, const int *__restrict__ marks,
                 const T *__restrict__ tab /* [2][nlev]: quantizers, dequantize volumes */, int nlev, int64_t shift,
                 T *__restrict__ acc) {
  __shared__ T s_tab[2][kMaxLevels];
  stage_tables<kQaThreads>(tab, nlev, s_tab);
  __syncthreads();

  auto value = [&](int64_t qd, int level) -> T {
    const T volume = m.calc_vol ? s_tab[1][level] : (T)1;
    return (s_tab[0][level] * volume) * (T)(qd - shift);
  };
  constexpr int VN = Vec16<T>::N;
  typedef T NV __attribute__((ext_vector_type(VN)));
  typedef int64_t Q2 __attribute__((ext_vector_type(2)));  // (16 bytes: a vector of T takes VN / 2 of them)
  stream_levels<kQaThreads, VN>(
      m, marks, total, aligned16(q, acc),
      [&](size_t i, LevelCursor &cur) {
        int64_t qd[VN];
#pragma unroll
        for (int u = 0; u < VN; u += 2) {
          const Q2 two = reinterpret_cast<const Q2 *>(q)[i * (VN / 2) + u / 2];
          qd[u] = two[0];
          qd[u + 1] = two[1];
        }
        NV y;
        if (!FIRST) y = reinterpret_cast<NV *>(acc)[i];
#pragma unroll
        for (int u = 0; u < VN; u++) {
          const T add = value(qd[u], cur.next(u + 1 < VN));
          y[u] = FIRST ? add : y[u] + add;
        }
        reinterpret_cast<NV *>(acc)[i] = y;
      },
      [&](size_t k, int level) {
        const T add = value(q[k], level);
        acc[k] = FIRST ? add : acc[k] + add;
      });
}

// k_dequantize_add_linear: k_dequantize_add on a WINDOW of the level-linearised order (reorder = 1; the
// reader of the level-ordered precision layers). q[0 .. count) are the integers at positions
// [first, first + count) of the linearised array, outliers written back already (k_outlier_restore_window);
// acc is the whole accumulator in the same order, of which only that window is read or written.
//
// In this order the level of a position needs no marks and no division: level l occupies [N_{l-1}, N_l)
// with N_l = prod(level_shape(l)) (LinMeta::lshape; linearized_position, kernels_v1.hpp, puts a node of
// level `level` at base = N_{level-1} plus its rank inside the level). The offsets N_0 < ... < N_L come by
// value and are staged in LDS beside the two tables of mgh_dequantize. The numbering is the dequantizer's:
// linearized_position takes `level` as the largest per-dimension mark of the node, level_of (kernels_v1.hpp,
// what k_dequantize and LevelCursor index qz[] and vol[] with) is the same maximum over the same marks, and
// both count 0 = coarsest (lshape[0] is the coarsest grid; upload_quantizers fills qz[l] for l = 0 .. L in
// that order). With calc_vol == 0 (s = inf) k_dequantize reads entry 0 of the quantizers for every node and
// no volume; so does this kernel.
//
// A pure stream: persistent workgroups, no atomics, no barrier behind the staging. Where q and acc + first
// are 16-byte aligned a thread moves whole vectors (VN elements of T, VN / 2 pairs of integers) and takes
// one level for the vector when its last element lies below the level's end, else one level per element;
// the tail, or all of a misaligned window, goes element by element. STORE stores the value (never added to
// zero: -0.0 stays -0.0); otherwise acc = acc + value, one IEEE add behind k_dequantize's two multiplies.
struct LinOffsets {
  uint32_t n[kMaxLevels];  // n[l] = N_l (the entry points refuse 2^32 elements and more)
};

template <typename T, bool STORE>
__global__ void __launch_bounds__(kQaThreads)
k_dequantize_add_linear(LinOffsets off, int nlev, int calc_vol, const int64_t *__restrict__ q, uint32_t first,
                        size_t count, const T *__restrict__ tab /* [2][nlev]: quantizers, dequantize volumes */,
                        int64_t shift, T *__restrict__ acc_all) {
  __shared__ T s_tab[2][kMaxLevels];
  __shared__ uint32_t s_off[kMaxLevels];
  stage_tables<kQaThreads>(tab, nlev, s_tab);
  for (int i = threadIdx.x; i < nlev; i += kQaThreads) s_off[i] = off.n[i];
  __syncthreads();

  const int top = nlev - 1;
  // (most positions lie in the finest levels: from the top down, one comparison for the finest)
  auto level_at = [&](uint32_t p) -> int {
    int l = 0;
    if (calc_vol) {
      l = top;
      while (l > 0 && p < s_off[l - 1]) l--;
    }
    return l;
  };
  auto value = [&](int64_t qd, int level) -> T {
    const T volume = calc_vol ? s_tab[1][level] : (T)1;
    return (s_tab[0][level] * volume) * (T)(qd - shift);
  };
  constexpr int VN = Vec16<T>::N;
  typedef T NV __attribute__((ext_vector_type(VN)));
  typedef int64_t Q2 __attribute__((ext_vector_type(2)));
  T *acc = acc_all + first;  // acc[k] is position first + k, like q[k]
  const size_t tid = (size_t)blockIdx.x * kQaThreads + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * kQaThreads;
  size_t done = 0;
  if (aligned16(q, acc)) {
    const size_t nvec = count / VN;
    for (size_t i = tid; i < nvec; i += nth) {
      const uint32_t p0 = first + (uint32_t)(i * VN);
      int64_t qd[VN];
#pragma unroll
      for (int u = 0; u < VN; u += 2) {
        const Q2 two = reinterpret_cast<const Q2 *>(q)[i * (VN / 2) + u / 2];
        qd[u] = two[0];
        qd[u + 1] = two[1];
      }
      NV y;
      if (!STORE) y = reinterpret_cast<NV *>(acc)[i];
      const int l0 = level_at(p0);
      // (the vector ends inside level l0: one level; else it straddles a boundary, element by element)
      const bool one_level = !calc_vol || p0 + (VN - 1) < s_off[l0];
#pragma unroll
      for (int u = 0; u < VN; u++) {
        const T add = value(qd[u], one_level ? l0 : level_at(p0 + u));
        y[u] = STORE ? add : y[u] + add;
      }
      reinterpret_cast<NV *>(acc)[i] = y;
    }
    done = nvec * VN;
  }
  for (size_t k = done + tid; k < count; k += nth) {
    const T add = value(q[k], level_at(first + (uint32_t)k));
    acc[k] = STORE ? add : acc[k] + add;
  }
}

}  // namespace mgh
