// Reconstruction at a coarser level of the hierarchy (mgh_*_to_level), gfx950: the kernels that
// restrict the stages in front of the level loop to the COARSE CORNER BOX of the reordered layout,
// [0, m_0) x ... x [0, m_{D-1}) with m = level_shape(level) -- all a stop below the finest level
// reads. The level loops themselves are the kernels of the full reconstruction, run with the
// strides of that box and stopped early (capi.hip).
//
//   k_box_gather          : the box out of the full (possibly pitched) coefficient array as a
//                           compact array (DataRefactor::Recompose reads the same nodes through
//                           SubArrays of the full array, DataRefactoring.hpp:233-274).
//   k_box_dequantize      : the same out of the quantized integers, dequantized on the way with
//                           the arithmetic of k_dequantize (kernels_v1.hpp; LinearQuantization.hpp
//                           :146-264) -- the level of a node from the level marks of its indices.
//   k_outlier_restore_in_box : OutlierRestore (LinearQuantization.hpp:304-350) for the entries of
//                           the list that lie inside the box, written IN PLACE into the full
//                           quantized array; the rest of the array is left alone.
//   k_shell_from_linear, k_outlier_restore_window, k_box_refine_fill : ONE level step from the level's own
//                           segment of a level-linearised array (mgh_refine_level; further down).
// One wave per PIECE of a row of the box (the piece's position is scalar arithmetic, the lanes stream
// it), as k_widen_box does per row; rows longer than kLevelBoxPiece elements are cut into pieces, so
// that the one row of a 1-D array (or the few of a flat 2-D one) is spread over the device too.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_v1.hpp"

namespace mgh {

constexpr uint32_t kLevelBoxPiece = 4096;  // elements of a row one wave copies

struct LevelBox {
  int D;
  uint32_t m[5];   // the box
  uint32_t n[5];   // the full array
  uint64_t ss[5];  // element strides of the source array
};

// element offset of row `row` of the box (all dimensions but the fastest) in the source array
__device__ __forceinline__ uint64_t level_box_row(const LevelBox &B, uint64_t row, uint32_t *idx) {
  uint64_t off = 0;
  for (int d = B.D - 2; d >= 0; d--) {
    idx[d] = (uint32_t)(row % B.m[d]);
    row /= B.m[d];
    off += idx[d] * B.ss[d];
  }
  return off;
}

template <typename T>
__global__ void __launch_bounds__(256)
k_box_gather(LevelBox B, const T *__restrict__ src, T *__restrict__ dst, uint64_t rows) {
  const int lane = threadIdx.x & 63;
  const uint32_t mf = B.m[B.D - 1];
  const uint32_t npiece = (mf + kLevelBoxPiece - 1) / kLevelBoxPiece;
  const uint64_t units = rows * npiece;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += (uint64_t)gridDim.x * 4) {
    const uint64_t row = u / npiece;
    const uint32_t f0 = (uint32_t)(u - row * npiece) * kLevelBoxPiece, f1 = min(mf, f0 + kLevelBoxPiece);
    uint32_t idx[5];
    const T *s = src + level_box_row(B, row, idx);
    T *d = dst + row * mf;
    for (uint32_t f = f0 + lane; f < f1; f += 64) d[f] = s[f];
  }
}

template <typename T>
__global__ void __launch_bounds__(256)
k_box_dequantize(LevelBox B, QuantMeta m, const int64_t *__restrict__ q, const int *__restrict__ marks,
                 const T *__restrict__ qz, const T *__restrict__ vol, int64_t dict_size, int prep_huffman,
                 T *__restrict__ dst, uint64_t rows) {
  const int lane = threadIdx.x & 63;
  const uint32_t mf = B.m[B.D - 1];
  const uint32_t npiece = (mf + kLevelBoxPiece - 1) / kLevelBoxPiece;
  const uint64_t units = rows * npiece;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += (uint64_t)gridDim.x * 4) {
    const uint64_t row = u / npiece;
    const uint32_t f0 = (uint32_t)(u - row * npiece) * kLevelBoxPiece, f1 = min(mf, f0 + kLevelBoxPiece);
    uint32_t idx[5];
    const int64_t *s = q + level_box_row(B, row, idx);
    int row_level = 0;
    if (m.calc_vol)
      for (int d = 0; d < B.D - 1; d++) row_level = max(row_level, marks[m.markoff[d] + idx[d]]);
    T *d = dst + row * mf;
    for (uint32_t f = f0 + lane; f < f1; f += 64) {
      const int level = m.calc_vol ? max(row_level, marks[m.markoff[B.D - 1] + f]) : 0;
      int64_t qd = s[f];
      if (prep_huffman) qd -= dict_size / 2;
      const T volume = m.calc_vol ? vol[level] : (T)1;
      d[f] = (qz[level] * volume) * (T)qd;
    }
  }
}

__global__ void __launch_bounds__(256)
k_outlier_restore_in_box(int64_t *__restrict__ q, LevelBox B, const uint64_t *__restrict__ idx,
                         const int64_t *__restrict__ val, uint64_t count) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const uint64_t lin0 = idx[k];
  uint64_t lin = lin0;
  bool inside = true;
  for (int d = B.D - 1; d >= 1; d--) {
    inside &= (uint32_t)(lin % B.n[d]) < B.m[d];
    lin /= B.n[d];
  }
  // (an index outside the array can only come from a damaged stream: it falls outside the box too)
  inside &= lin < B.m[0];
  if (inside) q[lin0] = val[k];
}

// ---- the box of a level straight out of the head of a level-linearised array --------------------
// k_box_from_linear: the first N_level = prod(level_shape(level)) integers of a level-linearised
// array (config.reorder == 1, linearized_position in kernels_v1.hpp) are the corner box of `level`,
// level by level: level 0 in natural order, then for j = 1 .. level the fine grid of level j in
// natural order with its coarse nodes left out. In that order a natural row of level j whose slow
// indices include a level-j node is ONE contiguous run (coarse-f and odd-f nodes interleaved); a
// row whose slow indices are all coarse keeps only its odd-f nodes, again one run. So the inverse
// permutation restricted to the box streams: one wave per piece of a run, the run's first stream
// position and its row of the box computed once (scalar work), the lanes read the stream with unit
// stride and store the de-interleaved halves to the one or two row pieces of the box they belong
// to. Every element of the box is written exactly once, nothing at or behind N_level is read.
struct LinBox {
  int level;
  uint64_t bs[5];                       // element strides of the box (dense in level_shape(level))
  uint64_t unit0[kLinMaxLevels + 2];    // first unit of level j (units: pieces of runs); [level + 1]: all
};

// Two neighbours of the stream as one load. The permutation moves bits: E is int64_t for 8-byte elements
// (the integers, double coefficients) and int32_t for 4-byte ones (float coefficients,
// mgh_recompose_linear_to_level).
template <typename E> struct LinPair;
template <> struct LinPair<int64_t> { typedef int64_t type __attribute__((ext_vector_type(2), aligned(8))); };
template <> struct LinPair<int32_t> { typedef int32_t type __attribute__((ext_vector_type(2), aligned(4))); };

// One piece of a run of level j >= 1 (unit `ul` of that level) into a box with strides `bs`; `lj` is
// where the level's own integers start (lin + N_{j-1} in the whole array, or a segment that holds the
// level alone). All arguments but the lane are wave-uniform.
template <typename E>
__device__ __forceinline__ void lin_run_to_box(const LinMeta &m, int j, uint32_t ul, const uint64_t *bs,
                                               const E *__restrict__ lj, E *__restrict__ box, int lane) {
  const int D = m.D;
  const uint32_t *F = m.lshape[j];
  const uint32_t Ff = F[D - 1];
  const uint32_t npiece = (Ff + kLevelBoxPiece - 1) / kLevelBoxPiece;
  uint32_t row = ul / npiece;
  const uint32_t e0 = (ul - row * npiece) * kLevelBoxPiece;  // first stream element of the piece in its run
  const uint32_t *C = m.lshape[j - 1];
  const uint32_t Cf = C[D - 1];
  // natural slow coordinates of the row in level j's fine grid: its row of the box, and the part of
  // linearized_position's sums that does not depend on the fastest coordinate
  uint64_t off = 0, stride = Ff, cstride = Ff / 2 + 1, to = 0, co = 0;
  bool mixed = false;
  for (int d = D - 2; d >= 0; d--) {
    const uint32_t g = row % F[d];
    row /= F[d];
    const bool odd = (g & 1u) && g != F[d] - 1;  // a level-j node along d
    mixed |= odd;
    const uint32_t idx = odd ? C[d] + (g - 1) / 2 : (g == F[d] - 1 && F[d] % 2 == 0 ? F[d] / 2 : g / 2);
    off += (uint64_t)idx * bs[d];
    to += (uint64_t)g * stride;
    stride *= F[d];
    if (odd) co = 0;
    if (g) co += (uint64_t)((g - 1) / 2 + 1) * cstride;
    cstride *= F[d] / 2 + 1;
  }
  // (an all-coarse row starts at its first odd-f node, g = 1: one element on, one coarse node before it)
  const E *s = lj + (to - co);
  E *dst = box + off;
  if (mixed) {
    // the whole natural row: nodes 2k and 2k + 1 side by side in the stream
    const uint32_t e1 = min(Ff, e0 + kLevelBoxPiece);
    const bool even_last = Ff % 2 == 0;  // node Ff - 1 of an even extent is the last COARSE node
    for (uint32_t g = e0 + 2 * lane; g < e1; g += 128) {
      const uint32_t k = g / 2;
      if (g + 1 < e1) {
        typedef typename LinPair<E>::type pair_t;
        const pair_t v = *reinterpret_cast<const pair_t *>(s + g);
        dst[k] = v.x;
        dst[(even_last && g + 1 == Ff - 1) ? Ff / 2 : Cf + k] = v.y;
      } else {
        dst[k] = s[g];
      }
    }
  } else {
    // only the odd-f nodes: Ff - Cf of them in a row
    const uint32_t cnt = Ff - Cf;
    const uint32_t e1 = min(cnt, e0 + kLevelBoxPiece);
    for (uint32_t k = e0 + lane; k < e1; k += 64) dst[Cf + k] = s[k];
  }
}

template <typename E>
__global__ void __launch_bounds__(256)
k_box_from_linear(LinMeta m, LinBox B, const E *__restrict__ lin, E *__restrict__ box) {
  const int lane = threadIdx.x & 63;
  const int D = m.D;
  const uint64_t units = B.unit0[B.level + 1];
  const uint64_t wave0 = __builtin_amdgcn_readfirstlane((uint32_t)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  for (uint64_t u = wave0; u < units; u += (uint64_t)gridDim.x * 4) {
    int j = 0;
    while (u >= B.unit0[j + 1]) j++;
    const uint32_t ul = (uint32_t)(u - B.unit0[j]);
    if (j == 0) {
      // level 0: the first N_0 integers in natural order, row by row into the box
      const uint32_t *F = m.lshape[0];
      const uint32_t Ff = F[D - 1];
      const uint32_t npiece = (Ff + kLevelBoxPiece - 1) / kLevelBoxPiece;
      uint32_t row = ul / npiece;
      const uint32_t e0 = (ul - row * npiece) * kLevelBoxPiece;
      uint64_t off = 0;
      const uint64_t src = (uint64_t)row * Ff;
      for (int d = D - 2; d >= 0; d--) {
        off += (uint64_t)(row % F[d]) * B.bs[d];
        row /= F[d];
      }
      const uint32_t e1 = min(Ff, e0 + kLevelBoxPiece);
      for (uint32_t f = e0 + lane; f < e1; f += 64) box[off + f] = lin[src + f];
      continue;
    }
    // (the integers of level j start behind those of the levels below: N_{j-1} of them)
    uint64_t below = 1;
    for (int d = 0; d < D; d++) below *= m.lshape[j - 1][d];
    lin_run_to_box(m, j, ul, B.bs, lin + below, box, lane);
  }
}

// ---- one level step (mgh_refine_level): the SHELL of a level's box out of the level's own segment --
// k_shell_from_linear: the level-`level` part of k_box_from_linear alone. `seg` holds the integers
// [N_{level-1}, N_level) of the level-linearised array -- the coefficients of that level, nothing
// else -- and the box is the compact box of level_shape(level): units [0, unit0[1]) are the pieces of
// the level's runs (lin_run_to_box with the stream rebased to the segment). The inner box of
// level - 1 holds no coefficient of this level. The node restore of the fused level loop still LOADS
// the even-even-even position of every cell (a value it does not use), so where that loop runs the
// units [unit0[1], unit0[2]) store `inner` there -- the integer that dequantizes to 0 -- instead of
// leaving the loads to whatever the buffer held.
__global__ void __launch_bounds__(256)
k_shell_from_linear(LinMeta m, LinBox B, const int64_t *__restrict__ seg, int64_t *__restrict__ box, int64_t inner) {
  const int lane = threadIdx.x & 63;
  const int D = m.D;
  const uint64_t units = B.unit0[2];
  const uint64_t wave0 = __builtin_amdgcn_readfirstlane((uint32_t)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  for (uint64_t u = wave0; u < units; u += (uint64_t)gridDim.x * 4) {
    if (u < B.unit0[1]) {
      lin_run_to_box(m, B.level, (uint32_t)u, B.bs, seg, box, lane);
      continue;
    }
    const uint32_t *C = m.lshape[B.level - 1];
    const uint32_t Cf = C[D - 1];
    const uint32_t npiece = (Cf + kLevelBoxPiece - 1) / kLevelBoxPiece;
    const uint32_t ul = (uint32_t)(u - B.unit0[1]);
    uint32_t row = ul / npiece;
    const uint32_t e0 = (ul - row * npiece) * kLevelBoxPiece, e1 = min(Cf, e0 + kLevelBoxPiece);
    uint64_t off = 0;
    for (int d = D - 2; d >= 0; d--) {
      off += (uint64_t)(row % C[d]) * B.bs[d];
      row /= C[d];
    }
    for (uint32_t f = e0 + lane; f < e1; f += 64) box[off + f] = inner;
  }
}

// OutlierRestore for the entries of the list at positions [lo, hi), written into a buffer that holds
// that window alone (q[0] is position lo); every other entry is skipped.
__global__ void __launch_bounds__(256)
k_outlier_restore_window(int64_t *__restrict__ q, uint64_t lo, uint64_t hi, const uint64_t *__restrict__ idx,
                         const int64_t *__restrict__ val, uint64_t count) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const uint64_t p = idx[t];
  if (p >= lo && p < hi) q[p - lo] = val[t];
}

// The compact box of a level for the level loops that read floating-point coefficients in place
// (mgh_refine_level on the shapes the fused kernels do not take): the inner box of level - 1 from
// the dense nodal array `coarse` of that level, the shell dequantized from the compact integer box
// `q` with the arithmetic of k_box_dequantize. B.m: the level's box, B.n: the inner box; q and dst
// are dense in B.m.
template <typename T>
__global__ void __launch_bounds__(256)
k_box_refine_fill(LevelBox B, QuantMeta m, const int64_t *__restrict__ q, const T *__restrict__ coarse,
                  const int *__restrict__ marks, const T *__restrict__ qz, const T *__restrict__ vol,
                  int64_t dict_size, int prep_huffman, T *__restrict__ dst, uint64_t rows) {
  const int lane = threadIdx.x & 63;
  const uint32_t mf = B.m[B.D - 1], cf = B.n[B.D - 1];
  const uint32_t npiece = (mf + kLevelBoxPiece - 1) / kLevelBoxPiece;
  const uint64_t units = rows * npiece;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += (uint64_t)gridDim.x * 4) {
    const uint64_t row = u / npiece;
    const uint32_t f0 = (uint32_t)(u - row * npiece) * kLevelBoxPiece, f1 = min(mf, f0 + kLevelBoxPiece);
    uint32_t idx[5];
    (void)level_box_row(B, row, idx);
    int row_level = 0;
    bool inner_row = true;
    uint64_t crow = 0;
    for (int d = 0; d < B.D - 1; d++) {
      if (m.calc_vol) row_level = max(row_level, marks[m.markoff[d] + idx[d]]);
      inner_row &= idx[d] < B.n[d];
      crow = crow * B.n[d] + idx[d];
    }
    const int64_t *s = q + row * mf;
    const T *c = coarse + crow * cf;
    T *d = dst + row * mf;
    for (uint32_t f = f0 + lane; f < f1; f += 64) {
      if (inner_row && f < cf) {
        d[f] = c[f];
        continue;
      }
      const int level = m.calc_vol ? max(row_level, marks[m.markoff[B.D - 1] + f]) : 0;
      int64_t qd = s[f];
      if (prep_huffman) qd -= dict_size / 2;
      const T volume = m.calc_vol ? vol[level] : (T)1;
      d[f] = (qz[level] * volume) * (T)qd;
    }
  }
}

} // namespace mgh
