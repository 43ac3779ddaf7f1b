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

} // namespace mgh
