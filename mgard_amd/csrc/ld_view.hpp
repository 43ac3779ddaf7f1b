// Rows of an array that is not dense in memory (mgh_set_ld; a box of a larger array): all dimensions
// but the fastest, right-aligned with leading 1s, and the element strides of those dimensions. The
// row-wise kernels (k_ld_copy, k_norm_ld, k_compare_ld) walk an array through it.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../include/mgard_hip.h"

namespace mgh {

struct LdView {
  uint32_t ext[MGH_MAX_DIM];
  uint64_t stride[MGH_MAX_DIM];
  uint64_t rows;
};

// element offset of the first element of row `row`
__device__ __forceinline__ uint64_t ld_row_offset(const LdView &V, uint64_t row) {
  uint64_t r = row, off = 0;
#pragma unroll
  for (int d = MGH_MAX_DIM - 2; d >= 0; d--) {
    const uint64_t q = r / V.ext[d];
    off += (r - q * V.ext[d]) * V.stride[d];
    r = q;
  }
  return off;
}

}  // namespace mgh
