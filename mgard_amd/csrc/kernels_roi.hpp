// Region of interest: the two streaming kernels behind mgh_box_residual_ / mgh_box_add_ (the scheme, the bound and
// the trailer: roi_plan.hpp).
//   k_box_residual   one pass over a box of x and of b, two dense arrays of the same shape: the dense residual
//                    r = fl_T(x - b) of the box, and per workgroup one partial of max |r|, max |x| (over the finite
//                    ones) and the count of positions whose x or r is not finite. k_box_stats_final, one workgroup,
//                    folds the partials. Maxima and integer counts: the result does not depend on the order, so it
//                    is deterministic, and nothing is an atomic.
//   k_box_add        out[box] = fl_T(out[box] + r), in place; nothing outside the box is touched.
// Both reach the box through an LdView (ld_view.hpp: the box's extents and the array's element strides, right-
// aligned) and a pointer that already stands on the box's first element. Rows run along the last dimension. A group
// of 2^lg lanes owns a row at a time and walks it with its lanes along the row, so the loads and stores of a row are
// contiguous; a wave holds 64 >> lg rows. The host picks lg = 6 for rows of more than 32 elements and the smallest
// group that covers the row below that (as mgh_pwrel_inverse_sampled_ does), so short rows do not leave most of a
// wave idle. Offsets are 64-bit; the row is unravelled once per row, an element costs no division.
// -ffp-contract=off (the build's): x - b and out + r are one rounding each.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ld_view.hpp"

namespace mgh {
namespace roi {

constexpr int kThreads = 256;  // four waves
constexpr int kWaves = kThreads / 64;
constexpr unsigned kMaxBlocks = 256 * 8;  // grid cap of the grid-stride loops

// mgh_box_stats: what mgh_box_residual_ leaves at the start of its scratch; the partials lie behind it
struct BoxStats {
  double max_abs_r, max_abs_x;
  unsigned long long n_nonfinite, pad;
};

__device__ inline bool box_finite(double a) { return a <= 1.7976931348623157e308; }  // (a = |v|: false for NaN, Inf)

__device__ inline void box_stats_store(double mr, double mx, unsigned long long nf, BoxStats *out) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double a = __shfl_xor(mr, off), b = __shfl_xor(mx, off);
    mr = a > mr ? a : mr;
    mx = b > mx ? b : mx;
    nf += __shfl_xor(nf, off);
  }
  __shared__ double sr[kWaves], sx[kWaves];
  __shared__ unsigned long long sn[kWaves];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    sr[wv] = mr;
    sx[wv] = mx;
    sn[wv] = nf;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; w++) {
      mr = sr[w] > mr ? sr[w] : mr;
      mx = sx[w] > mx ? sx[w] : mx;
      nf += sn[w];
    }
    out->max_abs_r = mr;
    out->max_abs_x = mx;
    out->n_nonfinite = nf;
    out->pad = 0;
  }
}

// x, b: on the box's first element; V: the box in the array; r: dense, V.rows rows of nf; partials[gridDim.x]
template <typename T>
__global__ void __launch_bounds__(kThreads)
k_box_residual(const T *__restrict__ x, const T *__restrict__ b, LdView V, uint32_t nf, int lg, T *__restrict__ r,
               BoxStats *__restrict__ partials) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t group = 1u << lg, j0 = lane & (group - 1), per_wave = 64u >> lg;
  const uint64_t wave = (uint64_t)blockIdx.x * kWaves + wv, nwaves = (uint64_t)gridDim.x * kWaves;
  double mr = 0, mx = 0;
  unsigned long long bad = 0;
  for (uint64_t row = wave * per_wave + (lane >> lg); row < V.rows; row += nwaves * per_wave) {
    const uint64_t off = ld_row_offset(V, row);
    const T *xr = x + off, *br = b + off;
    T *rr = r + row * nf;
    for (uint32_t j = j0; j < nf; j += group) {
      const T xv = xr[j], rv = xv - br[j];
      rr[j] = rv;
      const double ax = xv < 0 ? -(double)xv : (double)xv, ar = rv < 0 ? -(double)rv : (double)rv;
      const bool fx = box_finite(ax), fr = box_finite(ar);
      bad += (fx && fr) ? 0 : 1;
      mx = fx && ax > mx ? ax : mx;
      mr = fr && ar > mr ? ar : mr;
    }
  }
  box_stats_store(mr, mx, bad, partials + blockIdx.x);  // (every lane of the workgroup arrives)
}

static __global__ void __launch_bounds__(kThreads)
k_box_stats_final(const BoxStats *__restrict__ partials, uint32_t count, BoxStats *out) {
  double mr = 0, mx = 0;
  unsigned long long bad = 0;
  for (uint32_t i = threadIdx.x; i < count; i += kThreads) {
    const BoxStats p = partials[i];
    mr = p.max_abs_r > mr ? p.max_abs_r : mr;
    mx = p.max_abs_x > mx ? p.max_abs_x : mx;
    bad += p.n_nonfinite;
  }
  box_stats_store(mr, mx, bad, out);
}

// out: on the box's first element; r: dense, V.rows rows of nf
template <typename T>
__global__ void __launch_bounds__(kThreads)
k_box_add(T *__restrict__ out, LdView V, uint32_t nf, int lg, const T *__restrict__ r) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t group = 1u << lg, j0 = lane & (group - 1), per_wave = 64u >> lg;
  const uint64_t wave = (uint64_t)blockIdx.x * kWaves + wv, nwaves = (uint64_t)gridDim.x * kWaves;
  for (uint64_t row = wave * per_wave + (lane >> lg); row < V.rows; row += nwaves * per_wave) {
    T *o = out + ld_row_offset(V, row);
    const T *rr = r + row * nf;
    for (uint32_t j = j0; j < nf; j += group) o[j] = o[j] + rr[j];
  }
}

}  // namespace roi
}  // namespace mgh
