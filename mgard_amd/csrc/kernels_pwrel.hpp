// Pointwise relative error bound: the streaming kernels behind mgh_pwrel_forward_ / mgh_pwrel_inverse_ /
// mgh_pwrel_inverse_sampled_ / mgh_compare_pwrel_ (classes, tolerance and trailer: pwrel_plan.hpp).
//   k_pwrel_forward   one pass over x: y = (T)log2((double)|x|) at valid positions (0 at masked ones, which the
//                     fill overwrites), the mask word and the flag word of every 64 elements -- two wave ballots --
//                     and the statistics: counts, and minimum / maximum of y over the valid elements as the ordered
//                     64-bit keys of kernels_mask.hpp. Everything reduced is order-independent and goes through the
//                     wave, then the workgroup, then ONE integer atomic each per workgroup: the result is
//                     deterministic. It stands in for k_mask_scan in the writer, so the array is read once.
//   k_pwrel_inverse   one pass, in place over the decoded y': quiet NaN (masked and flag), +0.0 (masked), else
//                     +-(T)exp2((double)y') with the magnitude clamped to [smallest normal, largest finite] of T.
//   k_compare_pwrel   one pass over an original and a reconstruction in the reduction structure of
//                     kernels_compare.hpp: workgroup g reduces slab g (compare_plan.hpp) into one partial,
//                     k_compare_pwrel_final folds the partials in ascending order. Maxima with the lowest index on
//                     a tie, and counts: no floating-point sum, so the result does not depend on the order at all.
//   k_pwrel_inverse_sampled  the same over a level array, a coarsened array or a window, with the two bits taken from
//                     the full array's maps through the view's node lists (mgh_pwrel_inverse_sampled_).
// Only vector stores: lane 0 of a wave stores the wave's two words.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>

#include "../../include/mgard_hip.h"
#include "compare_plan.hpp"
#include "kernels_mask.hpp"
#include "pwrel_plan.hpp"

namespace mgh {
namespace pwrel {

using mask::kScanUnroll;
using mask::kThreads;
using mask::kWaves;

// stats as six 64-bit words while the forward pass runs: [0] unused, [1] masked, [2] nonfinite, [3] flag bits,
// [4] key of the minimum of y, [5] key of the maximum
static __global__ void k_pwrel_stats_begin(unsigned long long *s) {
  if (threadIdx.x == 0) {
    s[0] = 0;
    s[1] = 0;
    s[2] = 0;
    s[3] = 0;
    s[4] = ~0ull;
    s[5] = 0;
  }
}
// ... and as mgh_pwrel_stats {n, n_masked, n_nonfinite, n_flag, ymin, ymax} afterwards
static __global__ void k_pwrel_stats_end(unsigned long long *s, unsigned long long n) {
  if (threadIdx.x == 0) {
    const bool none = s[1] >= n;  // no valid element: ymin = ymax = 0
    s[0] = n;
    s[4] = none ? 0ull : (unsigned long long)__double_as_longlong(mask::key_value(s[4]));
    s[5] = none ? 0ull : (unsigned long long)__double_as_longlong(mask::key_value(s[5]));
  }
}

__device__ inline bool sign_bit(float v) { return __float_as_uint(v) >> 31; }
__device__ inline bool sign_bit(double v) { return (unsigned long long)__double_as_longlong(v) >> 63; }

// x and y may be the same array (every lane reads x[i] before it writes y[i], and nothing else), so neither is
// __restrict__.
template <typename T>
__global__ void __launch_bounds__(kThreads)
k_pwrel_forward(const T *x, uint64_t n, uint64_t nwords, double floor_eff, T *y, unsigned long long *__restrict__ mwords,
                unsigned long long *__restrict__ fwords, unsigned long long *stats) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t wave = (uint64_t)blockIdx.x * kWaves + wv, nwaves = (uint64_t)gridDim.x * kWaves;
  unsigned long long kmin = ~0ull, kmax = 0, masked = 0, nonfin = 0, flags = 0;
  // (the loop bounds are the wave's: every lane reaches every ballot)
  for (uint64_t w0 = wave * kScanUnroll; w0 < nwords; w0 += nwaves * kScanUnroll) {
    T v[kScanUnroll];
    bool in[kScanUnroll];
#pragma unroll
    for (int u = 0; u < kScanUnroll; u++) {
      const uint64_t i = (w0 + u) * 64 + lane;  // (a word past the last one lies past n as a whole)
      in[u] = i < n;
      v[u] = in[u] ? x[i] : T(1);
    }
#pragma unroll
    for (int u = 0; u < kScanUnroll; u++) {
      const int cls = pwrel_classify((double)v[u], floor_eff);
      const bool m = in[u] && cls != kPwrelValid;
      const bool f = in[u] && (cls == kPwrelNonfinite || (cls == kPwrelValid && sign_bit(v[u])));
      // the tail's lanes vote 0: the unused high bits of the last words are zero
      const unsigned long long mbits = __ballot(m), fbits = __ballot(f);
      if (lane == 0 && w0 + u < nwords) {
        mwords[w0 + u] = mbits;
        fwords[w0 + u] = fbits;
        masked += (unsigned long long)__popcll(mbits);
        nonfin += (unsigned long long)__popcll(mbits & fbits);
        flags += (unsigned long long)__popcll(fbits);
      }
      if (in[u]) {
        const double a = v[u] < 0 ? -(double)v[u] : (double)v[u];
        const T yv = m ? T(0) : (T)log2(a);
        y[(w0 + u) * 64 + lane] = yv;
        if (!m) {
          const unsigned long long k = mask::order_key((double)yv);
          kmin = k < kmin ? k : kmin;
          kmax = k > kmax ? k : kmax;
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long a = __shfl_xor(kmin, off), b = __shfl_xor(kmax, off);
    kmin = a < kmin ? a : kmin;
    kmax = b > kmax ? b : kmax;
  }
  __shared__ unsigned long long part[5][kWaves];
  if (lane == 0) {
    part[0][wv] = kmin;
    part[1][wv] = kmax;
    part[2][wv] = masked;
    part[3][wv] = nonfin;
    part[4][wv] = flags;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; w++) {
      kmin = part[0][w] < kmin ? part[0][w] : kmin;
      kmax = part[1][w] > kmax ? part[1][w] : kmax;
      masked += part[2][w];
      nonfin += part[3][w];
      flags += part[4][w];
    }
    if (masked) atomicAdd(&stats[1], masked);
    if (nonfin) atomicAdd(&stats[2], nonfin);
    if (flags) atomicAdd(&stats[3], flags);
    if (kmin != ~0ull) {  // (the workgroup saw a valid element)
      atomicMin(&stats[4], kmin);
      atomicMax(&stats[5], kmax);
    }
  }
}

// What a position decodes to: the class from its mask bit m and its flag bit f, the value from y'.
template <typename T>
__device__ inline T pwrel_inverse_value(bool m, bool f, T y) {
  const double lo = (double)std::numeric_limits<T>::min(), hi = (double)std::numeric_limits<T>::max();
  if (m) return f ? std::numeric_limits<T>::quiet_NaN() : T(0);
  double mag = exp2((double)y);
  mag = mag < lo ? lo : mag;  // (comparisons, not fmin / fmax: a NaN stays one)
  mag = mag > hi ? hi : mag;
  return f ? -(T)mag : (T)mag;
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
k_pwrel_inverse(const unsigned long long *__restrict__ mwords, const unsigned long long *__restrict__ fwords, uint64_t n,
                T *__restrict__ data) {
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  // (a wave's 64 elements share one word of each map: i / 64 is the wave's)
  for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    const bool m = (mwords[i >> 6] >> (i & 63)) & 1, f = (fwords[i >> 6] >> (i & 63)) & 1;
    data[i] = pwrel_inverse_value<T>(m, f, m ? T(0) : data[i]);
  }
}

// mgh_pwrel_inverse_sampled_: k_pwrel_inverse over the dense view y' of A.out_shape -- a level or coarsened array, a
// window -- whose element (i_0 ...) takes its two bits from element (idx_0[i_0] ...) of the FULL array's maps
// (mwords, fwords: the packed maps of an array of A.shape). It stands in for k_mask_sample twice and
// k_pwrel_inverse: the bits are read in place, and no sampled map is stored.
// Rows run along the last dimension (mask_plan.hpp: mask_row_begin). A group of 2^lg lanes owns a row at a time and
// walks it with its lanes along the row, so the loads and stores of y' are contiguous; a wave holds 64 >> lg rows.
// The host picks lg = 6 for rows of more than 32 elements and the smallest group that covers the row below that, so
// that short rows (the coarse levels') do not leave most of a wave idle. The row is unravelled once, by the group's
// lanes alike: an element costs no division. An entry outside A.shape reads nothing and counts as both bits clear.
// Nothing is reduced and no lane waits for another: the result does not depend on the grid.
template <typename T>
__global__ void __launch_bounds__(kThreads)
k_pwrel_inverse_sampled(const unsigned long long *__restrict__ mwords, const unsigned long long *__restrict__ fwords,
                        mask::MaskSampleArgs A, uint32_t rows, int lg, T *__restrict__ data) {
  constexpr int M = kMaskMaxDim;
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t group = 1u << lg, j0 = lane & (group - 1), per_wave = 64u >> lg;
  const uint32_t nf = A.out_shape[M - 1];
  const uint64_t wave = (uint64_t)blockIdx.x * kWaves + wv, nwaves = (uint64_t)gridDim.x * kWaves;
  for (uint64_t r0 = wave * per_wave + (lane >> lg); r0 < rows; r0 += nwaves * per_wave) {
    const MaskRow r = mask_row_begin(M, A.shape, A.out_shape, A.idx, (uint32_t)r0);
    T *row = data + r0 * nf;
    for (uint32_t j = j0; j < nf; j += group) {
      uint64_t flat;
      bool m = false, f = false;
      if (mask_row_source(r, A.shape[M - 1], A.idx[M - 1], j, flat)) {
        m = (mwords[flat >> 6] >> (flat & 63)) & 1;
        f = (fwords[flat >> 6] >> (flat & 63)) & 1;
      }
      row[j] = pwrel_inverse_value<T>(m, f, row[j]);
    }
  }
}

// ---- compare -------------------------------------------------------------------------------------------------
// What a lane, a wave, a workgroup has gathered: mgh_pwrel_compare with "no position yet" told by the counts.
MGH_CMP_HD inline void pwrel_merge(mgh_pwrel_compare &into, const mgh_pwrel_compare &part) {
  // max_rel_err: the larger, and on a tie the lower index; a part without a measured position carries argmax ~0
  if (part.argmax != ~(uint64_t)0 &&
      (into.argmax == ~(uint64_t)0 || part.max_rel_err > into.max_rel_err ||
       (part.max_rel_err == into.max_rel_err && part.argmax < into.argmax))) {
    into.max_rel_err = part.max_rel_err;
    into.argmax = part.argmax;
  }
  into.n += part.n;
  into.n_valid += part.n_valid;
  into.n_zeroed += part.n_zeroed;
  into.n_nonfinite += part.n_nonfinite;
  into.max_zeroed_abs = part.max_zeroed_abs > into.max_zeroed_abs ? part.max_zeroed_abs : into.max_zeroed_abs;
  into.n_class_mismatch += part.n_class_mismatch;
  into.n_sign_mismatch += part.n_sign_mismatch;
}

__device__ inline mgh_pwrel_compare pwrel_empty() {
  mgh_pwrel_compare r;
  r.n = r.n_valid = r.n_zeroed = r.n_nonfinite = 0;
  r.max_rel_err = 0;
  r.argmax = ~(uint64_t)0;
  r.max_zeroed_abs = 0;
  r.n_class_mismatch = r.n_sign_mismatch = 0;
  return r;
}

__device__ inline mgh_pwrel_compare pwrel_shuffled_down(const mgh_pwrel_compare &r, int off) {
  mgh_pwrel_compare o;
  o.n = __shfl_down((unsigned long long)r.n, off, 64);
  o.n_valid = __shfl_down((unsigned long long)r.n_valid, off, 64);
  o.n_zeroed = __shfl_down((unsigned long long)r.n_zeroed, off, 64);
  o.n_nonfinite = __shfl_down((unsigned long long)r.n_nonfinite, off, 64);
  o.max_rel_err = __shfl_down(r.max_rel_err, off, 64);
  o.argmax = __shfl_down((unsigned long long)r.argmax, off, 64);
  o.max_zeroed_abs = __shfl_down(r.max_zeroed_abs, off, 64);
  o.n_class_mismatch = __shfl_down((unsigned long long)r.n_class_mismatch, off, 64);
  o.n_sign_mismatch = __shfl_down((unsigned long long)r.n_sign_mismatch, off, 64);
  return o;
}

// wave64 shuffle reduction, then the four waves through LDS; thread 0 stores
__device__ inline void pwrel_store_partial(mgh_pwrel_compare acc, mgh_pwrel_compare *out) {
  for (int off = 32; off > 0; off >>= 1) pwrel_merge(acc, pwrel_shuffled_down(acc, off));
  __shared__ mgh_pwrel_compare sm[kCompareThreads / 64];
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)(kCompareThreads / 64); w++) pwrel_merge(acc, sm[w]);
    *out = acc;
  }
}

// a: the original, b: the reconstruction. Slab [lo, hi) of workgroup g; a lane meets its positions in ascending
// order, so `>` keeps the lowest index.
template <typename T>
__global__ void __launch_bounds__(256)
k_compare_pwrel(const T *__restrict__ a, const T *__restrict__ b, uint64_t n, uint64_t slab, double floor_eff,
                mgh_pwrel_compare *partials) {
  const uint64_t lo = (uint64_t)blockIdx.x * slab;
  const uint64_t hi = lo + slab < n ? lo + slab : n;
  mgh_pwrel_compare acc = pwrel_empty();
  for (uint64_t i = lo + threadIdx.x; i < hi; i += kCompareThreads) {
    const T x = a[i], r = b[i];
    const double xd = (double)x, rd = (double)r;
    const int cls = pwrel_classify(xd, floor_eff);
    const bool r_nan = r != r, r_fin = pwrel_classify(rd, 0.0) != kPwrelNonfinite;
    acc.n++;
    if (cls == kPwrelNonfinite) {
      acc.n_nonfinite++;
      acc.n_class_mismatch += r_nan ? 0 : 1;
    } else if (cls == kPwrelZeroed) {
      const double ax = xd < 0 ? -xd : xd;
      acc.n_zeroed++;
      acc.max_zeroed_abs = ax > acc.max_zeroed_abs ? ax : acc.max_zeroed_abs;
      acc.n_class_mismatch += (r == T(0) && !sign_bit(r)) ? 0 : 1;  // +0.0 to the bit
    } else {
      acc.n_valid++;
      const bool ok = r_fin && r != T(0);
      acc.n_class_mismatch += ok ? 0 : 1;
      acc.n_sign_mismatch += ok && sign_bit(r) != sign_bit(x) ? 1 : 0;
      if (r_fin) {
        const double d = rd - xd, ax = xd < 0 ? -xd : xd;
        const double e = (d < 0 ? -d : d) / ax;
        if (acc.argmax == ~(uint64_t)0 || e > acc.max_rel_err) {
          acc.max_rel_err = e;
          acc.argmax = i;
        }
      }
    }
  }
  pwrel_store_partial(acc, partials + blockIdx.x);
}

// The partials into one result, the lower workgroups first; a result without a measured position reports
// max_rel_err 0 at index 0.
static __global__ void __launch_bounds__(256)
k_compare_pwrel_final(const mgh_pwrel_compare *__restrict__ partials, uint32_t count, mgh_pwrel_compare *out) {
  const uint32_t per = (count + kCompareThreads - 1) / kCompareThreads;
  mgh_pwrel_compare r = pwrel_empty();
  const uint32_t i0 = threadIdx.x * per;
  for (uint32_t i = i0; i < i0 + per && i < count; i++) pwrel_merge(r, partials[i]);
  for (int off = 32; off > 0; off >>= 1) pwrel_merge(r, pwrel_shuffled_down(r, off));
  __shared__ mgh_pwrel_compare sm[kCompareThreads / 64];
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)(kCompareThreads / 64); w++) pwrel_merge(r, sm[w]);
    if (r.argmax == ~(uint64_t)0) {
      r.max_rel_err = 0;
      r.argmax = 0;
    }
    *out = r;
  }
}

}  // namespace pwrel
}  // namespace mgh
