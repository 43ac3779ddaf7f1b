// Missing-value masks: the three streaming kernels behind mgh_mask_scan / mgh_mask_fill /
// mgh_mask_restore (include/mgard_hip.h; geometry and fill rule: mask_plan.hpp).
//   k_mask_scan     classifies every element, packs the mask -- one wave ballot is one word -- and reduces
//                   count, minimum and maximum of the VALID elements. All three are order-independent, so
//                   plain integer atomics give a deterministic result: the extremes travel as 64-bit keys
//                   whose unsigned order is the order of the doubles (-0.0 below +0.0).
//   k_mask_fill     one wave per segment of at most 1024 elements of a row. The wave keeps the segment's valid
//                   bits, re-aligned to the segment's first element, in 16 words of LDS; a masked element finds
//                   its source with count-leading / find-first on them. Only copies: nothing is computed.
//   k_mask_restore  stores one value at every masked position.
//   k_mask_sample   (mgh_mask_sample_) gathers the packed mask of a level grid, a coarsened grid or a window out of
//                   the array's: one wave ballot is one output word. Sampling -- a node is masked when the element
//                   it stands on is; valid values near masked regions still carry the fill's influence.
// fill and restore move bit patterns (W = uint32_t / uint64_t), so NaN payloads and -0.0 survive.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mask_plan.hpp"

namespace mgh {
namespace mask {

constexpr int kThreads = 256;                // four waves
constexpr int kWaves = kThreads / 64;
constexpr int kScanUnroll = 4;               // words (of 64 elements) a wave has in flight
constexpr unsigned kMaxBlocks = 256 * 8;     // grid cap of the grid-stride loops

__device__ inline unsigned long long order_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double key_value(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

__device__ inline bool nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
__device__ inline bool nonfinite(double v) {
  return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
}

// stats as four 64-bit words while the scan runs: [0] unused, [1] masked count, [2] key of the minimum,
// [3] key of the maximum
static __global__ void k_mask_stats_begin(unsigned long long *s) {
  if (threadIdx.x == 0) {
    s[0] = 0;
    s[1] = 0;
    s[2] = ~0ull;
    s[3] = 0;
  }
}
// ... and as mgh_mask_stats {n, n_masked, vmin, vmax} afterwards
static __global__ void k_mask_stats_end(unsigned long long *s, unsigned long long n) {
  if (threadIdx.x == 0) {
    const bool none = s[1] >= n;  // no valid element: vmin = vmax = 0
    s[0] = n;
    s[2] = none ? 0ull : (unsigned long long)__double_as_longlong(key_value(s[2]));
    s[3] = none ? 0ull : (unsigned long long)__double_as_longlong(key_value(s[3]));
  }
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
k_mask_scan(const T *__restrict__ data, uint64_t n, uint64_t nwords, int flags, T fill,
            unsigned long long *__restrict__ words, unsigned long long *stats) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t wave = (uint64_t)blockIdx.x * kWaves + wv, nwaves = (uint64_t)gridDim.x * kWaves;
  unsigned long long kmin = ~0ull, kmax = 0, masked = 0;
  // (the loop bounds are the wave's: every lane reaches every ballot)
  for (uint64_t w0 = wave * kScanUnroll; w0 < nwords; w0 += nwaves * kScanUnroll) {
    T v[kScanUnroll];
    bool in[kScanUnroll];
#pragma unroll
    for (int u = 0; u < kScanUnroll; u++) {
      const uint64_t i = (w0 + u) * 64 + lane;  // (a word past the last one lies past n as a whole)
      in[u] = i < n;
      v[u] = in[u] ? data[i] : T(0);
    }
#pragma unroll
    for (int u = 0; u < kScanUnroll; u++) {
      const bool m = in[u] && (((flags & 1) && nonfinite(v[u])) || ((flags & 2) && v[u] == fill));
      const unsigned long long bits = __ballot(m);  // the tail's lanes vote 0: the unused high bits are zero
      if (lane == 0 && w0 + u < nwords) {
        words[w0 + u] = bits;
        masked += (unsigned long long)__popcll(bits);
      }
      if (in[u] && !m) {
        const unsigned long long k = order_key((double)v[u]);
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long a = __shfl_xor(kmin, off), b = __shfl_xor(kmax, off);
    kmin = a < kmin ? a : kmin;
    kmax = b > kmax ? b : kmax;
  }
  __shared__ unsigned long long part[3][kWaves];
  if (lane == 0) {
    part[0][wv] = kmin;
    part[1][wv] = kmax;
    part[2][wv] = masked;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; w++) {
      kmin = part[0][w] < kmin ? part[0][w] : kmin;
      kmax = part[1][w] > kmax ? part[1][w] : kmax;
      masked += part[2][w];
    }
    if (masked) atomicAdd(&stats[1], masked);
    if (kmin != ~0ull) {  // (the workgroup saw a valid element)
      atomicMin(&stats[2], kmin);
      atomicMax(&stats[3], kmax);
    }
  }
}

// data and out may be the same array (in place: valid elements are not touched, and they are all a masked
// element ever reads), so neither is __restrict__.
template <typename W>
__global__ void __launch_bounds__(kThreads)
k_mask_fill(const W *data, const unsigned long long *__restrict__ words, uint64_t nwords, MaskSegments G, W c, W *out) {
  __shared__ unsigned long long valid[kWaves][kMaskSegmentWords];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool in_place = (const W *)out == data;
  // (the loop bounds are the workgroup's: every wave reaches both barriers, with or without a segment)
  for (uint64_t s0 = (uint64_t)blockIdx.x * kWaves; s0 < G.total; s0 += (uint64_t)gridDim.x * kWaves) {
    const uint64_t seg = s0 + wv;
    uint64_t start = 0, len = 0;
    if (seg < G.total) mask_segment(G, seg, start, len);
    if (lane < kMaskSegmentWords) {
      // valid bits of the segment's elements [64 lane, 64 lane + 64), bit k for element 64 lane + k: the
      // array's words shifted down by the bit the segment starts at, cut at the segment's end
      unsigned long long vb = 0;
      const uint64_t e0 = (uint64_t)lane * 64;
      if (e0 < len) {
        const uint64_t w = (start >> 6) + lane;  // (holds element start + e0 < n: w < nwords)
        const int sh = (int)(start & 63);
        unsigned long long m = words[w] >> sh;
        if (sh && w + 1 < nwords) m |= words[w + 1] << (64 - sh);
        const uint64_t left = len - e0;
        vb = ~m & (left >= 64 ? ~0ull : ((1ull << left) - 1));
      }
      valid[wv][lane] = vb;
    }
    __syncthreads();
    for (uint64_t e0 = 0; e0 < len; e0 += 64) {
      const uint64_t e = e0 + lane;
      if (e >= len) continue;
      const int cw = (int)(e0 >> 6);
      const unsigned long long vw = valid[wv][cw];
      if ((vw >> lane) & 1) {
        if (!in_place) out[start + e] = data[start + e];
        continue;
      }
      // the nearest valid element below, else the nearest above, else the constant
      int src = -1;
      const unsigned long long below = vw & ((1ull << lane) - 1);
      if (below) {
        src = cw * 64 + 63 - __clzll((long long)below);
      } else {
        for (int j = cw - 1; j >= 0 && src < 0; j--) {
          const unsigned long long u = valid[wv][j];
          if (u) src = j * 64 + 63 - __clzll((long long)u);
        }
      }
      if (src < 0) {
        const unsigned long long above = lane == 63 ? 0ull : vw & (~0ull << (lane + 1));
        if (above) {
          src = cw * 64 + __ffsll((long long)above) - 1;
        } else {
          for (int j = cw + 1; j < kMaskSegmentWords && src < 0; j++) {
            const unsigned long long u = valid[wv][j];
            if (u) src = j * 64 + __ffsll((long long)u) - 1;
          }
        }
      }
      out[start + e] = src >= 0 ? data[start + (uint64_t)src] : c;
    }
    __syncthreads();
  }
}

template <typename W>
__global__ void __launch_bounds__(kThreads)
k_mask_restore(const unsigned long long *__restrict__ words, uint64_t n, W value, W *__restrict__ data) {
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride)
    if ((words[i >> 6] >> (i & 63)) & 1) data[i] = value;
}

// mgh_mask_sample_: the packed mask of a dense array of A.out_shape whose element (i_0 ...) is the source's
// element (idx_0[i_0] ...). Shapes and lists are right-aligned in kMaskMaxDim dimensions with leading 1s, so
// every loop over them unrolls; a NULL list is the identity.
struct MaskSampleArgs {
  uint32_t shape[kMaskMaxDim], out_shape[kMaskMaxDim];
  const uint32_t *idx[kMaskMaxDim];
};

// One wave owns one output word at a time: lane l unravels output element 64 w + l, maps its coordinates through
// the lists (plain cached loads: the lists are small and every wave reads them) and reads the source bit; the
// ballot is the word. An entry outside the source's shape is not read for and votes 0, as a lane past the end
// does. count (may be NULL): masked outputs, one integer atomic per workgroup.
__global__ void __launch_bounds__(kThreads)
k_mask_sample(const unsigned long long *__restrict__ words, MaskSampleArgs A, uint64_t n_out, uint64_t nwords_out,
              unsigned long long *__restrict__ out_words, unsigned long long *count) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t wave = (uint64_t)blockIdx.x * kWaves + wv, nwaves = (uint64_t)gridDim.x * kWaves;
  unsigned long long masked = 0;
  // (the loop bounds are the wave's: every lane reaches the ballot)
  for (uint64_t w = wave; w < nwords_out; w += nwaves) {
    const uint64_t e = w * 64 + lane;
    bool m = false;
    if (e < n_out) {
      uint64_t flat;
      if (mask_sample_source(kMaskMaxDim, A.shape, A.out_shape, A.idx, (uint32_t)e, flat))
        m = (words[flat >> 6] >> (flat & 63)) & 1;
    }
    const unsigned long long bits = __ballot(m);
    if (lane == 0) {
      out_words[w] = bits;
      masked += (unsigned long long)__popcll(bits);
    }
  }
  if (!count) return;  // (uniform: no barrier is skipped by a part of the workgroup)
  __shared__ unsigned long long part[kWaves];
  if (lane == 0) part[wv] = masked;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; w++) masked += part[w];
    if (masked) atomicAdd(count, masked);
  }
}

} // namespace mask
} // namespace mgh
