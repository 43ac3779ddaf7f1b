// Error statistics of two arrays in one pass (mgh_compare, mgh_verify): mgh_error_stats of
// a (the reference) against b. Two stages, no floating-point atomics:
//   k_compare / k_compare_ld   workgroup g reduces the contiguous slab g of the LOGICAL array
//                              (compare_plan.hpp) and stores ONE partial mgh_error_stats;
//   k_compare_final            one workgroup folds the partials in ascending order with merge().
// Which element a lane takes, and in which order anything is added, depends on the number of
// elements and, for dense arrays, on where a lies relative to a 16-byte boundary (the scalar head of
// a slab): with both the same, the result is bit-reproducible from call to call. The same data at
// another alignment of a keeps every exact field and may round the two sums differently.
// Per element: d = a - b and |d| in T (ErrorCalculator.h:57-64), the sums in double. A position
// whose d is not finite is counted and takes part in nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "compare_plan.hpp"
#include "kernels_v1.hpp"
#include "ld_view.hpp"

namespace mgh {

// What a lane (then a wave) has gathered. Empty: no position yet -- the extremes are set so that
// any finite position replaces them.
template <typename T> struct CompareAcc {
  uint64_t fin = 0, bad = 0;  // positions that took part / whose difference is not finite
  T maxe = (T)-1;
  uint64_t arg = ~(uint64_t)0;
  double sse = 0, rss = 0;
  T rmin = std::numeric_limits<T>::infinity(), rmax = -std::numeric_limits<T>::infinity(), ramax = (T)-1;

  // one position; a lane meets its positions in ascending order of idx, so `>` keeps the lowest
  __device__ __forceinline__ void take(T a, T b, uint64_t idx) {
    const T d = a - b;
    const bool ok = isfinite(d);  // (then a and b are finite too)
    const T e = abs_t(d), aa = abs_t(a);
    const double ed = (double)e, ad = (double)a;
    fin += ok ? 1 : 0;
    bad += ok ? 0 : 1;
    if (ok && e > maxe) {
      maxe = e;
      arg = idx;
    }
    sse += ok ? ed * ed : 0.0;
    rss += ok ? ad * ad : 0.0;
    rmin = ok && a < rmin ? a : rmin;
    rmax = ok && a > rmax ? a : rmax;
    ramax = ok && aa > ramax ? aa : ramax;
  }
  // `o` covers positions BEHIND this one's in the order of the sums (a higher lane, a later wave)
  __device__ __forceinline__ void fold(const CompareAcc &o) {
    fin += o.fin;
    bad += o.bad;
    if (o.maxe > maxe || (o.maxe == maxe && o.arg < arg)) {
      maxe = o.maxe;
      arg = o.arg;
    }
    sse += o.sse;
    rss += o.rss;
    rmin = o.rmin < rmin ? o.rmin : rmin;
    rmax = o.rmax > rmax ? o.rmax : rmax;
    ramax = o.ramax > ramax ? o.ramax : ramax;
  }
  __device__ __forceinline__ CompareAcc shuffled_down(int off) const {
    CompareAcc o;
    o.fin = __shfl_down((unsigned long long)fin, off, 64);
    o.bad = __shfl_down((unsigned long long)bad, off, 64);
    o.maxe = __shfl_down(maxe, off, 64);
    o.arg = __shfl_down((unsigned long long)arg, off, 64);
    o.sse = __shfl_down(sse, off, 64);
    o.rss = __shfl_down(rss, off, 64);
    o.rmin = __shfl_down(rmin, off, 64);
    o.rmax = __shfl_down(rmax, off, 64);
    o.ramax = __shfl_down(ramax, off, 64);
    return o;
  }
  __device__ __forceinline__ mgh_error_stats stats() const {
    mgh_error_stats s;
    s.n = fin + bad;
    s.nonfinite = bad;
    s.max_abs_err = fin ? (double)maxe : 0.0;
    s.argmax = fin ? arg : 0;
    s.sum_sq_err = sse;
    s.ref_min = fin ? (double)rmin : 0.0;
    s.ref_max = fin ? (double)rmax : 0.0;
    s.ref_abs_max = fin ? (double)ramax : 0.0;
    s.ref_sum_sq = rss;
    return s;
  }
};

// wave64 shuffle reduction, then the four waves through LDS in ascending order; thread 0 stores
template <typename T>
__device__ __forceinline__ void compare_store_partial(CompareAcc<T> acc, mgh_error_stats *out) {
  for (int off = 32; off > 0; off >>= 1) acc.fold(acc.shuffled_down(off));
  __shared__ mgh_error_stats sm[kCompareThreads / 64];
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc.stats();
  __syncthreads();
  if (threadIdx.x == 0) {
    mgh_error_stats r = sm[0];
    for (int w = 1; w < (int)(kCompareThreads / 64); w++) merge(r, sm[w], 0);
    *out = r;
  }
}

// Dense arrays. Slab [lo, hi) of workgroup g: a scalar head up to the first 16-byte boundary of a,
// 16-byte loads over the body (b with whatever alignment it has there), a scalar tail.
template <typename T>
__global__ void __launch_bounds__(256)
k_compare(const T *__restrict__ a, const T *__restrict__ b, uint64_t n, uint64_t slab, mgh_error_stats *partials) {
  constexpr int VN = Vec16<T>::N;
  typedef T NV __attribute__((ext_vector_type(VN)));
  typedef T NVU __attribute__((ext_vector_type(VN), aligned(sizeof(T))));  // b: element alignment only
  const uint64_t lo = (uint64_t)blockIdx.x * slab;
  const uint64_t hi = lo + slab < n ? lo + slab : n;
  const uint64_t len = hi - lo;
  const uint32_t t = threadIdx.x;
  const T *pa = a + lo, *pb = b + lo;
  CompareAcc<T> acc;
  const uint32_t mis = (uint32_t)((reinterpret_cast<uintptr_t>(pa) & 15) / sizeof(T));
  uint64_t head = mis ? VN - mis : 0;
  head = head < len ? head : len;
  if (t < head) acc.take(pa[t], pb[t], lo + t);
  const uint64_t nv = (len - head) / VN;
  const NV *va = reinterpret_cast<const NV *>(pa + head);
  const T *vb = pb + head;
  const uint64_t first = lo + head;
  // one 16-byte load per array and lane in flight, plain loads ("Error statistics")
  auto body = [&](auto load_b) {
    for (uint64_t v = t; v < nv; v += kCompareThreads) {
      const NV x = va[v], y = load_b(v);
#pragma unroll
      for (int u = 0; u < VN; u++) acc.take(x[u], y[u], first + v * VN + u);
    }
  };
  if ((reinterpret_cast<uintptr_t>(vb) & 15) == 0) {
    const NV *q = reinterpret_cast<const NV *>(vb);
    body([&](uint64_t v) -> NV { return q[v]; });
  } else {
    const NVU *q = reinterpret_cast<const NVU *>(vb);
    body([&](uint64_t v) -> NV { return (NV)q[v]; });
  }
  const uint64_t done = head + nv * VN;
  if (done + t < len) acc.take(pa[done + t], pb[done + t], lo + done + t);
  compare_store_partial(acc, partials + blockIdx.x);
}

// Arrays with strides (a leading dimension; a box of a larger array), each its own view of the same
// logical shape. The slab is a range of the logical array: the rows it meets, one wave per row.
template <typename T>
__global__ void __launch_bounds__(256)
k_compare_ld(const T *__restrict__ a, LdView Va, const T *__restrict__ b, LdView Vb, uint64_t n, uint64_t slab,
             mgh_error_stats *partials) {
  const uint64_t lo = (uint64_t)blockIdx.x * slab;
  const uint64_t hi = lo + slab < n ? lo + slab : n;
  const uint32_t nf = Va.ext[MGH_MAX_DIM - 1];
  const int lane = threadIdx.x & 63;
  CompareAcc<T> acc;
  const uint64_t r0 = lo / nf, r1 = (hi - 1) / nf;
  for (uint64_t row = r0 + (threadIdx.x >> 6); row <= r1; row += kCompareThreads / 64) {
    const uint64_t base = row * nf;
    const uint32_t c0 = row == r0 ? (uint32_t)(lo - base) : 0u;
    const uint32_t c1 = row == r1 ? (uint32_t)(hi - base) : nf;
    const T *pa = a + ld_row_offset(Va, row);
    const T *pb = b + ld_row_offset(Vb, row);
    for (uint32_t k = c0 + lane; k < c1; k += 64) acc.take(pa[k], pb[k], base + k);
  }
  compare_store_partial(acc, partials + blockIdx.x);
}

// k_compare_ld with a mask (mgh_compare_masked_, mgh_verify_masked): a position whose bit is set takes part in
// nothing. The mask is a bit array seen through a view of its own: element (i_0 ...) has bit bit0 + the view's
// offset, so a box of a larger array is held against that array's mask where it lies. The 64 positions a wave
// takes at once are 64 consecutive bits: the one or two words that hold them are read at a wave-uniform
// address, once for the 64 lanes, and shifted into place. Which lane takes which position, and in which order,
// is k_compare_ld's: with an all-zero mask the two give the same bits.
template <typename T>
__global__ void __launch_bounds__(256)
k_compare_masked(const T *__restrict__ a, LdView Va, const T *__restrict__ b, LdView Vb,
                 const unsigned long long *__restrict__ words, LdView Vm, uint64_t bit0, uint64_t n, uint64_t slab,
                 mgh_error_stats *partials) {
  const uint64_t lo = (uint64_t)blockIdx.x * slab;
  const uint64_t hi = lo + slab < n ? lo + slab : n;
  const uint32_t nf = Va.ext[MGH_MAX_DIM - 1];
  const int lane = threadIdx.x & 63;
  CompareAcc<T> acc;
  const uint64_t r0 = lo / nf, r1 = (hi - 1) / nf;
  for (uint64_t row = r0 + (threadIdx.x >> 6); row <= r1; row += kCompareThreads / 64) {
    const uint64_t base = row * nf;
    const uint32_t c0 = row == r0 ? (uint32_t)(lo - base) : 0u;
    const uint32_t c1 = row == r1 ? (uint32_t)(hi - base) : nf;
    const T *pa = a + ld_row_offset(Va, row);
    const T *pb = b + ld_row_offset(Vb, row);
    const uint64_t mrow = bit0 + ld_row_offset(Vm, row);
    for (uint32_t k0 = c0; k0 < c1; k0 += 64) {  // (k0 is the wave's)
      const uint64_t p = mrow + k0;
      const int sh = (int)(p & 63);
      const uint32_t left = c1 - k0 < 64u ? c1 - k0 : 64u;
      unsigned long long m = words[p >> 6] >> sh;
      if (compare_mask_second_word(p, left)) m |= words[(p >> 6) + 1] << (64 - sh);  // (only where the bits reach it)
      const uint32_t k = k0 + lane;
      if (k < c1 && !((m >> lane) & 1)) acc.take(pa[k], pb[k], base + k);
    }
  }
  compare_store_partial(acc, partials + blockIdx.x);
}

// The partials (their argmax already an index of the whole logical array) into one result: lane t
// folds the contiguous run [t * per, (t + 1) * per), then lanes, then waves, always the lower
// workgroups first.
__global__ void __launch_bounds__(256)
k_compare_final(const mgh_error_stats *__restrict__ partials, uint32_t count, mgh_error_stats *out) {
  const uint32_t per = (count + kCompareThreads - 1) / kCompareThreads;
  mgh_error_stats r{};
  const uint32_t i0 = threadIdx.x * per;
  for (uint32_t i = i0; i < i0 + per && i < count; i++) merge(r, partials[i], 0);
  for (int off = 32; off > 0; off >>= 1) {
    mgh_error_stats o;
    o.n = __shfl_down((unsigned long long)r.n, off, 64);
    o.nonfinite = __shfl_down((unsigned long long)r.nonfinite, off, 64);
    o.max_abs_err = __shfl_down(r.max_abs_err, off, 64);
    o.argmax = __shfl_down((unsigned long long)r.argmax, off, 64);
    o.sum_sq_err = __shfl_down(r.sum_sq_err, off, 64);
    o.ref_min = __shfl_down(r.ref_min, off, 64);
    o.ref_max = __shfl_down(r.ref_max, off, 64);
    o.ref_abs_max = __shfl_down(r.ref_abs_max, off, 64);
    o.ref_sum_sq = __shfl_down(r.ref_sum_sq, off, 64);
    merge(r, o, 0);
  }
  __shared__ mgh_error_stats sm[kCompareThreads / 64];
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)(kCompareThreads / 64); w++) merge(r, sm[w], 0);
    *out = r;
  }
}

}  // namespace mgh
