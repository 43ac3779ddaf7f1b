// Histograms of the symbols the quantizer WOULD store, for several tolerances at once, from one read
// of the coefficient array (mgh_quantize_histograms; size_plan.hpp prices a record from them).
//
// For every element and every tolerance k the kernel computes what k_quantize computes with
// prep_huffman = 1 -- quantize_one() itself with the level's quantizer of tolerance k and the level's
// volume, plus dict / 2 -- and counts it: in its bin when it lies in [0, dict), else in bin 0 and in
// the outlier count of k (the quantizer stores 0 for an outlier, and huff::k_histogram counts that 0).
//
// The K histograms are privatised in LDS (K x dict 32-bit counters: four of 8192 bins are 128 KB of
// the CU's 160), few persistent workgroups stride over the array, and a workgroup ends with one global
// atomic per used bin and one per tolerance with outliers, like huff::k_histogram.
//
// The level of an element is the largest of its per-dimension marks (level_of). The array is walked in
// 16-byte vectors of the fastest dimension where the pointer allows it: a vector divides its linear
// index once (32-bit: the entry point refuses 2^32 elements and more, the counters are 32-bit), takes
// the level of the slow dimensions from the row index, and moves on by one column per element.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_v1.hpp"
#include "kernels_fused.hpp"  // kMaxLevels

namespace mgh {

constexpr int kQhThreads = 512;

template <typename T, int K>
__global__ void __launch_bounds__(kQhThreads)
k_quantize_histograms(QuantMeta m, size_t total, const T *__restrict__ v, const int *__restrict__ marks,
                      const T *__restrict__ qz /* [K][nlev] */, const T *__restrict__ vol /* [nlev] */, int nlev,
                      int dict, unsigned *__restrict__ freq /* [K][dict] */,
                      unsigned long long *__restrict__ outliers /* [K] */) {
  extern __shared__ unsigned qh_bins[];  // [K][dict]
  __shared__ T s_qz[K * kMaxLevels];
  __shared__ T s_vol[kMaxLevels];
  __shared__ unsigned s_out[(kQhThreads / 64) * K];
  for (int i = threadIdx.x; i < K * dict; i += kQhThreads) qh_bins[i] = 0;
  for (int i = threadIdx.x; i < K * nlev; i += kQhThreads) s_qz[i] = qz[i];
  for (int i = threadIdx.x; i < nlev; i += kQhThreads) s_vol[i] = vol[i];
  __syncthreads();

  const int64_t half = (int64_t)dict / 2;
  unsigned oc[K];
#pragma unroll
  for (int k = 0; k < K; k++) oc[k] = 0;
  auto count = [&](T t, int level) {
    const T volume = m.calc_vol ? s_vol[level] : (T)1;
#pragma unroll
    for (int k = 0; k < K; k++) {
      int64_t q = quantize_one(t, s_qz[k * nlev + level], volume);
      q += half;
      if (q >= 0 && q < (int64_t)dict) {
        atomicAdd(&qh_bins[k * dict + (int)q], 1u);
      } else {
        atomicAdd(&qh_bins[k * dict], 1u);
        oc[k]++;
      }
    }
  };
  // rows of the fastest dimension: lin = row * nf + col
  const int fd = m.D - 1;
  const uint32_t nf = m.shape[fd];
  const int *__restrict__ fmarks = marks + m.markoff[fd];
  auto slow_level = [&](uint32_t row) {
    int level = 0;
    for (int d = fd - 1; d >= 0; d--) {
      const uint32_t id = row % m.shape[d];
      row /= m.shape[d];
      const int lv = marks[m.markoff[d] + id];
      level = lv > level ? lv : level;
    }
    return level;
  };

  constexpr int VN = Vec16<T>::N;
  typedef T NV __attribute__((ext_vector_type(VN)));
  const size_t tid = (size_t)blockIdx.x * kQhThreads + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * kQhThreads;
  size_t done = 0;
  if ((reinterpret_cast<uintptr_t>(v) & 15) == 0) {
    const size_t nvec = total / VN;
    const NV *vv = reinterpret_cast<const NV *>(v);
    for (size_t i = tid; i < nvec; i += nth) {
      const NV x = vv[i];
      const uint32_t lin = (uint32_t)(i * VN);
      uint32_t row = 0, col = 0;
      int rl = 0;
      if (m.calc_vol) {
        row = lin / nf;
        col = lin - row * nf;
        rl = slow_level(row);
      }
#pragma unroll
      for (int u = 0; u < VN; u++) {
        int level = 0;
        if (m.calc_vol) {
          const int lv = fmarks[col];
          level = lv > rl ? lv : rl;
          if (++col == nf) {  // (the vector runs on into the next row)
            col = 0;
            row++;
            if (u + 1 < VN) rl = slow_level(row);
          }
        }
        count(x[u], level);
      }
    }
    done = nvec * VN;
  }
  for (size_t k = done + tid; k < total; k += nth) {
    int level = 0;
    if (m.calc_vol) {
      const uint32_t lin = (uint32_t)k, row = lin / nf, col = lin - row * nf;
      const int rl = slow_level(row), lv = fmarks[col];
      level = lv > rl ? lv : rl;
    }
    count(v[k], level);
  }

  // outlier counts: wave, workgroup, one global atomic per tolerance
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; k++) {
    unsigned c = oc[k];
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if (lane == 0) s_out[wave * K + k] = c;
  }
  __syncthreads();  // (also: every count of the workgroup is in the bins)
  if (threadIdx.x < K) {
    unsigned long long c = 0;
    for (int w = 0; w < kQhThreads / 64; w++) c += s_out[w * K + threadIdx.x];
    if (c) atomicAdd(&outliers[threadIdx.x], c);
  }
  for (int i = threadIdx.x; i < K * dict; i += kQhThreads)
    if (qh_bins[i]) atomicAdd(&freq[i], qh_bins[i]);
}

}  // namespace mgh
