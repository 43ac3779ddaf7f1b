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
// The walk is stream_levels (kernels_qwalk.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_qwalk.hpp"

namespace mgh {

constexpr int kQhThreads = 512;

template <typename T, int K>
__global__ void __launch_bounds__(kQhThreads)
k_quantize_histograms(QuantMeta m, size_t total, const T *__restrict__ v, const int *__restrict__ marks,
                      const T *__restrict__ qz /* [K][nlev] */, const T *__restrict__ vol /* [nlev] */, int nlev,
                      int dict, unsigned *__restrict__ freq /* [K][dict] */,
                      unsigned long long *__restrict__ outliers /* [K] */) {
  extern __shared__ unsigned qh_bins[];  // [K][dict]
  __shared__ T s_qz[K][kMaxLevels];
  __shared__ T s_vol[1][kMaxLevels];
  __shared__ unsigned s_out[(kQhThreads / 64) * K];
  for (int i = threadIdx.x; i < K * dict; i += kQhThreads) qh_bins[i] = 0;
  stage_tables<kQhThreads>(qz, nlev, s_qz);
  stage_tables<kQhThreads>(vol, nlev, s_vol);
  __syncthreads();

  const int64_t half = (int64_t)dict / 2;
  unsigned oc[K];
#pragma unroll
  for (int k = 0; k < K; k++) oc[k] = 0;
  auto count = [&](T t, int level) {
    const T volume = m.calc_vol ? s_vol[0][level] : (T)1;
#pragma unroll
    for (int k = 0; k < K; k++) {
      int64_t q = quantize_one(t, s_qz[k][level], volume);
      q += half;
      if (q >= 0 && q < (int64_t)dict) {
        atomicAdd(&qh_bins[k * dict + (int)q], 1u);
      } else {
        atomicAdd(&qh_bins[k * dict], 1u);
        oc[k]++;
      }
    }
  };
  constexpr int VN = Vec16<T>::N;
  typedef T NV __attribute__((ext_vector_type(VN)));
  stream_levels<kQhThreads, VN>(
      m, marks, total, aligned16(v),
      [&](size_t i, LevelCursor &cur) {
        const NV x = reinterpret_cast<const NV *>(v)[i];
#pragma unroll
        for (int u = 0; u < VN; u++) count(x[u], cur.next(u + 1 < VN));
      },
      [&](size_t k, int level) { count(v[k], level); });

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
