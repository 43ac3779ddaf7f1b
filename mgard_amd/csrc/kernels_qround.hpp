// What the decoder will see of a coefficient array at a given tolerance, without the integers ever
// being stored (mgh_quantize_roundtrip; mgh_achieved_errors recomposes and compares the result).
//
// For every element the kernel computes what k_quantize computes -- quantize_one() itself with the
// level's reciprocal quantizer and the level's volume -- and then what k_dequantize computes from that
// integer, in k_dequantize's own expression: (qz[level] * volume) * (T)q. The dictionary shift of
// prep_huffman cancels (k_quantize adds dict / 2, k_dequantize subtracts it, both in int64) and an
// out-of-dictionary value travels through the outlier list as the same int64, so neither appears here.
//
// FOUR tables, not three: mgh_quantize uploads the reciprocal quantizers with the volumes
// level_volume(l, false), mgh_dequantize the quantizers with the volumes level_volume(l, true) -- the
// square root of the product of the RECIPROCAL cell volumes, which is not the bit-wise reciprocal of
// the first. All four live in LDS.
//
// A pure stream: one read and one write per element, no atomics. The walk is k_quantize_histograms's
// (kernels_qhist.hpp): persistent workgroups stride over the array in 16-byte vectors of the fastest
// dimension where both pointers allow it; a vector divides its linear index once (32-bit: the entry
// point refuses 2^32 elements and more), takes the level of the slow dimensions from the row index and
// moves on by one column per element. A thread reads its vector before it writes it and no thread
// touches another's, so out == v (in place) is allowed; the pointers are therefore not __restrict__.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_v1.hpp"
#include "kernels_fused.hpp"  // kMaxLevels

namespace mgh {

constexpr int kQrThreads = 256;

template <typename T>
__global__ void __launch_bounds__(kQrThreads)
k_quantize_roundtrip(QuantMeta m, size_t total, const T *v, const int *__restrict__ marks,
                     const T *__restrict__ tab /* [4][nlev]: rqz, quantize volumes, qz, dequantize volumes */,
                     int nlev, T *out) {
  __shared__ T s_rqz[kMaxLevels];
  __shared__ T s_qvol[kMaxLevels];
  __shared__ T s_qz[kMaxLevels];
  __shared__ T s_dvol[kMaxLevels];
  for (int i = threadIdx.x; i < nlev; i += kQrThreads) {
    s_rqz[i] = tab[i];
    s_qvol[i] = tab[nlev + i];
    s_qz[i] = tab[2 * nlev + i];
    s_dvol[i] = tab[3 * nlev + i];
  }
  __syncthreads();

  auto roundtrip = [&](T t, int level) -> T {
    const int64_t qd = quantize_one(t, s_rqz[level], m.calc_vol ? s_qvol[level] : (T)1);
    const T volume = m.calc_vol ? s_dvol[level] : (T)1;
    return (s_qz[level] * volume) * (T)qd;
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
  const size_t tid = (size_t)blockIdx.x * kQrThreads + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * kQrThreads;
  size_t done = 0;
  if (((reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(out)) & 15) == 0) {
    const size_t nvec = total / VN;
    const NV *vv = reinterpret_cast<const NV *>(v);
    NV *ov = reinterpret_cast<NV *>(out);
    for (size_t i = tid; i < nvec; i += nth) {
      const NV x = vv[i];
      NV y;
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
        y[u] = roundtrip(x[u], level);
      }
      ov[i] = y;
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
    out[k] = roundtrip(v[k], level);
  }
}

}  // namespace mgh
