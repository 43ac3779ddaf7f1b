// What the decoder will see of a coefficient array at a given tolerance, without the integers ever
// being stored (mgh_quantize_roundtrip; mgh_achieved_errors recomposes and compares the result).
//
// For every element the kernel computes what k_quantize computes -- quantize_one() itself with the
// level's reciprocal quantizer and the level's volume -- and then what k_dequantize computes from that
// integer, in k_dequantize's own expression: (qz[level] * volume) * (T)q. The dictionary shift of
// prep_huffman cancels (k_quantize adds dict / 2, k_dequantize subtracts it, both in int64) and an
// out-of-dictionary value travels through the outlier list as the same int64, so neither appears here.
//
// Four tables in LDS (QTab, kernels_qwalk.hpp).
//
// A pure stream: one read and one write per element, no atomics; the walk is stream_levels
// (kernels_qwalk.hpp). A thread reads its vector before it writes it and no thread touches another's, so
// out == v (in place) is allowed; the pointers are therefore not __restrict__.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_qwalk.hpp"

namespace mgh {

constexpr int kQrThreads = 256;

template <typename T>
__global__ void __launch_bounds__(kQrThreads)
k_quantize_roundtrip(QuantMeta m, size_t total, const T *v, const int *__restrict__ marks,
                     const T *__restrict__ tab /* [4][nlev]: rqz, quantize volumes, qz, dequantize volumes */,
                     int nlev, T *out) {
  __shared__ T s_tab[4][kMaxLevels];
  stage_tables<kQrThreads>(tab, nlev, s_tab);
  __syncthreads();

  auto roundtrip = [&](T t, int level) -> T {
    const int64_t qd = quantize_one(t, s_tab[kTabRqz][level], m.calc_vol ? s_tab[kTabQvol][level] : (T)1);
    const T volume = m.calc_vol ? s_tab[kTabDvol][level] : (T)1;
    return (s_tab[kTabQz][level] * volume) * (T)qd;
  };
  constexpr int VN = Vec16<T>::N;
  typedef T NV __attribute__((ext_vector_type(VN)));
  stream_levels<kQrThreads, VN>(
      m, marks, total, aligned16(v, out),
      [&](size_t i, LevelCursor &cur) {
        const NV x = reinterpret_cast<const NV *>(v)[i];
        NV y;
#pragma unroll
        for (int u = 0; u < VN; u++) y[u] = roundtrip(x[u], cur.next(u + 1 < VN));
        reinterpret_cast<NV *>(out)[i] = y;
      },
      [&](size_t k, int level) { out[k] = roundtrip(v[k], level); });
}

}  // namespace mgh
