// Precision layers (DESIGN.md sections 4 and 8): tier k of a layer set stores the quantized residual the
// tiers before it left in the COEFFICIENTS, so the two kernels here are the quantizer with one more
// output (writer) and the dequantizer that adds to what is there (reader).
//
// k_quantize_symbols_residual is k_quantize_symbols (kernels_qsym.hpp) -- the same walk, quantize_one()
// with the level's reciprocal quantizer and volume plus dict / 2, symbol 0 and an (index, int64) pair for
// an out-of-dictionary value, one slot request per workgroup and round, a counter that counts past the
// capacity, the optional LDS histogram -- which in addition stores, per element,
//     r_out = r - (qz[level] * vol_d[level]) * (T)q
// with q the exact int64 BEFORE the dictionary shift (for an outlier: the value that travels through the
// list, never the symbol 0 stored in its place) and the subtrahend k_dequantize's own expression on
// k_dequantize's own two tables. So FOUR tables in LDS, as in k_quantize_roundtrip (kernels_qround.hpp):
// the quantizer's volumes are not the bit-wise reciprocals of the dequantizer's. Multiply, multiply and
// subtract are three IEEE operations (the build has -ffp-contract=off). A thread reads its vector before
// it writes it and no thread touches another's, so r_out == v (in place) is allowed; the two pointers are
// therefore not __restrict__.
//
// k_dequantize_add is k_dequantize on int64 integers whose outliers are written back already
// (k_outlier_restore), vectorised like k_quantize_roundtrip: persistent workgroups, the row's level once
// per vector, the two tables in LDS. FIRST stores k_dequantize's value (it is not added to zero: -0.0
// stays -0.0); otherwise acc = acc + that value, one IEEE add. 8 + esz bytes read (2 esz with the
// accumulator) and esz written per element, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_v1.hpp"
#include "kernels_fused.hpp"  // kMaxLevels
#include "kernels_qsym.hpp"   // kQsThreads

namespace mgh {

template <typename T, bool HIST>
__global__ void __launch_bounds__(kQsThreads)
k_quantize_symbols_residual(QuantMeta m, size_t total, const T *v, const int *__restrict__ marks,
                            const T *__restrict__ tab /* [4][nlev]: rqz, quantize volumes, qz, dequantize volumes */,
                            int nlev, int dict, uint16_t *__restrict__ sym, unsigned *__restrict__ freq /* [dict], HIST only */,
                            unsigned long long *outlier_count, uint64_t *__restrict__ outlier_idx,
                            int64_t *__restrict__ outlier_val, unsigned long long outlier_cap, T *r_out) {
  extern __shared__ unsigned qs_bins[];  // [dict], HIST only
  __shared__ T s_rqz[kMaxLevels];
  __shared__ T s_qvol[kMaxLevels];
  __shared__ T s_qz[kMaxLevels];
  __shared__ T s_dvol[kMaxLevels];
  __shared__ unsigned wcnt[kQsThreads / 64];
  __shared__ unsigned long long gbase;
  if (HIST)
    for (int i = threadIdx.x; i < dict; i += kQsThreads) qs_bins[i] = 0;
  for (int i = threadIdx.x; i < nlev; i += kQsThreads) {
    s_rqz[i] = tab[i];
    s_qvol[i] = tab[nlev + i];
    s_qz[i] = tab[2 * nlev + i];
    s_dvol[i] = tab[3 * nlev + i];
  }
  __syncthreads();

  const int64_t half = (int64_t)dict / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
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
  typedef uint16_t SV __attribute__((ext_vector_type(VN)));
  const bool vec_in = (reinterpret_cast<uintptr_t>(v) & 15) == 0;
  const bool vec_out = (reinterpret_cast<uintptr_t>(sym) & (sizeof(SV) - 1)) == 0;
  const bool vec_res = (reinterpret_cast<uintptr_t>(r_out) & 15) == 0;
  const size_t ngroup = (total + VN - 1) / VN;
  unsigned centre = 0;  // HIST: symbols dict / 2 this thread has seen
  // (uniform trip count per workgroup: the barriers below are reached by every thread)
  const size_t stride = (size_t)gridDim.x * kQsThreads;
  for (size_t gb = (size_t)blockIdx.x * kQsThreads; gb < ngroup; gb += stride) {
    const size_t g = gb + threadIdx.x;
    const size_t lin0 = g * VN;
    const int cnt = g < ngroup ? (int)(total - lin0 < (size_t)VN ? total - lin0 : (size_t)VN) : 0;
    const bool whole = cnt == VN;
    NV x;
#pragma unroll
    for (int u = 0; u < VN; u++) x[u] = (T)0;
    if (whole && vec_in) {
      x = reinterpret_cast<const NV *>(v)[g];
    } else {
#pragma unroll
      for (int u = 0; u < VN; u++)
        if (u < cnt) x[u] = v[lin0 + u];
    }
    int64_t qd[VN];
    bool outl[VN];
    NV res;
    unsigned mine = 0;
    uint32_t row = 0, col = 0;
    int rl = 0;
    if (m.calc_vol && cnt > 0) {
      const uint32_t lin = (uint32_t)lin0;
      row = lin / nf;
      col = lin - row * nf;
      rl = slow_level(row);
    }
#pragma unroll
    for (int u = 0; u < VN; u++) {
      qd[u] = 0;
      outl[u] = false;
      res[u] = (T)0;
      if (u < cnt) {
        int level = 0;
        if (m.calc_vol) {
          const int lv = fmarks[col];
          level = lv > rl ? lv : rl;
          if (++col == nf) {  // (the group runs on into the next row)
            col = 0;
            row++;
            if (u + 1 < cnt) rl = slow_level(row);
          }
        }
        const int64_t q = quantize_one(x[u], s_rqz[level], m.calc_vol ? s_qvol[level] : (T)1);
        const T volume = m.calc_vol ? s_dvol[level] : (T)1;
        const T back = (s_qz[level] * volume) * (T)q;  // (k_dequantize's value of this integer)
        res[u] = x[u] - back;
        qd[u] = q + half;
        outl[u] = !(qd[u] >= 0 && qd[u] < (int64_t)dict);
        mine += outl[u] ? 1u : 0u;
      }
    }
    if (whole && vec_res) {
      reinterpret_cast<NV *>(r_out)[g] = res;
    } else {
#pragma unroll
      for (int u = 0; u < VN; u++)
        if (u < cnt) r_out[lin0 + u] = res[u];
    }
    if (__syncthreads_or((int)mine)) {
      unsigned incl = mine;  // inclusive scan of the counts inside the wave
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
      }
      if (lane == 63) wcnt[wave] = incl;
      __syncthreads();
      if (threadIdx.x == 0) {
        unsigned tot = 0;
        for (int w = 0; w < kQsThreads / 64; w++) {
          const unsigned c = wcnt[w];
          wcnt[w] = tot;
          tot += c;
        }
        gbase = tot ? atomicAdd(outlier_count, (unsigned long long)tot) : 0ull;
      }
      __syncthreads();
      unsigned long long o = gbase + wcnt[wave] + (incl - mine);
#pragma unroll
      for (int u = 0; u < VN; u++)
        if (outl[u]) {
          if (o < outlier_cap) {
            outlier_idx[o] = lin0 + u;
            outlier_val[o] = qd[u];
          }
          qd[u] = 0;
          o++;
        }
      __syncthreads();  // (wcnt / gbase are rewritten by the next round)
    }
    SV s;
#pragma unroll
    for (int u = 0; u < VN; u++) {
      s[u] = (uint16_t)qd[u];
      if (HIST && u < cnt) {
        if (qd[u] == half) centre++;
        else atomicAdd(&qs_bins[(int)qd[u]], 1u);
      }
    }
    if (whole && vec_out) {
      reinterpret_cast<SV *>(sym)[g] = s;
    } else {
#pragma unroll
      for (int u = 0; u < VN; u++)
        if (u < cnt) sym[lin0 + u] = s[u];
    }
  }

  if (HIST) {
    for (int off = 32; off > 0; off >>= 1) centre += __shfl_down(centre, off, 64);
    if (lane == 0 && centre) atomicAdd(&qs_bins[(int)half], centre);
    __syncthreads();  // (every count of the workgroup is in the bins)
    for (int i = threadIdx.x; i < dict; i += kQsThreads)
      if (qs_bins[i]) atomicAdd(&freq[i], qs_bins[i]);
  }
}

constexpr int kQaThreads = 256;

template <typename T, bool FIRST>
__global__ void __launch_bounds__(kQaThreads)
k_dequantize_add(QuantMeta m, size_t total, const int64_t *__restrict__ q, const int *__restrict__ marks,
                 const T *__restrict__ tab /* [2][nlev]: quantizers, dequantize volumes */, int nlev, int64_t shift,
                 T *__restrict__ acc) {
  __shared__ T s_qz[kMaxLevels];
  __shared__ T s_dvol[kMaxLevels];
  for (int i = threadIdx.x; i < nlev; i += kQaThreads) {
    s_qz[i] = tab[i];
    s_dvol[i] = tab[nlev + i];
  }
  __syncthreads();

  auto value = [&](int64_t qd, int level) -> T {
    const T volume = m.calc_vol ? s_dvol[level] : (T)1;
    return (s_qz[level] * volume) * (T)(qd - shift);
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
  typedef int64_t Q2 __attribute__((ext_vector_type(2)));  // (16 bytes: a vector of T takes VN / 2 of them)
  const size_t tid = (size_t)blockIdx.x * kQaThreads + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * kQaThreads;
  size_t done = 0;
  if (((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(acc)) & 15) == 0) {
    const size_t nvec = total / VN;
    const Q2 *qv = reinterpret_cast<const Q2 *>(q);
    NV *av = reinterpret_cast<NV *>(acc);
    for (size_t i = tid; i < nvec; i += nth) {
      int64_t qd[VN];
#pragma unroll
      for (int u = 0; u < VN; u += 2) {
        const Q2 two = qv[i * (VN / 2) + u / 2];
        qd[u] = two[0];
        qd[u + 1] = two[1];
      }
      NV y;
      if (!FIRST) y = av[i];
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
        const T add = value(qd[u], level);
        y[u] = FIRST ? add : y[u] + add;
      }
      av[i] = y;
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
    const T add = value(q[k], level);
    acc[k] = FIRST ? add : acc[k] + add;
  }
}

}  // namespace mgh
