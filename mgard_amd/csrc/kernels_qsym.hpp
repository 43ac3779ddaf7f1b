// A coefficient array to what the lossless stage reads, in one pass (mgh_quantize_symbols; the second
// entry into the high-level writer): 16-bit symbols, the outlier list and,
// optionally, the histogram of the symbols.
//
// For every element the kernel computes what k_quantize computes with prep_huffman = 1 --
// quantize_one() itself with the level's reciprocal quantizer and the level's volume, plus dict / 2 --
// and stores it as uint16_t when it lies in [0, dict); else it stores symbol 0 and appends (linear
// index, that int64) to the outlier list, as k_quantize does.
//
// Outlier slots are requested ONCE per workgroup and round (k_quantize's scheme: a request per wave
// queues on the counter), and none in a round without outliers. The counter goes
// on counting past `outlier_cap`; nothing is written past it.
//
// HIST: the stored symbols are counted in bins privatised in LDS (dict <= 16384: 64 KB); a workgroup
// ends with one global atomic per used bin, like huff::k_histogram, which this replaces. An outlier
// counts in bin 0, the symbol stored for it. The centre symbol dict / 2 -- most of a smooth field --
// is counted in a register and reaches its bin once per wave.
//
// The walk is k_quantize_histograms's (kernels_qhist.hpp): persistent workgroups stride over the array
// in groups of one 16-byte vector of the fastest dimension; a group divides its linear index once
// (32-bit: the entry point refuses 2^32 elements and more), takes the level of the slow dimensions from
// the row index and moves on by one column per element. A group is loaded as one vector where the
// pointer is 16-byte aligned and the group is whole, element by element otherwise (a misaligned view,
// the tail); its symbols leave as one plain vector store (8 bytes per 4 floats) on the same terms.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_v1.hpp"
#include "kernels_fused.hpp"  // kMaxLevels

namespace mgh {

constexpr int kQsThreads = 256;

template <typename T, bool HIST>
__global__ void __launch_bounds__(kQsThreads)
k_quantize_symbols(QuantMeta m, size_t total, const T *__restrict__ v, const int *__restrict__ marks,
                   const T *__restrict__ tab /* [2][nlev]: reciprocal quantizers, volumes */, int nlev, int dict,
                   uint16_t *__restrict__ sym, unsigned *__restrict__ freq /* [dict], HIST only */,
                   unsigned long long *outlier_count, uint64_t *__restrict__ outlier_idx,
                   int64_t *__restrict__ outlier_val, unsigned long long outlier_cap) {
  extern __shared__ unsigned qs_bins[];  // [dict], HIST only
  __shared__ T s_qz[kMaxLevels];
  __shared__ T s_vol[kMaxLevels];
  __shared__ unsigned wcnt[kQsThreads / 64];
  __shared__ unsigned long long gbase;
  if (HIST)
    for (int i = threadIdx.x; i < dict; i += kQsThreads) qs_bins[i] = 0;
  for (int i = threadIdx.x; i < nlev; i += kQsThreads) {
    s_qz[i] = tab[i];
    s_vol[i] = tab[nlev + i];
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
        qd[u] = quantize_one(x[u], s_qz[level], m.calc_vol ? s_vol[level] : (T)1) + half;
        outl[u] = !(qd[u] >= 0 && qd[u] < (int64_t)dict);
        mine += outl[u] ? 1u : 0u;
      }
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

}  // namespace mgh
