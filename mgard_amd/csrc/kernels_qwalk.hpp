// What the streaming quantizer passes share: k_quantize_histograms
// (kernels_qhist.hpp), k_quantize_roundtrip (kernels_qround.hpp), k_quantize_symbols,
// k_quantize_symbols_residual and k_dequantize_add (kernels_qsym.hpp). Device code only.
//
// THE WALK. Persistent workgroups stride over a dense array in 16-byte vectors of the fastest dimension.
// The level of an element is the largest of its per-dimension marks (level_of). A vector divides its
// linear index once (32-bit: the entry points refuse 2^32 elements and more) into row and column, takes
// the level of the slow dimensions from the row index, and moves on by one column per element; where it
// runs on into the next row it takes that row's level, unless no element of it is left to read. With
// m.calc_vol == 0 every level is 0 and `marks` is never read.
//
// The level tables arrive as rows of `nlev` values and are staged in LDS rows of kMaxLevels (the
// launchers refuse more levels). Where a pass reads the tables of the quantizer AND of the dequantizer it
// takes four rows, in the order of QTab: mgh_quantize uploads the reciprocal quantizers with the volumes
// level_volume(l, false), mgh_dequantize the quantizers with the volumes level_volume(l, true) -- the
// square root of the product of the RECIPROCAL cell volumes, which is not the bit-wise reciprocal of the
// first.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_v1.hpp"
#include "kernels_fused.hpp"  // kMaxLevels

namespace mgh {

enum QTab { kTabRqz = 0, kTabQvol = 1, kTabQz = 2, kTabDvol = 3 };

// rows of the fastest dimension: lin = row * nf + col
struct LevelCursor {
  const QuantMeta &m;
  const int *__restrict__ marks;
  const int *__restrict__ fmarks;
  const int fd;
  const uint32_t nf;
  uint32_t cur_row = 0, cur_col = 0;
  int rl = 0;  // level of the slow dimensions of cur_row

  __device__ __forceinline__ LevelCursor(const QuantMeta &m_, const int *__restrict__ marks_)
      : m(m_), marks(marks_), fmarks(marks_ + m_.markoff[m_.D - 1]), fd(m_.D - 1), nf(m_.shape[m_.D - 1]) {}

  __device__ __forceinline__ int slow_level(uint32_t row) const {
    int level = 0;
    for (int d = fd - 1; d >= 0; d--) {
      const uint32_t id = row % m.shape[d];
      row /= m.shape[d];
      const int lv = marks[m.markoff[d] + id];
      level = lv > level ? lv : level;
    }
    return level;
  }

  __device__ __forceinline__ void seek(uint32_t lin) {
    if (m.calc_vol) {
      cur_row = lin / nf;
      cur_col = lin - cur_row * nf;
      rl = slow_level(cur_row);
    }
  }

  // The level of the element under the cursor, which moves on by one. `more`: the caller will read
  // another element after this one.
  __device__ __forceinline__ int next(bool more) {
    int level = 0;
    if (m.calc_vol) {
      const int lv = fmarks[cur_col];
      level = lv > rl ? lv : rl;
      if (++cur_col == nf) {  // (the vector runs on into the next row)
        cur_col = 0;
        cur_row++;
        if (more) rl = slow_level(cur_row);
      }
    }
    return level;
  }

  // The level of the single element `lin`; the cursor stays where it is.
  __device__ __forceinline__ int at(uint32_t lin) const {
    int level = 0;
    if (m.calc_vol) {
      const uint32_t row = lin / nf, col = lin - row * nf;
      const int sl = slow_level(row), lv = fmarks[col];
      level = lv > sl ? lv : sl;
    }
    return level;
  }
};

// tab[NT][nlev] to NT rows in LDS (no barrier).
template <int THREADS, int NT, typename T>
__device__ __forceinline__ void stage_tables(const T *__restrict__ tab, int nlev, T (&s_tab)[NT][kMaxLevels]) {
  for (int i = threadIdx.x; i < nlev; i += THREADS) {
#pragma unroll
    for (int t = 0; t < NT; t++) s_tab[t][i] = tab[t * nlev + i];
  }
}

// The loop of a pure stream (one pass, no barriers): whole vectors of VN elements where `aligned` says
// that every pointer the kernel moves vectors through is 16-byte aligned, then a scalar tail -- all of
// the array where it is not. vec(i, cursor) loads vector i, takes the VN levels from cursor.next() and
// stores; one(k, level) does the same for the single element k.
template <int THREADS, int VN, typename VecF, typename OneF>
__device__ __forceinline__ void stream_levels(const QuantMeta &m, const int *__restrict__ marks, size_t total,
                                              bool aligned, VecF vec, OneF one) {
  LevelCursor cur(m, marks);
  const size_t tid = (size_t)blockIdx.x * THREADS + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * THREADS;
  size_t done = 0;
  if (aligned) {
    const size_t nvec = total / VN;
    for (size_t i = tid; i < nvec; i += nth) {
      cur.seek((uint32_t)(i * VN));
      vec(i, cur);
    }
    done = nvec * VN;
  }
  for (size_t k = done + tid; k < total; k += nth) one(k, cur.at((uint32_t)k));
}

template <typename... P> __device__ __forceinline__ bool aligned16(const P *...p) {
  return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) == 0;
}

// Out-of-dictionary values of one round of a workgroup to the outlier list: thread by thread `mine` of
// them, marked in outl[], as (lin0 + u, qd[u]); qd[u] becomes 0, the symbol stored in their place.
// Slots are requested ONCE per workgroup and round (k_quantize's scheme: a request per wave queues on
// the counter), and none -- one barrier instead of four, no scan -- in a round
// without outliers. The counter goes on counting past `cap`; nothing is written past it.
// Every thread of the workgroup calls this in every round: it holds barriers.
template <int THREADS, int VN>
__device__ __forceinline__ void append_outliers(unsigned mine, const bool (&outl)[VN], int64_t (&qd)[VN], size_t lin0,
                                                unsigned long long *count, uint64_t *__restrict__ idx,
                                                int64_t *__restrict__ val, unsigned long long cap) {
  __shared__ unsigned wcnt[THREADS / 64];
  __shared__ unsigned long long gbase;
  if (!__syncthreads_or((int)mine)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned incl = mine;  // inclusive scan of the counts inside the wave
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  if (lane == 63) wcnt[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned tot = 0;
    for (int w = 0; w < THREADS / 64; w++) {
      const unsigned c = wcnt[w];
      wcnt[w] = tot;
      tot += c;
    }
    gbase = tot ? atomicAdd(count, (unsigned long long)tot) : 0ull;
  }
  __syncthreads();
  unsigned long long o = gbase + wcnt[wave] + (incl - mine);
#pragma unroll
  for (int u = 0; u < VN; u++)
    if (outl[u]) {
      if (o < cap) {
        idx[o] = lin0 + u;
        val[o] = qd[u];
      }
      qd[u] = 0;
      o++;
    }
  __syncthreads();  // (wcnt / gbase are rewritten by the next round)
}

// The end of a workgroup that counted symbols in `n` bins privatised in LDS: `centre`, the thread's
// count of the symbol centre_bin that it kept in a register, reaches its bin once per wave; then one
// global atomic per used bin, like huff::k_histogram. Every thread calls this: it holds a barrier.
template <int THREADS>
__device__ __forceinline__ void flush_bins(unsigned *bins, int n, unsigned centre, int centre_bin,
                                           unsigned *__restrict__ freq) {
  for (int off = 32; off > 0; off >>= 1) centre += __shfl_down(centre, off, 64);
  if ((threadIdx.x & 63) == 0 && centre) atomicAdd(&bins[centre_bin], centre);
  __syncthreads();  // (every count of the workgroup is in the bins)
  for (int i = threadIdx.x; i < n; i += THREADS)
    if (bins[i]) atomicAdd(&freq[i], bins[i]);
}

}  // namespace mgh
