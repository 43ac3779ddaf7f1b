// Which kernel solves a tridiagonal (Thomas) system along one axis of a compact box, and with which
// launch parameters: the ONE place where that choice is made. Host-only and free of HIP, so that
// the choice can be compiled by a plain C++ compiler and pinned by the CPU suite
// (tests/test_ipk_plan_cpu.py; per family on small arrays: tests/ipk_family_cases.py and
// tests/ipk_stream_cases.py, which the GPU suite holds against the plan log); capi.hip's ipk_launch
// makes the plan and dispatches on it.
// IpkKernel lists the families in the order in which ipk_plan() considers them.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace mgh {

// The MGH_IPK_* developer switches the plan depends on (capi.hip: ipk_tuning_from_env), the compute units of
// the device, and the warm-up length the Thomas tables of the hierarchy need.
struct IpkTuning {
  size_t num_cu = 256;  // compute units of the device (hipDeviceAttributeMultiprocessorCount)
  // MGH_IPK_STREAM: 1 = streaming Thomas solves (kernels_ipk_stream.hpp) on the levels whose
  // LDS-staged solve needs more than one round of resident workgroups (default), 0 = never
  int stream = 1;
  // MGH_IPK_DMA: 1 = strided float pencils whose tiles are all resident at once run k_ipk_dma
  // (kernels_ipk_dma.hpp: LDS-DMA front end, everything requested up front; default), 0 = never
  int dma = 1;
  size_t dma_min = 512;  // MGH_IPK_DMA_MIN: fewest tiles of a level for k_ipk_dma (two per CU; set in ipk_tuning_from_env)
  int dma_rounds = 4;  // MGH_IPK_DMA_ROUNDS: k_ipk_dma also for levels whose tiles need up to this many rounds of resident workgroups
  int spec = 1;     // MGH_IPK_SPEC: few long contiguous pencils (1-D arrays) are solved in chunks, each verified against the sequential sweep (kernels_ipk_spec.hpp); 0 = one lane per pencil
  int spec_k = 0;   // MGH_IPK_SPEC_K: warm-up length of a chunk (0 = 64 floats / 128 doubles; tiny values make the verification fail and exercise the repair)
  int spec_long = 1024;  // MGH_IPK_SPEC_LONG: strided pencils of this length and more, one round of tiles at most, run in verified chunks too (0: never)
  uint32_t spec_max = 16384;  // MGH_IPK_SPEC_MAX: most pencils of a solve whose pencils do not fit LDS that still run in verified chunks
  int chunk = 1;    // MGH_IPK_CHUNK: the LDS-staged solve of contiguous pencils shares a tile's sweeps between the four waves (thomas_chunked: chunks verified against the sequential sweep)
  int chunk_k = 0;  // MGH_IPK_CHUNK_K: warm-up length of a chunk (0 = from the tables, chunk_warmup_need; small values make the verification fail and exercise the fall-back)
  int chunk_need = 0;  // warm-up length that the Thomas tables of this hierarchy need (set with the tables; stays 0 for D > 3)
  uint32_t w = 64;             // MGH_IPK_W: widest solver wave of the streaming Thomas solves
  size_t wpc = 8;              // MGH_IPK_WPC: most one-wave solver workgroups per CU the host plans with
  int kr16 = 1;                // MGH_IPK_KR16: 16 register-resident batches for float pencils of 512+ elements
  size_t contig_rounds = 4;    // MGH_IPK_CONTIG: rounds of the LDS-staged contiguous solve from which the streaming one takes over
};

// The pencils of a solve along `axis` of the compact (m[0], m[1], m[2]) box: pencil p = o * n_inner + i
// starts at o * outer_stride + i * inner_stride, its elements are `stride` apart.
// axis 0 only: `nbatch` boxes `batch_stride` elements apart (the slices of a 4-D level).
struct IpkGeom {
  uint32_t n = 0;        // elements of a pencil
  uint32_t npencil = 0;
  uint32_t n_inner = 0;
  size_t outer_stride = 0, inner_stride = 0, stride = 0;
};

inline IpkGeom ipk_geom(int axis, const uint32_t m[3], uint32_t nbatch, size_t batch_stride) {
  IpkGeom g;
  g.n = m[axis];
  if (axis == 2) {
    g.npencil = m[0] * m[1];
    g.n_inner = g.npencil; g.outer_stride = 0; g.inner_stride = g.n; g.stride = 1;
  } else if (axis == 1) {
    g.npencil = m[0] * m[2];
    g.n_inner = m[2]; g.outer_stride = (size_t)m[1] * m[2]; g.inner_stride = 1; g.stride = m[2];
  } else {
    g.npencil = nbatch * m[1] * m[2];
    g.n_inner = m[1] * m[2]; g.outer_stride = batch_stride; g.inner_stride = 1; g.stride = (size_t)m[1] * m[2];
  }
  return g;
}

enum class IpkKernel {
  Spec,              // k_ipk_spec_*: few long pencils in chunks verified against the sequential sweep (kernels_ipk_spec.hpp)
  LdsContigChunked,  // k_ipk_lds_contig<T, true>: contiguous pencils staged in LDS, a tile's sweeps shared by the four waves
  Dma,               // k_ipk_dma: strided float pencils, LDS-DMA front end (kernels_ipk_dma.hpp)
  Stream,            // k_ipk_stream, KR = 16 or 8 (kernels_ipk_stream.hpp)
  LdsContig,         // k_ipk_lds_contig<T>: contiguous pencils staged in LDS, one lane per pencil
  LdsStrided,        // k_ipk_lds_strided<T, W>: strided pencils staged in LDS
  Thread             // k_ipk: one thread per pencil straight from global memory
};

// A family and everything its launch needs that is not a pointer. Members that a family does not
// use stay 0.
struct IpkPlan {
  IpkKernel kernel = IpkKernel::Thread;
  IpkGeom geom;
  uint32_t KR = 0;      // Dma, Stream: register-resident batches
  uint32_t W = 0;       // Stream: tile width; LdsStrided: the template's tile width (best_w)
  uint32_t P = 0;       // LdsContig, LdsContigChunked: pencils of a tile (best_w)
  uint32_t n_glob = 0;  // Stream: leading elements of a pencil parked in place in global memory
  uint32_t K = 0;       // LdsContigChunked, Spec: warm-up length of a chunk
  uint32_t S = 0, nchunk = 0;   // Spec: chunk size, chunks of a pencil
  uint32_t pad = 0, magic = 0;  // LdsContig, LdsContigChunked: row padding in LDS, 2^32 / n rounded up (e / n for e < 2^17)
  size_t lds = 0;       // dynamic LDS of the launch, bytes
  size_t lds_attr = 0;  // hipFuncAttributeMaxDynamicSharedMemorySize the kernel is given (0: none)
  uint32_t grid = 0, grid_y = 1, block = 64;  // (Spec: grid and block of the forward and backward sweeps)
  uint32_t check_grid = 0, fix_grid = 0, apply_grid = 0;  // Spec: its other kernels (256, 64, 256 threads)
  bool per_batch = false;  // Thread, nbatch > 1: the boxes run one call each
};

// LDS budget for the IPK tiles: whole pencils of 64 (or 32) lanes must fit.
constexpr size_t kLdsPerCU = 160 * 1024;
// (five 32 KB allocations do not fit one CU although 5 * 32 KB = 160 KB: leave a margin)
constexpr size_t kLdsMarginWave = 4096;
// the chunked LDS-staged solve has static LDS of its own beside the tile
constexpr size_t kLdsMarginChunked = 8192;
// the streaming and DMA kernels address a box with 32-bit byte offsets
constexpr size_t kIpkBoxBytesLimit = (size_t)1 << 32;

// Staging area of the contiguous streaming kernel, in elements (TileIO<T, U>::stage_elems,
// kernels_ipk_stream.hpp, which asserts the equality).
constexpr size_t ipk_stream_stage_elems(uint32_t U) { return 64 * ((size_t)U + 1); }

// f-solve and c-solve of a level in one launch (k_ipk_plane_fc): a coarse plane fits in LDS.
inline bool ipk_plane_fits_lds(size_t elem_size, const uint32_t m[3]) {
  return (size_t)m[1] * (m[2] | 1u) * elem_size <= 150 * 1024 && m[1] <= 1024 && m[2] <= 1024;
}

inline IpkPlan ipk_plan(const IpkTuning &t, size_t elem_size, int axis, const uint32_t m[3],
                        uint32_t nbatch, size_t batch_stride) {
  IpkPlan p;
  p.geom = ipk_geom(axis, m, nbatch, batch_stride);
  const uint32_t n = p.geom.n, npencil = p.geom.npencil;
  // tile width (pencils per workgroup): whole pencils must fit in LDS; among the fitting
  // widths take the one that needs the fewest "rounds" of resident workgroups
  const size_t pencil_bytes = (size_t)(n + (axis == 2 && n % 2 == 0 ? 1 : 0)) * elem_size;
  // Few long pencils (a 1-D array: ONE pencil per level): parallel inside the pencil, every chunk
  // verified against the sequential sweep (kernels_ipk_spec.hpp)
  auto spec_solve = [&] {
    p.kernel = IpkKernel::Spec;
    p.K = t.spec_k > 0 ? (uint32_t)t.spec_k : (elem_size == 4 ? 64u : 128u);
    const uint32_t S = std::max<uint32_t>(128, std::min<uint32_t>(1024, n / 16384));
    p.S = (S + 7) / 8 * 8;
    p.nchunk = (n + p.S - 1) / p.S;
    const size_t total = (size_t)npencil * n, edges = (size_t)npencil * p.nchunk;
    p.grid = (uint32_t)((edges + 63) / 64);
    p.fix_grid = (npencil + 63) / 64;
    p.check_grid = (uint32_t)((edges + 255) / 256);
    p.apply_grid = (uint32_t)std::min<size_t>((total + 255) / 256, 4096);
    return p;
  };
  // (the batches of a 4-D level: only back to back -- the chunk buffers and the add-to pass see one array)
  const bool spec_ok = t.spec && (nbatch == 1 || batch_stride == (size_t)m[0] * m[1] * m[2]);
  if (axis == 2 && nbatch == 1 && t.spec && npencil <= 64 && n >= 2048) return spec_solve();
  int best_w = 0;
  size_t best_rounds = ~(size_t)0;
  for (int w : {64, 48, 32, 16}) {
    const size_t lds = w * pencil_bytes;
    if (lds > kLdsPerCU) continue;
    const size_t per_cu = std::min<size_t>(kLdsPerCU / lds, 8);
    const size_t blocks = (npencil + w - 1) / w;
    const size_t rounds = (blocks + per_cu * t.num_cu - 1) / (per_cu * t.num_cu);
    if (rounds < best_rounds) {
      best_rounds = rounds;
      best_w = w;
    }
  }
  // Long strided pencils, few enough of them to be one round of tiles with most of the chip idle
  // (16395 x 64 x 64: the r-solve of the 2051 x 9 x 9 level is 6 tiles and a chain of 2051 steps down
  // and 2051 back at ~40 ns each in LDS -- 161 us for 0.7 MB; the levels above it 91 and 53 us): the
  // verified chunks put a wave on every piece of every pencil. MGH_IPK_SPEC_LONG: the pencil length
  // from which on (default 1024; 0: never).
  if (axis != 2 && spec_ok && t.spec_long && n >= (uint32_t)t.spec_long &&
      npencil <= 64u * (uint32_t)t.num_cu && npencil <= t.spec_max)
    return spec_solve();
  // Contiguous pencils, LDS-staged tiles whose sweeps are shared by the four waves (thomas_chunked;
  // warm-up length from the tables, chunk_need), ahead of the streaming kernels: 512^3 f32 top
  // level 53 -> 44 us, f64 120 -> 109 us, 1024^3 554 -> 543 us. (The same for strided pencils and
  // for the plane kernel of the small levels was measured and dropped: profiles/NOTES.md.)
  auto lds_contig = [&](IpkKernel kernel, uint32_t K, size_t lds_attr) {
    p.kernel = kernel;
    p.K = K;
    p.pad = (n % 2 == 0) ? 1u : 0u;
    p.magic = (uint32_t)((((uint64_t)1 << 32) + n - 1) / n);  // e/n for e < 2^17
    p.P = (uint32_t)best_w;
    p.grid = (npencil + p.P - 1) / p.P;
    p.block = 256;
    p.lds = p.P * pencil_bytes;
    p.lds_attr = lds_attr;
    return p;
  };
  if (t.chunk && axis == 2 && best_w && n >= 64 && best_w * pencil_bytes + kLdsMarginChunked <= kLdsPerCU) {
    const uint32_t K = t.chunk_k > 0 ? (uint32_t)t.chunk_k : (uint32_t)t.chunk_need;
    if (K > 0 && K <= n / 2) return lds_contig(IpkKernel::LdsContigChunked, K, kLdsPerCU - kLdsMarginChunked);
  }
  // Streaming solves: every wave a solver, forward results parked in registers + LDS +
  // (the leading n_glob elements) in place in global memory. Where the forward results are parked
  // decides how many pencils a CU works on at once, and residency is the throughput of these
  // latency-bound chains: the host picks the tile width W and n_glob that need the FEWEST rounds
  // of resident workgroups (up to wpc one-wave workgroups per CU), then the least global
  // parking. Used when the LDS-staged tiles need more than one round (strided pencils), or --
  // contiguous pencils, where the LDS-staged kernel is the better one at one or two rounds --
  // from four rounds on (1024^3: 2 KB pencils leave ONE staged tile per CU, 16 rounds).
  // batches of 64 bytes per lane: 16 floats / 8 doubles; the last KR batches stay in registers.
  // KR = 8 (a third of the register file: two or more waves per SIMD), or -- float pencils of
  // 512+ elements, MGH_IPK_KR16 -- KR = 16: 256 values of every pencil in registers, one wave per
  // SIMD, so that most of the rest fits in LDS and little is parked in global memory (1024^3:
  // PMC traffic of a solve 2.0-2.5 GB for 1.08 GB algorithmic with KR = 8).
  const uint32_t U = (uint32_t)(64 / elem_size);
  const size_t box_bytes = (nbatch > 1 ? nbatch * batch_stride : (size_t)m[0] * m[1] * m[2]) * elem_size;
  // Strided float pencils, every tile of the level resident at once: the LDS-DMA variant
  // (kernels_ipk_dma.hpp). KR register-resident batches: as many as keep two waves per SIMD.
  if (elem_size == 4 && t.dma && axis != 2 && box_bytes < kIpkBoxBytesLimit) {
    const uint32_t KR = 10;
    const size_t lds = n < KR * U ? 0 : (size_t)(n - KR * U) * 64 * elem_size;
    if (n >= KR * U && lds <= kLdsPerCU - kLdsMarginWave) {
      const size_t per_cu = lds ? std::min<size_t>((kLdsPerCU - kLdsMarginWave) / lds, 8) : 8;
      const size_t tiles = ((size_t)npencil + 63) / 64;
      // (a level with fewer than two tiles per CU is served better by the LDS-staged kernels, whose
      // four waves per tile stream it in and out: 129^3, 261 tiles, 18.8 vs 16.1 us)
      // (MGH_IPK_DMA_MIN: that threshold in tiles, 0 in the tests that run this kernel on small shapes: the
      // solves that get here, not the f- and c-solve of a fused level whose planes fit LDS -- tests/ipk_family_cases.py)
      // (round 6: short pencils -- four or more tiles per CU -- also when the level needs up to
      // MGH_IPK_DMA_ROUNDS rounds of resident workgroups: the 8 x 512^3 slab's 5168 tiles of
      // 257-element pencils, ipk_c 242 -> 213 us, ipk_r 204 -> 190 us against k_ipk_stream; long
      // pencils with ONE tile per CU lose badly that way -- 1024^3's 513-element pencils 430 -> 850 us)
      const size_t rounds = per_cu >= 4 ? (size_t)t.dma_rounds : 1;
      if (tiles <= per_cu * t.num_cu * rounds && tiles >= t.dma_min) {
        p.kernel = IpkKernel::Dma;
        p.KR = KR;
        p.grid = (uint32_t)((tiles + 7) / 8 * 8);
        p.lds = lds;
        p.lds_attr = kLdsPerCU;
        return p;
      }
    }
  }
  auto stream_plan = [&](uint32_t KR, size_t wpc_cap) {
    const size_t wpc = std::min(t.wpc, wpc_cap);
    const uint32_t nb = n / U;
    // (strided pencils: measured inside the step at 512^3, ipk_c 59 -> 52 us, ipk_r of
    // all levels 128 -> 103 us, but the contiguous solve 60 -> 65 us)
    const size_t min_rounds = axis == 2 ? t.contig_rounds : 2;
    if (!(t.stream && best_w && best_rounds >= min_rounds && nb >= KR && box_bytes < kIpkBoxBytesLimit))
      return false;
    const uint32_t parked = (nb - KR) * U;  // elements per pencil outside the registers
    // (contiguous pencils: + the staging area of the wave-cooperative loads and stores)
    const size_t stage_bytes = axis == 2 ? ipk_stream_stage_elems(U) * elem_size : 0;
    uint32_t W = 0, n_glob = 0;
    size_t w_rounds = ~(size_t)0;
    for (uint32_t ng = 0; ng <= parked; ng += U) {
      for (uint32_t w : {64u, 60u, 56u, 48u, 40u, 32u, 24u, 16u}) {
        if (w > t.w) continue;
        const size_t lds = (size_t)w * (parked - ng) * elem_size + stage_bytes;
        // ~230 VGPRs (KR = 8): two waves per SIMD = 8 one-wave workgroups per CU; KR = 16:
        // ~400 VGPRs, one wave per SIMD = 4 per CU (the caps the host plans with)
        const size_t per_cu = lds ? std::min<size_t>((kLdsPerCU - kLdsMarginWave) / lds, wpc) : wpc;
        if (!per_cu) continue;
        const size_t blocks = ((size_t)npencil + w - 1) / w;
        const size_t rounds = (blocks + per_cu * t.num_cu - 1) / (per_cu * t.num_cu);
        if (rounds < w_rounds) {
          w_rounds = rounds;
          W = w;
          n_glob = ng;
        }
      }
      if (w_rounds == 1) break;
    }
    if (!(W && w_rounds < best_rounds)) return false;
    p.kernel = IpkKernel::Stream;
    p.KR = KR;
    p.W = W;
    p.n_glob = n_glob;
    p.lds = (size_t)W * (parked - n_glob) * elem_size + stage_bytes;
    p.lds_attr = kLdsPerCU;
    p.grid = ((npencil + W - 1) / W + 7) / 8 * 8;
    return true;
  };
  if (elem_size == 4 && t.kr16 && n / U >= 32 && stream_plan(16, 4)) return p;
  if (stream_plan(8, 16)) return p;
  if (axis == 2 && best_w) return lds_contig(IpkKernel::LdsContig, 0, kLdsPerCU);
  if (axis != 2 && best_w) {
    p.kernel = IpkKernel::LdsStrided;
    p.W = (uint32_t)best_w;
    p.lds = best_w * pencil_bytes;
    p.lds_attr = kLdsPerCU;
    p.grid = ((npencil + best_w - 1) / best_w + 7) / 8 * 8;  // XCD-contiguous tile ranges
    p.block = 256;
    return p;
  }
  // pencils too long for LDS. Not too many of them (a 4194304 x 9 array: 9 strided pencils of
  // 2^21 elements per level; 100 x 100 x 6000: 2601 contiguous ones of 3001): in verified chunks
  if (spec_ok && n >= 2048 && npencil <= t.spec_max) return spec_solve();
  // ... else one thread per pencil straight from global memory
  p.kernel = IpkKernel::Thread;
  p.per_batch = nbatch > 1;
  p.grid = (m[axis == 2 ? 1 : 2] + 63) / 64;
  p.grid_y = m[axis == 0 ? 1 : 0];
  return p;
}

} // namespace mgh
