// Launch plan of the prolongation kernel (kernels_prolong.hpp): the tile of coarse nodes a workgroup
// owns and the march along r, from the coarse extents of the level step. No HIP needed: the planner
// is host code, and the one rule the kernel shares with it (prolong_chunk) compiles for both sides.
#pragma once
#include <algorithm>
#include <cstdint>

#ifdef __HIPCC__
#define MGH_PLAN_HD __host__ __device__
#else
#define MGH_PLAN_HD
#endif

namespace mgh {

struct ProlongPlan {
  int TC, TF;       // coarse nodes per workgroup along c and f: 4 x 64 (wide) or 64 x 4 (tall)
  int gxm, ntile;   // tiles along f; tiles of an r-plane
  int rch, nchunk;  // coarse planes per workgroup; the last chunk takes what is left
};

// Workgroups a launch should reach before the marches get longer: four per compute unit of a
// 256-CU device. (A workgroup is 256 threads with no LDS, so eight are resident per CU; half of
// that keeps a wave on every SIMD when the tiles at the edges are mostly empty.) Nothing measured.
constexpr int64_t kProlongWant = 1024;
constexpr int kProlongMaxChunk = 16;

// m: coarse extents (r, c, f) of the level step, all >= 1. tall_ok: 64 x 4 tiles are allowed where
// the fastest extent is short (the rule of the fused level passes: m_f <= 16 and m_c >= 48).
inline ProlongPlan prolong_plan(const uint32_t m[3], bool tall_ok) {
  ProlongPlan p{};
  const bool tall = tall_ok && m[2] <= 16 && m[1] >= 48;
  p.TC = tall ? 64 : 4;
  p.TF = tall ? 4 : 64;
  p.gxm = (int)((m[2] + (uint32_t)p.TF - 1) / (uint32_t)p.TF);
  p.ntile = p.gxm * (int)((m[1] + (uint32_t)p.TC - 1) / (uint32_t)p.TC);
  // long marches where there are plenty of tiles, short ones (more workgroups) on the small
  // levels: a chunk costs one extra coarse plane of interpolants only
  const int64_t per = (int64_t)m[0] * p.ntile / kProlongWant;
  p.rch = (int)std::max<int64_t>(1, std::min<int64_t>(kProlongMaxChunk, per));
  p.nchunk = ((int)m[0] + p.rch - 1) / p.rch;
  return p;
}

// first and one-past-last coarse plane of chunk k of a march over m_r planes (the kernel's own rule)
MGH_PLAN_HD inline void prolong_chunk(int rch, int nchunk, int m_r, int k, int *R0, int *R1) {
  *R0 = k * rch;
  *R1 = k == nchunk - 1 ? m_r : *R0 + rch;
}

} // namespace mgh
