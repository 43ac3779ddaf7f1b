// How one level box runs on the fused level kernels (kernels_fused2.hpp, kernels_box.hpp): tile
// shape, face tiles, size class, march length, r-chunks and grid -- the ONE place where that is
// decided. Host-only and free of HIP, so that a plain C++ compiler can build it and the CPU suite
// can pin it (tests/test_fused_plan_cpu.py); capi.hip's launch_fused2_t / launch_fused4_t make the
// plan and launch what it says. The residency of the kernel instances comes in as numbers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace mgh {

constexpr int kFusedMaxMarch = 16;          // coarse planes per r-chunk k_level_fused2 is compiled for (RCH)
constexpr long long kFusedPolicyMaxRounds = 2;  // most rounds of a launch a planned march may need (fused_plan_march)
constexpr unsigned kXcdRangeMinTiles = 64;  // (below: at most 8 tiles an XCD, one more or less is 12 % and more)

// The MGH_* developer switches the plan depends on (read in capi.hip's mgh_hierarchy_create) and the
// start-up cost of the march model.
struct FusedTuning {
  int faces = 1;  // MGH_FUSED_FACES: 1 = face tiles for the remainder columns / rows of a level (default), 0 = off
  int tall = 1;   // MGH_FUSED_TALL: 64 x 4 tiles for levels with a short fastest extent (default 1)
  int xcd = 1;    // MGH_FUSED_XCD: tiles of a level in contiguous ranges per XCD (default 1)
  int wide = 1;   // MGH_FUSED_WIDE: 4 x 64 tiles for 0 = no level, 1 = long marches, 2 = all (unset: 1 for floats, 0 for doubles)
  // MGH_BOX: levels up to this march class (0 = few tiles, 1 = mid-size, 2 = long marches) run
  // the box kernel (kernels_box.hpp: no march, every phase once over a 4 x 4 x 8 box) instead of
  // the marching tile kernel; 0 = none, 1 = class 0 (default), 2 = classes 0-1, 3 = every level
  int box = 1;
  size_t cls1 = 256, cls2 = 2048;  // MGH_CLS1 / MGH_CLS2: tile-count thresholds of the march classes
  int rch[3] = {1, 4, 16};         // MGH_RCH=a,b,c: coarse planes per workgroup of the three classes
  // MGH_RCH, MGH_CLS1 or MGH_CLS2 set: every class marches rch[class], whatever the residency
  bool pinned = false;
  // MGH_FUSED_SLOTS: workgroups the device holds at once, instead of what the runtime reports for
  // the kernel instance (0 = not set)
  long slots_override = 0;
  // S of the march model, in plane pairs, per tile shape (8 x 32, 4 x 64, 64 x 4): what a workgroup
  // pays before its first plane pair (tables into LDS, first plane, priming the ring).
  // profiles/NOTES.md has the sweep it comes from: level 8 of 512^3 f32 (8 x 32 tiles), three rounds
  // of 4 against one round of 13, 77.5 against 69.0 us, gives 1.4; the other two shapes have no
  // sweep of their own and take the same value.
  double startup[3] = {1.5, 1.5, 1.5};
};

// Size class of a level for the fused kernels: 2 = plenty of tiles (long marches, RCH = 16),
// 1 = mid-size (RCH = 4), 0 = few tiles (one coarse plane per workgroup).
// nz: t-slices a launch of the D = 4 path covers (their workgroups count like tiles: 8 x 16395 x 39 x 39
// f64 has 3 tiles a slice and ran its 16395 planes in marches of 4 -- 5.6 ms, 4.6 with marches of 16).
inline int level_class(const FusedTuning &t, const uint32_t m[3], size_t nz = 1) {
  constexpr int TC = 8, TF = 32;
  const size_t gx = (m[2] + TF - 1) / TF, gy = (m[1] + TC - 1) / TC;
  if (gx * gy * nz * ((m[0] + 15) / 16) >= t.cls2) return 2;
  if (gx * gy * nz * ((m[0] + 3) / 4) >= t.cls1) return 1;
  return 0;
}

// Tile shape: long marches (class 2) run 4 x 64 coarse nodes per tile -- every row a wave reads or
// writes is 512 contiguous bytes instead of 256, which the memory system rewards more than the
// larger halo (1.41 x instead of 1.24 x re-read) costs: top level of 512^3 f32 435 -> 383 us, same
// box, alternating runs. The short marches of the lower levels are a few us faster on 8 x 32.
// (... where the rows are long enough to fill them: 33 coarse nodes along f are one 8 x 32 tile and a
// face tile, or half a 4 x 64 tile)
inline bool fused_wide_tiles(const FusedTuning &t, int cls, uint32_t mf) {
  if (t.wide >= 2) return true;
  if (t.wide != 1 || cls != 2) return false;
  auto filled = [&](uint32_t tf) {  // share of a main tile's columns that hold nodes
    const uint32_t nfull = (mf - 1) / tf, rem = mf - nfull * tf;
    if (t.faces && nfull >= 1 && rem <= 4) return 1.0;  // (the remainder goes to a face tile)
    return (double)mf / (double)((mf + tf - 1) / tf * tf);
  };
  return filled(64) + 0.1 >= filled(32);
}
// A short FASTEST extent (AoS-like data: 2048 x 2048 x 17, 512^3 x 5): nine coarse nodes along f fill a
// quarter of an 8 x 32 tile's lanes, three of them a tenth. Tiles of 64 x 4 coarse nodes there -- the face
// tiles' shape as the main one (the (c, f) plane of such a level is nearly contiguous in memory, the short
// rows cost little). MGH_FUSED_TALL=0: never.
inline bool fused_tall_tiles(const FusedTuning &t, const uint32_t m[3]) {
  return t.tall && m[2] <= 16 && m[1] >= 48;
}

// r-chunks of a level on the fused kernel: chunks of rch coarse planes, the last one takes what is
// left (one plane more for sizes 2^k + 1)
inline int fused_nchunk(int m_r, int rch) { return std::max(1, (m_r - 1 + rch - 1) / rch); }

// Coarse planes of chunk k of a level of m_r coarse planes -- the kernel's own arithmetic.
inline int fused_chunk_planes(int m_r, int rch, int nchunk, int k) {
  return k == nchunk - 1 ? m_r - k * rch : rch;
}

enum FusedShape { kShape8x32 = 0, kShape4x64 = 1, kShape64x4 = 2 };

// One level box on the fused kernels. fused_plan_tiles() fills everything above `rch`; the
// caller looks up the residency of the kernel instance that (shape, faces) select, and
// fused_plan_march() fills the rest.
struct FusedPlan {
  int cls = 0;        // level_class
  int shape = kShape8x32, TC = 8, TF = 32;
  // the tiles of a launch (Fused2Grid has the same fields)
  int gxm = 0, n_main = 0;  // main tiles TC x TF: gxm along f, n_main in all
  int ff_F0 = 0, n_ff = 0;  // f-face: tiles of 64 x 4 at F0 = ff_F0, C0 = k * 64 (n_ff = 0: none)
  int cf_C0 = 0, n_cf = 0;  // c-face: tiles of 4 x 64 at C0 = cf_C0, F0 = k * 64 (n_cf = 0: none)
  bool faces = false;       // the launch has face tiles (the FACES instance of the kernel)
  int ntile = 0;
  int xcd_ranges = 0;       // tiles handed to the XCDs in contiguous ranges (grid.x padded to 8)
  unsigned grid_x = 0;
  // the march
  int rch = 0, nchunk = 0;  // r-chunks of rch coarse planes; the last one takes what is left (<= rch + 1)
  bool by_policy = false;   // rch was chosen against the residency (else: rch[cls] of the tuning)
  long long workgroups[2] = {0, 0}, slots[2] = {0, 0}, rounds[2] = {0, 0};  // per launch of the level (D = 4: even, odd slices)
};

// Tiles of one launch. Sizes 2^k + 1 leave one coarse column / row / plane beyond the last full
// tile: a remainder of up to 4 coarse columns / rows beyond the full tiles goes to face tiles.
// nz_class: the `nz` of level_class (1, or the odd t-slices of a D = 4 level).
inline FusedPlan fused_plan_tiles(const FusedTuning &t, const uint32_t m[3], size_t nz_class = 1) {
  FusedPlan p;
  p.cls = level_class(t, m, nz_class);
  if (fused_tall_tiles(t, m)) {
    p.shape = kShape64x4; p.TC = 64; p.TF = 4;
  } else if (fused_wide_tiles(t, p.cls, m[2])) {
    p.shape = kShape4x64; p.TC = 4; p.TF = 64;
  }
  const int TC = p.TC, TF = p.TF;
  const int mfi = (int)m[2], mci = (int)m[1];
  const int nfull_f = (mfi - 1) / TF, rem_f = mfi - nfull_f * TF;
  const int nfull_c = (mci - 1) / TC, rem_c = mci - nfull_c * TC;
  const bool face_f = t.faces && nfull_f >= 1 && rem_f <= 4;
  const bool face_c = t.faces && nfull_c >= 1 && rem_c <= 4;
  p.gxm = face_f ? nfull_f : (mfi + TF - 1) / TF;
  const int gym = face_c ? nfull_c : (mci + TC - 1) / TC;
  p.n_main = p.gxm * gym;
  p.ff_F0 = nfull_f * TF;
  p.n_ff = face_f ? (mci + 63) / 64 : 0;
  p.cf_C0 = nfull_c * TC;
  p.n_cf = face_c ? ((face_f ? p.ff_F0 : mfi) + 63) / 64 : 0;
  p.faces = p.n_ff || p.n_cf;
  p.ntile = p.n_main + p.n_ff + p.n_cf;
  // (contiguous tile ranges per XCD only where there are tiles to hand out -- a cross-section of three
  // tiles padded to eight put every workgroup that had work on XCDs 0..2 -- 16395 x 39 x 39 f64: top
  // level 778 us; without the ranges the r-chunks rotate the tiles over the XCDs)
  p.xcd_ranges = (unsigned)p.ntile >= kXcdRangeMinTiles ? t.xcd : 0;
  p.grid_x = p.xcd_ranges ? ((unsigned)p.ntile + 7) / 8 * 8 : (unsigned)p.ntile;
  return p;
}

inline long long fused_rounds(long long workgroups, long long slots) {
  return slots > 0 ? (workgroups + slots - 1) / slots : 0;
}

// The march of the level: rch, nchunk, and per launch workgroups / slots / rounds.
// nlaunch launches share the march (1, or the even and the odd t-slices of a D = 4 level):
// launch i has nz[i] slices (0 = not launched) and the device holds slots[i] workgroups of its
// kernel instance at once (0 = unknown).
//
// The top (long-march) class and a pinned tuning march rch[class]. The other marching levels are
// bound by instruction issue along the dependent chain of a workgroup's march, not by bytes, and a
// pass takes rounds x (rch + S): rounds = ceil(workgroups / slots) rounds of resident workgroups,
// each a march of rch plane pairs behind a start-up of S. Among the lengths 1 .. 16 the cheapest
// one runs, the longer of two equal ones (less r-halo). (If that one needs more than two rounds of a
// launch, the level keeps rch[class]: below.) The workgroups are the launch's own:
// face tiles, the padding of grid.x under XCD ranges, the slices of a D = 4 launch.
inline void fused_plan_march(FusedPlan &p, const FusedTuning &t, int m_r, int nlaunch, const size_t nz[],
                             const long long slots_in[]) {
  long long slots[2] = {0, 0};
  bool known = true;
  for (int i = 0; i < nlaunch && i < 2; i++) {
    slots[i] = t.slots_override > 0 ? t.slots_override : slots_in[i];
    if (nz[i] > 0 && slots[i] <= 0) known = false;
  }
  auto wgs = [&](int nchunk, int i) { return (long long)p.grid_x * nchunk * (long long)nz[i]; };
  int rch = std::max(1, std::min(kFusedMaxMarch, t.rch[p.cls]));
  p.by_policy = !t.pinned && p.cls < 2 && known;
  if (p.by_policy) {
    double best = -1;
    for (int r = 1; r <= kFusedMaxMarch; r++) {
      const int nchunk = fused_nchunk(m_r, r);
      double cost = 0;
      for (int i = 0; i < nlaunch && i < 2; i++)
        if (nz[i] > 0) cost += (double)fused_rounds(wgs(nchunk, i), slots[i]) * ((double)r + t.startup[p.shape]);
      if (best < 0 || cost <= best) {
        best = cost;
        rch = r;
      }
    }
  }
  // The model was fitted where a pass takes one to three rounds (profiles/NOTES.md). A level whose best
  // plan still needs more than kFusedPolicyMaxRounds rounds of a launch is bound by the throughput of
  // all its workgroups, where the rounding of the round count decides nothing: it keeps rch[class].
  if (p.by_policy)
    for (int i = 0; i < nlaunch && i < 2; i++)
      if (nz[i] > 0 && fused_rounds(wgs(fused_nchunk(m_r, rch), i), slots[i]) > kFusedPolicyMaxRounds) p.by_policy = false;
  if (!p.by_policy) rch = std::max(1, std::min(kFusedMaxMarch, t.rch[p.cls]));
  p.rch = rch;
  p.nchunk = fused_nchunk(m_r, rch);
  for (int i = 0; i < 2; i++) {
    const bool on = i < nlaunch && nz[i] > 0;
    p.workgroups[i] = on ? wgs(p.nchunk, i) : 0;
    p.slots[i] = on ? slots[i] : 0;
    p.rounds[i] = on ? fused_rounds(p.workgroups[i], slots[i]) : 0;
  }
}

// Values of one record of the plan log (mgh_debug_fused_plans_read), in this order.
constexpr int kFusedPlanFields = 20;
inline void fused_plan_record(const FusedPlan &p, int elem, const uint32_t m[3], const size_t nz[2],
                              long long out[kFusedPlanFields]) {
  const long long v[kFusedPlanFields] = {
      p.cls, elem, m[0], m[1], m[2], p.TC, p.TF, p.faces, p.ntile, p.grid_x,
      p.rch, p.nchunk, p.by_policy, (long long)nz[0], (long long)nz[1], p.workgroups[0], p.workgroups[1],
      p.slots[0], std::max(p.rounds[0], p.rounds[1]), p.slots[1]};
  std::copy(v, v + kFusedPlanFields, out);
}

} // namespace mgh
