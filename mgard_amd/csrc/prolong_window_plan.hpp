// Window form of the prolongation (kernels_prolong_win.hpp): which nodes of every level a window of
// the full grid depends on, and the launch plan of one window step. No HIP needed, like
// prolong_plan.hpp, whose tile rule and chunk rule (prolong_chunk) are reused.
//
// Padded coordinates as everywhere: real index i of an extent n sits at P = i, except the last node
// of an even n, which sits at P = n (the ghost at P = n - 1 has no output). An even P is coarse node
// P / 2, an odd P the interpolant of the coarse nodes (P - 1) / 2 and (P + 1) / 2. So the real
// range [a, b] of level l needs the coarse nodes [P(a) >> 1, (P(b) + 1) >> 1] of level l - 1, and
// nothing else: with zero coefficients there is no load vector, no solve and no correction.
#pragma once
#include <cstdint>
#include <vector>

#include "prolong_plan.hpp"

namespace mgh {

// padded coordinate of real index i of an extent n
inline int64_t win_padded(int64_t i, int64_t n) { return (n % 2 == 0 && i == n - 1) ? n : i; }

// One level step down: the closed real range [*a, *b] of an extent n (level l) to the closed range
// of the m coarse nodes (level l - 1) it depends on. A dimension the step does not coarsen
// (m == n) passes through.
inline void win_coarse_range(int64_t n, int64_t m, int64_t *a, int64_t *b) {
  if (m == n) return;
  *a = win_padded(*a, n) >> 1;
  *b = (win_padded(*b, n) + 1) >> 1;
}

// The chain of a window: level_shape[l][d] (l = 0 .. L, the hierarchy's own) and the window
// [lo_d, lo_d + ext_d) of the full grid (level L) give, for l = level .. L and every dimension, the
// closed range of real node indices of level l the window depends on:
//   out[(l - level) * 2 * D + 2 * d] = first, out[... + 1] = last.
// Returns false on a bad argument (level outside 0 .. L, ext_d == 0, lo_d + ext_d > shape_d).
inline bool prolong_window_chain(const std::vector<std::vector<uint64_t>> &level_shape, int level, const uint64_t *lo,
                                 const uint64_t *ext, std::vector<int64_t> &out) {
  const int L = (int)level_shape.size() - 1;
  if (L < 0 || level < 0 || level > L) return false;
  const int D = (int)level_shape[L].size();
  for (int d = 0; d < D; d++)
    if (ext[d] == 0 || lo[d] > level_shape[L][d] || ext[d] > level_shape[L][d] - lo[d]) return false;
  out.assign((size_t)(L - level + 1) * 2 * D, 0);
  for (int d = 0; d < D; d++) {
    int64_t a = (int64_t)lo[d], b = (int64_t)(lo[d] + ext[d] - 1);
    for (int l = L; l >= level; l--) {
      out[(size_t)(l - level) * 2 * D + 2 * d] = a;
      out[(size_t)(l - level) * 2 * D + 2 * d + 1] = b;
      if (l > level) win_coarse_range((int64_t)level_shape[l][d], (int64_t)level_shape[l - 1][d], &a, &b);
    }
  }
  return true;
}

// Launch plan of one window step l - 1 -> l of a 3-D hierarchy. A cell J of a dimension holds the
// nodes P = 2J and P = 2J + 1; the real range [a, b] of level l lies in the cells
// J0 = P(a) >> 1 .. J1 = P(b) >> 1. The tiles and the march are those prolong_plan gives for a level
// step with as many coarse nodes as the window has cells.
struct ProlongWinPlan {
  int J0[3], nJ[3];  // first cell and number of cells per dimension (r, c, f)
  ProlongPlan p;     // tiles over nJ[1] x nJ[2], march over nJ[0]
};

// n: extents of level l (r, c, f); a, b: the closed real range of level l per dimension.
inline ProlongWinPlan prolong_window_plan(const uint32_t n[3], const int64_t a[3], const int64_t b[3], bool tall_ok) {
  ProlongWinPlan w{};
  uint32_t cells[3];
  for (int k = 0; k < 3; k++) {
    const int64_t J0 = win_padded(a[k], n[k]) >> 1, J1 = win_padded(b[k], n[k]) >> 1;
    w.J0[k] = (int)J0;
    w.nJ[k] = (int)(J1 - J0 + 1);
    cells[k] = (uint32_t)w.nJ[k];
  }
  w.p = prolong_plan(cells, tall_ok);
  return w;
}

} // namespace mgh
