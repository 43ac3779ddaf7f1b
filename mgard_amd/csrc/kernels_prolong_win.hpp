// Prolongation of a box of a level's nodal array to the next finer level (gfx950): the window form of
// k_prolong3 (kernels_prolong.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_v1.hpp"
#include "prolong_window_plan.hpp"

namespace mgh {

// ---------------------------------------------------------------------------------------------
// The march of k_prolong3 over the cells J0 .. J0 + nJ - 1 per dimension instead of all of them.
// Positions are GLOBAL: a thread's cell (Jc, Jf), the planes R of its march, the ratio entries and
// the ghost / last-node rules are those of the whole level step, so every value is made by the same
// operations from the same operands as in k_prolong3. What differs is where values are read and
// written:
//  - the source is the box c0 .. c0 + sm - 1 (per dimension) of the coarse level, element strides
//    (sI, sJ, 1), `src` at its first element: the caller's whole level array in place, or a compact
//    window array. Loads are unconditional from addresses clamped to that box; a clamped value only
//    ever feeds a node outside the destination range, which is not stored;
//  - the destination is the real range d0 .. d0 + dn - 1 (per dimension) of the fine level, element
//    strides (dI, dJ, 1), `dst` at its first element: a compact window array, or a sub-box of a
//    larger output. Only nodes inside the range are stored: a range may begin or end on an odd P,
//    end on the last node of an even extent (P = n) or begin there, right behind the ghost.
// Paired streaming stores where both nodes of a pair are inside and the address is aligned, scalar
// stores elsewhere. No LDS, no barrier. 32-bit offsets inside a source plane (fewer than 2^31
// elements between the first and the last element of the box's plane), size_t elsewhere.
// ---------------------------------------------------------------------------------------------
template <typename T> struct ProlongWinArgs {
  const T *src;
  size_t sI, sJ;
  int c0[3], sm[3];
  T *dst;
  size_t dI, dJ;
  int d0[3], dn[3];
  int n[3], m[3];      // extents of the fine and the coarse level (whole level step)
  int J0[3], nJ[3];    // cells of the launch
  const T *ratio[3];   // of the fine level, per dimension (r, c, f), whole tables
  int gxm;             // tiles along f
  int rch, nchunk;     // cell planes per workgroup; the last chunk takes what is left
};

template <typename T, int TC, int TF>
__global__ void __launch_bounds__(TC * TF)
k_prolong3_win(ProlongWinArgs<T> A) {
  const int nr = A.n[0], nc = A.n[1], nf = A.n[2];
  const int mr = A.m[0], mc = A.m[1], mf = A.m[2];
  const int b = blockIdx.x;
  const int jf = (b % A.gxm) * TF + (int)threadIdx.x % TF, jc = (b / A.gxm) * TC + (int)threadIdx.x / TF;
  int R0, R1;
  prolong_chunk(A.rch, A.nchunk, A.nJ[0], (int)blockIdx.y, &R0, &R1);
  if (jc >= A.nJ[1] || jf >= A.nJ[2]) return;
  R0 += A.J0[0];
  R1 += A.J0[0];
  const int Jc = A.J0[1] + jc, Jf = A.J0[2] + jf;
  const int Pmax_r = 2 * mr - 2, Pmax_c = 2 * mc - 2, Pmax_f = 2 * mf - 2;
  const int ghost_r = (nr % 2 == 0) ? nr - 1 : -7;
  const int ghost_c = (nc % 2 == 0) ? nc - 1 : -7;
  const int ghost_f = (nf % 2 == 0) ? nf - 1 : -7;
  // the odd neighbours of the column exist?
  const bool vco = 2 * Jc + 1 <= Pmax_c && 2 * Jc + 1 != ghost_c;
  const bool vfo = 2 * Jf + 1 <= Pmax_f && 2 * Jf + 1 != ghost_f;
  const T rc = vco ? A.ratio[1][2 * Jc] : (T)0, rf = vfo ? A.ratio[2][2 * Jf] : (T)0;
  // ... and which of the column's nodes lie in the destination range (real positions; an odd node
  // that exists is its own real position)
  const int cE = min(2 * Jc, nc - 1) - A.d0[1], fE = min(2 * Jf, nf - 1) - A.d0[2];
  const int cO = 2 * Jc + 1 - A.d0[1], fO = 2 * Jf + 1 - A.d0[2];
  const bool sEc = cE >= 0 && cE < A.dn[1], sOc = vco && cO >= 0 && cO < A.dn[1];
  const bool sEf = fE >= 0 && fE < A.dn[2], sOf = vfo && fO >= 0 && fO < A.dn[2];
  // source columns, clamped to the box (local positions)
  const int lc0 = Jc - A.c0[1], lf0 = Jf - A.c0[2];
  const int lc1 = min(lc0 + 1, A.sm[1] - 1), lf1 = min(lf0 + 1, A.sm[2] - 1);
  const uint32_t sJ = (uint32_t)A.sJ;
  const uint32_t o00 = (uint32_t)lc0 * sJ + (uint32_t)lf0, o01 = (uint32_t)lc0 * sJ + (uint32_t)lf1,
                 o10 = (uint32_t)lc1 * sJ + (uint32_t)lf0, o11 = (uint32_t)lc1 * sJ + (uint32_t)lf1;
  const size_t outE = (size_t)max(cE, 0) * A.dJ, outO = (size_t)max(cO, 0) * A.dJ;

  // the four corners of the column in coarse plane R (clamped: always an address inside the box)
  auto request = [&](int R, T(&v)[4]) {
    const T *cp = A.src + (size_t)(min(R, A.c0[0] + A.sm[0] - 1) - A.c0[0]) * A.sI;
    v[0] = cp[o00];
    v[1] = cp[o01];
    v[2] = cp[o10];
    v[3] = cp[o11];
  };
  // the four interpolants (node, f, c, fc) of a coarse plane at this column: f innermost, then c
  auto interp_from = [&](const T(&v)[4], T(&Gv)[4]) {
    const T g0 = lerp_ref(v[0], v[1], rf), g1 = lerp_ref(v[2], v[3], rf);
    Gv[0] = v[0];
    Gv[1] = g0;
    Gv[2] = lerp_ref(v[0], v[2], rc);
    Gv[3] = lerp_ref(g0, g1, rc);
  };
  // Streaming stores: the output is not read again by this launch
  auto store_pair = [](T *p, T a, T b2) {
    typedef T V2 __attribute__((ext_vector_type(2)));
    V2 v;
    v[0] = a;
    v[1] = b2;
    __builtin_nontemporal_store(v, reinterpret_cast<V2 *>(p));
  };
  auto store_row = [&](T *row, T e, T o) {
    if (sEf && sOf && (reinterpret_cast<uintptr_t>(row + fE) & (2 * sizeof(T) - 1)) == 0) {
      store_pair(row + fE, e, o);
    } else {
      if (sEf) row[fE] = e;
      if (sOf) row[fO] = o;
    }
  };
  // one fine plane (real index rp, inside the range?) out: the four node values of the cell
  auto store_plane = [&](int rp, const T(&val)[4]) {
    const int lr = rp - A.d0[0];
    if (lr < 0 || lr >= A.dn[0]) return;
    T *pl = A.dst + (size_t)lr * A.dI;
    if (sEc) store_row(pl + outE, val[0], val[1]);
    if (sOc) store_row(pl + outO, val[2], val[3]);
  };

  T cur[4], nxt[4], Gp[4];
  request(R0, cur);
  interp_from(cur, Gp);
  request(R0 + 1, cur);
  for (int R = R0; R < R1; R++) {
    if (R + 1 < R1) request(R + 2, nxt);  // (loads of the next pair before this one is finished)
    // ---- even plane P = 2R (real index min(2R, nr - 1)): the coarse node itself, three interpolants
    {
      T val[4];
      val[0] = Gp[0];
      val[1] = (T)0 + Gp[1];
      val[2] = (T)0 + Gp[2];
      val[3] = (T)0 + Gp[3];
      store_plane(min(2 * R, nr - 1), val);
    }
    // ---- odd plane P = 2R + 1: r-lerp of the interpolants of the coarse planes R and R + 1
    T Gn[4];
    interp_from(cur, Gn);
    const int P = 2 * R + 1;
    if (P <= Pmax_r && P != ghost_r) {
      const T rr = A.ratio[0][2 * R];
      T val[4];
#pragma unroll
      for (int k = 0; k < 4; k++) val[k] = (T)0 + lerp_ref(Gp[k], Gn[k], rr);
      store_plane(P, val);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      Gp[k] = Gn[k];
      if (R + 1 < R1) cur[k] = nxt[k];
    }
  }
}

} // namespace mgh
