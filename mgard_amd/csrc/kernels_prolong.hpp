// Prolongation of a level's nodal array to the next finer level (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_v1.hpp"
#include "prolong_plan.hpp"

namespace mgh {

// ---------------------------------------------------------------------------------------------
// One level step l-1 -> l of a 3-D hierarchy with every coefficient of level l zero: what the
// recomposition of the reference leaves of itself then (load vector, Thomas solves and correction
// are zero) -- the interpolation f, then c, then r of GpkRev3D (GridProcessingKernel3D.hpp:1231-2352).
//
// The march of the node restore (k_level_restore3_q, kernels_recompose2.hpp) without its
// coefficient loads: a thread owns one CELL column -- coarse node (Jc, Jf) and its three odd
// neighbours -- and marches along r over a chunk of coarse planes. The interpolants G(R) of coarse
// plane R serve the even plane 2R directly and, r-lerped with G(R + 1), the odd plane 2R + 1;
// G(R + 1) is then carried on. 4 coarse loads and 12 lerps per cell and plane pair; no LDS, no
// barrier; a wave writes whole rows (64 consecutive node pairs).
// Padded coordinates as everywhere (even size: real last node at P = n, ghost at P = n - 1, which
// has no output). Loads are unconditional, from clamped addresses; only the odd row / column /
// plane that does not exist is not stored.
// Per value the operations of the element code (gpk_rev_elem, kernels_v1.hpp) on a zero
// coefficient, in the same order: an interpolated node is (T)0 + interpolant -- the addition stays,
// it makes the sign of a zero what the full call gives --, a coarse node is copied.
// 32-bit offsets inside an r-plane (coarse and fine planes of fewer than 2^29 elements), size_t
// across planes.
// ---------------------------------------------------------------------------------------------
template <typename T> struct ProlongArgs {
  const T *coarse;     // dense m[0] x m[1] x m[2]
  T *fine;             // n[0] x n[1] x n[2] with the element strides (fI, fJ, 1)
  size_t fI, fJ;
  int n[3], m[3];
  const T *ratio[3];   // of level l, per dimension (r, c, f)
  int gxm;             // tiles along f
  int rch, nchunk;     // coarse planes per workgroup; the last chunk takes what is left
};

template <typename T, int TC, int TF>
__global__ void __launch_bounds__(TC * TF)
k_prolong3(ProlongArgs<T> A) {
  const int nr = A.n[0], nc = A.n[1], nf = A.n[2];
  const int mr = A.m[0], mc = A.m[1], mf = A.m[2];
  const int b = blockIdx.x;
  const int Jf = (b % A.gxm) * TF + (int)threadIdx.x % TF, Jc = (b / A.gxm) * TC + (int)threadIdx.x / TF;
  int R0, R1;
  prolong_chunk(A.rch, A.nchunk, mr, (int)blockIdx.y, &R0, &R1);
  if (Jc >= mc || Jf >= mf) return;
  const int Pmax_r = 2 * mr - 2, Pmax_c = 2 * mc - 2, Pmax_f = 2 * mf - 2;
  const int ghost_r = (nr % 2 == 0) ? nr - 1 : -7;
  const int ghost_c = (nc % 2 == 0) ? nc - 1 : -7;
  const int ghost_f = (nf % 2 == 0) ? nf - 1 : -7;
  // the odd neighbours of the column exist?
  const bool vco = 2 * Jc + 1 <= Pmax_c && 2 * Jc + 1 != ghost_c;
  const bool vfo = 2 * Jf + 1 <= Pmax_f && 2 * Jf + 1 != ghost_f;
  const T rc = vco ? A.ratio[1][2 * Jc] : (T)0, rf = vfo ? A.ratio[2][2 * Jf] : (T)0;
  const int c1 = min(Jc + 1, mc - 1), f1 = min(Jf + 1, mf - 1);
  const uint32_t o00 = (uint32_t)(Jc * mf + Jf), o01 = (uint32_t)(Jc * mf + f1), o10 = (uint32_t)(c1 * mf + Jf),
                 o11 = (uint32_t)(c1 * mf + f1);
  const size_t mI = (size_t)mc * mf;
  // real positions of the cell's nodes in the output plane
  const int cE = min(2 * Jc, nc - 1), fE = min(2 * Jf, nf - 1);
  const uint32_t outE = (uint32_t)cE * (uint32_t)A.fJ + (uint32_t)fE;            // row E
  const uint32_t outO = (uint32_t)(2 * Jc + 1) * (uint32_t)A.fJ + (uint32_t)fE;  // row O (vco)

  // the four corners of the column in coarse plane R (clamped: always a valid address)
  auto request = [&](int R, T(&v)[4]) {
    const T *cp = A.coarse + (size_t)min(R, mr - 1) * mI;
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
  // Streaming stores: the output is not read again by this launch, and it is eight times what is read
  auto store_pair = [](T *p, T a, T b2) {
    typedef T V2 __attribute__((ext_vector_type(2)));
    V2 v;
    v[0] = a;
    v[1] = b2;
    __builtin_nontemporal_store(v, reinterpret_cast<V2 *>(p));
  };
  // one fine plane (real index rp) out: the four node values of the cell
  auto store_plane = [&](int rp, const T(&val)[4]) {
    T *pl = A.fine + (size_t)rp * A.fI;
    T *rowE = pl + outE, *rowO = pl + outO;
    if (vfo && (reinterpret_cast<uintptr_t>(rowE) & (2 * sizeof(T) - 1)) == 0) {
      store_pair(rowE, val[0], val[1]);
    } else {
      rowE[0] = val[0];
      if (vfo) rowE[1] = val[1];
    }
    if (vco) {
      if (vfo && (reinterpret_cast<uintptr_t>(rowO) & (2 * sizeof(T) - 1)) == 0) {
        store_pair(rowO, val[2], val[3]);
      } else {
        rowO[0] = val[2];
        if (vfo) rowO[1] = val[3];
      }
    }
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
