// How an array is cut into subdomains, and the rules every decomposed path (mgh_compress, the multi-device
// and the one-rank-per-GPU calls, and all their readers) must agree on for a container written by one to be
// read by the others: the geometry, where the auto-split lands, the slab sizes, the norm of the whole domain,
// the bound of one subdomain, the header of one slab and the `[u64 size][record]` frames. Host-only and free
// of HIP, so that a plain C++ compiler builds it and the CPU suite pins it (tests/test_domain_plan_cpu.py):
// part of this reads a header nobody vouches for. It asks no environment and no device.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/mgard_hip_compress.h"
#include "format.hpp"
#include "hierarchy.hpp"

namespace mgh {

// A refusal: status code and message, msg == nullptr when all is well. The caller reports it. Functions that
// refuse with one code only return the message alone and name the code in their comment.
struct Refusal {
  int code = MGH_SUCCESS;
  const char *msg = nullptr;
};

struct Decomposer {
  int D = 0;
  std::vector<uint64_t> shape;
  bool decomposed = false;
  int method = MGH_DD_MAXDIM;
  uint64_t dim = 0, size = 0;        // MaxDim: (dim, size); Block: size; Variable: dim
  std::vector<uint64_t> var_sizes;   // Variable
  uint64_t num = 1;

  // Slabs of `size` planes of the slowest dimension (the last one may be shorter), the way the multi-device
  // and the one-rank-per-GPU paths share an array out: a MaxDim decomposition of dimension 0.
  static Decomposer slabs_of_dim0(const std::vector<uint64_t> &shape, uint64_t size) {
    Decomposer dd;  // (MaxDim, dim 0)
    dd.D = (int)shape.size();
    dd.shape = shape;
    dd.size = size;
    dd.num = (shape[0] - 1) / size + 1;
    dd.decomposed = dd.num > 1;
    return dd;
  }

  std::vector<uint64_t> dim_num_subdomain() const {  // DomainDecomposer.hpp:90-103
    std::vector<uint64_t> r(D, 1);
    if (!decomposed) return r;
    if (method == MGH_DD_MAXDIM || method == MGH_DD_VARIABLE) r[dim] = num;
    else for (int d = 0; d < D; d++) r[d] = (shape[d] - 1) / size + 1;
    return r;
  }
  std::vector<uint64_t> dim_subdomain_id(uint64_t id) const {  // :105-113
    const auto nd = dim_num_subdomain();
    std::vector<uint64_t> r(D);
    for (int d = D - 1; d >= 0; d--) {
      r[d] = id % nd[d];
      id /= nd[d];
    }
    return r;
  }
  std::vector<uint64_t> subdomain_shape(uint64_t id) const {  // :124-168
    if (!decomposed) return shape;
    std::vector<uint64_t> r = shape;
    if (method == MGH_DD_MAXDIM) {
      r[dim] = id < shape[dim] / size ? size : shape[dim] % size;
    } else if (method == MGH_DD_BLOCK) {
      const auto sid = dim_subdomain_id(id);
      for (int d = 0; d < D; d++) r[d] = sid[d] < shape[d] / size ? size : shape[d] % size;
    } else {
      r[dim] = var_sizes[id];
    }
    return r;
  }
  std::vector<uint64_t> subdomain_offset(uint64_t id) const {  // :115-122, 690-700
    std::vector<uint64_t> r(D, 0);
    if (!decomposed) return r;
    if (method == MGH_DD_MAXDIM) {
      r[dim] = id * size;
    } else if (method == MGH_DD_BLOCK) {
      const auto sid = dim_subdomain_id(id);
      for (int d = 0; d < D; d++) r[d] = sid[d] * size;
    } else {
      for (uint64_t k = 0; k < id; k++) r[dim] += var_sizes[k];
    }
    return r;
  }
  // A subdomain is one contiguous run of the full array when it spans every dimension but the
  // slowest completely; then it can be used in place (no copy) if the array is device memory.
  bool contiguous(uint64_t id) const {
    const auto ext = subdomain_shape(id);
    for (int d = 1; d < D; d++)
      if (ext[d] != shape[d]) return false;
    return true;
  }
  uint64_t linear_offset(uint64_t id) const {
    uint64_t inner = 1;
    for (int d = 1; d < D; d++) inner *= shape[d];
    return subdomain_offset(id)[0] * inner;
  }
  bool all_contiguous() const {
    for (uint64_t id = 0; id < num; id++)
      if (!contiguous(id)) return false;
    return true;
  }
  uint64_t max_subdomain_elems() const {
    uint64_t m = 0;
    for (uint64_t id = 0; id < num; id++) {
      uint64_t c = 1;
      for (uint64_t e : subdomain_shape(id)) c *= e;
      m = std::max(m, c);
    }
    return m;
  }
};

// A hierarchy needs 3 nodes per dimension: asked of the decomposition an (untrusted) header describes. MGH_ERR_FORMAT.
inline const char *check_extents(const Decomposer &dd) {
  for (uint64_t id = 0; id < dd.num; id++)
    for (uint64_t e : dd.subdomain_shape(id))
      if (e < 3) return "header: subdomain with fewer than 3 nodes";
  return nullptr;
}

// ---- where the auto-split lands --------------------------------------------------------------------
// Device bytes the REFERENCE plans for one subdomain of this shape -- its formula, so that the
// MaxDim / Block auto-splits land on the reference's subdomain sizes
// (DomainDecomposer::EstimateMemoryFootprint, DomainDecomposer.hpp:24-69, with
// Hierarchy.hpp:420-, Compressor.hpp:84-116, DataRefactor.hpp:50-70, LinearQuantization.hpp:547-552,
// Lossless.hpp:58-71, HuffmanWorkspace.hpp:58-92):
//   [input N T + output N 8 + ratio 8 + hierarchy tables]  (x 2 with prefetch)
//   + refactoring workspace prod(n_d + 2) T (twice for D > 3) + quantizers + Huffman workspace
//     (outlier lists 16 N ratio, codes 8 N, chunk tables 24 nchunk, code-book scratch ~ 80 dict)
//     + the int64 array 8 N when T is narrower than 8 bytes.
// Left out, because they depend on the reference's runtime and are a few KB: the allocation pitch
// of the fastest dimension (hipMallocPitch), the radix sort's temporary storage for `dict`
// keys, 2 (warps-per-block x CUs + 1) status words. This implementation itself needs less
// (no (n+2)^D workspace, 16-bit symbols), so following the reference only means splitting earlier.
inline size_t estimate_footprint(const std::vector<uint64_t> &shape, size_t elem, double estimate_outlier_ratio,
                                 uint64_t huff_dict_size, uint64_t huff_block_size, bool prefetch) {
  const int D = (int)shape.size();
  double n = 1, ws = 1;
  for (uint64_t e : shape) {
    n *= (double)e;
    ws *= (double)(e + 2);
  }
  const double ratio = estimate_outlier_ratio;
  // levels: every dim is halved until the smallest reaches 2 (Hierarchy.hpp:428-446)
  int L = 64;
  for (uint64_t e : shape) {
    int k = 0;
    for (uint64_t m = e; m > 2; m = m / 2 + 1) k++;
    L = std::min(L, k);
  }
  double hier = 0;  // per level and dim: shape words, ranges, coordinates, dist, ratio, am, bm, volumes
  for (int l = 0; l <= L; l++) {
    for (uint64_t e : shape) {
      uint64_t m = e;
      for (int k = 0; k < L - l; k++) m = m / 2 + 1;
      hier += 6.0 * (double)(m + 1) * elem;
    }
    hier += (double)D * 8 * 2;
  }
  double b = n * elem + n * 8 + ratio * 8 + hier;
  if (prefetch) b *= 2;
  const double dict = (double)huff_dict_size;
  const double nchunk = std::floor((n - 1) / (double)huff_block_size) + 1;
  double lossless = 8 + n * ratio * 16 + dict * 4 + dict * 8 + (8 * 128 + 8 * dict) + n * 8 + 3 * nchunk * 8 +
                    4 + dict * 4 + dict * 8 + 4 * dict * 4 + 6 * dict * 4 + 8 * dict + 64;
  double comp = ws * elem * (D > 3 ? 2 : 1) + elem + (L + 1) * (double)elem + lossless + elem;
  if (8 > elem) comp += 8 * n;
  return (size_t)(b + comp);
}

// Device bytes THIS implementation keeps for a compression with `nlanes` pipeline lanes and
// `nbufs` input buffers (upper bound): per lane the quantized array (8 N: int64 where the 16-bit
// symbols do not apply), its level-linearised copy, the outlier lists (16 per estimated outlier),
// the hierarchy's workspace (levels below the top, per-slice vectors; the generic N-D path keeps
// three whole arrays) and the lossless stage's code units (a subdomain that does not compress
// below its own size is stored raw); per input buffer one dense subdomain.
inline size_t own_resident_bytes(int D, uint64_t max_elems, size_t elem, bool reorder, uint64_t ocap, int nlanes, int nbufs) {
  const double n = (double)max_elems;
  const double hier = (D <= 3 ? 0.5 : D == 4 ? 1.5 : 4.0) * n * (double)elem;
  const double lane = 8 * n + (reorder ? 8 * n : 0) + 16.0 * (double)ocap + hier + (n * (double)elem + 4096) +
                      (double)(64 << 20);  // (tables, chunk states, synchronisation points, allocator granularity)
  return (size_t)(lane * nlanes + (double)nbufs * n * (double)elem);
}

// The decomposition of a compression that may plan with `avail` device bytes: none while the array fits (MaxDim
// only), else the largest dimension / the blocks halved until the reference's estimate fits, or the caller's sizes.
inline Refusal split_domain(Decomposer &dd, int D, const uint64_t *shape, size_t elem, size_t avail, int method,
                            uint64_t block_size, int var_dim, const uint64_t *var_sizes, uint64_t nvar,
                            double estimate_outlier_ratio, uint64_t huff_dict_size, uint64_t huff_block_size) {
  dd.D = D;
  dd.shape.assign(shape, shape + D);
  auto need = [&](const std::vector<uint64_t> &s, bool prefetch) {
    return estimate_footprint(s, elem, estimate_outlier_ratio, huff_dict_size, huff_block_size, prefetch) >= avail;
  };
  dd.method = method;
  if (!need(dd.shape, false) && dd.method != MGH_DD_BLOCK && dd.method != MGH_DD_VARIABLE) {
    dd.decomposed = false;  // DomainDecomposer.hpp:303-311
    dd.dim = 0;
    dd.size = shape[0];
    dd.num = 1;
    return {};
  }
  dd.decomposed = true;
  if (dd.method == MGH_DD_MAXDIM) {  // :209-236
    uint64_t mx = 0;
    for (int d = 0; d < D; d++)
      if (shape[d] > mx) {
        mx = shape[d];
        dd.dim = d;
      }
    std::vector<uint64_t> cs = dd.shape;
    bool prefetch = false;
    while (need(cs, prefetch)) {
      if (cs[dd.dim] <= 3) return {MGH_ERR_OUT_OF_MEMORY, "domain decomposition: not enough device memory"};
      cs[dd.dim] = (cs[dd.dim] - 1) / 2 + 1;
      prefetch = (shape[dd.dim] - 1) / cs[dd.dim] + 1 > 1;
    }
    dd.size = cs[dd.dim];
    dd.num = (shape[dd.dim] - 1) / dd.size + 1;
  } else if (dd.method == MGH_DD_BLOCK) {  // :238-263, 335-349
    dd.size = block_size;
    if (dd.size < 3) return {MGH_ERR_INVALID_ARGUMENT, "block_size"};
    for (;;) {
      std::vector<uint64_t> cs(D, dd.size);
      uint64_t cnt = 1;
      for (int d = 0; d < D; d++) cnt *= (shape[d] - 1) / dd.size + 1;
      if (!need(cs, cnt > 1)) break;
      if (dd.size <= 3) return {MGH_ERR_OUT_OF_MEMORY, "domain decomposition: not enough device memory"};
      dd.size = (dd.size - 1) / 2 + 1;
    }
    dd.num = 1;
    for (int d = 0; d < D; d++) dd.num *= (shape[d] - 1) / dd.size + 1;
  } else if (dd.method == MGH_DD_VARIABLE) {  // :350-357
    if (var_dim < 0 || var_dim >= D || !var_sizes || !nvar)
      return {MGH_ERR_INVALID_ARGUMENT, "Variable domain decomposition needs dim and sizes"};
    dd.dim = var_dim;
    dd.var_sizes.assign(var_sizes, var_sizes + nvar);
    uint64_t sum = 0;
    for (uint64_t v : dd.var_sizes) sum += v;
    if (sum != shape[dd.dim]) return {MGH_ERR_INVALID_ARGUMENT, "Variable sizes do not add up to the extent"};
    dd.num = dd.var_sizes.size();
    dd.size = dd.var_sizes[0];
  } else {
    return {MGH_ERR_INVALID_ARGUMENT, "domain_decomposition"};
  }
  for (uint64_t id = 0; id < dd.num; id++)
    for (uint64_t e : dd.subdomain_shape(id))
      if (e < 3) return {MGH_ERR_INVALID_ARGUMENT, "domain decomposition leaves a subdomain with fewer than 3 nodes in a dimension"};
  return {};
}

// ceil(n0 / ndev) planes per slab, grown until the last slab has at least 3 planes (a hierarchy needs them)
inline uint64_t multi_slab_size(uint64_t n0, int ndev) {
  uint64_t size = (n0 + ndev - 1) / ndev;
  size = std::max<uint64_t>(size, 3);
  while (size < n0 && n0 % size != 0 && n0 % size < 3) size++;
  return size;
}

// slabs of dimension 0 in rank order: all of one size, the last one may be shorter. MGH_ERR_INVALID_ARGUMENT.
inline const char *dist_slab_size(const std::vector<uint64_t> &n0, uint64_t *size) {
  *size = n0[0];
  for (size_t r = 0; r + 1 < n0.size(); r++)
    if (n0[r] != *size) return "mgh_*_dist: every rank but the last must hold the same number of planes";
  if (n0.back() > *size || n0.back() < 3) return "mgh_*_dist: the last rank holds more planes than the others, or fewer than 3";
  return nullptr;
}

// ---- what a header says of the decomposition (extents are not looked at: check_extents, stitched_layout) ----
inline Refusal decomposer_from_header(const fmt::Header &hd, const uint64_t *var_sizes, uint64_t nvar, Decomposer &dd) {
  dd.D = (int)hd.shape.size();
  dd.shape = hd.shape;
  dd.decomposed = hd.dd_method != fmt::DD_NOOP;
  dd.dim = hd.dd_dim;
  dd.size = hd.dd_size;
  dd.num = 1;
  if (!dd.decomposed) return {};
  if (dd.dim >= (uint64_t)dd.D || dd.size == 0) return {MGH_ERR_FORMAT, "header: domain decomposition"};
  if (hd.dd_method == fmt::DD_MAX_DIMENSION) {
    dd.method = MGH_DD_MAXDIM;
    dd.num = (dd.shape[dd.dim] - 1) / dd.size + 1;
  } else if (hd.dd_method == fmt::DD_BLOCK) {
    dd.method = MGH_DD_BLOCK;
    for (int d = 0; d < dd.D; d++) dd.num *= (dd.shape[d] - 1) / dd.size + 1;
  } else if (hd.dd_method == fmt::DD_VARIABLE) {
    // the header records one size only; like the reference the caller's config supplies the
    // list (DomainDecomposer.hpp:448-452)
    dd.method = MGH_DD_VARIABLE;
    if (!var_sizes || !nvar)
      return {MGH_ERR_INVALID_ARGUMENT, "Variable domain decomposition: pass the sizes in the config"};
    dd.var_sizes.assign(var_sizes, var_sizes + nvar);
    uint64_t sum = 0;
    for (uint64_t v : dd.var_sizes) sum += v;
    if (sum != dd.shape[dd.dim]) return {MGH_ERR_INVALID_ARGUMENT, "Variable sizes do not add up to the extent"};
    dd.num = dd.var_sizes.size();
  } else {
    return {MGH_ERR_FORMAT, "header: unknown domain decomposition"};
  }
  return {};
}

// ---- a decomposed container after `halvings` coarsenings of every subdomain --------------------------
// Every subdomain has its own hierarchy and l_target, so a level number means a different resolution in
// each; the number of halvings (n -> n/2 + 1, the hierarchy's rule) means the same in all of them.
// Subdomain i is taken at level l_target_i - halvings, and because every block gets exactly `halvings`
// coarsenings its extent along d depends on its extent along d alone: the level arrays stitch into a
// tensor-product array for MaxDim, Block and Variable decompositions alike.
struct StitchedLayout {
  int K = 0;                                 // min over the subdomains of l_target: the most halvings possible
  std::vector<uint64_t> shape;               // of the stitched array
  std::vector<std::vector<uint64_t>> ext;    // [d][j]: extent of the block at grid position j after the halvings
  std::vector<std::vector<uint64_t>> off;    // [d][j]: its offset in the stitched array
  std::vector<std::vector<uint64_t>> nodes;  // [d]: index in the FULL array of every node of the stitched grid
};
// halvings < 0: only K. Extents are validated here (a header is untrusted). The node list is made for
// nodes_of_dim alone (it is as long as the extent of the full array).
inline Refusal stitched_layout(const Decomposer &dd, uint64_t max_level, int halvings, StitchedLayout &sl,
                               int nodes_of_dim = -1) {
  const int D = dd.D;
  if (D < 1 || D > MGH_MAX_DIM) return {MGH_ERR_UNSUPPORTED_DIMENSION, "header: dimension"};
  if (const char *bad = check_extents(dd)) return {MGH_ERR_FORMAT, bad};
  sl.K = std::numeric_limits<int>::max();
  for (uint64_t id = 0; id < dd.num; id++) {
    const auto s = dd.subdomain_shape(id);
    sl.K = std::min(sl.K, mgh::hierarchy_l_target(s.size(), s.data(), max_level));
  }
  if (halvings < 0) return {};
  if (halvings > sl.K) return {MGH_ERR_INVALID_ARGUMENT, "halvings outside 0 .. the smallest l_target of the subdomains"};
  const auto nd = dd.dim_num_subdomain();
  sl.shape.assign(D, 0);
  sl.ext.assign(D, {});
  sl.off.assign(D, {});
  sl.nodes.assign(D, {});
  std::vector<uint64_t> idx;
  for (int d = 0; d < D; d++) {
    uint64_t stride = 1;  // subdomain ids are row-major over the decomposition grid
    for (int e = d + 1; e < D; e++) stride *= nd[e];
    for (uint64_t j = 0; j < nd[d]; j++) {
      const uint64_t id = j * stride;  // (grid position j along d, 0 elsewhere)
      const uint64_t n = dd.subdomain_shape(id)[d], at = dd.subdomain_offset(id)[d];
      uint64_t m = n;
      for (int k = 0; k < halvings; k++) m = m / 2 + 1;
      sl.ext[d].push_back(m);
      sl.off[d].push_back(sl.shape[d]);
      sl.shape[d] += m;
      if (d != nodes_of_dim) continue;
      mgh::level_nodes(n, halvings, idx);
      for (uint64_t i : idx) sl.nodes[d].push_back(at + i);
    }
  }
  return {};
}

// ---- the error budget of a decomposed domain -----------------------------------------------------------
// The norm of the whole domain from the norms of its subdomains (ErrorToleranceCalculator.hpp:69-89): their
// maximum for s = inf, else the root of the sum of their squares, un-normalised by the element count when the
// coordinates are normalised. A rank of the distributed path adds its own norm and reduces `acc` over the ranks.
struct NormAccumulator {
  bool inf = false, normalize = false;
  double acc = 0;
  void add(double ln, uint64_t count) {
    if (inf) acc = std::max(acc, ln);
    else acc += ln * ln * (normalize ? (double)count : 1.0);  // un-normalised square
  }
  double result(uint64_t total) const {
    if (inf) return acc;
    return normalize ? std::sqrt(acc / (double)total) : std::sqrt(acc);
  }
};

// calc_local_abs_tol (ErrorToleranceCalculator.hpp:134-155), in the data type
template <typename T> T local_abs_tol(int ebtype, T norm, T tol, T s, uint64_t nsub) {
  if (ebtype == MGH_REL) {
    if (s == std::numeric_limits<T>::infinity()) return tol * norm;
    return std::sqrt((tol * norm) * (tol * norm) / (T)nsub);
  }
  if (s == std::numeric_limits<T>::infinity()) return tol;
  return std::sqrt((tol * tol) / (T)nsub);
}

// ---- one slab of a container as a container of its own ---------------------------------------------------
// The header of slab `id` of a container cut along dimension 0: everything the stream says about itself (reorder,
// lossless choice, dictionary, ...) stays; only what describes the slab changes.
inline fmt::Header slab_header(const fmt::Header &hd, const Decomposer &dd, uint64_t id, double local_tol) {
  fmt::Header sh = hd;
  sh.shape = dd.subdomain_shape(id);
  if (!hd.uniform) {
    const uint64_t o0 = dd.subdomain_offset(id)[0];
    sh.coords[0].assign(hd.coords[0].begin() + o0, hd.coords[0].begin() + o0 + sh.shape[0]);
  }
  sh.rel = false;
  sh.tol = local_tol;
  sh.norm = 0.0;
  sh.dd_method = fmt::DD_NOOP;
  sh.dd_dim = 0;
  sh.dd_size = 0;
  return sh;
}

// The records follow the header as `[u64 size][record]` frames in id order (GPUPipelines.hpp:189-193). A frame at
// byte `at` of `size`: whether its prefix may be read, and with the prefix `cs` where the next starts. MGH_ERR_FORMAT.
inline const char *frame_prefix(size_t size, size_t at) { return at + 8 > size ? "truncated stream" : nullptr; }
inline const char *frame_next(size_t size, size_t at, uint64_t cs, size_t *next) {
  if (cs > size - at - 8) return "truncated record";
  *next = at + 8 + (size_t)cs;
  return nullptr;
}

} // namespace mgh
