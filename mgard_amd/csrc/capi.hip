// C ABI implementation (include/mgard_hip.h) of the MI355X-native MGARD-X hot
// path. Host orchestration only: the level loop of
// multi_dimension::decompose/recompose
// (reference include/mgard-x/DataRefactoring/MultiDimension/DataRefactoring.hpp:25-317)
// over the HIP kernels in kernels_*.hpp.
#include "../../include/mgard_hip.h"
#include "../../include/mgard_hip_level_layers.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "env.hpp"
#include "hierarchy.hpp"
#include "ld_view.hpp"
#include "ipk_plan.hpp"
#include "fused_plan.hpp"
#include "kernels_v1.hpp"
#include "kernels_ipk.hpp"
#include "kernels_ipk_stream.hpp"
#include "kernels_ipk_spec.hpp"
#include "kernels_ipk_dma.hpp"
#include "kernels_fused.hpp"
#include "kernels_fused2.hpp"
#include "kernels_box.hpp"
#include "kernels_tail.hpp"
#include "kernels_recompose.hpp"
#include "kernels_recompose2.hpp"
#include "kernels_nd.hpp"
#include "kernels_level.hpp"
#include "kernels_prolong.hpp"
#include "kernels_prolong_win.hpp"
#include "prolong_plan.hpp"
#include "prolong_window_plan.hpp"
#include "compare_plan.hpp"
#include "kernels_compare.hpp"
#include "size_plan.hpp"
#include "kernels_qhist.hpp"
#include "target_plan.hpp"
#include "kernels_qround.hpp"
#include "kernels_qsym.hpp"
#include "kernels_mask.hpp"
#include "kernels_pwrel.hpp"
#include "kernels_roi.hpp"

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      return fail(_e == hipErrorOutOfMemory ? MGH_ERR_OUT_OF_MEMORY : MGH_ERR_DEVICE,          \
                  std::string(#expr) + ": " + hipGetErrorString(_e));                          \
  } while (0)

struct ProfileEntry {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  double total_ms = 0;
  uint64_t launches = 0;
};

} // namespace

struct mgh_hierarchy {
  int dtype = MGH_FLOAT;
  int device = 0;
  size_t num_cu = 256;  // compute units of the device (hipDeviceAttributeMultiprocessorCount)
  int D = 0, L = 0;
  uint64_t total = 0;
  uint64_t plane_elems = 0;  // product of the two fastest dimensions
  void *host = nullptr;  // HostHierarchy<T>*
  void *impl = nullptr;  // DeviceState<T>*
  bool profiling = false;
  int nd_rows = 1;  // MGH_ND_ROWS: the generic N-D path runs its row-wise kernels (kernels_nd.hpp; 0 = one thread per element, cross-check)
  bool force_nd_ipk = false;  // MGH_ND_IPK=1: the generic N-D path solves with its own one-thread-per-pencil kernel (cross-check)
  bool force_v1 = false;  // MGH_FORCE_V1=1: run the one-thread-per-element kernels only (unset: also for thin shapes, see mgh_hierarchy_create; 0: never)
  int force_v1_env = -1;
  bool force_nd = false;  // MGH_FORCE_ND=1: run the generic N-D kernels also for D <= 3 (cross-check)
  std::string prof_filter;  // empty = every kernel
  mgh::IpkTuning ipk;  // MGH_IPK_*: what the Thomas-solve planner goes by (ipk_plan.hpp)
  int absmax_warm_mb = 192;  // MGH_ABSMAX_WARM_MB: the norm pass reads all but the last so many MB of the input with nontemporal loads
  // MGH_FUSED_FACES / _TALL / _XCD / _WIDE, MGH_BOX, MGH_CLS1 / MGH_CLS2, MGH_RCH, MGH_FUSED_SLOTS: what
  // the planner of the fused level passes goes by (fused_plan.hpp)
  mgh::FusedTuning fused;
  // workgroups per CU of the k_level_fused2 instances this hierarchy can launch, as the runtime
  // reports them when the hierarchy is created (fused_residency_init; key: fused_instance_key)
  std::map<int, int> fused_wg_per_cu;
  int slice_batch = 1;  // MGH_SLICE_BATCH: D = 4 decompression, all t-slices of a kind in one launch (default 1)
  int fused_fixed = 1; // MGH_FUSED_FIXED: the int64 + dictionary variant of the level kernel (default 1)
  int fused4 = 1;     // MGH_FUSED4: D = 4 through the 3-D tile code, slice by slice (default 1)
  int outlier_agg = 2;  // MGH_OUTLIER_AGG: the level kernel asks for outlier slots once per workgroup and pair step instead of once per wave and plane (kernels_fused2.hpp: OutlierShared): 0 never, 1 always, 2 when the previous call on this hierarchy left more than 0.5 % of its values (and more than 200 000) in the outlier list
  int sym16_mixed = 1;  // MGH_SYM16_MIXED: 16-bit symbols for the finest level only, int64 below it (default), 0 = 16-bit symbols on every level
  int tail_solves = 1;  // MGH_TAIL_SOLVES: the tail kernel runs the Thomas solves of the level above it
  // (the rest of the developer switches, env.hpp; all read when the hierarchy is created)
  int ipk_range_mb = 128;          // MGH_IPK_RANGE_MB: f- and c-solve of a load vector bigger than twice this run in r-plane ranges of this size (0 = off)
  bool no_head = false;            // MGH_NO_RECOMPOSE_HEAD
  bool debug_sync = false;         // MGH_DEBUG_SYNC: name every launch on stderr and synchronise behind it
  std::map<std::string, ProfileEntry> prof;
  // while `profiling`: one record per Thomas solve that went through ipk_launch, the first
  // kIpkLogCap of them (mgh_debug_ipk_plans_read; MGH_IPK_PLAN_FIELDS values each, in its order)
  std::vector<std::array<long long, MGH_IPK_PLAN_FIELDS>> ipk_log;
  // while `profiling`: one record per level that went through the fused planner, the first
  // kIpkLogCap of them (mgh_debug_fused_plans_read; MGH_FUSED_PLAN_FIELDS values each)
  std::vector<std::array<long long, MGH_FUSED_PLAN_FIELDS>> fused_log;
  size_t device_bytes = 0;
  uint64_t shape[MGH_MAX_DIM] = {};
  // mgh_set_ld: leading dimensions of the caller's T arrays, [MGH_LD_IN / MGH_LD_OUT][dim]
  uint64_t ld[2][MGH_MAX_DIM] = {};
  bool has_ld[2] = {false, false};
};

namespace {

using namespace mgh;

// Warm-up length of the chunked sweeps (thomas_chunked) for one Thomas table: a chunk starts
// from state 0 instead of the true state, an error of the size of the data; after K steps it is
// that times the product of the K multipliers it passed. For the two runs to MEET (and not
// only to be close) the error has to fall far below one unit in the last place: the smallest K
// for which every window of K consecutive multipliers has a product below 2^-(mantissa + 12),
// rounded up to 8. (A bad guess costs time, not correctness: a chunk that has not met is
// detected and the tile solved again by one lane per pencil.)
template <typename T> int chunk_warmup_need(const std::vector<T> &tt) {
  const size_t n = tt.size() / 3;
  if (n < 2) return 0;
  const double target = -((sizeof(T) == 4 ? 24 : 53) + 12);
  std::vector<double> lf(n), lb(n);
  for (size_t i = 0; i < n; i++) {
    const double f = std::fabs((double)tt[i]);
    const double b = tt[2 * n + i] != 0 ? std::fabs((double)tt[n + i] / (double)tt[2 * n + i]) : 0.0;
    lf[i] = f > 0 ? std::log2(f) : -64.0;
    lb[i] = b > 0 ? std::log2(b) : -64.0;
  }
  int need = 0;
  for (const auto *lg : {&lf, &lb}) {
    for (size_t i = 0; i < n; i++) {  // windows starting at i (either direction: the same products)
      double acc = 0;
      size_t k = 0;
      while (i + k < n && acc > target) acc += (*lg)[i + k++];
      if (acc > target) break;  // the window ran into the end of the table: shorter ones are exact starts
      need = std::max(need, (int)k);
    }
  }
  return (need + 7) / 8 * 8;
}

template <typename T> struct LevelTables {
  // index k = 0,1,2 <-> (r, c, f) of the 3-D view; nullptr for inactive dims
  const T *ratio[3] = {nullptr, nullptr, nullptr};   // fine level l
  const T *mass[3] = {nullptr, nullptr, nullptr};    // l -> l-1
  const T *thomas[3] = {nullptr, nullptr, nullptr};  // coarse level l-1
  Box3 box;
  bool active[3] = {false, false, false};
};

template <typename T> struct DeviceState {
  HostHierarchy<T> *hh = nullptr;
  T *tables = nullptr;
  int *marks = nullptr;
  std::vector<LevelTables<T>> lt;  // [l], l >= 1 (3-D view, D <= 3)
  std::vector<size_t> lt_end;      // [l]: element offset in `tables` where the tables of level l end
                                   // (levels are laid out 1, 2, ... back to back: the tail kernel
                                   // copies the block of its levels to LDS in one pass)
  struct NdLevel {
    const T *ratio[kNd], *mass[kNd], *thomas[kNd];
  };
  std::vector<NdLevel> nd;         // [l], l >= 1 (all D dims; used by the D > 3 path)
  T *nd_w = nullptr, *nd_a = nullptr, *nd_b = nullptr;  // N-D scratch (lazily allocated)
  size_t nd_cap = 0;               // ... elements of each (a stop below the finest level needs that level's box only)
  // fused D = 4 path (lazily allocated): compact coarse arrays per level, per-slice load vectors
  // of the biggest level (padded slice positions), t-swept load vector / correction
  std::vector<T *> nodal4;
  T *load4 = nullptr, *corr4 = nullptr;
  bool state4_ready = false;       // set only once every allocation of ensure_state4 succeeded
  std::vector<T *> nodal;          // [l] compact nodal buffers, l = 0..L-1
  T *t1 = nullptr, *t2 = nullptr, *t3 = nullptr;
  int t12_level = 0;               // t1 / t2 hold the sweeps of levels up to this one (0: not allocated)
  T *level_box = nullptr;          // compact coefficients of the corner box of a stop level (mgh_*_to_level; grown on demand)
  size_t level_box_elems = 0;
  T *lin_box = nullptr;            // mgh_recompose_linear_to_level: the compact box of the level out of the linearised head (grown on demand)
  size_t lin_box_elems = 0;
  T *scratch_full = nullptr;      // lazily allocated full-size copy
  // mgh_prolong_window: the window's part of two consecutive levels (grown on demand, sized by the
  // window), and on the shapes without a window kernel the full-grid array the window is cut from
  T *win[2] = {nullptr, nullptr};
  size_t win_elems[2] = {0, 0};
  T *win_full = nullptr;
  size_t win_full_elems = 0;
  T *qz = nullptr;                 // 2*(L+1): quantizers, volumes
  T *qh_tab = nullptr;             // mgh_quantize_histograms: [ntol][L+1] quantizers, [L+1] volumes (grown on demand)
  size_t qh_tab_elems = 0;
  T *qr_tab = nullptr;             // mgh_quantize_roundtrip: 4*(L+1): reciprocal quantizers, their volumes, quantizers, theirs
  size_t qr_tab_elems = 0;
  unsigned long long *scalar = nullptr;  // 8-byte device scalar (norm / counters)
  // fused device-norm path: fscal[slot] is zero on entry, the other slot is zeroed by
  // k_make_qparams for the next call; `fscal_dirty` marks a call that died in between
  unsigned long long *fscal = nullptr;
  int scalar_slot = 0;
  bool fscal_dirty = false;
  // mgh_norm_stream_begin/add: the slot of the NEXT fused call already holds the reduction of its
  // input (accumulated slab by slab while the input was arriving from the host)
  bool norm_streamed = false;
  T *normval = nullptr;                  // norm as T, written by k_make_qparams
  unsigned long long *oh_key = nullptr;  // outlier table of the 16-bit symbol path (grown on demand)
  long long *oh_val = nullptr;
  size_t oh_slots = 0;
  int64_t *qbox = nullptr;               // ... and its compact int64 copy of the coarse corner box
  size_t qbox_elems = 0;
  // chunked Thomas solves of few long pencils (kernels_ipk_spec.hpp): forward results, chunk-edge values
  T *spec_y = nullptr, *spec_a = nullptr, *spec_b = nullptr;
  size_t spec_y_elems = 0, spec_edge_elems = 0;
  unsigned long long *spec_fixed = nullptr;  // chunks that had to be recomputed (diagnostics)
  // outlier count of an earlier call, written by its last kernel into host memory (hipHostMalloc;
  // the device writes through the same pointer): picks the level kernel's variant, see outlier_agg
  unsigned long long *outliers_seen = nullptr;
  QuantMeta qmeta;
  size_t full_I = 0, full_J = 0;   // strides of the full array in the 3-D view
  T *pack_in = nullptr, *pack_out = nullptr;  // dense copies of pitched arrays (lazily allocated)
};

template <typename T> HostHierarchy<T> *HH(const mgh_hierarchy *h) {
  return static_cast<HostHierarchy<T> *>(h->host);
}
template <typename T> DeviceState<T> *DS(const mgh_hierarchy *h) {
  return static_cast<DeviceState<T> *>(h->impl);
}

// ---- profiled launch -------------------------------------------------------
template <typename F> int launch(mgh_hierarchy *h, const char *name, hipStream_t s, F &&f) {
  // MGH_DEBUG_SYNC=1: name every launch on stderr and synchronise behind it, so that a GPU
  // memory fault can be attributed to a kernel (developer aid)
  if (h->debug_sync) {
    std::fprintf(stderr, "[mgh] %s\n", name);
    std::fflush(stderr);
    f();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return MGH_SUCCESS;
  }
  if (!h->profiling || (!h->prof_filter.empty() && h->prof_filter != name)) {
    f();
    HIP_TRY(hipGetLastError());
    return MGH_SUCCESS;
  }
  hipEvent_t a, b;
  HIP_TRY(hipEventCreate(&a));
  HIP_TRY(hipEventCreate(&b));
  HIP_TRY(hipEventRecord(a, s));
  f();
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(b, s));
  h->prof[name].pending.emplace_back(a, b);
  return MGH_SUCCESS;
}

// The same for ONE kernel whose timing is read inside timed regions (the level pass: bench.py
// keeps HIP events on the dominant kernel during the timed steps): hipExtLaunchKernelGGL stamps
// the start and stop events from the dispatch itself instead of two marker packets around the
// launch. Cost of the events per 512^3 step (tools/exp_gap.py, 20 steps each, same box): none
// 0.899-0.905 ms, marker packets +4 us, kernel-attached +1.5 us. (The ~6 us gaps a rocprofv3
// timeline shows on either side of the profiled kernel are there with both kinds of events.)
template <typename K, typename... Args>
int launch_kernel(mgh_hierarchy *h, const char *name, hipStream_t s, K kernel, dim3 grid, dim3 block,
                  size_t lds, Args... args) {
  if (h->debug_sync || !h->profiling || (!h->prof_filter.empty() && h->prof_filter != name))
    return launch(h, name, s, [&] { hipLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, s, args...); });
  hipEvent_t a, b;
  HIP_TRY(hipEventCreate(&a));
  HIP_TRY(hipEventCreate(&b));
  hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, s, a, b, 0, args...);
  HIP_TRY(hipGetLastError());
  h->prof[name].pending.emplace_back(a, b);
  return MGH_SUCCESS;
}

#define TRY(expr)                 \
  do {                            \
    int _rc = (expr);             \
    if (_rc != MGH_SUCCESS) return _rc; \
  } while (0)

inline dim3 grid3(uint32_t n0, uint32_t n1, uint32_t n2, dim3 blk) {
  return dim3((n2 + blk.x - 1) / blk.x, (n1 + blk.y - 1) / blk.y, n0);
}

template <typename T> int dev_alloc(mgh_hierarchy *h, T **p, size_t count) {
  *p = nullptr;
  if (count == 0) return MGH_SUCCESS;
  HIP_TRY(hipMalloc((void **)p, count * sizeof(T)));
  h->device_bytes += count * sizeof(T);
  return MGH_SUCCESS;
}

// mirror of dev_alloc: frees *p (if any) and takes its bytes out of the handle's footprint
template <typename T> void dev_free(mgh_hierarchy *h, T **p, size_t count) {
  if (!*p) return;
  if (hipFree(*p) == hipSuccess) h->device_bytes -= std::min(h->device_bytes, count * sizeof(T));
  *p = nullptr;
}

template <typename T> int build_device_state(mgh_hierarchy *h) {
  HostHierarchy<T> *hh = HH<T>(h);
  auto *ds = new DeviceState<T>();
  h->impl = ds;
  ds->hh = hh;
  const int D = hh->D, L = hh->L;
  if (D > 3) {
    // generic per-dim tables for the N-D kernels
    std::vector<T> arena;
    auto push = [&](const std::vector<T> &v) {
      size_t off = arena.size();
      arena.insert(arena.end(), v.begin(), v.end());
      while (arena.size() % 4) arena.push_back(0);
      return off;
    };
    struct Off { size_t r[kNd], m[kNd], t[kNd]; };
    std::vector<Off> offs(L + 1);
    for (int l = 1; l <= L; l++)
      for (int d = 0; d < D; d++) {
        offs[l].r[d] = push(hh->lv[l][d].ratio);
        offs[l].m[d] = push(hh->mass_table(l, d));
        offs[l].t[d] = push(hh->thomas_table(l - 1, d));
      }
    TRY(dev_alloc(h, &ds->tables, arena.size()));
    HIP_TRY(hipMemcpy(ds->tables, arena.data(), arena.size() * sizeof(T), hipMemcpyHostToDevice));
    ds->nd.resize(L + 1);
    for (int l = 1; l <= L; l++)
      for (int d = 0; d < D; d++) {
        ds->nd[l].ratio[d] = ds->tables + offs[l].r[d];
        ds->nd[l].mass[d] = ds->tables + offs[l].m[d];
        ds->nd[l].thomas[d] = ds->tables + offs[l].t[d];
      }
    std::vector<int> marks;
    ds->qmeta.D = D;
    ds->qmeta.calc_vol = 0;
    for (int d = 0; d < D; d++) {
      ds->qmeta.shape[d] = (uint32_t)hh->shape[d];
      ds->qmeta.markoff[d] = (uint32_t)marks.size();
      marks.insert(marks.end(), hh->marks[d].begin(), hh->marks[d].end());
    }
    TRY(dev_alloc(h, &ds->marks, marks.size()));
    HIP_TRY(hipMemcpy(ds->marks, marks.data(), marks.size() * sizeof(int), hipMemcpyHostToDevice));
    TRY(dev_alloc(h, &ds->qz, (size_t)2 * (L + 1)));
    TRY(dev_alloc(h, &ds->scalar, (size_t)2));
    TRY(dev_alloc(h, &ds->fscal, (size_t)2));
    HIP_TRY(hipMemset(ds->fscal, 0, 16));
    TRY(dev_alloc(h, &ds->normval, (size_t)2));
    return MGH_SUCCESS;
  }

  // ---- spacing tables: one arena, one upload --------------------------------
  std::vector<T> arena;
  auto push = [&](const std::vector<T> &v) {
    size_t off = arena.size();
    arena.insert(arena.end(), v.begin(), v.end());
    while (arena.size() % 4) arena.push_back(0);  // keep 16-byte alignment for f32
    return off;
  };
  struct Off {
    size_t ratio[3], mass[3], thomas[3];
  };
  std::vector<Off> offs(L + 1);
  ds->lt.resize(L + 1);
  for (int l = 1; l <= L; l++) {
    LevelTables<T> &t = ds->lt[l];
    for (int k = 0; k < 3; k++) {
      const int d = D - 3 + k;
      if (d < 0) {
        t.box.n[k] = t.box.m[k] = 1;
        t.active[k] = false;
        continue;
      }
      t.active[k] = true;
      t.box.n[k] = (uint32_t)hh->level_shape[l][d];
      t.box.m[k] = (uint32_t)hh->level_shape[l - 1][d];
      offs[l].ratio[k] = push(hh->lv[l][d].ratio);
      offs[l].mass[k] = push(hh->mass_table(l, d));
      const std::vector<T> tt = hh->thomas_table(l - 1, d);
      h->ipk.chunk_need = std::max(h->ipk.chunk_need, chunk_warmup_need(tt));
      offs[l].thomas[k] = push(tt);
    }
  }
  TRY(dev_alloc(h, &ds->tables, arena.size()));
  HIP_TRY(hipMemcpy(ds->tables, arena.data(), arena.size() * sizeof(T), hipMemcpyHostToDevice));
  ds->lt_end.assign(L + 1, 0);
  for (int l = 1; l <= L; l++) {
    size_t next = arena.size();
    for (int l2 = l + 1; l2 <= L && next == arena.size(); l2++)
      for (int k = 0; k < 3; k++)
        if (ds->lt[l2].active[k]) {
          next = offs[l2].ratio[k];
          break;
        }
    ds->lt_end[l] = next;
  }
  for (int l = 1; l <= L; l++)
    for (int k = 0; k < 3; k++)
      if (ds->lt[l].active[k]) {
        ds->lt[l].ratio[k] = ds->tables + offs[l].ratio[k];
        ds->lt[l].mass[k] = ds->tables + offs[l].mass[k];
        ds->lt[l].thomas[k] = ds->tables + offs[l].thomas[k];
      }

  // per-dim view of the same tables for the generic N-D kernels (cross-check path)
  ds->nd.resize(L + 1);
  for (int l = 1; l <= L; l++)
    for (int d = 0; d < D; d++) {
      const int k = d + 3 - D;
      ds->nd[l].ratio[d] = ds->lt[l].ratio[k];
      ds->nd[l].mass[d] = ds->lt[l].mass[k];
      ds->nd[l].thomas[d] = ds->lt[l].thomas[k];
    }

  // ---- level marks ------------------------------------------------------------
  std::vector<int> marks;
  ds->qmeta.D = D;
  ds->qmeta.calc_vol = 0;
  for (int d = 0; d < D; d++) {
    ds->qmeta.shape[d] = (uint32_t)hh->shape[d];
    ds->qmeta.markoff[d] = (uint32_t)marks.size();
    marks.insert(marks.end(), hh->marks[d].begin(), hh->marks[d].end());
  }
  TRY(dev_alloc(h, &ds->marks, marks.size()));
  HIP_TRY(hipMemcpy(ds->marks, marks.data(), marks.size() * sizeof(int), hipMemcpyHostToDevice));

  // ---- workspace ----------------------------------------------------------------
  ds->nodal.assign(L + 1, nullptr);
  for (int l = 0; l < L; l++) {
    size_t cnt = 1;
    for (int d = 0; d < D; d++) cnt *= hh->level_shape[l][d];
    TRY(dev_alloc(h, &ds->nodal[l], cnt));
  }
  if (L >= 1) {
    const Box3 &b = ds->lt[L].box;
    // t1 / t2 (intermediate sweeps of the one-thread-per-element path) are allocated on first
    // use: the fused 3-D path never needs them
    TRY(dev_alloc(h, &ds->t3, (size_t)b.m[0] * b.m[1] * b.m[2]));
  }
  TRY(dev_alloc(h, &ds->qz, (size_t)2 * (L + 1)));
  TRY(dev_alloc(h, &ds->scalar, (size_t)2));
  TRY(dev_alloc(h, &ds->fscal, (size_t)2));
  HIP_TRY(hipMemset(ds->fscal, 0, 16));
  TRY(dev_alloc(h, &ds->normval, (size_t)2));
  ds->full_J = hh->shape[D - 1];
  ds->full_I = (D >= 2 ? hh->shape[D - 2] : 1) * ds->full_J;
  return MGH_SUCCESS;
}

template <typename T> void destroy_state(mgh_hierarchy *h) {
  auto *ds = DS<T>(h);
  if (ds) {
    (void)hipFree(ds->tables);
    (void)hipFree(ds->marks);
    for (T *p : ds->nodal) (void)hipFree(p);
    (void)hipFree(ds->t1);
    (void)hipFree(ds->t2);
    (void)hipFree(ds->t3);
    (void)hipFree(ds->scratch_full);
    (void)hipFree(ds->win[0]);
    (void)hipFree(ds->win[1]);
    (void)hipFree(ds->win_full);
    (void)hipFree(ds->pack_in);
    (void)hipFree(ds->pack_out);
    (void)hipFree(ds->nd_w);
    (void)hipFree(ds->nd_a);
    (void)hipFree(ds->nd_b);
    for (T *p : ds->nodal4) (void)hipFree(p);
    (void)hipFree(ds->load4);
    (void)hipFree(ds->corr4);
    (void)hipFree(ds->qz);
    (void)hipFree(ds->qh_tab);
    (void)hipFree(ds->qr_tab);
    (void)hipFree(ds->scalar);
    (void)hipFree(ds->fscal);
    (void)hipFree(ds->normval);
    (void)hipFree(ds->oh_key);
    (void)hipFree(ds->oh_val);
    (void)hipFree(ds->qbox);
    (void)hipFree(ds->level_box);
    (void)hipFree(ds->lin_box);
    (void)hipFree(ds->spec_y);
    (void)hipFree(ds->spec_a);
    (void)hipFree(ds->spec_b);
    (void)hipFree(ds->spec_fixed);
    (void)hipHostFree(ds->outliers_seen);
    delete ds;
  }
  delete HH<T>(h);
}

template <typename T> int ensure_scratch(mgh_hierarchy *h) {
  auto *ds = DS<T>(h);
  if (!ds->scratch_full) TRY(dev_alloc(h, &ds->scratch_full, (size_t)h->total));
  return MGH_SUCCESS;
}

// (`bytes`: the dynamic part; a kernel with static LDS of its own asks for that much less)
template <typename K> int allow_big_lds(K kernel, size_t bytes = kLdsPerCU) {
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return MGH_SUCCESS;
}
// ... once per DEVICE (the attribute belongs to the function on the current device) and safe
// from several host threads: `done` holds one bit per device ordinal.
template <typename K> int allow_big_lds_once(K kernel, std::atomic<uint64_t> &done, size_t bytes = kLdsPerCU) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  const uint64_t bit = (uint64_t)1 << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return MGH_SUCCESS;
  TRY(allow_big_lds(kernel, bytes));
  done.fetch_or(bit, std::memory_order_release);
  return MGH_SUCCESS;
}

// ---- Thomas solves: one launcher per family of ipk_plan.hpp ------------------
// A run-time value as a compile-time one: f(std::integral_constant<int, V>) with the V that equals v.
template <int... V, typename F> int with_value(int v, F &&f) {
  int rc = MGH_ERR_INVALID_ARGUMENT;
  (void)((v == V ? (rc = f(std::integral_constant<int, V>{}), true) : false) || ...);
  return rc;
}

// What every launcher is given beside the plan: pointers, sign and where to launch.
template <typename T> struct IpkArgs {
  mgh_hierarchy *h;
  const char *name;  // profile name of the axis
  T *x;
  const T *tt;
  T *add_to;
  int sign;
  hipStream_t s;
  int add() const { return add_to ? (sign > 0 ? 1 : -1) : 0; }
};

// Scratch of the verified-chunk solve, grown on demand: forward results of `total` elements,
// two arrays of `edges` chunk-edge values, the repair counter and mismatch flags.
template <typename T> int spec_scratch(mgh_hierarchy *h, size_t total, size_t edges, hipStream_t s) {
  auto *ds = DS<T>(h);
  if (total > ds->spec_y_elems) {
    (void)hipFree(ds->spec_y);
    ds->spec_y = nullptr;
    ds->spec_y_elems = 0;
    HIP_TRY(hipMalloc(&ds->spec_y, total * sizeof(T)));
    ds->spec_y_elems = total;
  }
  if (edges > ds->spec_edge_elems) {
    (void)hipFree(ds->spec_a);
    (void)hipFree(ds->spec_b);
    ds->spec_a = ds->spec_b = nullptr;
    ds->spec_edge_elems = 0;
    HIP_TRY(hipMalloc(&ds->spec_a, edges * sizeof(T)));
    HIP_TRY(hipMalloc(&ds->spec_b, edges * sizeof(T)));
    ds->spec_edge_elems = edges;
  }
  if (!ds->spec_fixed) {  // [0]: chunks repaired so far, [1]: mismatch flags of the two sweeps of a call
    HIP_TRY(hipMalloc(&ds->spec_fixed, 16));
    HIP_TRY(hipMemsetAsync(ds->spec_fixed, 0, 16, s));
  }
  return MGH_SUCCESS;
}

template <typename T> int ipk_launch_spec(const IpkPlan &p, const IpkArgs<T> &a, int axis) {
  const IpkGeom &g = p.geom;
  const SpecGeom G{g.n, p.S, p.K, p.nchunk, g.npencil, g.n_inner, g.outer_stride, g.inner_stride, g.stride, axis != 2};
  const size_t total = (size_t)g.npencil * g.n;
  TRY(spec_scratch<T>(a.h, total, (size_t)g.npencil * p.nchunk, a.s));
  auto *ds = DS<T>(a.h);
  T *x = a.x, *y = ds->spec_y, *ea = ds->spec_a, *eb = ds->spec_b;
  unsigned long long *fx = ds->spec_fixed;
  unsigned *mm = reinterpret_cast<unsigned *>(ds->spec_fixed + 1);
  hipStream_t s = a.s;
  HIP_TRY(hipMemsetAsync(mm, 0, 8, s));
  return launch(a.h, a.name, s, [&] {
    k_ipk_spec_fwd<T><<<p.grid, 64, 0, s>>>(G, x, y, a.tt, ea, eb);
    k_ipk_spec_check<T><<<p.check_grid, 256, 0, s>>>(p.nchunk, g.npencil, ea, eb, +1, mm);
    k_ipk_spec_fix<T><<<p.fix_grid, 64, 0, s>>>(G, x, y, a.tt, ea, eb, +1, fx, mm);
    k_ipk_spec_bwd<T><<<p.grid, 64, 0, s>>>(G, y, x, a.tt, ea, eb);
    k_ipk_spec_check<T><<<p.check_grid, 256, 0, s>>>(p.nchunk, g.npencil, ea, eb, -1, mm + 1);
    k_ipk_spec_fix<T><<<p.fix_grid, 64, 0, s>>>(G, y, x, a.tt, ea, eb, -1, fx, mm + 1);
    if (a.add_to) k_ipk_spec_apply<T><<<p.apply_grid, 256, 0, s>>>(total, a.add_to, x, a.sign);
  });
}

template <typename T, bool CHUNKED> int ipk_launch_lds_contig(const IpkPlan &p, const IpkArgs<T> &a) {
  static std::atomic<uint64_t> once{0};
  TRY(allow_big_lds_once(k_ipk_lds_contig<T, CHUNKED>, once, p.lds_attr));
  return launch(a.h, a.name, a.s, [&] {
    k_ipk_lds_contig<T, CHUNKED><<<p.grid, p.block, p.lds, a.s>>>(p.geom.npencil, p.geom.n, p.pad, p.magic, p.P,
                                                                  a.x, a.tt, a.add_to, a.sign, p.K);
  });
}

template <typename T, int ADD> int ipk_launch_dma(const IpkPlan &p, const IpkArgs<T> &a) {
  constexpr uint32_t U = 64 / sizeof(T), KR = 10;
  const IpkGeom &g = p.geom;
  static std::atomic<uint64_t> once{0};
  TRY(allow_big_lds_once(k_ipk_dma<T, U, KR, ADD>, once, p.lds_attr));
  return launch(a.h, a.name, a.s, [&] {
    k_ipk_dma<T, U, KR, ADD><<<p.grid, p.block, p.lds, a.s>>>(g.npencil, g.n_inner, g.outer_stride, 1, g.stride,
                                                              g.n, a.x, a.tt, a.add_to);
  });
}

template <typename T, int KR, bool CONTIG> int ipk_launch_stream(const IpkPlan &p, const IpkArgs<T> &a) {
  constexpr uint32_t U = 64 / sizeof(T);
  const IpkGeom &g = p.geom;
  static std::atomic<uint64_t> once{0};
  TRY(allow_big_lds_once(k_ipk_stream<T, U, KR, 1, CONTIG, false>, once, p.lds_attr));
  return launch(a.h, a.name, a.s, [&] {
    k_ipk_stream<T, U, KR, 1, CONTIG, false><<<p.grid, p.block, p.lds, a.s>>>(
        g.npencil, g.n_inner, g.outer_stride, g.inner_stride, g.stride, g.n, p.W, p.n_glob, a.x, a.tt, a.add_to,
        a.sign);
  });
}

template <typename T, int W> int ipk_launch_lds_strided(const IpkPlan &p, const IpkArgs<T> &a) {
  const IpkGeom &g = p.geom;
  static std::atomic<uint64_t> once{0};
  TRY(allow_big_lds_once(k_ipk_lds_strided<T, W>, once, p.lds_attr));
  return launch(a.h, a.name, a.s, [&] {
    k_ipk_lds_strided<T, W><<<p.grid, p.block, p.lds, a.s>>>(g.npencil / g.n_inner, g.n_inner, g.outer_stride,
                                                             g.stride, g.n, a.x, a.tt, a.add_to, a.sign);
  });
}

template <typename T, int AXIS> int ipk_launch_thread(const IpkPlan &p, const IpkArgs<T> &a, const uint32_t *m) {
  return launch(a.h, a.name, a.s, [&] {
    k_ipk<T, AXIS><<<dim3(p.grid, p.grid_y, 1), dim3(p.block, 1, 1), 0, a.s>>>(m[0], m[1], m[2], a.x, a.tt,
                                                                             a.add_to, a.sign);
  });
}

constexpr size_t kIpkLogCap = 512;  // records mgh_hierarchy::ipk_log keeps

// Thomas solve along `axis` of the compact (m[0], m[1], m[2]) box, by the kernel ipk_plan() picks.
// axis 0 only: `nbatch` boxes `batch_stride` elements apart in ONE launch (the slices of a 4-D level).
template <typename T>
int ipk_launch(mgh_hierarchy *h, int axis, const uint32_t *m, T *x, const T *tt, T *add_to,
               int sign, hipStream_t s, uint32_t nbatch = 1, size_t batch_stride = 0) {
  if (nbatch > 1 && axis != 0) return fail(MGH_ERR_INVALID_ARGUMENT, "ipk_launch: batches along the slowest axis only");
  static const char *names[3] = {"ipk_r", "ipk_c", "ipk_f"};
  const IpkArgs<T> a{h, names[axis], x, tt, add_to, sign, s};
  const IpkPlan p = ipk_plan(h->ipk, sizeof(T), axis, m, nbatch, batch_stride);
  // (the boxes of a Thread plan with batches come back here one by one: a record each, none for the whole)
  if (h->profiling && !p.per_batch && h->ipk_log.size() < kIpkLogCap)
    h->ipk_log.push_back({(long long)p.kernel, axis, (long long)sizeof(T), m[0], m[1], m[2], nbatch, p.geom.n,
                          p.geom.npencil, p.W, p.n_glob, p.KR, p.P, p.K, a.add(), (long long)batch_stride});
  switch (p.kernel) {
  case IpkKernel::Spec: return ipk_launch_spec<T>(p, a, axis);
  case IpkKernel::LdsContigChunked: return ipk_launch_lds_contig<T, true>(p, a);
  case IpkKernel::Dma:
    if constexpr (sizeof(T) == 4)
      return with_value<0, 1, -1>(a.add(), [&](auto add) { return ipk_launch_dma<T, add()>(p, a); });
    break;  // (planned for 4-byte elements only)
  case IpkKernel::Stream:
    if constexpr (sizeof(T) == 4)
      if (p.KR == 16)
        return axis == 2 ? ipk_launch_stream<T, 16, true>(p, a) : ipk_launch_stream<T, 16, false>(p, a);
    return axis == 2 ? ipk_launch_stream<T, 8, true>(p, a) : ipk_launch_stream<T, 8, false>(p, a);
  case IpkKernel::LdsContig: return ipk_launch_lds_contig<T, false>(p, a);
  case IpkKernel::LdsStrided:
    return with_value<64, 48, 32, 16>((int)p.W, [&](auto w) { return ipk_launch_lds_strided<T, w()>(p, a); });
  case IpkKernel::Thread:
    if (p.per_batch) {
      for (uint32_t bi = 0; bi < nbatch; bi++)
        TRY(ipk_launch<T>(h, axis, m, x + (size_t)bi * batch_stride, tt,
                          add_to ? add_to + (size_t)bi * batch_stride : nullptr, sign, s));
      return MGH_SUCCESS;
    }
    return with_value<0, 1, 2>(axis, [&](auto ax) { return ipk_launch_thread<T, ax()>(p, a, m); });
  }
  return fail(MGH_ERR_INVALID_ARGUMENT, "ipk_launch: no kernel for this plan");
}

// f-solve and c-solve of a compact (m0, m1, m2) box: one launch when a coarse plane fits in LDS
// (every level but the biggest), else the two tiled kernels.
template <typename T>
int ipk_fc_launch(mgh_hierarchy *h, const uint32_t *m, T *x, const T *tt_f, const T *tt_c,
                  hipStream_t s) {
  const uint32_t pitch = m[2] | 1u;
  if (ipk_plane_fits_lds(sizeof(T), m)) {
    static std::atomic<uint64_t> once{0};
    TRY(allow_big_lds_once(k_ipk_plane_fc<T>, once));
    const uint32_t magic = (uint32_t)((((uint64_t)1 << 32) + m[2] - 1) / m[2]);  // e / m2, e < 2^32 / m2
    return launch(h, "ipk_fc", s, [&] {
      k_ipk_plane_fc<T><<<m[0], 256, (size_t)m[1] * pitch * sizeof(T), s>>>(m[1], m[2], pitch, magic,
                                                                              x, tt_f, tt_c);
    });
  }
  TRY(ipk_launch<T>(h, 2, m, x, tt_f, nullptr, +1, s));
  return ipk_launch<T>(h, 1, m, x, tt_c, nullptr, +1, s);
}

// ---- correction = IPK(LPK(coefficients)) then +/- into nodal[l-1] --------------
// CalcCorrection3D (Correction/CalcCorrection3D.hpp:26-185) + AddND/SubtractND.
template <typename T>
int correction(mgh_hierarchy *h, int l, const T *coef, size_t cI, size_t cJ, T *target, int sign,
               hipStream_t s, int top_level = -1) {
  auto *ds = DS<T>(h);
  const LevelTables<T> &t = ds->lt[l];
  const Box3 &b = t.box;
  const dim3 blk(64, 4, 1);
  // (top_level: the last level this call's loop runs -- a stop below the finest level sizes the
  // sweeps by its own box; -1: the finest)
  const int tl = top_level < 0 ? h->L : top_level;
  if (ds->t12_level < tl) {
    if (ds->t12_level >= 1) {
      const Box3 &ob = ds->lt[ds->t12_level].box;
      dev_free(h, &ds->t1, (size_t)ob.n[0] * ob.n[1] * ob.m[2]);
      dev_free(h, &ds->t2, (size_t)ob.n[0] * ob.m[1] * ob.m[2]);
      ds->t12_level = 0;
    }
    // (growing frees buffers that earlier launches on the caller's stream may still read: safe
    // because hipFree waits for the device; a failed attempt leaves nothing behind)
    const Box3 &tb = ds->lt[tl].box;
    const size_t c1 = (size_t)tb.n[0] * tb.n[1] * tb.m[2], c2 = (size_t)tb.n[0] * tb.m[1] * tb.m[2];
    int rc = dev_alloc(h, &ds->t1, c1);
    if (rc == MGH_SUCCESS) rc = dev_alloc(h, &ds->t2, c2);
    if (rc != MGH_SUCCESS) {
      dev_free(h, &ds->t1, c1);
      dev_free(h, &ds->t2, c2);
      return rc;
    }
    ds->t12_level = tl;
  }
  // LPK1 along f: (nr, nc, nf) -> (nr, nc, ff)
  TRY(launch(h, "lpk_f", s, [&] {
    k_lpk<T, 2><<<grid3(b.n[0], b.n[1], b.m[2], blk), blk, 0, s>>>(
        b.n[0], b.n[1], b.n[2], b.n[2], b.m[2], coef, cI, cJ, ds->t1, (size_t)b.n[1] * b.m[2],
        (size_t)b.m[2], t.mass[2], b.m[0], b.m[1]);
  }));
  T *cur = ds->t1;
  if (t.active[1]) {
    TRY(launch(h, "lpk_c", s, [&] {
      k_lpk<T, 1><<<grid3(b.n[0], b.m[1], b.m[2], blk), blk, 0, s>>>(
          b.n[0], b.n[1], b.m[2], b.n[1], b.m[1], cur, (size_t)b.n[1] * b.m[2], (size_t)b.m[2],
          ds->t2, (size_t)b.m[1] * b.m[2], (size_t)b.m[2], t.mass[1], 0, 0);
    }));
    cur = ds->t2;
  }
  if (t.active[0]) {
    TRY(launch(h, "lpk_r", s, [&] {
      k_lpk<T, 0><<<grid3(b.m[0], b.m[1], b.m[2], blk), blk, 0, s>>>(
          b.n[0], b.m[1], b.m[2], b.n[0], b.m[0], cur, (size_t)b.m[1] * b.m[2], (size_t)b.m[2],
          ds->t3, (size_t)b.m[1] * b.m[2], (size_t)b.m[2], t.mass[0], 0, 0);
    }));
    cur = ds->t3;
  }
  // IPK along f, c, r; the last one applies the correction to `target`
  const int last = t.active[0] ? 0 : (t.active[1] ? 1 : 2);
  TRY(ipk_launch<T>(h, 2, b.m, cur, t.thomas[2], last == 2 ? target : nullptr, sign, s));
  if (t.active[1])
    TRY(ipk_launch<T>(h, 1, b.m, cur, t.thomas[1], last == 1 ? target : nullptr, sign, s));
  if (t.active[0]) TRY(ipk_launch<T>(h, 0, b.m, cur, t.thomas[0], target, sign, s));
  return MGH_SUCCESS;
}

// What a quantizer makes: the integers (always dense), and the out-of-dictionary values.
struct QuantOut {
  uint64_t dict_size;
  int prep_huffman;
  int64_t *q;
  uint16_t *sym16;  // instead of q: 16-bit dictionary symbols (mgh_decompose_quantize_sym16)
  uint64_t *ocount, *oidx;
  int64_t *oval;
  uint64_t ocap;
};

// What the fused kernels quantize with: the output, and the table -- built on the host
// (LinearQuantization.hpp:495-545 + volumes :186-195) or left on the device by k_make_qparams.
template <typename T> struct QuantParams {
  QuantOut out{};
  std::vector<T> qz, vol;   // per level
  const T *d_qp = nullptr;  // device table [2 * (L + 1)] instead of qz / vol
};

template <typename T>
void host_quant_table(mgh_hierarchy *h, int ebtype, double tol, double s, double norm, QuantParams<T> &qp) {
  auto *hh = HH<T>(h);
  qp.qz.resize(h->L + 1);
  qp.vol.resize(h->L + 1);
  hh->quantizers(ebtype, (T)tol, (T)s, (T)norm, true, qp.qz.data());
  const bool calc_vol = !((T)s == std::numeric_limits<T>::infinity());
  for (int l = 0; l <= h->L; l++) qp.vol[l] = calc_vol ? hh->level_volume(l, false) : (T)1;
}

// The quantizer fields of the fused kernels' argument block.
template <typename T> void fused_quant_args(const mgh_hierarchy *h, const QuantParams<T> &qp, FusedArgs<T> &A) {
  A.q = qp.out.q;
  A.q16 = qp.out.sym16;
  A.dict_size = (int64_t)qp.out.dict_size;
  A.prep_huffman = qp.out.prep_huffman;
  A.outlier_count = (unsigned long long *)qp.out.ocount;
  A.outlier_idx = qp.out.oidx;
  A.outlier_val = qp.out.oval;
  A.outlier_cap = qp.out.ocap;
  A.qp = qp.d_qp;
  A.nlev = h->L + 1;
}

// ---- the fused level passes: plan (fused_plan.hpp), residency, launch -----------------------
inline bool fused_tall_tiles(const mgh_hierarchy *h, const Box3 &b) { return fused_tall_tiles(h->fused, b.m); }

// The instance of k_level_fused2 a launch runs, as one number (RCH is 16 everywhere).
constexpr int fused_instance_key(int out, int tc, int faces, int tmode, int agg) {
  return (((out * 3 + (tc == 8 ? kShape8x32 : tc == 4 ? kShape4x64 : kShape64x4)) * 2 + faces) * 3 + tmode) * 2 + agg;
}

// Workgroups per CU of one instance, asked of the runtime (256 threads, no dynamic LDS: the tile
// lives in static LDS). Once per process, device and instance.
template <typename T, int OUTK, int TC, int TF, bool FACES, int TMODE, bool AGG>
int fused_residency_query(mgh_hierarchy *h) {
  static std::mutex mu;
  static std::map<int, int> per_device;
  std::lock_guard<std::mutex> lock(mu);
  auto it = per_device.find(h->device);
  if (it == per_device.end()) {
    int n = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &n, k_level_fused2<T, OUTK, TC, TF, kFusedMaxMarch, FACES, TMODE, AGG>, 256, 0));
    if (n <= 0) return fail(MGH_ERR_DEVICE, "k_level_fused2: the runtime reports no resident workgroup");
    it = per_device.emplace(h->device, n).first;
  }
  h->fused_wg_per_cu[fused_instance_key(OUTK, TC, FACES, TMODE, AGG)] = it->second;
  return MGH_SUCCESS;
}
template <typename T, int OUTK, int TMODE, bool AGG> int fused_residency_shapes(mgh_hierarchy *h) {
  TRY((fused_residency_query<T, OUTK, 8, 32, false, TMODE, AGG>(h)));
  TRY((fused_residency_query<T, OUTK, 8, 32, true, TMODE, AGG>(h)));
  TRY((fused_residency_query<T, OUTK, 4, 64, false, TMODE, AGG>(h)));
  TRY((fused_residency_query<T, OUTK, 4, 64, true, TMODE, AGG>(h)));
  TRY((fused_residency_query<T, OUTK, 64, 4, false, TMODE, AGG>(h)));
  TRY((fused_residency_query<T, OUTK, 64, 4, true, TMODE, AGG>(h)));
  return MGH_SUCCESS;
}
// Every instance decompose_fused (D <= 3) / decompose_fused4 (D = 4) can launch on this hierarchy.
template <typename T> int fused_residency_init(mgh_hierarchy *h) {
  if (h->D == 4) {
    TRY((fused_residency_shapes<T, OUT_T, 1, false>(h)));
    TRY((fused_residency_shapes<T, OUT_T, 2, false>(h)));
    TRY((fused_residency_shapes<T, OUT_Q, 1, false>(h)));
    TRY((fused_residency_shapes<T, OUT_Q, 2, false>(h)));
    TRY((fused_residency_shapes<T, OUT_Q, 1, true>(h)));
    TRY((fused_residency_shapes<T, OUT_Q, 2, true>(h)));
  } else if (h->D <= 3) {
    TRY((fused_residency_shapes<T, OUT_T, 0, false>(h)));
    TRY((fused_residency_shapes<T, OUT_Q, 0, false>(h)));
    TRY((fused_residency_shapes<T, OUT_QH, 0, false>(h)));
    TRY((fused_residency_shapes<T, OUT_Q, 0, true>(h)));
    TRY((fused_residency_shapes<T, OUT_QH, 0, true>(h)));
  }
  return MGH_SUCCESS;
}
// Workgroups the device holds at once of an instance (0: the hierarchy did not ask for it).
inline long long fused_slots(const mgh_hierarchy *h, int key) {
  auto it = h->fused_wg_per_cu.find(key);
  return it == h->fused_wg_per_cu.end() ? 0 : (long long)it->second * (long long)h->num_cu;
}

inline Fused2Grid fused_grid_of(const FusedPlan &p) {
  Fused2Grid G{};
  G.gxm = p.gxm; G.n_main = p.n_main;
  G.ff_F0 = p.ff_F0; G.n_ff = p.n_ff;
  G.cf_C0 = p.cf_C0; G.n_cf = p.n_cf;
  G.rch = p.rch; G.nchunk = p.nchunk;
  G.chunk_hi = p.nchunk;
  G.xcd_ranges = p.xcd_ranges;
  return G;
}
inline void fused_log_plan(mgh_hierarchy *h, const FusedPlan &p, int elem, const Box3 &b, const size_t nz[2]) {
  if (!h->profiling || h->fused_log.size() >= kIpkLogCap) return;
  std::array<long long, MGH_FUSED_PLAN_FIELDS> r;
  static_assert(MGH_FUSED_PLAN_FIELDS == kFusedPlanFields, "mgard_hip.h and fused_plan.hpp agree on the record");
  fused_plan_record(p, elem, b.m, nz, r.data());
  h->fused_log.push_back(r);
}

// Level loop on the fused kernels (3 active dims): per level one fused
// coefficient/quantize/load-vector pass, three Thomas solves (the last one adds
// the correction into the coarse nodal array), then the head.
// `after_first` (the quantizer set-up) is issued right in front of the first launch that needs it.
// One level on the second-generation fused kernel (kernels_fused2.hpp), as fused_plan.hpp plans it
// (`p`: its tiles; the march is chosen here, against the residency of the instance that runs).
template <typename T, int OUTK, int TC, int TF, bool AGG = false>
int launch_fused2_t(mgh_hierarchy *h, const FusedArgs<T> &A, const Box3 &b, FusedPlan p, const char *nm,
                    hipStream_t s) {
  const size_t nz[2] = {1, 0};
  const long long slots[2] = {fused_slots(h, fused_instance_key(OUTK, TC, p.faces, 0, AGG)), 0};
  fused_plan_march(p, h->fused, (int)b.m[0], 1, nz, slots);
  fused_log_plan(h, p, (int)sizeof(T), b, nz);
  const Fused2Grid G = fused_grid_of(p);
  const dim3 grid(p.grid_x, (unsigned)G.nchunk, 1);
  if (p.faces)
    return launch_kernel(h, nm, s, k_level_fused2<T, OUTK, TC, TF, kFusedMaxMarch, true, 0, AGG>, grid, dim3(256), 0,
                         A, G, Fused4<T>{});
  return launch_kernel(h, nm, s, k_level_fused2<T, OUTK, TC, TF, kFusedMaxMarch, false, 0, AGG>, grid, dim3(256), 0,
                       A, G, Fused4<T>{});
}

template <typename T, int OUTK, bool AGG = false>
int launch_fused2(mgh_hierarchy *h, const FusedArgs<T> &A, const Box3 &b, const FusedPlan &p, const char *nm,
                  hipStream_t s) {
  if (p.shape == kShape64x4) return launch_fused2_t<T, OUTK, 64, 4, AGG>(h, A, b, p, nm, s);
  if (p.shape == kShape4x64) return launch_fused2_t<T, OUTK, 4, 64, AGG>(h, A, b, p, nm, s);
  return launch_fused2_t<T, OUTK, 8, 32, AGG>(h, A, b, p, nm, s);
}

// Which variant of the level kernel: the one that asks for outlier slots per wave and plane
// (right when few values leave the dictionary) or per workgroup and pair step (OutlierShared in
// kernels_fused2.hpp: more registers and LDS traffic, but the requests no longer queue on the one
// counter when many do). The last kernel of every call leaves the call's outlier count in host
// memory; what is found there now -- from the previous call or an earlier one, no synchronisation
// -- decides.
template <typename T> bool outlier_agg_now(mgh_hierarchy *h, const QuantParams<T> *qp) {
  auto *ds = DS<T>(h);
  if (!qp || !qp->out.prep_huffman || !qp->out.ocount) return false;
  if (!ds->outliers_seen && h->outlier_agg == 2) {
    if (hipHostMalloc(&ds->outliers_seen, sizeof(unsigned long long), hipHostMallocDefault) == hipSuccess)
      *ds->outliers_seen = 0;
    else
      ds->outliers_seen = nullptr, (void)hipGetLastError();
  }
  const unsigned long long seen =
      ds->outliers_seen ? *reinterpret_cast<volatile unsigned long long *>(ds->outliers_seen) : 0;
  // (more than 0.5 % of the values AND enough of them for the requests to queue: on a 65^3 block,
  // where most outliers come from the small levels' own kernels, the stash only costs -- 64 blocks
  // of 65^3: 15.3 vs 16.9 ms per mgh_compress)
  return h->outlier_agg == 1 ||
         (h->outlier_agg == 2 && seen * 200 > (unsigned long long)h->total && seen > 200000);
}

__global__ void k_publish_count(const unsigned long long *count, unsigned long long *seen) { *seen = *count; }

// The fused kernels index inside an r-plane with 32-bit offsets (and the emit pass with 32-bit
// byte offsets): planes of 2^29 elements or more go through the one-thread-per-element kernels.
inline bool fused_ok(const mgh_hierarchy *h) {
  return h->D == 3 && h->L >= 1 && h->plane_elems < ((uint64_t)1 << 29);
}
// compression side: also D = 4 (decompose_fused4); arrays of < 2^32 elements per t-slice
inline bool fused4_ok(const mgh_hierarchy *h) {
  return h->D == 4 && h->fused4 && !h->force_nd && h->L >= 1 && h->plane_elems < ((uint64_t)1 << 29);
}
inline bool fusedc_ok(const mgh_hierarchy *h) { return fused_ok(h) || fused4_ok(h); }
// ... and not switched off: the route of the fused level loops
inline bool fused_route(const mgh_hierarchy *h) { return fusedc_ok(h) && !h->force_v1; }

// ---- layouts of T arrays (mgh_set_ld; mgard_x::Array::ld, Array.hpp:70-84: hipMallocPitch pads the
// fastest dimension; SubArray.hpp:136-139 carries one ld per dimension) ------------------------
// Rows of the array (all dimensions but the fastest, right-aligned, leading 1s) and the element
// strides of those dimensions.
// (struct LdView: ld_view.hpp)
// How a T array of the full shape lies in memory. A layout belongs to an ARGUMENT: it is made where
// the caller's pointer enters the library (caller_layout, in the extern "C" entry points) and passed
// down beside the pointer; the buffers of the hierarchy are dense (dense_layout). A function without
// a layout parameter takes dense arrays; one with it says which layouts it takes in place, and
// ld_pack / LdOut make a dense copy for the rest.
struct Layout {
  LdView view{};         // for the row-wise kernels (k_ld_copy, k_norm_ld) and level_box_of
  size_t I = 0, J = 0;   // strides of the two slower dimensions of the 3-D view (fused kernels)
  bool pitched = false;  // false: dense
  // pitched, and the fused 3-D kernels can read / write it in place: D = 3 on the fused path, planes
  // addressable in 32 bits like the dense ones
  bool native3 = false;
};
// ext[d]: elements between two steps of dimension d - 1 (the extent, or a leading dimension)
inline Layout make_layout(const mgh_hierarchy *h, const uint64_t *ext, bool pitched) {
  Layout lay;
  const int D = h->D;
  uint64_t st = 1, str[MGH_MAX_DIM] = {};
  for (int d = D - 1; d >= 0; d--) {
    str[d] = st;
    st *= ext[d];
  }
  lay.view.rows = 1;
  for (int k = 0; k < MGH_MAX_DIM; k++) {
    const int d = k - (MGH_MAX_DIM - D);
    lay.view.ext[k] = d >= 0 ? (uint32_t)h->shape[d] : 1u;
    lay.view.stride[k] = d >= 0 ? str[d] : 0;
    if (k < MGH_MAX_DIM - 1) lay.view.rows *= lay.view.ext[k];
  }
  lay.J = (size_t)ext[D - 1];
  lay.I = (size_t)((D >= 2 ? ext[D - 2] : 1) * ext[D - 1]);
  lay.pitched = pitched;
  lay.native3 = pitched && fused_ok(h) && !h->force_v1 && lay.I < ((size_t)1 << 30);
  return lay;
}
inline Layout dense_layout(const mgh_hierarchy *h) { return make_layout(h, h->shape, false); }
// The layout mgh_set_ld gave the T arrays an entry point reads (MGH_LD_IN) or writes (MGH_LD_OUT).
inline Layout caller_layout(const mgh_hierarchy *h, int which) {
  return h->has_ld[which] ? make_layout(h, h->ld[which], true) : dense_layout(h);
}

template <typename T, int OUT, typename AfterFirst>
int decompose_fused4(mgh_hierarchy *h, const T *data, T *coeff, const QuantParams<T> *qp,
                     hipStream_t s, AfterFirst &&after_first);

// in: dense, or a pitched array the kernels of the finest level read in place (Layout::native3)
template <typename T, int OUT, typename AfterFirst>
int decompose_fused(mgh_hierarchy *h, const T *data, const Layout &in, T *coeff, const QuantParams<T> *qp,
                    hipStream_t s, AfterFirst &&after_first) {
  if (h->D == 4) return decompose_fused4<T, OUT>(h, data, coeff, qp, s, after_first);
  auto *ds = DS<T>(h);
  const int L = h->L;
  const size_t fI = ds->full_I, fJ = ds->full_J;
  const T *src = data;
  size_t sI = in.I, sJ = in.J;

  FusedArgs<T> A{};
  A.coef = coeff;
  A.dI = fI;
  A.dJ = fJ;
  if (OUT == OUT_Q) fused_quant_args(h, *qp, A);
  const bool agg = OUT == OUT_Q && outlier_agg_now<T>(h, qp);
  // levels whose working set fits in one workgroup's LDS run inside the tail kernel
  constexpr size_t kTailLdsMax = 150 * 1024;
  int l_tail = 0;  // levels l_tail .. 1 go to the tail (0 = none)
  for (int l = std::min(L, kTailMaxLevels); l >= 1; l--) {
    // (the table block of the tail's levels, plus the level above whose solves it may run)
    const size_t tab = ds->lt_end[std::min(l + 1, L)];
    if ((tail_lds_elems(ds->lt[l].box) + tab) * sizeof(T) + tail_header_bytes<T>() <= kTailLdsMax) {
      l_tail = l;
      break;
    }
  }
  bool tail_pre = false;  // the tail kernel also runs the solves of level l_tail + 1
  for (int l = L; l > l_tail; l--) {
    const LevelTables<T> &t = ds->lt[l];
    const Box3 &b = t.box;
    for (int k = 0; k < 3; k++) {
      A.n[k] = (int)b.n[k];
      A.m[k] = (int)b.m[k];
      A.ratio[k] = t.ratio[k];
      A.mass[k] = t.mass[k];
    }
    A.u = src;
    A.uI = sI;
    A.uJ = sJ;
    A.coarse = ds->nodal[l - 1];
    A.load = ds->t3;
    A.level = l;
    if (OUT == OUT_Q && !qp->d_qp) {
      A.quantizer = qp->qz[l];
      A.volume = qp->vol[l];
    }
    const FusedPlan plan = fused_plan_tiles(h->fused, b.m);
    const int cls = plan.cls;
    if (l == L) TRY(after_first());
    // (the level kernels test the dictionary range in 32 bits: the entry points send larger
    // dictionaries through decompose + quantize)
    if (OUT == OUT_Q && qp->out.dict_size > ((uint64_t)1 << 30))
      return fail(MGH_ERR_INVALID_ARGUMENT, "fused path: dict_size must be at most 2^30");
    if (cls < h->fused.box) {
      // small level: no march (kernels_box.hpp)
      constexpr int BR = 4, BC = 4, BF = 8;
      const int bx = ((int)b.m[2] + BF - 1) / BF, by = ((int)b.m[1] + BC - 1) / BC,
                bz = ((int)b.m[0] + BR - 1) / BR;
      TRY(launch(h, OUT == OUT_Q ? "level_box_q" : "level_box", s, [&] {
        k_level_box<T, OUT, BR, BC, BF><<<(unsigned)(bx * by * bz), 256, 0, s>>>(A, bx, by);
      }));
    } else {
      // long marches (RCH = 16: 9% r-halo) when there are plenty of tiles, short ones
      // (RCH = 4) on the small levels where the march length is pure latency
      const char *nm = cls == 2 ? (OUT == OUT_Q ? "level_fused_q" : "level_fused")
                                : (OUT == OUT_Q ? "level_fused_q_small" : "level_fused_small");
      if (OUT == OUT_Q && agg) {  // (many outliers last time: slot requests per workgroup)
        if (A.prep_huffman && !A.q16 && h->fused_fixed)
          TRY((launch_fused2<T, OUT == OUT_Q ? OUT_QH : OUT, OUT == OUT_Q>(h, A, b, plan, nm, s)));
        else
          TRY((launch_fused2<T, OUT, OUT == OUT_Q>(h, A, b, plan, nm, s)));
      } else if (OUT == OUT_Q && A.prep_huffman && !A.q16 && h->fused_fixed)
        TRY((launch_fused2<T, OUT == OUT_Q ? OUT_QH : OUT>(h, A, b, plan, nm, s)));
      else
        TRY((launch_fused2<T, OUT>(h, A, b, plan, nm, s)));
    }
    // (the level right above the tail leaves its three solves to the tail kernel, which needs the
    // box in LDS anyway)
    tail_pre = h->tail_solves && l == l_tail + 1 && l_tail >= 1;
    if (!tail_pre) {
      // A load vector that does not fit the 256 MB memory-side cache (1024^3: 540 MB) is solved
      // in ranges of r-planes, f then c per range (both are independent per plane): the c-solve
      // finds what the f-solve just wrote in the cache instead of in HBM. MGH_IPK_RANGE_MB = size of
      // a range (0 = never).
      const size_t box_b = (size_t)b.m[0] * b.m[1] * b.m[2] * sizeof(T);
      const size_t range_b = (size_t)h->ipk_range_mb << 20;
      if (range_b && box_b > 2 * range_b) {
        const uint32_t nrange = (uint32_t)((box_b + range_b - 1) / range_b);
        for (uint32_t k = 0; k < nrange; k++) {
          const uint32_t R_lo = (uint32_t)((uint64_t)b.m[0] * k / nrange), R_hi = (uint32_t)((uint64_t)b.m[0] * (k + 1) / nrange);
          if (R_hi == R_lo) continue;  // (fewer planes than ranges: 3 x 16385 x 16385)
          const uint32_t ms[3] = {R_hi - R_lo, b.m[1], b.m[2]};
          TRY(ipk_fc_launch<T>(h, ms, ds->t3 + (size_t)R_lo * b.m[1] * b.m[2], t.thomas[2], t.thomas[1], s));
        }
      } else {
        TRY(ipk_fc_launch<T>(h, b.m, ds->t3, t.thomas[2], t.thomas[1], s));
      }
      TRY(ipk_launch<T>(h, 0, b.m, ds->t3, t.thomas[0], ds->nodal[l - 1], +1, s));
    }
    src = ds->nodal[l - 1];
    sJ = b.m[2];
    sI = (size_t)b.m[1] * b.m[2];
  }
  if (L <= l_tail) TRY(after_first());
  if (l_tail >= 1) {
    TailArgs<T> TA{};
    TA.nlevels = l_tail;
    TA.fine = src;
    TA.fI = sI;
    TA.fJ = sJ;
    if (tail_pre) {
      TA.pre_load = ds->t3;
      for (int k = 0; k < 3; k++) TA.pre_thomas[k] = ds->lt[l_tail + 1].thomas[k];
    }
    for (int l = l_tail; l >= 1; l--) {
      TailLevel<T> &tl = TA.lv[l_tail - l];
      const LevelTables<T> &t = ds->lt[l];
      tl.b = t.box;
      for (int k = 0; k < 3; k++) {
        tl.ratio[k] = t.ratio[k];
        tl.mass[k] = t.mass[k];
        tl.thomas[k] = t.thomas[k];
      }
      tl.level = l;
      if (OUT == OUT_Q && !qp->d_qp) {
        tl.quantizer = qp->qz[l];
        tl.volume = qp->vol[l];
      }
    }
    if (OUT == OUT_Q && !qp->d_qp) {
      TA.head_quantizer = qp->qz[0];
      TA.head_volume = qp->vol[0];
    }
    TA.out = A;
    TA.outliers_seen = OUT == OUT_Q && A.prep_huffman ? ds->outliers_seen : nullptr;
    const size_t tab = ds->lt_end[tail_pre ? l_tail + 1 : l_tail];
    TA.tab_base = ds->tables;
    TA.tab_count = (uint32_t)tab;
    const size_t lds = (tail_lds_elems(ds->lt[l_tail].box) + tab) * sizeof(T) + tail_header_bytes<T>();
    static std::atomic<uint64_t> once{0};
    TRY(allow_big_lds_once(k_tail<T, OUT>, once));
    TRY(launch(h, "tail", s, [&] { k_tail<T, OUT><<<1, 1024, lds, s>>>(TA); }));
  } else {
    const Box3 &b = ds->lt[1].box;
    if (OUT == OUT_Q && !qp->d_qp) {
      A.quantizer = qp->qz[0];
      A.volume = qp->vol[0];
    }
    TRY(launch(h, "head_out", s, [&] {
      // (a hierarchy with one long and two short dimensions has few levels and a long head)
      const size_t tot = (size_t)b.m[0] * b.m[1] * b.m[2];
      k_head_out<T, OUT><<<(unsigned)std::min<size_t>((tot + 255) / 256, 1024), 256, 0, s>>>(
          (int)b.m[0], (int)b.m[1], (int)b.m[2], ds->nodal[0], A);
    }));
    if (OUT == OUT_Q && A.prep_huffman && A.outlier_count && ds->outliers_seen)
      k_publish_count<<<1, 1, 0, s>>>(A.outlier_count, ds->outliers_seen);
  }
  return MGH_SUCCESS;
}

// D = 4 on the 3-D tile code (kernels_fused2.hpp: TMODE 1 / 2, k_tsweep): per level the even
// slices of the slowest dimension t run the 3-D pass of the slice, the odd slices the TODD
// variant that interpolates across t as well; the fourth mass/restriction sweep and the four
// Thomas solves (f, c, r, t; the last one adds the correction into the coarse array) follow on
// the N/16-sized arrays. Order of every operation as in CalcCoefficientsND.hpp:25-236 and
// CalcCorrectionND.hpp:25-267 (dims D-1 .. 0): bit-identical to the generic N-D kernels.
// D = 4: the even and the odd slices of one level (kernels_fused2.hpp, TMODE 1 / 2)
template <typename T, int OUT, int TC, int TF, bool AGG = false>
int launch_fused4_t(mgh_hierarchy *h, const FusedArgs<T> &A, const Fused4<T> &Q, const Box3 &b, FusedPlan p,
                    int n_t, int m_t, hipStream_t s) {
    const size_t nz[2] = {(size_t)m_t, (size_t)(n_t - m_t)};  // even, odd slices
    const long long slots[2] = {fused_slots(h, fused_instance_key(OUT, TC, p.faces, 1, AGG)),
                                fused_slots(h, fused_instance_key(OUT, TC, p.faces, 2, AGG))};
    fused_plan_march(p, h->fused, (int)b.m[0], 2, nz, slots);
    fused_log_plan(h, p, (int)sizeof(T), b, nz);
    const Fused2Grid G = fused_grid_of(p);
    const unsigned gx = p.grid_x;
    const bool faces = p.faces;
    const unsigned n_even = (unsigned)nz[0], n_odd = (unsigned)nz[1];
#define MGH_F4(RCH, TMODE, NZ, NAME)                                                          \
  if ((NZ) > 0) {                                                                             \
    const dim3 grid(gx, (unsigned)G.nchunk, (NZ));                                            \
    if (faces)                                                                                \
      TRY(launch_kernel(h, NAME, s, k_level_fused2<T, OUT, TC, TF, RCH, true, TMODE, AGG>, grid, dim3(256), 0, A, G, Q));  \
    else                                                                                      \
      TRY(launch_kernel(h, NAME, s, k_level_fused2<T, OUT, TC, TF, RCH, false, TMODE, AGG>, grid, dim3(256), 0, A, G, Q)); \
  }
    MGH_F4(kFusedMaxMarch, 1, n_even, "level4_even")
    MGH_F4(kFusedMaxMarch, 2, n_odd, "level4_odd")
#undef MGH_F4
    return MGH_SUCCESS;
}

// D = 4: the mass/restriction sweep along t of the per-slice load vectors: every input slice read
// once where the pencils are short enough for registers (k_tsweep_once), else slice by slice.
template <typename T>
int tsweep_launch(mgh_hierarchy *h, const T *load, T *corr, size_t M, int m_t, const T *mass, hipStream_t s) {
  constexpr int MT = 9;
  if (m_t <= MT) {
    const unsigned blocks = (unsigned)std::min<size_t>((M + 255) / 256, (size_t)h->num_cu * 32);
    return launch(h, "tsweep", s, [&] { k_tsweep_once<T, MT><<<blocks, 256, 0, s>>>(load, corr, M, m_t, mass); });
  }
  const dim3 grid((unsigned)std::min<size_t>((M + 255) / 256, 4096), (unsigned)m_t, 1);
  return launch(h, "tsweep", s, [&] { k_tsweep<T><<<grid, 256, 0, s>>>(load, corr, M, m_t, mass); });
}

// D = 4: Thomas solve along t of the correction (m_t, M) with the result added to / subtracted
// from the coarse array: short pencils go through registers (k_tsolve_apply), others through the
// generic strided solve.
template <typename T>
int tsolve_apply(mgh_hierarchy *h, T *corr, T *coarse, size_t M, int m_t, size_t m_rc, size_t m_f,
                 const T *tt, int sign, hipStream_t s) {
  constexpr int MT = 9;
  if (m_t <= MT) {
    const unsigned blocks = (unsigned)std::min<size_t>((M + 255) / 256, (size_t)h->num_cu * 32);
    return launch(h, "ipk_t", s, [&] {
      k_tsolve_apply<T, MT><<<blocks, 256, 0, s>>>(corr, coarse, M, m_t, tt, sign);
    });
  }
  const uint32_t m3t[3] = {(uint32_t)m_t, (uint32_t)m_rc, (uint32_t)m_f};
  return ipk_launch<T>(h, 0, m3t, corr, tt, coarse, sign, s);
}

// D = 4 work arrays: compact nodal arrays of the levels below the top, per-slice load vectors
// (padded positions of t) and the correction of the biggest coarse box
template <typename T> int ensure_state4(mgh_hierarchy *h) {
  auto *ds = DS<T>(h);
  auto *hh = HH<T>(h);
  const int L = h->L;
  const auto &sh = hh->level_shape;
  if (ds->state4_ready) return MGH_SUCCESS;
  // a failed attempt (out of memory on a big slab) leaves nothing behind -- neither memory nor its
  // share of mgh_device_bytes(): the next call starts over
  const size_t M = (size_t)sh[L - 1][1] * sh[L - 1][2] * sh[L - 1][3];
  auto nodal_count = [&](int l) { return (size_t)sh[l][0] * sh[l][1] * sh[l][2] * sh[l][3]; };
  const size_t load_count = (2 * (size_t)sh[L - 1][0] - 1) * M, corr_count = (size_t)sh[L - 1][0] * M;
  auto drop = [&] {
    for (size_t l = 0; l < ds->nodal4.size(); l++) dev_free(h, &ds->nodal4[l], nodal_count((int)l));
    ds->nodal4.clear();
    dev_free(h, &ds->load4, load_count);
    dev_free(h, &ds->corr4, corr_count);
  };
  drop();
  ds->nodal4.assign(L + 1, nullptr);
  int rc = MGH_SUCCESS;
  for (int l = 0; l < L && rc == MGH_SUCCESS; l++) rc = dev_alloc(h, &ds->nodal4[l], nodal_count(l));
  if (rc == MGH_SUCCESS) rc = dev_alloc(h, &ds->load4, load_count);
  if (rc == MGH_SUCCESS) rc = dev_alloc(h, &ds->corr4, corr_count);
  if (rc != MGH_SUCCESS) {
    drop();
    return rc;
  }
  ds->state4_ready = true;
  return MGH_SUCCESS;
}

template <typename T, int OUT, typename AfterFirst>
int decompose_fused4(mgh_hierarchy *h, const T *data, T *coeff, const QuantParams<T> *qp,
                     hipStream_t s, AfterFirst &&after_first) {
  auto *ds = DS<T>(h);
  auto *hh = HH<T>(h);
  const int L = h->L;
  const auto &sh = hh->level_shape;  // [l][d]
  const size_t full[4] = {(size_t)sh[L][1] * sh[L][2] * sh[L][3], (size_t)sh[L][2] * sh[L][3],
                          (size_t)sh[L][3], 1};
  TRY(ensure_state4<T>(h));
  FusedArgs<T> A{};
  A.coef = coeff;
  A.dI = full[1];
  A.dJ = full[2];
  if (OUT == OUT_Q) fused_quant_args(h, *qp, A);
  TRY(after_first());
  const bool agg = OUT == OUT_Q && outlier_agg_now<T>(h, qp);
  const T *src = data;
  size_t sT = full[0], sI = full[1], sJ = full[2];
  for (int l = L; l >= 1; l--) {
    const auto &N = sh[l], &Mc = sh[l - 1];
    Box3 b;
    for (int k = 0; k < 3; k++) {
      b.n[k] = (uint32_t)N[1 + k];
      b.m[k] = (uint32_t)Mc[1 + k];
      A.n[k] = (int)N[1 + k];
      A.m[k] = (int)Mc[1 + k];
      A.ratio[k] = ds->nd[l].ratio[1 + k];
      A.mass[k] = ds->nd[l].mass[1 + k];
    }
    const size_t M = (size_t)Mc[1] * Mc[2] * Mc[3];
    const int n_t = (int)N[0], m_t = (int)Mc[0];
    A.u = src;
    A.uI = sI;
    A.uJ = sJ;
    A.coarse = ds->nodal4[l - 1];
    A.load = ds->load4;
    A.level = l;
    if (OUT == OUT_Q && !qp->d_qp) {
      A.quantizer = qp->qz[l];
      A.volume = qp->vol[l];
    }
    Fused4<T> Q{};
    Q.ratio_t = ds->nd[l].ratio[0];
    Q.uT = sT;
    Q.dT = full[0];
    Q.cT = M;
    Q.n_t = n_t;
    Q.m_t = m_t;
    // an even n_t has a ghost slice (padded position n_t - 1): its load vector is zero
    if (n_t % 2 == 0)
      HIP_TRY(hipMemsetAsync(ds->load4 + (size_t)(n_t - 1) * M, 0, M * sizeof(T), s));
    const FusedPlan plan = fused_plan_tiles(h->fused, b.m, (size_t)std::max(1, n_t - m_t));
    const bool wide = plan.shape == kShape4x64, tall = plan.shape == kShape64x4;
    if (OUT == OUT_Q && agg) {
      if (tall) TRY((launch_fused4_t<T, OUT, 64, 4, OUT == OUT_Q>(h, A, Q, b, plan, n_t, m_t, s)));
      else if (wide) TRY((launch_fused4_t<T, OUT, 4, 64, OUT == OUT_Q>(h, A, Q, b, plan, n_t, m_t, s)));
      else TRY((launch_fused4_t<T, OUT, 8, 32, OUT == OUT_Q>(h, A, Q, b, plan, n_t, m_t, s)));
    } else if (tall)
      TRY((launch_fused4_t<T, OUT, 64, 4>(h, A, Q, b, plan, n_t, m_t, s)));
    else if (wide)
      TRY((launch_fused4_t<T, OUT, 4, 64>(h, A, Q, b, plan, n_t, m_t, s)));
    else
      TRY((launch_fused4_t<T, OUT, 8, 32>(h, A, Q, b, plan, n_t, m_t, s)));
    // t-sweep, then the Thomas solves f, c, r, t on the coarse box (m_t, m_r, m_c, m_f)
    {
      TRY((tsweep_launch<T>(h, ds->load4, ds->corr4, M, m_t, ds->nd[l].mass[0], s)));
    }
    const uint32_t m3a[3] = {(uint32_t)(m_t * Mc[1]), (uint32_t)Mc[2], (uint32_t)Mc[3]};
    TRY(ipk_launch<T>(h, 2, m3a, ds->corr4, ds->nd[l].thomas[3], nullptr, +1, s));
    TRY(ipk_launch<T>(h, 1, m3a, ds->corr4, ds->nd[l].thomas[2], nullptr, +1, s));
    TRY(ipk_launch<T>(h, 0, b.m, ds->corr4, ds->nd[l].thomas[1], nullptr, +1, s, (uint32_t)m_t, M));
    TRY((tsolve_apply<T>(h, ds->corr4, ds->nodal4[l - 1], M, m_t, Mc[1] * Mc[2], Mc[3], ds->nd[l].thomas[0], +1, s)));
    src = ds->nodal4[l - 1];
    sT = M;
    sI = (size_t)Mc[2] * Mc[3];
    sJ = Mc[3];
  }
  // head: the level-0 nodal values
  {
    if (OUT == OUT_Q && !qp->d_qp) {
      A.quantizer = qp->qz[0];
      A.volume = qp->vol[0];
    }
    const auto &M0 = sh[0];
    const size_t tot = (size_t)M0[0] * M0[1] * M0[2] * M0[3];
    TRY(launch(h, "head_out", s, [&] {
      k_head_out4<T, OUT><<<(unsigned)std::min<size_t>((tot + 1023) / 1024, 1024), 1024, 0, s>>>(
          (int)M0[0], (int)M0[1], (int)M0[2], (int)M0[3], ds->nodal4[0], A, full[0]);
    }));
    if (OUT == OUT_Q && A.prep_huffman && A.outlier_count && ds->outliers_seen)
      k_publish_count<<<1, 1, 0, s>>>(A.outlier_count, ds->outliers_seen);
  }
  return MGH_SUCCESS;
}

template <typename T, int OUT>
int decompose_fused(mgh_hierarchy *h, const T *data, const Layout &in, T *coeff, const QuantParams<T> *qp,
                    hipStream_t s) {
  return decompose_fused<T, OUT>(h, data, in, coeff, qp, s, [] { return (int)MGH_SUCCESS; });
}

// ---- N-D path (D = 4, 5): in place on `v` (full array, reordered as levels proceed) -------
// (count: elements of the array the level loop runs on -- the full one, or the dense box of a stop level)
template <typename T> int nd_ensure(mgh_hierarchy *h, size_t count = 0) {
  auto *ds = DS<T>(h);
  if (!count) count = (size_t)h->total;
  if (ds->nd_cap < count) {
    dev_free(h, &ds->nd_w, ds->nd_cap);
    dev_free(h, &ds->nd_a, ds->nd_cap);
    dev_free(h, &ds->nd_b, ds->nd_cap);
    ds->nd_cap = 0;
    int rc = dev_alloc(h, &ds->nd_w, count);
    if (rc == MGH_SUCCESS) rc = dev_alloc(h, &ds->nd_a, count);
    if (rc == MGH_SUCCESS) rc = dev_alloc(h, &ds->nd_b, count);
    if (rc != MGH_SUCCESS) {
      dev_free(h, &ds->nd_w, count);
      dev_free(h, &ds->nd_a, count);
      dev_free(h, &ds->nd_b, count);
      return rc;
    }
    ds->nd_cap = count;
  }
  return MGH_SUCCESS;
}

// (array_level: the array the box lies in is the dense array of that level's shape -- the compact
// corner box of a stop level; -1: the full array)
template <typename T> NdBox nd_box(mgh_hierarchy *h, int l, int array_level = -1) {
  auto *hh = HH<T>(h);
  NdBox b{};
  b.D = h->D;
  uint64_t sacc = 1;
  for (int d = h->D - 1; d >= 0; d--) {
    b.n[d] = (uint32_t)hh->level_shape[l][d];
    b.m[d] = (uint32_t)hh->level_shape[l - 1][d];
    b.fs[d] = sacc;
    sacc *= array_level < 0 ? hh->shape[d] : hh->level_shape[array_level][d];
  }
  return b;
}

inline unsigned nd_grid(uint64_t total) {
  return (unsigned)std::min<uint64_t>((total + 255) / 256, 256 * 16);
}

// correction of level l from the reordered coefficients in v; returns the compact result
// the row-wise kernels' view of a level (dimensions right-aligned to kNd)
inline NdRowBox nd_row_box(const NdBox &b) {
  NdRowBox r{};
  const int sh = kNd - b.D;
  for (int k = 0; k < kNd; k++) {
    r.n[k] = r.m[k] = 1;
    r.fs[k] = r.ns[k] = 0;
  }
  uint64_t sacc = 1;
  for (int d = b.D - 1; d >= 0; d--) {
    r.n[d + sh] = b.n[d];
    r.m[d + sh] = b.m[d];
    r.fs[d + sh] = b.fs[d];
    r.ns[d + sh] = sacc;
    sacc *= b.n[d];
  }
  r.rows = 1;
  for (int k = 0; k < kNd - 1; k++) r.rows *= r.n[k];
  return r;
}
inline unsigned nd_row_grid(uint64_t rows) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((rows + 4 * kNdRowsPerWave - 1) / (4 * kNdRowsPerWave), 1u << 20));
}
// the coefficient kernel's view of a level; false: an offset does not fit 32 bits (k_nd_coeff then)
inline bool nd_coeff_box(const NdBox &b, uint64_t nn, NdCoeffBox *out) {
  const NdRowBox rb = nd_row_box(b);
  uint64_t span = 0;
  for (int k = 0; k < kNd; k++) span += (uint64_t)(rb.n[k] - 1) * rb.fs[k];
  // rows of a group: eight where that still leaves every SIMD a wave (8 x 8 x 64^3: 13.5 us on the
  // second level with eight, 16.9 us with two), fewer on the small levels (7.7 -> 4.5 us on the third)
  const uint64_t lines = (uint64_t)rb.n[0] * rb.n[1] * rb.n[2];
  uint32_t gsz = kNdRowsPerWave;
  while (gsz > 2 && lines * ((rb.n[3] + gsz - 1) / gsz) < 4 * 1024) gsz /= 2;
  const uint64_t gpl = (rb.n[3] + gsz - 1) / gsz;
  const uint64_t groups = lines * gpl;
  if (span >= ((uint64_t)1 << 31) || nn >= ((uint64_t)1 << 31) || groups >= ((uint64_t)1 << 31)) return false;
  NdCoeffBox c{};
  for (int k = 0; k < kNd; k++) {
    c.n[k] = rb.n[k];
    c.m[k] = rb.m[k];
    c.fs[k] = (uint32_t)rb.fs[k];
    c.ns[k] = (uint32_t)rb.ns[k];
  }
  c.gsz = gsz;
  c.gpl = (uint32_t)gpl;
  c.groups = (uint32_t)groups;
  *out = c;
  return true;
}
template <typename T>
int nd_coeff_launch(mgh_hierarchy *h, const NdBox &b, const NdTables<T> &tb, T *w, T *v, uint64_t nn, int mode,
                    hipStream_t st) {
  NdCoeffBox cb;
  if (h->nd_rows && b.fs[b.D - 1] == 1 && nd_coeff_box(b, nn, &cb)) {
    NdTables<T> ta{};
    for (int d = 0; d < b.D; d++) ta.ratio[d + kNd - b.D] = tb.ratio[d];
    const unsigned grid = (unsigned)std::max<uint32_t>(1, std::min<uint32_t>((cb.groups + 3) / 4, 1u << 20));
    return launch(h, "nd_coeff", st, [&] { k_nd_coeff_rows<T><<<grid, 256, 0, st>>>(cb, ta, w, v, mode); });
  }
  return launch(h, "nd_coeff", st, [&] { k_nd_coeff<T><<<nd_grid(nn), 256, 0, st>>>(b, tb, w, v, nn, mode); });
}

// the first sweep's view (along the fastest dimension, s.a = D - 1); false: too many rows for 32 bits
inline bool nd_fast_sweep(const NdSweep &s, NdFastSweep *out) {
  NdFastSweep f{};
  const int sh = kNd - s.D;
  for (int k = 0; k < kNd - 1; k++) {
    f.e[k] = 1;
    f.is[k] = 0;
    f.mc[k] = 1;
  }
  for (int d = 0; d < s.D - 1; d++) {
    f.e[d + sh] = s.e[d];
    f.is[d + sh] = s.is[d];
    f.mc[d + sh] = s.mc[d];
  }
  f.sf = s.is[s.D - 1];
  f.n = s.n;
  f.m = s.m;
  f.zero_all_coarse = s.zero_all_coarse;
  const uint64_t lines = (uint64_t)f.e[0] * f.e[1] * f.e[2];
  uint32_t gsz = kNdRowsPerWave;
  while (gsz > 2 && lines * ((f.e[3] + gsz - 1) / gsz) < 4 * 1024) gsz /= 2;  // (as nd_coeff_box)
  const uint64_t gpl = (f.e[3] + gsz - 1) / gsz;
  if (lines * gpl >= ((uint64_t)1 << 31)) return false;
  f.gsz = gsz;
  f.gpl = (uint32_t)gpl;
  f.groups = (uint32_t)(lines * gpl);
  *out = f;
  return true;
}

template <typename T>
int nd_correction(mgh_hierarchy *h, int l, const T *v, const NdBox &b, T **out, hipStream_t st) {
  auto *ds = DS<T>(h);
  const int D = h->D;
  NdSweep s{};
  s.D = D;
  for (int d = 0; d < D; d++) {
    s.e[d] = b.n[d];
    s.is[d] = b.fs[d];
    s.mc[d] = b.m[d];
  }
  const T *cur = v;
  T *bufs[2] = {ds->nd_a, ds->nd_b};
  int which = 0;
  for (int a = D - 1; a >= 0; a--) {
    s.a = a;
    s.n = b.n[a];
    s.m = b.m[a];
    s.zero_all_coarse = (a == D - 1) ? 1 : 0;
    uint64_t total = 1;
    for (int d = 0; d < D; d++) total *= (d == a ? s.m : s.e[d]);
    T *dst = bufs[which];
    NdFastSweep fs;
    uint64_t outer = 1, inner = 1;
    for (int d = 0; d < a; d++) outer *= s.e[d];
    for (int d = a + 1; d < D; d++) inner *= s.e[d];
    const uint64_t plane = (uint64_t)s.m * inner, tiles = (plane + 1023) / 1024;
    if (h->nd_rows && a < D - 1 && (uint64_t)s.n * inner < ((uint64_t)1 << 31) && outer * tiles < ((uint64_t)1 << 31)) {
      // (the compact result of the sweep before: a 3-D view is all there is to it)
      const NdMidSweep ms{(uint32_t)outer, s.n, s.m, (uint32_t)inner, (uint32_t)plane, (uint32_t)tiles};
      const unsigned grid = (unsigned)std::min<uint64_t>(outer * tiles, 1u << 20);
      TRY(launch(h, "nd_lpk", st, [&] { k_nd_lpk_mid<T><<<grid, 256, 0, st>>>(ms, cur, dst, ds->nd[l].mass[a]); }));
    } else if (h->nd_rows && a == D - 1 && nd_fast_sweep(s, &fs)) {
      const unsigned grid = (unsigned)std::max<uint32_t>(1, std::min<uint32_t>((fs.groups + 3) / 4, 1u << 20));
      TRY(launch(h, "nd_lpk", st, [&] { k_nd_lpk_fast<T><<<grid, 256, 0, st>>>(fs, cur, dst, ds->nd[l].mass[a]); }));
    } else if (h->nd_rows) {
      NdRowSweep rs{};
      const int sh = kNd - D;
      for (int k = 0; k < kNd; k++) {
        rs.eo[k] = 1;
        rs.is[k] = 0;
        rs.mc[k] = 1;
      }
      for (int d = 0; d < D; d++) {
        rs.eo[d + sh] = d == a ? s.m : s.e[d];
        rs.is[d + sh] = s.is[d];
        rs.mc[d + sh] = s.mc[d];
      }
      rs.a = a + sh;
      rs.n = s.n;
      rs.m = s.m;
      rs.zero_all_coarse = s.zero_all_coarse;
      rs.rows = 1;
      for (int k = 0; k < kNd - 1; k++) rs.rows *= rs.eo[k];
      TRY(launch(h, "nd_lpk", st, [&] {
        k_nd_lpk_rows<T><<<nd_row_grid(rs.rows), 256, 0, st>>>(rs, cur, dst, ds->nd[l].mass[a]);
      }));
    } else {
      TRY(launch(h, "nd_lpk", st, [&] {
        k_nd_lpk<T><<<nd_grid(total), 256, 0, st>>>(s, cur, dst, ds->nd[l].mass[a], total);
      }));
    }
    cur = dst;
    which ^= 1;
    s.e[a] = s.m;
    uint64_t sacc = 1;
    for (int d = D - 1; d >= 0; d--) {
      s.is[d] = sacc;
      sacc *= s.e[d];
    }
  }
  T *x = const_cast<T *>(cur);
  for (int a = D - 1; a >= 0; a--) {
    uint64_t np = 1;
    for (int d = 0; d < D; d++)
      if (d != a) np *= s.e[d];
    // the box is compact: a solve along dim a is the strided (or, a = D - 1, contiguous) solve of
    // the 3-D view (dims before a, a, dims behind a) -- the tuned kernels of ipk_launch (LDS-staged,
    // streaming, verified chunks for long pencils) instead of one thread per pencil walking global
    // memory (5 x 5 x 5 x 5 x 40000: 1.5 ms per launch). Same arithmetic, same bits.
    uint64_t outer = 1, inner = 1;
    for (int d = 0; d < a; d++) outer *= s.e[d];
    for (int d = a + 1; d < D; d++) inner *= s.e[d];
    const uint64_t na = s.e[a];
    if (!h->force_nd_ipk && outer * na * inner < ((uint64_t)1 << 31) && na >= 2) {
      if (a == D - 1) {
        const uint32_t m3[3] = {(uint32_t)outer, 1u, (uint32_t)na};
        TRY(ipk_launch<T>(h, 2, m3, x, ds->nd[l].thomas[a], nullptr, +1, st));
      } else {
        const uint32_t m3[3] = {(uint32_t)outer, (uint32_t)na, (uint32_t)inner};
        TRY(ipk_launch<T>(h, 1, m3, x, ds->nd[l].thomas[a], nullptr, +1, st));
      }
      continue;
    }
    TRY(launch(h, "nd_ipk", st, [&] {
      k_nd_ipk<T><<<nd_grid(np), 256, 0, st>>>(D, a, s, x, ds->nd[l].thomas[a], np);
    }));
  }
  *out = x;
  return MGH_SUCCESS;
}

// src_top: the input when it is another array than v (out of place): the top level, whose fine box
// IS the array, reads it where it is -- neither the copy into v nor the one into the natural-order
// work array happen (two passes over the data; every element of v is written by that level).
template <typename T> int decompose_nd(mgh_hierarchy *h, T *v, hipStream_t st, const T *src_top = nullptr) {
  auto *ds = DS<T>(h);
  TRY(nd_ensure<T>(h));
  if (src_top && !(h->L >= 1 && nd_box_is_whole_array(nd_box<T>(h, h->L)))) {
    HIP_TRY(hipMemcpyAsync(v, src_top, h->total * sizeof(T), hipMemcpyDeviceToDevice, st));
    src_top = nullptr;
  }
  for (int l = h->L; l >= 1; l--) {
    const NdBox b = nd_box<T>(h, l);
    NdTables<T> tb{};
    uint64_t nn = 1, mm = 1;
    for (int d = 0; d < h->D; d++) {
      tb.ratio[d] = ds->nd[l].ratio[d];
      nn *= b.n[d];
      mm *= b.m[d];
    }
    T *w = ds->nd_w;
    if (l == h->L && src_top) {
      w = const_cast<T *>(src_top);  // (mode 0 only reads it)
    } else if (nd_box_is_whole_array(b)) {  // the top level: the fine box IS the array -- a plain copy
      TRY(launch(h, "nd_gather", st, [&] {
        (void)hipMemcpyAsync(ds->nd_w, v, nn * sizeof(T), hipMemcpyDeviceToDevice, st);
      }));
    } else {
      TRY(launch(h, "nd_gather", st, [&] {
        k_nd_gather<T><<<nd_grid(nn), 256, 0, st>>>(b, v, ds->nd_w, nn, 0);
      }));
    }
    TRY(nd_coeff_launch<T>(h, b, tb, w, v, nn, 0, st));
    T *corr = nullptr;
    TRY(nd_correction<T>(h, l, v, b, &corr, st));
    TRY(launch(h, "nd_apply", st, [&] {
      k_nd_apply<T><<<nd_grid(mm), 256, 0, st>>>(b, corr, v, mm, +1);
    }));
  }
  return MGH_SUCCESS;
}

// (stop >= 0: `v` is the dense corner box of level `stop`, and the loop ends there; start >= 1: the
// corner box of level start - 1 inside `v` holds that level's nodal values, and the loop begins at start)
template <typename T> int recompose_nd(mgh_hierarchy *h, T *v, hipStream_t st, int stop = -1, int start = 0) {
  auto *ds = DS<T>(h);
  size_t count = 0;
  if (stop >= 0) {
    count = 1;
    for (int d = 0; d < h->D; d++) count *= HH<T>(h)->level_shape[stop][d];
  }
  TRY(nd_ensure<T>(h, count));
  for (int l = std::max(1, start); l <= (stop < 0 ? h->L : stop); l++) {
    const NdBox b = nd_box<T>(h, l, stop);
    NdTables<T> tb{};
    uint64_t nn = 1, mm = 1;
    for (int d = 0; d < h->D; d++) {
      tb.ratio[d] = ds->nd[l].ratio[d];
      nn *= b.n[d];
      mm *= b.m[d];
    }
    T *corr = nullptr;
    TRY(nd_correction<T>(h, l, v, b, &corr, st));
    TRY(launch(h, "nd_apply", st, [&] {
      k_nd_apply<T><<<nd_grid(mm), 256, 0, st>>>(b, corr, v, mm, -1);
    }));
    TRY(nd_coeff_launch<T>(h, b, tb, ds->nd_w, v, nn, 1, st));
    TRY(nd_coeff_launch<T>(h, b, tb, ds->nd_w, v, nn, 2, st));
    if (nd_box_is_whole_array(b)) {
      TRY(launch(h, "nd_gather", st, [&] {
        (void)hipMemcpyAsync(v, ds->nd_w, nn * sizeof(T), hipMemcpyDeviceToDevice, st);
      }));
    } else {
      TRY(launch(h, "nd_gather", st, [&] {
        k_nd_gather<T><<<nd_grid(nn), 256, 0, st>>>(b, v, ds->nd_w, nn, 1);
      }));
    }
  }
  return MGH_SUCCESS;
}

template <typename T>
int decompose_dense(mgh_hierarchy *h, const T *data, T *coeff, hipStream_t s) {
  auto *ds = DS<T>(h);
  if (fused4_ok(h) && !h->force_v1) {
    const T *src4 = data;
    if ((const void *)data == (const void *)coeff) {
      TRY(ensure_scratch<T>(h));
      HIP_TRY(hipMemcpyAsync(ds->scratch_full, data, h->total * sizeof(T), hipMemcpyDeviceToDevice, s));
      src4 = ds->scratch_full;
    }
    return decompose_fused<T, OUT_T>(h, src4, dense_layout(h), coeff, nullptr, s);
  }
  if (h->D > 3 || h->force_nd)
    return decompose_nd<T>(h, coeff, s, (const void *)data != (const void *)coeff ? data : nullptr);
  const int L = h->L;
  const size_t fI = ds->full_I, fJ = ds->full_J;
  const T *src = data;
  size_t sI = fI, sJ = fJ;
  if ((const void *)data == (const void *)coeff) {
    TRY(ensure_scratch<T>(h));
    HIP_TRY(hipMemcpyAsync(ds->scratch_full, data, h->total * sizeof(T), hipMemcpyDeviceToDevice, s));
    src = ds->scratch_full;
  }
  if (fused_ok(h) && !h->force_v1) return decompose_fused<T, OUT_T>(h, src, dense_layout(h), coeff, nullptr, s);
  const dim3 blk(64, 4, 1);
  for (int l = L; l >= 1; l--) {
    const LevelTables<T> &t = ds->lt[l];
    const Box3 &b = t.box;
    T *coarse = ds->nodal[l - 1];
    TRY(launch(h, "gpk_reo", s, [&] {
      k_gpk_reo<T><<<grid3(b.n[0], b.n[1], b.n[2], blk), blk, 0, s>>>(
          b, src, sI, sJ, coarse, coeff, fI, fJ, t.ratio[0], t.ratio[1], t.ratio[2]);
    }));
    TRY(correction<T>(h, l, coeff, fI, fJ, coarse, +1, s));
    src = coarse;
    sJ = b.m[2];
    sI = (size_t)b.m[1] * b.m[2];
  }
  // level-0 nodal values are the head of the coefficient array
  if (L >= 1) {
    const Box3 &b = ds->lt[1].box;
    TRY(launch(h, "copy_box", s, [&] {
      k_copy_box<T><<<grid3(b.m[0], b.m[1], b.m[2], blk), blk, 0, s>>>(
          b.m[0], b.m[1], b.m[2], ds->nodal[0], (size_t)b.m[1] * b.m[2], (size_t)b.m[2], coeff, fI,
          fJ);
    }));
  } else if ((const void *)data != (const void *)coeff) {
    HIP_TRY(hipMemcpyAsync(coeff, data, h->total * sizeof(T), hipMemcpyDeviceToDevice, s));
  }
  return MGH_SUCCESS;
}


template <typename T, typename QT, typename QTL = QT>
int recompose_levels(mgh_hierarchy *h, RecomposeArgs<T> A, const std::vector<T> &level_qv, T *data, const Layout &out,
                     hipStream_t st, const RecomposeArgs<T> *AL = nullptr, int ntop = 1, int stop = -1, int start = 0);

template <typename T, typename QT, typename QTL = QT>
int recompose_levels4(mgh_hierarchy *h, RecomposeArgs<T> A, const std::vector<T> &level_qv, T *data,
                      hipStream_t st, const RecomposeArgs<T> *AL = nullptr, size_t A_sT = 0, int ntop = 1,
                      int stop = -1, int start = 0);

// The one D == 4 dispatch of the fused level loops. A_sT as in recompose_levels4, `out` as in
// recompose_levels: each takes its own.
template <typename T, typename QT, typename QTL = QT>
int recompose_levels_any(mgh_hierarchy *h, const RecomposeArgs<T> &A, size_t A_sT, const std::vector<T> &level_qv,
                         T *data, const Layout &out, hipStream_t st, const RecomposeArgs<T> *AL = nullptr,
                         int ntop = 1, int stop = -1, int start = 0) {
  if (h->D == 4) return recompose_levels4<T, QT, QTL>(h, A, level_qv, data, st, AL, A_sT, ntop, stop, start);
  return recompose_levels<T, QT, QTL>(h, A, level_qv, data, out, st, AL, ntop, stop, start);
}

// The level loop of the one-thread-per-element kernels (D <= 3): coefficients C with strides
// (cI, cJ, 1) in the 3-D view, levels 1 .. Ls. Ls == L: `data` has the full array's strides;
// below (mgh_*_to_level) it is the dense array of level Ls. start >= 1 (mgh_refine_level): levels
// start .. Ls alone, with the nodal values of level start - 1 in ds->nodal[start - 1] already.
template <typename T>
int recompose_v1_levels(mgh_hierarchy *h, const T *C, size_t cI, size_t cJ, T *data, int Ls, hipStream_t s,
                        int start = 0) {
  auto *ds = DS<T>(h);
  const int L = h->L;
  const dim3 blk(64, 4, 1);
  if (start < 1) {
    const Box3 &b = ds->lt[1].box;
    TRY(launch(h, "copy_box", s, [&] {
      k_copy_box<T><<<grid3(b.m[0], b.m[1], b.m[2], blk), blk, 0, s>>>(
          b.m[0], b.m[1], b.m[2], C, cI, cJ, Ls == 0 ? data : ds->nodal[0], (size_t)b.m[1] * b.m[2],
          (size_t)b.m[2]);
    }));
  }
  for (int l = std::max(1, start); l <= Ls; l++) {
    const LevelTables<T> &t = ds->lt[l];
    const Box3 &b = t.box;
    T *coarse = ds->nodal[l - 1];
    TRY(correction<T>(h, l, C, cI, cJ, coarse, -1, s, Ls));
    T *out = (l == Ls) ? data : ds->nodal[l];
    const size_t oJ = (l == L) ? ds->full_J : b.n[2];
    const size_t oI = (l == L) ? ds->full_I : (size_t)b.n[1] * b.n[2];
    TRY(launch(h, "gpk_rev", s, [&] {
      k_gpk_rev<T><<<grid3(b.n[0], b.n[1], b.n[2], blk), blk, 0, s>>>(
          b, coarse, C, cI, cJ, out, oI, oJ, t.ratio[0], t.ratio[1], t.ratio[2]);
    }));
  }
  return MGH_SUCCESS;
}

template <typename T>
int recompose_dense(mgh_hierarchy *h, const T *coeff, T *data, hipStream_t s) {
  auto *ds = DS<T>(h);
  if (fused4_ok(h) && !h->force_v1) {
    // D = 4 on the slice-by-slice level loop, reading floating-point coefficients
    const T *C = coeff;
    if ((const void *)data == (const void *)coeff) {
      TRY(ensure_scratch<T>(h));
      HIP_TRY(hipMemcpyAsync(ds->scratch_full, coeff, h->total * sizeof(T), hipMemcpyDeviceToDevice, s));
      C = ds->scratch_full;
    }
    RecomposeArgs<T> A{};
    A.coef = C;
    return recompose_levels4<T, T>(h, A, std::vector<T>(h->L + 1, (T)1), data, s);
  }
  if (h->D > 3 || h->force_nd) {
    if ((const void *)data != (const void *)coeff)
      HIP_TRY(hipMemcpyAsync(data, coeff, h->total * sizeof(T), hipMemcpyDeviceToDevice, s));
    return recompose_nd<T>(h, data, s);
  }
  const int L = h->L;
  const size_t fI = ds->full_I, fJ = ds->full_J;
  const T *C = coeff;
  if ((const void *)data == (const void *)coeff) {
    if (L == 0) return MGH_SUCCESS;
    TRY(ensure_scratch<T>(h));
    HIP_TRY(hipMemcpyAsync(ds->scratch_full, coeff, h->total * sizeof(T), hipMemcpyDeviceToDevice, s));
    C = ds->scratch_full;
  }
  if (L == 0) {
    HIP_TRY(hipMemcpyAsync(data, coeff, h->total * sizeof(T), hipMemcpyDeviceToDevice, s));
    return MGH_SUCCESS;
  }
  if (fused_ok(h) && !h->force_v1) {
    // the level loop of the fused decompression, reading floating-point coefficients
    RecomposeArgs<T> A{};
    A.coef = C;
    A.dI = fI;
    A.dJ = fJ;
    return recompose_levels<T, T>(h, A, std::vector<T>(L + 1, (T)1), data, dense_layout(h), s);
  }
  return recompose_v1_levels<T>(h, C, fI, fJ, data, L, s);
}


// ---- reconstruction at a coarser level (mgh_*_to_level) -----------------------------------------
// The corner box of `level` in the full array: extents, and the element strides of the source array.
template <typename T> LevelBox level_box_of(const mgh_hierarchy *h, int level, const Layout &src) {
  auto *hh = HH<T>(h);
  LevelBox b{};
  b.D = h->D;
  for (int d = 0; d < h->D; d++) {
    b.m[d] = (uint32_t)hh->level_shape[level][d];
    b.n[d] = (uint32_t)hh->shape[d];
    b.ss[d] = src.view.stride[MGH_MAX_DIM - h->D + d];
  }
  return b;
}
inline uint64_t level_box_rows(const LevelBox &b) {
  uint64_t rows = 1;
  for (int d = 0; d < b.D - 1; d++) rows *= b.m[d];
  return rows;
}
// (one wave per piece of a row, four waves a workgroup: kernels_level.hpp)
inline unsigned level_box_grid(const LevelBox &b) {
  const uint64_t units = level_box_rows(b) * ((b.m[b.D - 1] + kLevelBoxPiece - 1) / kLevelBoxPiece);
  return (unsigned)std::min<uint64_t>((units + 3) / 4, 256 * 32);
}

// Fused decompression: outlier restore, then per level (coarse to fine) the load vector
// straight from the quantized coefficients, three Thomas solves subtracting the correction
// from the coarse nodes, and the node restore with the dequantizer fused in
// (Compressor::Decompress lines 256-257 = Dequantize + Recompose). With QT = T the same level
// loop runs on floating-point coefficients (Compressor::Recompose on its own).
// Node restore of one level (or one t-slice of a 4-D level): the marching kernel
// (kernels_recompose2.hpp).
// (TC x TF coarse nodes per workgroup: 4 x 64, or 64 x 4 where the fastest extent is short -- fused_tall_tiles)
template <typename T, typename QT, bool TODD, int TC, int TF>
int launch_restore3(mgh_hierarchy *h, const RecomposeArgs<T> &A, const Box3 &b, const char *nm, hipStream_t st) {
    Restore3Grid G{};
    G.gxm = ((int)b.m[2] + TF - 1) / TF;
    G.ntile = G.gxm * (((int)b.m[1] + TC - 1) / TC);
    // chunk length: long marches where there are plenty of tiles, short ones (more workgroups)
    // on the small levels -- a chunk costs one extra coarse plane of interpolants only
    const int nslice = A.zb_mode ? (A.zb_mode == 2 ? A.zb_mt : A.zb_nt - A.zb_mt) : 1;
    const int want = 2048;
    G.rch = std::max(1, std::min(16, (int)((int64_t)b.m[0] * G.ntile * nslice / want)));
    G.nchunk = ((int)b.m[0] + G.rch - 1) / G.rch;
    const dim3 grid((unsigned)G.ntile, (unsigned)G.nchunk, (unsigned)nslice);
    return launch(h, nm, st, [&] { k_level_restore3_q<T, QT, TODD, TC, TF><<<grid, TC * TF, 0, st>>>(A, G); });
}

template <typename T, typename QT, bool TODD>
int launch_restore(mgh_hierarchy *h, const RecomposeArgs<T> &A, const Box3 &b, const char *nm, hipStream_t st) {
  if (fused_tall_tiles(h, b)) return launch_restore3<T, QT, TODD, 64, 4>(h, A, b, nm, st);
  return launch_restore3<T, QT, TODD, 4, 64>(h, A, b, nm, st);
}
// Load-vector pass of the decompression side (one level, or one t-slice of a 4-D level):
// one plane per step, march length by the number of tiles.
template <typename T, typename QT, int TC, int TF>
int launch_loadvec_t(mgh_hierarchy *h, const RecomposeArgs<T> &A, const Box3 &b, hipStream_t st) {
  const unsigned gx = (b.m[2] + TF - 1) / TF, gy = (b.m[1] + TC - 1) / TC;
  // (A.zb_mode == 1: all the padded t positions of a 4-D level in this launch, the r-chunks of one
  // behind those of the other in grid.z -- which holds 65535 at most: shorter marches only where
  // they fit)
  const unsigned ns = A.zb_mode == 1 ? (unsigned)(2 * A.zb_mt - 1) : 1u;
  const unsigned z16 = (b.m[0] + 15) / 16, z4 = (b.m[0] + 3) / 4, z1 = b.m[0];
  RecomposeArgs<T> B = A;
  if ((size_t)gx * gy * z16 * ns >= 2048 || (size_t)z4 * ns > 65535) {
    B.zb_nz = (int)z16;
    return launch(h, "loadvec_q", st, [&] {
      k_level_loadvec_q<T, QT, TC, TF, 16><<<dim3(gx, gy, z16 * ns), 256, 0, st>>>(B);
    });
  }
  if ((size_t)gx * gy * z4 * ns >= 256 || (size_t)z1 * ns > 65535) {
    B.zb_nz = (int)z4;
    return launch(h, "loadvec_q_small", st, [&] {
      k_level_loadvec_q<T, QT, TC, TF, 4><<<dim3(gx, gy, z4 * ns), 256, 0, st>>>(B);
    });
  }
  B.zb_nz = (int)z1;
  return launch(h, "loadvec_q_small", st, [&] {
    k_level_loadvec_q<T, QT, TC, TF, 1><<<dim3(gx, gy, z1 * ns), 256, 0, st>>>(B);
  });
}

// (8 x 32 coarse nodes per workgroup, or 64 x 4 where the fastest extent is short -- fused_tall_tiles)
template <typename T, typename QT>
int launch_loadvec(mgh_hierarchy *h, const RecomposeArgs<T> &A, const Box3 &b, hipStream_t st) {
  if (fused_tall_tiles(h, b)) return launch_loadvec_t<T, QT, 64, 4>(h, A, b, st);
  return launch_loadvec_t<T, QT, 8, 32>(h, A, b, st);
}

// QTL / AL: coefficient source of the `ntop` FINEST levels when it differs from that of the levels
// below (16-bit symbols for the finest levels, int64 of the coarse corner box for the rest:
// dequantize_recompose_fused16); AL == nullptr: one source for all levels.
// out: the layout of `data` as the full array -- dense, or a pitched array the finest level's
// kernels write in place (Layout::native3).
// stop >= 0 (mgh_*_to_level): the loop ends at that level and `data` is the DENSE array of its
// shape -- the strides of the compact nodal buffer it stands in for.
// start >= 1 (mgh_refine_level): the levels start .. Ls alone, each with its own launches -- the
// corrected nodal values of level start - 1 are in ds->nodal[start - 1] already, nothing below is run.
template <typename T, typename QT, typename QTL>
int recompose_levels(mgh_hierarchy *h, RecomposeArgs<T> A, const std::vector<T> &level_qv, T *data, const Layout &out,
                     hipStream_t st, const RecomposeArgs<T> *AL, int ntop, int stop, int start) {
  auto *ds = DS<T>(h);
  const int L = h->L;
  const int Ls = stop < 0 ? L : stop;  // the last level run
  // levels 1 .. l_head run inside ONE single-workgroup kernel (their working set fits in LDS);
  // MGH_NO_RECOMPOSE_HEAD=1: every level with its own launches (cross-check)
  const bool no_head = h->no_head;
  int l_head = 0;
  if (!no_head && start < 1) {
    for (int l = 1; l <= std::min(std::min(AL ? L - ntop : L, Ls), kTailMaxLevels); l++) {
      if ((head_lds_elems(ds->lt[l].box) + ds->lt_end[l]) * sizeof(T) > 150 * 1024) break;
      l_head = l;
    }
  }
  if (l_head >= 1) {
    HeadArgs<T> HA{};
    HA.nlevels = l_head;
    for (int l = 1; l <= l_head; l++) {
      HeadLevel<T> &hl = HA.lv[l - 1];
      const LevelTables<T> &t = ds->lt[l];
      hl.b = t.box;
      for (int k = 0; k < 3; k++) {
        hl.ratio[k] = t.ratio[k];
        hl.mass[k] = t.mass[k];
        hl.thomas[k] = t.thomas[k];
      }
      hl.qv = level_qv[l];
    }
    HA.qv0 = level_qv[0];
    HA.in = A;
    const Box3 &bl = ds->lt[l_head].box;
    HA.out = (l_head == Ls) ? data : ds->nodal[l_head];
    HA.oJ = (l_head == L) ? out.J : bl.n[2];
    HA.oI = (l_head == L) ? out.I : (size_t)bl.n[1] * bl.n[2];
    HA.tab_base = ds->tables;
    HA.tab_count = (uint32_t)ds->lt_end[l_head];
    const size_t lds = (head_lds_elems(bl) + ds->lt_end[l_head]) * sizeof(T);
    static std::atomic<uint64_t> once{0};
    TRY(allow_big_lds_once(k_recompose_head<T, QT>, once));
    TRY(launch(h, "recompose_head", st, [&] { k_recompose_head<T, QT><<<1, 1024, lds, st>>>(HA); }));
  } else if (start < 1) {
    const Box3 &b = ds->lt[1].box;
    A.qv = level_qv[0];
    TRY(launch(h, "head_in", st, [&] {
      const size_t tot = (size_t)b.m[0] * b.m[1] * b.m[2];
      k_head_in_q<T, QT><<<(unsigned)std::min<size_t>((tot + 255) / 256, 1024), 256, 0, st>>>(
          (int)b.m[0], (int)b.m[1], (int)b.m[2], A, Ls == 0 ? data : ds->nodal[0]);
    }));
  }
  for (int l = std::max(l_head + 1, start); l <= Ls; l++) {
    const LevelTables<T> &t = ds->lt[l];
    const Box3 &b = t.box;
    const bool top = AL && l > L - ntop;
    RecomposeArgs<T> B = top ? *AL : A;
    for (int k = 0; k < 3; k++) {
      B.n[k] = (int)b.n[k];
      B.m[k] = (int)b.m[k];
      B.ratio[k] = t.ratio[k];
      B.mass[k] = t.mass[k];
    }
    B.qv = level_qv[l];
    B.load = ds->t3;
    B.coarse = ds->nodal[l - 1];
    if (top) TRY((launch_loadvec<T, QTL>(h, B, b, st)));
    else TRY((launch_loadvec<T, QT>(h, B, b, st)));
    TRY(ipk_fc_launch<T>(h, b.m, ds->t3, t.thomas[2], t.thomas[1], st));
    TRY(ipk_launch<T>(h, 0, b.m, ds->t3, t.thomas[0], ds->nodal[l - 1], -1, st));
    B.fine = (l == Ls) ? data : ds->nodal[l];
    B.fJ = (l == L) ? out.J : b.n[2];
    B.fI = (l == L) ? out.I : (size_t)b.n[1] * b.n[2];
    if (top) TRY((launch_restore<T, QTL, false>(h, B, b, "restore_q", st)));
    else TRY((launch_restore<T, QT, false>(h, B, b, "restore_q", st)));
  }
  return MGH_SUCCESS;
}

// D = 4, the mirror of decompose_fused4: per level (coarse to fine) the load vector of every
// t-slice with the 3-D kernel (odd slices: every node is a coefficient), the t-sweep, four Thomas
// solves subtracting the correction from the coarse nodes, then the node restore slice by slice
// (odd slices interpolate across t between the two neighbouring coarse slices).
// A_sT: element stride between two t-slices of A's source (0: the full array's). AL / QTL as in
// recompose_levels (the finest level's source has the full array's strides). start as there: the
// nodal values of level start - 1 are in ds->nodal4[start - 1].
template <typename T, typename QT, typename QTL>
int recompose_levels4(mgh_hierarchy *h, RecomposeArgs<T> A0, const std::vector<T> &level_qv, T *data,
                      hipStream_t st, const RecomposeArgs<T> *AL, size_t A_sT, int ntop, int stop, int start) {
  auto *ds = DS<T>(h);
  auto *hh = HH<T>(h);
  const int L = h->L;
  const int Ls = stop < 0 ? L : stop;  // the last level run; below L, `data` is dense in its shape
  const auto &sh = hh->level_shape;
  const size_t full[4] = {(size_t)sh[L][1] * sh[L][2] * sh[L][3], (size_t)sh[L][2] * sh[L][3],
                          (size_t)sh[L][3], 1};
  TRY(ensure_state4<T>(h));
  if (!A_sT) {
    A_sT = full[0];
    A0.dI = full[1];
    A0.dJ = full[2];
  }
  if (start < 1) {
    const auto &M0 = sh[0];
    const size_t tot = (size_t)M0[0] * M0[1] * M0[2] * M0[3];
    A0.qv = level_qv[0];
    TRY(launch(h, "head_in", st, [&] {
      k_head_in4_q<T, QT><<<(unsigned)std::min<size_t>((tot + 255) / 256, 1024), 256, 0, st>>>(
          (int)M0[0], (int)M0[1], (int)M0[2], (int)M0[3], A0, A_sT, Ls == 0 ? data : ds->nodal4[0]);
    }));
  }
  for (int l = std::max(1, start); l <= Ls; l++) {
    const bool top = AL && l > L - ntop;
    RecomposeArgs<T> A = top ? *AL : A0;
    const size_t sT = top ? full[0] : A_sT;
    if (top) {
      A.dI = full[1];
      A.dJ = full[2];
    }
    const auto &N = sh[l], &Mc = sh[l - 1];
    Box3 b;
    for (int k = 0; k < 3; k++) {
      b.n[k] = (uint32_t)N[1 + k];
      b.m[k] = (uint32_t)Mc[1 + k];
      A.n[k] = (int)N[1 + k];
      A.m[k] = (int)Mc[1 + k];
      A.ratio[k] = ds->nd[l].ratio[1 + k];
      A.mass[k] = ds->nd[l].mass[1 + k];
    }
    A.qv = level_qv[l];
    A.ratio_t = ds->nd[l].ratio[0];
    const size_t M = (size_t)Mc[1] * Mc[2] * Mc[3];
    const int n_t = (int)N[0], m_t = (int)Mc[0];
    // ---- load vectors of the padded t positions: one launch for all of them (grid.z limit
    // permitting; MGH_SLICE_BATCH=0: a launch per slice)
    const bool batch = h->slice_batch &&
                       (size_t)(2 * m_t - 1) * ((Mc[1] + 15) / 16) < 65536;  // (grid.z of the load-vector launch)
    if (n_t % 2 == 0)  // ghost slice
      HIP_TRY(hipMemsetAsync(ds->load4 + (size_t)(n_t - 1) * M, 0, M * sizeof(T), st));
    if (batch) {
      A.zb_mode = 1;
      A.zb_mt = m_t;
      A.zb_nt = n_t;
      A.zb_sT = sT;
      A.zb_M = M;
      A.load = ds->load4;
      if (top) TRY((launch_loadvec<T, QTL>(h, A, b, st)));
      else TRY((launch_loadvec<T, QT>(h, A, b, st)));
      A.zb_mode = 0;
    } else {
      for (int P = 0; P <= 2 * m_t - 2; P++) {
        if (n_t % 2 == 0 && P == n_t - 1) continue;
        A.allcoef = P & 1;
        A.lin_base = (size_t)((P & 1) ? m_t + (P - 1) / 2 : P / 2) * sT;
        A.load = ds->load4 + (size_t)P * M;
        if (top) TRY((launch_loadvec<T, QTL>(h, A, b, st)));
        else TRY((launch_loadvec<T, QT>(h, A, b, st)));
      }
    }
    A.allcoef = 0;
    // ---- t-sweep, Thomas solves f, c, r, t; the last one subtracts from the coarse nodes
    {
      TRY((tsweep_launch<T>(h, ds->load4, ds->corr4, M, m_t, ds->nd[l].mass[0], st)));
    }
    const uint32_t m3a[3] = {(uint32_t)(m_t * Mc[1]), (uint32_t)Mc[2], (uint32_t)Mc[3]};
    TRY(ipk_launch<T>(h, 2, m3a, ds->corr4, ds->nd[l].thomas[3], nullptr, +1, st));
    TRY(ipk_launch<T>(h, 1, m3a, ds->corr4, ds->nd[l].thomas[2], nullptr, +1, st));
    TRY(ipk_launch<T>(h, 0, b.m, ds->corr4, ds->nd[l].thomas[1], nullptr, +1, st, (uint32_t)m_t, M));
    TRY((tsolve_apply<T>(h, ds->corr4, ds->nodal4[l - 1], M, m_t, Mc[1] * Mc[2], Mc[3], ds->nd[l].thomas[0], -1, st)));
    // ---- node restore, slice by slice
    T *fine = (l == Ls) ? data : ds->nodal4[l];
    const size_t fT = (l == L) ? full[0] : (size_t)N[1] * N[2] * N[3];
    A.fI = (l == L) ? full[1] : (size_t)N[2] * N[3];
    A.fJ = (l == L) ? full[2] : (size_t)N[3];
    if (batch) {
      A.zb_mt = m_t;
      A.zb_nt = n_t;
      A.zb_sT = sT;
      A.zb_M = M;
      A.zb_fT = fT;
      A.fine = fine;
      A.coarse = ds->nodal4[l - 1];
      A.zb_mode = 2;
      if (top) TRY((launch_restore<T, QTL, false>(h, A, b, "restore_q", st)));
      else TRY((launch_restore<T, QT, false>(h, A, b, "restore_q", st)));
      if (n_t - m_t > 0) {
        A.zb_mode = 3;
        if (top) TRY((launch_restore<T, QTL, true>(h, A, b, "restore_q_odd", st)));
        else TRY((launch_restore<T, QT, true>(h, A, b, "restore_q_odd", st)));
      }
      continue;
    }
    for (int tp = 0; tp < n_t; tp++) {
      const bool last_even = n_t % 2 == 0 && tp == n_t - 1;  // the real last node: coarse m_t - 1
      A.fine = fine + (size_t)tp * fT;
      if (!(tp & 1) || last_even) {
        const int zi = last_even ? m_t - 1 : tp / 2;
        A.coarse = ds->nodal4[l - 1] + (size_t)zi * M;
        A.lin_base = (size_t)zi * sT;
        if (top) TRY((launch_restore<T, QTL, false>(h, A, b, "restore_q", st)));
        else TRY((launch_restore<T, QT, false>(h, A, b, "restore_q", st)));
      } else {
        const int zi = (tp - 1) / 2;
        A.coarse = ds->nodal4[l - 1] + (size_t)zi * M;
        A.coarse_b = ds->nodal4[l - 1] + (size_t)(zi + 1) * M;
        A.tpos = tp;
        A.lin_base = (size_t)(m_t + zi) * sT;
        if (top) TRY((launch_restore<T, QTL, true>(h, A, b, "restore_q_odd", st)));
        else TRY((launch_restore<T, QT, true>(h, A, b, "restore_q_odd", st)));
      }
    }
  }
  return MGH_SUCCESS;
}

// ---- what a reconstruction reads and makes: the descriptors of reconstruct() below ----------------
// Quantization parameters, and the out-of-dictionary values of the record.
struct QuantSpec {
  int ebtype;
  double tol, s, norm;
  uint64_t dict_size;
  int prep_huffman;
  const uint64_t *oidx;
  const int64_t *oval;
  uint64_t ocount;
};
inline int64_t dict_half(const QuantSpec &qs) { return qs.prep_huffman ? (int64_t)(qs.dict_size / 2) : 0; }

// The integers.
struct IntSource {
  enum Kind {
    Full,    // q: the full array, with the hierarchy's strides
    Box,     // q: the COMPACT corner box of the target's stop level (dense in its shape), outliers in it
    Linear,  // q: level-linearised -- its head up to the stop level, or (a level step) the stop level's segment
    Sym16    // sym: 16-bit dictionary symbols of the full array
  } kind;
  int64_t *q;
  const uint16_t *sym;
};

// What is made: the dense array of level `stop` (stop == l_target: the full array, in layout `lay`),
// from level 0 (start == 0), or in one level step (start == stop) from `coarse`, the dense array of
// level stop - 1.
struct Target {
  int stop, start;
  const void *coarse;
  void *out;
  Layout lay;
};

// Quantum of every level: its quantizer, times its volume factor when s != inf.
template <typename T> std::vector<T> level_quanta(const mgh_hierarchy *h, const QuantSpec &qs) {
  auto *hh = HH<T>(h);
  std::vector<T> qv(h->L + 1);
  hh->quantizers(qs.ebtype, (T)qs.tol, (T)qs.s, (T)qs.norm, false, qv.data());
  if (!((T)qs.s == std::numeric_limits<T>::infinity()))
    for (int l = 0; l <= h->L; l++) qv[l] = qv[l] * hh->level_volume(l, true);
  return qv;
}

// A device buffer of the handle grown to `count` elements (never shrunk; counted in mgh_device_bytes:
// a stop level's box is a fraction of the full call's).
template <typename U> int grow(mgh_hierarchy *h, U **p, size_t *elems, size_t count) {
  if (count <= *elems) return MGH_SUCCESS;
  dev_free(h, p, *elems);
  *elems = 0;
  TRY(dev_alloc(h, p, count));
  *elems = count;
  return MGH_SUCCESS;
}

// Row-major element strides of a dense box of extents m[0 .. D); returns its element count.
template <typename E, typename S> uint64_t compact_strides(int D, const E *m, S *ss) {
  uint64_t bs = 1;
  for (int d = D - 1; d >= 0; d--) {
    ss[d] = (S)bs;
    bs *= m[d];
  }
  return bs;
}
// ... as the source of the fused level loops (D = 3, 4): A.dI / A.dJ; returns the t-slice stride (D = 4)
template <typename T, typename E> size_t box_source(RecomposeArgs<T> &A, int D, const E *m) {
  size_t ss[MGH_MAX_DIM];
  compact_strides(D, m, ss);
  A.dJ = ss[D - 2];
  A.dI = ss[D - 3];
  return D == 4 ? ss[0] : 0;
}

// Out-of-dictionary values written over the integers that are about to be read. `kernel`: the one of
// k_outlier_restore (an array or its head), _in_box (corner box inside the full array), _box (widened
// compact box), _window (a segment of a linearised array) for what q holds; `where`: its arguments
// between q and the list.
template <typename K, typename... W>
int outliers_back(mgh_hierarchy *h, const QuantSpec &qs, const char *name, hipStream_t st, K kernel, int64_t *q,
                  W... where) {
  if (!qs.prep_huffman || !qs.ocount) return MGH_SUCCESS;
  return launch(h, name, st, [&] {
    kernel<<<(unsigned)((qs.ocount + 255) / 256), 256, 0, st>>>(q, where..., qs.oidx, qs.oval, qs.ocount);
  });
}

// The fused level loops from 16-bit dictionary symbols (what the Huffman decoder of the high-level
// path delivers; qs.prep_huffman is 1): no int64 array, the out-of-dictionary values are found
// through a hash table.
template <typename T>
int dequantize_recompose_fused16(mgh_hierarchy *h, const QuantSpec &qs, const uint16_t *sym, T *data,
                                 const Layout &out, hipStream_t st, int stop) {
  auto *ds = DS<T>(h);
  auto *hh = HH<T>(h);
  const int L = h->L;
  const uint64_t ocount = qs.ocount;
  RecomposeArgs<T> A{};
  const bool mixed = h->sym16_mixed && L >= 2 && h->total >= ((uint64_t)1 << 18);
  const int ntop = L >= 4 ? 2 : 1;
  // a stop at or below the levels that run on the widened box (mgh_*_to_level): the box of the stop
  // level is all there is to read -- no table, no symbol of the finest levels
  const bool box_only = mixed && stop <= L - ntop;
  if (ocount && !box_only) {
    size_t slots = 16;
    while (slots < 2 * ocount) slots *= 2;
    if (slots > ((size_t)1 << 31)) return fail(MGH_ERR_INVALID_ARGUMENT, "too many outliers");
    if (slots > ds->oh_slots) {
      (void)hipFree(ds->oh_key);
      (void)hipFree(ds->oh_val);
      ds->oh_key = nullptr;
      ds->oh_val = nullptr;
      ds->oh_slots = 0;
      HIP_TRY(hipMalloc(&ds->oh_key, slots * 8));
      HIP_TRY(hipMalloc(&ds->oh_val, slots * 8));
      ds->oh_slots = slots;
    }
    HIP_TRY(hipMemsetAsync(ds->oh_key, 0, slots * 8, st));
    TRY(launch(h, "outlier_table", st, [&] {
      k_outlier_hash_build<<<(unsigned)((ocount + 255) / 256), 256, 0, st>>>(
          qs.oidx, qs.oval, ocount, h->total, ds->oh_key, ds->oh_val, (uint32_t)(slots - 1));
    }));
    A.oh_key = ds->oh_key;
    A.oh_val = ds->oh_val;
    A.oh_mask = (uint32_t)(slots - 1);
  }
  A.q16 = sym;
  A.dI = ds->full_I;
  A.dJ = ds->full_J;
  A.half = dict_half(qs);
  const std::vector<T> level_qv = level_quanta<T>(h, qs);
  // Symbol width PER LEVEL: the finest levels -- where out-of-dictionary values are rare -- are
  // read as 16-bit symbols with the table look-up behind symbol 0. The levels below hold nearly
  // all the outliers, and a look-up there is a dependent global load inside latency-bound
  // kernels (measured: slower than the int64 path at 256^3). Their symbols -- the coarse corner
  // box of the reordered layout -- are widened to int64 in a compact box with the outliers
  // written over them, and those levels run the int64 kernels on it. Two levels stay on symbols
  // where the hierarchy is deep enough: the box is then 1/64 (D = 3) of the array instead of 1/8
  // (512^3: widening the 257^3 box cost 51 us, almost all of it the 136 MB of int64 stores).
  if (!mixed) return recompose_levels_any<T, uint16_t>(h, A, 0, level_qv, data, out, st, nullptr, 1, stop);
  const auto &Mc = hh->level_shape[box_only ? stop : L - ntop];
  const auto &N = hh->level_shape[L];
  BoxMap bm{};
  for (int k = 0; k < 4; k++) bm.m[k] = bm.n[k] = 1;
  for (int d = 0; d < h->D; d++) {
    bm.m[4 - h->D + d] = (uint32_t)Mc[d];
    bm.n[4 - h->D + d] = (uint32_t)N[d];
  }
  RecomposeArgs<T> A64{};
  const size_t sT = box_source(A64, 4, bm.m);
  const size_t box = sT * bm.m[0];
  TRY(grow(h, &ds->qbox, &ds->qbox_elems, box));
  const size_t rows = box / bm.m[3];
  if (rows >= ((size_t)1 << 32)) return fail(MGH_ERR_INVALID_ARGUMENT, "coarse box too large");
  TRY(launch(h, "widen_box", st, [&] {
    k_widen_box<<<(unsigned)std::min<size_t>((rows + 3) / 4, 256 * 32), 256, 0, st>>>(sym, ds->qbox, bm, (uint32_t)rows);
  }));
  TRY(outliers_back(h, qs, "outlier_restore", st, k_outlier_restore_box, ds->qbox, bm));
  A64.q = ds->qbox;
  A64.half = A.half;
  if (box_only) return recompose_levels_any<T, int64_t>(h, A64, sT, level_qv, data, out, st, nullptr, 1, stop);
  return recompose_levels_any<T, int64_t, uint16_t>(h, A64, sT, level_qv, data, out, st, &A, ntop, stop);
}

template <typename T>
int upload_quantizers(mgh_hierarchy *h, int ebtype, double tol, double s, double norm,
                      bool reciprocal, hipStream_t st) {
  auto *ds = DS<T>(h);
  auto *hh = HH<T>(h);
  const int L = h->L;
  std::vector<T> q(2 * (L + 1));
  hh->quantizers(ebtype, (T)tol, (T)s, (T)norm, reciprocal, q.data());
  const bool calc_vol = !((T)s == std::numeric_limits<T>::infinity());
  for (int l = 0; l <= L; l++) q[L + 1 + l] = calc_vol ? hh->level_volume(l, !reciprocal) : (T)1;
  ds->qmeta.calc_vol = calc_vol ? 1 : 0;
  // pageable-memory async copies are staged by the runtime before returning
  HIP_TRY(hipMemcpyAsync(ds->qz, q.data(), q.size() * sizeof(T), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  return MGH_SUCCESS;
}

// the stand-alone quantizer with the table already in ds->qz (uploaded, or made on the device)
template <typename T>
int quantize_launch(mgh_hierarchy *h, const T *coeff, const QuantOut &qo, hipStream_t st) {
  auto *ds = DS<T>(h);
  if (qo.ocount) HIP_TRY(hipMemsetAsync(qo.ocount, 0, sizeof(uint64_t), st));
  const size_t total = h->total;
  const unsigned grid = (unsigned)std::min<size_t>((total + kQuantPerRound - 1) / kQuantPerRound, 256 * 32);
  return launch(h, "quantize", st, [&] {
    k_quantize<T><<<grid, 256, 0, st>>>(ds->qmeta, total, coeff, ds->marks, ds->qz,
                                        ds->qz + (h->L + 1), (int64_t)qo.dict_size, qo.prep_huffman, qo.q,
                                        (unsigned long long *)qo.ocount, qo.oidx, qo.oval,
                                        (unsigned long long)qo.ocap);
  });
}

template <typename T>
int dequantize_dense(mgh_hierarchy *h, int64_t *q, const QuantSpec &qs, T *coeff, hipStream_t st) {
  auto *ds = DS<T>(h);
  TRY(upload_quantizers<T>(h, qs.ebtype, qs.tol, qs.s, qs.norm, false, st));
  const size_t total = h->total;
  TRY(outliers_back(h, qs, "outlier_restore", st, k_outlier_restore, q, h->total));
  const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 256 * 32);
  TRY(launch(h, "dequantize", st, [&] {
    k_dequantize<T><<<grid, 256, 0, st>>>(ds->qmeta, total, q, ds->marks, ds->qz,
                                          ds->qz + (h->L + 1), (int64_t)qs.dict_size, qs.prep_huffman,
                                          coeff);
  }));
  return MGH_SUCCESS;
}

uint64_t level_elems(const mgh_hierarchy *h, int level) {
  uint64_t n = 1;
  auto f = [&](auto *hh) {
    for (int d = 0; d < h->D; d++) n *= hh->level_shape[level][d];
  };
  if (h->dtype == MGH_FLOAT) f(HH<float>(h));
  else f(HH<double>(h));
  return n;
}

// A level step (Target::start >= 1) starts from the caller's dense array of `level`: the solves
// subtract the correction from the coarse nodes in place, so on a copy in the level loop's own buffer.
template <typename T> int coarse_in(mgh_hierarchy *h, T *nodal, const void *coarse, int level, hipStream_t st) {
  return launch(h, "refine_coarse_in", st, [&] {
    (void)hipMemcpyAsync(nodal, coarse, level_elems(h, level) * sizeof(T), hipMemcpyDeviceToDevice, st);
  });
}

// The level loop on a COMPACT corner box (dense array of level_shape(level)) for the shapes the
// fused kernels do not take: `fill(dst)` puts the box's coefficients there. The generic N-D kernels
// work in place, so the box is filled into the output itself; the node restore of the
// one-thread-per-element kernels reads the coefficients while it writes the output, so theirs is
// ds->level_box. start >= 1: the levels start .. level alone, on top of `coarse` (coarse_in).
template <typename T, typename Fill>
int recompose_box_to_level(mgh_hierarchy *h, int level, T *out, hipStream_t st, Fill &&fill, int start = 0,
                           const void *coarse = nullptr) {
  auto *ds = DS<T>(h);
  const int D = h->D;
  if (D > 3 || h->force_nd) {
    TRY(fill(out));
    return level == 0 ? (int)MGH_SUCCESS : recompose_nd<T>(h, out, st, level, start);
  }
  if (level == 0) return fill(out);
  size_t ss[3];
  const size_t count = compact_strides(D, HH<T>(h)->level_shape[level].data(), ss);
  TRY(grow(h, &ds->level_box, &ds->level_box_elems, count));
  TRY(fill(ds->level_box));
  if (start) TRY(coarse_in<T>(h, ds->nodal[start - 1], coarse, start - 1, st));
  // (the 3-D view: a dimension the array does not have steps over all of it)
  return recompose_v1_levels<T>(h, ds->level_box, D >= 3 ? ss[D - 3] : count, D >= 2 ? ss[D - 2] : count, out, level,
                                st, start);
}

// mgh_recompose_to_level, level < l_target. The fused kernels read the corner box in place, with
// the strides of the caller's array (any layout); the other paths gather it first (k_box_gather).
template <typename T>
int recompose_to_level_impl(mgh_hierarchy *h, const T *coeff, const Layout &in, int level, T *out, hipStream_t st) {
  const LevelBox lb = level_box_of<T>(h, level, in);
  const int D = h->D;
  if (fused_route(h) && (D == 4 || lb.ss[0] < ((uint64_t)1 << 30))) {
    RecomposeArgs<T> A{};
    A.coef = coeff;
    A.dI = (size_t)lb.ss[D - 3];
    A.dJ = (size_t)lb.ss[D - 2];
    return recompose_levels_any<T, T>(h, A, (size_t)lb.ss[0], std::vector<T>(h->L + 1, (T)1), out, dense_layout(h), st,
                                      nullptr, 1, level);
  }
  const uint64_t rows = level_box_rows(lb);
  return recompose_box_to_level<T>(h, level, out, st, [&](T *dst) {
    return launch(h, "box_gather", st, [&] {
      k_box_gather<T><<<level_box_grid(lb), 256, 0, st>>>(lb, coeff, dst, rows);
    });
  });
}

// ---- prolongation of a level to the full grid (mgh_prolong) ---------------------------------------
// The plan of the level step l - 1 -> l (prolong_plan.hpp) for this hierarchy's switches.
template <typename T> ProlongPlan prolong_plan_of(const mgh_hierarchy *h, int l) {
  return prolong_plan(DS<T>(h)->lt[l].box.m, h->fused.tall != 0);
}

template <typename T, int TC, int TF>
int launch_prolong3_t(mgh_hierarchy *h, const ProlongArgs<T> &A, hipStream_t st) {
  const dim3 grid((unsigned)(A.gxm * ((A.m[1] + TC - 1) / TC)), (unsigned)A.nchunk, 1);
  return launch(h, "prolong3", st, [&] { k_prolong3<T, TC, TF><<<grid, TC * TF, 0, st>>>(A); });
}

// Fused 3-D route: one launch per level level + 1 .. l_target, the intermediates in the compact
// nodal buffers of the level loops, the last launch into `out` (dense, the full array's strides).
template <typename T>
int prolong_fused3(mgh_hierarchy *h, int level, const T *lvl, T *out, hipStream_t st) {
  auto *ds = DS<T>(h);
  const int L = h->L;
  const T *coarse = lvl;
  for (int l = level + 1; l <= L; l++) {
    const LevelTables<T> &t = ds->lt[l];
    const Box3 &b = t.box;
    const ProlongPlan p = prolong_plan_of<T>(h, l);
    if (p.nchunk > 65535) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_prolong: slowest extent too long");
    ProlongArgs<T> A{};
    for (int k = 0; k < 3; k++) {
      A.n[k] = (int)b.n[k];
      A.m[k] = (int)b.m[k];
      A.ratio[k] = t.ratio[k];
    }
    A.coarse = coarse;
    A.fine = l == L ? out : ds->nodal[l];
    A.fJ = l == L ? ds->full_J : (size_t)b.n[2];
    A.fI = l == L ? ds->full_I : (size_t)b.n[1] * b.n[2];
    A.gxm = p.gxm;
    A.rch = p.rch;
    A.nchunk = p.nchunk;
    if (p.TC == 64) TRY((launch_prolong3_t<T, 64, 4>(h, A, st)));
    else TRY((launch_prolong3_t<T, 4, 64>(h, A, st)));
    coarse = A.fine;
  }
  return MGH_SUCCESS;
}

// Every other shape: the level loops the full calls run, from level + 1 on, over coefficients that
// are all zero. Full-sized (a memset and every pass of the finest levels), there so that the call
// means the same on every shape.
template <typename T>
int prolong_fallback(mgh_hierarchy *h, int level, const T *lvl, T *out, hipStream_t st) {
  auto *ds = DS<T>(h);
  auto *hh = HH<T>(h);
  const int D = h->D, L = h->L;
  if (D > 3 || h->force_nd) {
    // the generic N-D loop works in place: zero coefficients, the level's nodal values in its
    // corner box (in the reordered layout the corner box of a level IS its nodal array)
    HIP_TRY(hipMemsetAsync(out, 0, h->total * sizeof(T), st));
    size_t ms[MGH_MAX_DIM], fs[MGH_MAX_DIM];
    uint64_t m5[MGH_MAX_DIM], n5[MGH_MAX_DIM];
    for (int k = 0; k < MGH_MAX_DIM; k++) {
      const int d = k - (MGH_MAX_DIM - D);
      m5[k] = d >= 0 ? hh->level_shape[level][d] : 1;
      n5[k] = d >= 0 ? hh->shape[d] : 1;
    }
    compact_strides(MGH_MAX_DIM, m5, ms);
    compact_strides(MGH_MAX_DIM, n5, fs);
    const dim3 blk(64, 4, 1);
    for (uint64_t a = 0; a < m5[0]; a++)
      for (uint64_t b = 0; b < m5[1]; b++) {
        const T *src = lvl + a * ms[0] + b * ms[1];
        T *dst = out + a * fs[0] + b * fs[1];
        TRY(launch(h, "copy_box", st, [&] {
          k_copy_box<T><<<grid3((uint32_t)m5[2], (uint32_t)m5[3], (uint32_t)m5[4], blk), blk, 0, st>>>(
              (uint32_t)m5[2], (uint32_t)m5[3], (uint32_t)m5[4], src, ms[2], ms[3], dst, fs[2], fs[3]);
        }));
      }
    return recompose_nd<T>(h, out, st, -1, level + 1);
  }
  // one thread per element (D <= 3): the node restore reads the coefficients while it writes the
  // output, so the zeros are an array of their own; the level's values go where the loop expects
  // the corrected nodes of level `level`
  TRY(ensure_scratch<T>(h));
  HIP_TRY(hipMemsetAsync(ds->scratch_full, 0, h->total * sizeof(T), st));
  TRY(coarse_in<T>(h, ds->nodal[level], lvl, level, st));
  return recompose_v1_levels<T>(h, ds->scratch_full, ds->full_I, ds->full_J, out, L, st, level + 1);
}

template <typename T>
int prolong_impl(mgh_hierarchy *h, int level, const T *lvl, T *out, hipStream_t st) {
  if (level == h->L) {
    HIP_TRY(hipMemcpyAsync(out, lvl, h->total * sizeof(T), hipMemcpyDeviceToDevice, st));
    return MGH_SUCCESS;
  }
  if (fused_route(h) && h->D == 3) return prolong_fused3<T>(h, level, lvl, out, st);
  return prolong_fallback<T>(h, level, lvl, out, st);
}

// ---- the window form (mgh_prolong_window) -----------------------------------------------------------
template <typename T, int TC, int TF>
int launch_prolong3_win_t(mgh_hierarchy *h, const ProlongWinArgs<T> &A, hipStream_t st) {
  const dim3 grid((unsigned)(A.gxm * ((A.nJ[1] + TC - 1) / TC)), (unsigned)A.nchunk, 1);
  return launch(h, "prolong3_win", st, [&] { k_prolong3_win<T, TC, TF><<<grid, TC * TF, 0, st>>>(A); });
}

// dst (element strides ds[0 .. D), a box of extents ext) <- the box at `lo` of the dense array src of
// extents shape; D <= 5, the two slowest dimensions of the 5-D view on the host as in prolong_fallback
template <typename T>
int copy_window(mgh_hierarchy *h, int D, const uint64_t *shape, const T *src, const uint64_t *lo, const uint64_t *ext,
                T *dst, const uint64_t *dstr, hipStream_t st) {
  uint64_t n5[MGH_MAX_DIM], l5[MGH_MAX_DIM], e5[MGH_MAX_DIM], d5[MGH_MAX_DIM];
  size_t ss[MGH_MAX_DIM];
  for (int k = 0; k < MGH_MAX_DIM; k++) {
    const int d = k - (MGH_MAX_DIM - D);
    n5[k] = d >= 0 ? shape[d] : 1;
    l5[k] = d >= 0 ? lo[d] : 0;
    e5[k] = d >= 0 ? ext[d] : 1;
    d5[k] = d >= 0 ? dstr[d] : 0;
  }
  compact_strides(MGH_MAX_DIM, n5, ss);
  const dim3 blk(64, 4, 1);
  for (uint64_t a = 0; a < e5[0]; a++)
    for (uint64_t b = 0; b < e5[1]; b++) {
      const T *sp = src + (l5[0] + a) * ss[0] + (l5[1] + b) * ss[1] + l5[2] * ss[2] + l5[3] * ss[3] + l5[4];
      T *dp = dst + a * d5[0] + b * d5[1];
      TRY(launch(h, "copy_box", st, [&] {
        k_copy_box<T><<<grid3((uint32_t)e5[2], (uint32_t)e5[3], (uint32_t)e5[4], blk), blk, 0, st>>>(
            (uint32_t)e5[2], (uint32_t)e5[3], (uint32_t)e5[4], sp, ss[2], ss[3], dp, (size_t)d5[2], (size_t)d5[3]);
      }));
    }
  return MGH_SUCCESS;
}

// Fused 3-D route: one launch per level level + 1 .. l_target over the cells under the window. The
// first reads the caller's level array in place, the last writes the box of `out`; in between the
// window's part of a level lives in ds->win[l & 1].
template <typename T>
int prolong_window_fused3(mgh_hierarchy *h, int level, const T *lvl, const std::vector<int64_t> &chain, T *out,
                          const uint64_t *ostr, hipStream_t st) {
  auto *ds = DS<T>(h);
  auto *hh = HH<T>(h);
  const int L = h->L;
  auto range = [&](int l, int k, int64_t *a, int64_t *b) {
    *a = chain[(size_t)(l - level) * 6 + 2 * k];
    *b = chain[(size_t)(l - level) * 6 + 2 * k + 1];
  };
  for (int l = level + 1; l < L; l++) {
    size_t cnt = 1;
    for (int k = 0; k < 3; k++) {
      int64_t a, b;
      range(l, k, &a, &b);
      cnt *= (size_t)(b - a + 1);
    }
    TRY(grow(h, &ds->win[l & 1], &ds->win_elems[l & 1], cnt));
  }
  const T *src = lvl;
  size_t sI = (size_t)(hh->level_shape[level][1] * hh->level_shape[level][2]), sJ = (size_t)hh->level_shape[level][2];
  {
    int64_t a[3], b[3];
    for (int k = 0; k < 3; k++) range(level, k, &a[k], &b[k]);
    src += (size_t)a[0] * sI + (size_t)a[1] * sJ + (size_t)a[2];
  }
  for (int l = level + 1; l <= L; l++) {
    const LevelTables<T> &t = ds->lt[l];
    int64_t ca[3], cb[3], fa[3], fb[3];
    for (int k = 0; k < 3; k++) {
      range(l - 1, k, &ca[k], &cb[k]);
      range(l, k, &fa[k], &fb[k]);
    }
    const ProlongWinPlan w = prolong_window_plan(t.box.n, fa, fb, h->fused.tall != 0);
    if (w.p.nchunk > 65535) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_prolong_window: slowest extent too long");
    ProlongWinArgs<T> A{};
    for (int k = 0; k < 3; k++) {
      A.n[k] = (int)t.box.n[k];
      A.m[k] = (int)t.box.m[k];
      A.ratio[k] = t.ratio[k];
      A.c0[k] = (int)ca[k];
      A.sm[k] = (int)(cb[k] - ca[k] + 1);
      A.d0[k] = (int)fa[k];
      A.dn[k] = (int)(fb[k] - fa[k] + 1);
      A.J0[k] = w.J0[k];
      A.nJ[k] = w.nJ[k];
    }
    A.src = src;
    A.sI = sI;
    A.sJ = sJ;
    A.dst = l == L ? out : ds->win[l & 1];
    A.dI = l == L ? (size_t)ostr[0] : (size_t)A.dn[1] * A.dn[2];
    A.dJ = l == L ? (size_t)ostr[1] : (size_t)A.dn[2];
    A.gxm = w.p.gxm;
    A.rch = w.p.rch;
    A.nchunk = w.p.nchunk;
    if (w.p.TC == 64) TRY((launch_prolong3_win_t<T, 64, 4>(h, A, st)));
    else TRY((launch_prolong3_win_t<T, 4, 64>(h, A, st)));
    src = A.dst;
    sI = A.dI;
    sJ = A.dJ;
  }
  return MGH_SUCCESS;
}

// out_stride == nullptr: dense in ext. On the fused 3-D route the fastest stride must be 1.
template <typename T>
int prolong_window_impl(mgh_hierarchy *h, int level, const T *lvl, const uint64_t *lo, const uint64_t *ext, T *out,
                        const uint64_t *out_stride, hipStream_t st) {
  auto *ds = DS<T>(h);
  auto *hh = HH<T>(h);
  const int D = h->D;
  std::vector<int64_t> chain;
  if (!prolong_window_chain(hh->level_shape, level, lo, ext, chain))
    return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_prolong_window: level or window outside the hierarchy");
  uint64_t ostr[MGH_MAX_DIM];
  if (out_stride) std::copy(out_stride, out_stride + D, ostr);
  else compact_strides(D, ext, ostr);
  if (ostr[D - 1] != 1) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_prolong_window: the fastest stride must be 1");
  if (level == h->L) return copy_window<T>(h, D, hh->shape, lvl, lo, ext, out, ostr, st);
  if (fused_route(h) && D == 3) return prolong_window_fused3<T>(h, level, lvl, chain, out, ostr, st);
  // every other shape: the full call into an array of the hierarchy, and the window cut from it
  TRY(grow(h, &ds->win_full, &ds->win_full_elems, (size_t)h->total));
  TRY(prolong_impl<T>(h, level, lvl, ds->win_full, st));
  return copy_window<T>(h, D, hh->shape, ds->win_full, lo, ext, out, ostr, st);
}

// ---- kernels on pitched arrays (Layout::view) ----------------------------------------------------
// (ld_row_offset: ld_view.hpp)
// dense <-> pitched, one wave per row
template <typename T>
__global__ void __launch_bounds__(256) k_ld_copy(T *__restrict__ dense, T *__restrict__ pitched, LdView V, int to_dense) {
  const int lane = threadIdx.x & 63;
  const uint32_t nf = V.ext[MGH_MAX_DIM - 1];
  for (uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < V.rows; row += (uint64_t)gridDim.x * 4) {
    T *p = pitched + ld_row_offset(V, row);
    T *d = dense + row * nf;
    if (to_dense)
      for (uint32_t k = lane; k < nf; k += 64) d[k] = p[k];
    else
      for (uint32_t k = lane; k < nf; k += 64) p[k] = d[k];
  }
}
// the norm reductions over the rows of a pitched array (same accumulation into `out` as k_absmax / k_sqsum)
template <typename T, bool SQ>
__global__ void __launch_bounds__(256) k_norm_ld(const T *__restrict__ v, LdView V, unsigned long long *out) {
  const int lane = threadIdx.x & 63;
  const uint32_t nf = V.ext[MGH_MAX_DIM - 1];
  T acc = 0;
  for (uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < V.rows; row += (uint64_t)gridDim.x * 4) {
    const T *p = v + ld_row_offset(V, row);
    for (uint32_t k = lane; k < nf; k += 64) {
      const T x = p[k];
      if (SQ) {
        acc += x * x;
      } else {
        const T a = abs_t(x);
        acc = a > acc ? a : acc;
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const T o = __shfl_down(acc, off, 64);
    if (SQ) acc += o; else acc = o > acc ? o : acc;
  }
  if (lane == 0) {
    if (SQ) {
      atomicAdd(reinterpret_cast<double *>(out), (double)acc);
    } else if (sizeof(T) == 4) {
      atomicMax(out, (unsigned long long)__float_as_uint((float)acc));
    } else {
      atomicMax(out, (unsigned long long)__double_as_longlong((double)acc));
    }
  }
}
inline unsigned ld_grid(const LdView &V) { return (unsigned)std::min<uint64_t>((V.rows + 3) / 4, 256 * 32); }

// The norm reduction of `data` (dense, or pitched with the strides of `view`) accumulated into `slot`.
template <typename T>
int norm_reduce(mgh_hierarchy *h, const T *data, double s, unsigned long long *slot, const LdView *view,
                size_t n_cold, hipStream_t st) {
  const bool inf = (T)s == std::numeric_limits<T>::infinity();
  if (view) {
    if (inf) return launch(h, "absmax", st, [&] { k_norm_ld<T, false><<<ld_grid(*view), 256, 0, st>>>(data, *view, slot); });
    return launch(h, "sqsum", st, [&] { k_norm_ld<T, true><<<ld_grid(*view), 256, 0, st>>>(data, *view, slot); });
  }
  const size_t total = h->total;
  const unsigned grid = (unsigned)std::min<size_t>((total + 1023) / 1024, 256 * 8);
  if (inf) return launch(h, "absmax", st, [&] { k_absmax<T><<<grid, 256, 0, st>>>(data, total, slot, n_cold); });
  return launch(h, "sqsum", st, [&] { k_sqsum<T><<<grid, 256, 0, st>>>(data, total, (double *)slot, n_cold); });
}

// Launch the norm reduction (any layout: a pitched array row by row); the result stays in
// ds->scalar (absmax bits or double sum).
template <typename T> int norm_launch(mgh_hierarchy *h, const T *data, const Layout &in, double s, hipStream_t st) {
  auto *ds = DS<T>(h);
  HIP_TRY(hipMemsetAsync(ds->scalar, 0, 8, st));
  return norm_reduce<T>(h, data, s, ds->scalar, in.pitched ? &in.view : nullptr, 0, st);
}

// Quantizer table on the device from a device-resident norm (no host round trip).
template <typename T>
int fill_qparam_args(mgh_hierarchy *h, const T *d_norm, int ebtype, double tol, double s,
                     int decomposed, uint64_t nsub, uint64_t *reset_count, QParamArgs<T> &P) {
  auto *ds = DS<T>(h);
  auto *hh = HH<T>(h);
  if (h->L + 1 > kMaxLevels) return fail(MGH_ERR_INVALID_ARGUMENT, "too many levels");
  P = QParamArgs<T>{};
  P.d_norm = d_norm;
  P.scalar = ds->scalar;
  P.s_is_inf = ((T)s == std::numeric_limits<T>::infinity()) ? 1 : 0;
  P.rel = ebtype == MGH_REL ? 1 : 0;
  P.decomposed = decomposed;
  P.normalize = hh->normalize_coordinates ? 1 : 0;
  P.total = h->total;
  P.nsub = nsub;
  P.tol = (T)tol;
  P.nlev = h->L + 1;
  hh->quantizer_denominators((T)s, P.den);
  for (int l = 0; l <= h->L; l++) P.vol[l] = P.s_is_inf ? (T)1 : hh->level_volume(l, false);
  P.qp = ds->qz;
  P.norm_out = ds->normval;
  P.reset_count = (unsigned long long *)reset_count;
  return MGH_SUCCESS;
}

template <typename T>
int make_qparams_launch(mgh_hierarchy *h, const T *d_norm, int ebtype, double tol, double s,
                        int decomposed, uint64_t nsub, uint64_t *reset_count, hipStream_t st) {
  QParamArgs<T> P;
  TRY(fill_qparam_args<T>(h, d_norm, ebtype, tol, s, decomposed, nsub, reset_count, P));
  return launch(h, "make_qparams", st, [&] { k_make_qparams<T><<<1, 64, 0, st>>>(P); });
}

template <typename T>
int norm_impl(mgh_hierarchy *h, const T *data, const Layout &in, double s, double *out, hipStream_t st) {
  auto *ds = DS<T>(h);
  auto *hh = HH<T>(h);
  const size_t total = h->total;
  TRY(norm_launch<T>(h, data, in, s, st));
  T norm;
  if ((T)s == std::numeric_limits<T>::infinity()) {
    unsigned long long bits = 0;
    HIP_TRY(hipMemcpyAsync(&bits, ds->scalar, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (sizeof(T) == 4) {
      uint32_t b32 = (uint32_t)bits;
      float f;
      std::memcpy(&f, &b32, 4);
      norm = (T)f;
    } else {
      double d;
      std::memcpy(&d, &bits, 8);
      norm = (T)d;
    }
  } else {
    double sum = 0;
    HIP_TRY(hipMemcpyAsync(&sum, ds->scalar, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    norm = (T)sum;
    // NormCalculator.hpp:62-66
    norm = hh->normalize_coordinates ? std::sqrt(norm / (T)total) : std::sqrt(norm);
  }
  if (norm == 0) norm = std::numeric_limits<T>::epsilon();
  *out = (double)norm;
  return MGH_SUCCESS;
}

template <typename T>
int64_t table_impl(const mgh_hierarchy *h, int kind, int level, int dim, void *out, uint64_t cap) {
  auto *hh = HH<T>(h);
  if (dim < 0 || dim >= hh->D) return fail(MGH_ERR_INVALID_ARGUMENT, "dim");
  if (kind == 4) {
    const auto &m = hh->marks[dim];
    if (cap < m.size()) return fail(MGH_ERR_INVALID_ARGUMENT, "capacity");
    std::memcpy(out, m.data(), m.size() * sizeof(int));
    return (int64_t)m.size();
  }
  if (level < 0 || level > hh->L) return fail(MGH_ERR_INVALID_ARGUMENT, "level");
  const auto &q = hh->lv[level][dim];
  const std::vector<T> *v = kind == 0 ? &q.dist : kind == 1 ? &q.ratio : kind == 2 ? &q.am
                            : kind == 3 ? &q.bm : nullptr;
  if (!v) return fail(MGH_ERR_INVALID_ARGUMENT, "kind");
  if (cap < v->size()) return fail(MGH_ERR_INVALID_ARGUMENT, "capacity");
  std::memcpy(out, v->data(), v->size() * sizeof(T));
  return (int64_t)v->size();
}

// Dense view of a pitched array for the paths that do not take strides. ld_pack: the input copied
// into a dense buffer of the hierarchy (p then points there, and `lay` says so); LdOut: the kernels
// write a dense buffer, finish() spreads it into the caller's pitched array. native_ok: the callee
// runs the fused 3-D kernels, which take a Layout::native3 array as it is. Dense arrays pay nothing.
template <typename T> int ld_pack(mgh_hierarchy *h, const T *&p, Layout &lay, bool native_ok, hipStream_t st) {
  if (!lay.pitched || (native_ok && lay.native3)) return MGH_SUCCESS;
  auto *ds = DS<T>(h);
  if (!ds->pack_in) TRY(dev_alloc(h, &ds->pack_in, (size_t)h->total));
  const LdView V = lay.view;
  TRY(launch(h, "ld_pack", st, [&] { k_ld_copy<T><<<ld_grid(V), 256, 0, st>>>(ds->pack_in, const_cast<T *>(p), V, 1); }));
  p = ds->pack_in;
  lay = dense_layout(h);
  return MGH_SUCCESS;
}
template <typename T> struct LdOut {
  T *user = nullptr;
  LdView view{};
  int begin(mgh_hierarchy *h, T *&p, Layout &lay, bool native_ok) {  // (p == nullptr: no such argument)
    if (!p || !lay.pitched || (native_ok && lay.native3)) return MGH_SUCCESS;
    auto *ds = DS<T>(h);
    if (!ds->pack_out) TRY(dev_alloc(h, &ds->pack_out, (size_t)h->total));
    user = p;
    view = lay.view;
    p = ds->pack_out;
    lay = dense_layout(h);
    return MGH_SUCCESS;
  }
  int finish(mgh_hierarchy *h, hipStream_t st) {
    if (!user) return MGH_SUCCESS;
    auto *ds = DS<T>(h);
    return launch(h, "ld_unpack", st, [&] { k_ld_copy<T><<<ld_grid(view), 256, 0, st>>>(ds->pack_out, user, view, 0); });
  }
};

// ---- what a decomposition + quantization reads and makes: the descriptors of decompose_quantize()
// below (QuantOut, the integers: beside QuantParams) --------------------------------------------------
// The error bound.
struct Bound {
  int ebtype;
  double tol, s;
};

// The norm a REL bound is relative to.
struct NormSource {
  enum Kind {
    None,    // ABS bound: none involved
    Host,    // host: given by the caller (> 0)
    Device,  // device: the caller's pointer (T), never read on the host
    Compute  // REL without a norm: reduced here, or taken from the streamed slot (mgh_norm_stream_*)
  } kind;
  double host;
  const void *device;
  int decomposed;      // Device: the norm of a decomposed domain of nsub subdomains (a global norm)
  uint64_t nsub;
  double *h_norm_out;  // or NULL: the norm that was used (Compute: one synchronisation at the end)
};

// Where the coefficients go as well, if anywhere (coeff == nullptr: nowhere).
struct CoeffOut {
  void *coeff;
  Layout lay;
};

inline int outlier_args(const QuantOut &qo) {
  if (qo.prep_huffman && (!qo.ocount || (qo.ocap && (!qo.oidx || !qo.oval))))
    return fail(MGH_ERR_INVALID_ARGUMENT, "outlier buffers required with prep_huffman");
  return MGH_SUCCESS;
}

// ---- the stages on arrays of any layout ---------------------------------------------------------
template <typename T>
int decompose_impl(mgh_hierarchy *h, const T *data, Layout in, T *coeff, Layout out, hipStream_t st) {
  TRY(ld_pack<T>(h, data, in, false, st));
  LdOut<T> o;
  TRY(o.begin(h, coeff, out, false));
  TRY(decompose_dense<T>(h, data, coeff, st));
  return o.finish(h, st);
}

template <typename T>
int recompose_impl(mgh_hierarchy *h, const T *coeff, Layout in, T *data, Layout out, hipStream_t st) {
  TRY(ld_pack<T>(h, coeff, in, false, st));
  LdOut<T> o;
  TRY(o.begin(h, data, out, false));
  TRY(recompose_dense<T>(h, coeff, data, st));
  return o.finish(h, st);
}

// (the integers are always dense)
template <typename T>
int quantize_impl(mgh_hierarchy *h, const T *coeff, Layout in, const Bound &b, double norm, const QuantOut &qo,
                  hipStream_t st) {
  TRY(ld_pack<T>(h, coeff, in, false, st));
  TRY(upload_quantizers<T>(h, b.ebtype, b.tol, b.s, norm, true, st));
  return quantize_launch<T>(h, coeff, qo, st);
}

template <typename T>
int dequantize_impl(mgh_hierarchy *h, int64_t *q, const QuantSpec &qs, T *coeff, Layout out, hipStream_t st) {
  LdOut<T> o;
  TRY(o.begin(h, coeff, out, false));
  TRY(dequantize_dense<T>(h, q, qs, coeff, st));
  return o.finish(h, st);
}

// ---- the streaming quantizer passes (kernels_qwalk.hpp) ---------------------------------------------
// Their grid: persistent workgroups of `threads`, one vector of `vn` elements per thread and trip, as
// many per compute unit as its LDS holds beside the static tables with `lds` dynamic bytes each, `cap` at
// most; they stride over the rest. The kernels stage the level tables in LDS rows of kMaxLevels.
inline int stream_grid(mgh_hierarchy *h, int threads, int vn, size_t lds, size_t cap, unsigned *grid) {
  if (h->L + 1 > kMaxLevels) return fail(MGH_ERR_INVALID_ARGUMENT, "too many levels");
  const size_t per_cu = std::max<size_t>(1, std::min<size_t>(cap, kLdsPerCU / (lds + 4096)));
  const size_t per_wg = (size_t)threads * vn;
  *grid = (unsigned)std::min<size_t>((h->total + per_wg - 1) / per_wg, per_cu * h->num_cu);
  return MGH_SUCCESS;
}

// Level tables made by the host code of upload_quantizers (the volumes depend on s only), one row of
// L + 1 values per entry of `rows` -- which table (QTab) and for what tolerance -- side by side in *buf.
// `qm`: the hierarchy's quantizer metadata for this s.
struct QRow {
  QTab tab;
  double tol;
};

template <typename T>
int upload_level_rows(mgh_hierarchy *h, int ebtype, double s, double norm, const std::vector<QRow> &rows, T **buf,
                      size_t *buf_elems, QuantMeta &qm, hipStream_t st) {
  auto *hh = HH<T>(h);
  const int nlev = h->L + 1;
  const bool calc_vol = !((T)s == std::numeric_limits<T>::infinity());
  std::vector<T> tab(rows.size() * nlev);
  for (size_t r = 0; r < rows.size(); r++) {
    T *row = tab.data() + r * nlev;
    const bool dequant = rows[r].tab == kTabQz || rows[r].tab == kTabDvol;
    if (rows[r].tab == kTabRqz || rows[r].tab == kTabQz)
      hh->quantizers(ebtype, (T)rows[r].tol, (T)s, (T)norm, !dequant, row);
    else
      for (int l = 0; l < nlev; l++) row[l] = calc_vol ? hh->level_volume(l, dequant) : (T)1;
  }
  TRY(grow(h, buf, buf_elems, tab.size()));
  // pageable-memory async copies are staged by the runtime before returning
  HIP_TRY(hipMemcpyAsync(*buf, tab.data(), tab.size() * sizeof(T), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  qm = DS<T>(h)->qmeta;
  qm.calc_vol = calc_vol ? 1 : 0;
  return MGH_SUCCESS;
}

// mgh_quantize_histograms: the reciprocal quantizers of every tolerance and one row of volumes in
// ds->qh_tab, then the launches size_plan.hpp splits the tolerances into.
template <typename T, int K>
int qhist_launch(mgh_hierarchy *h, const QuantMeta &qm, const T *coeff, const T *qz, const T *vol, uint64_t dict,
                 uint32_t *freq, uint64_t *outliers, hipStream_t st) {
  static std::atomic<uint64_t> once{0};
  const size_t lds = (size_t)K * dict * 4;
  TRY(allow_big_lds_once(k_quantize_histograms<T, K>, once, kQhistLdsBytes));
  unsigned grid;
  TRY(stream_grid(h, kQhThreads, Vec16<T>::N, lds, 4, &grid));
  return launch(h, "quantize_histograms", st, [&] {
    k_quantize_histograms<T, K><<<grid, kQhThreads, lds, st>>>(qm, h->total, coeff, DS<T>(h)->marks, qz, vol, h->L + 1,
                                                              (int)dict, freq, (unsigned long long *)outliers);
  });
}

template <typename T>
int quantize_histograms_impl(mgh_hierarchy *h, const T *coeff, Layout in, int ebtype, int ntol, const double *tols,
                             double s, double norm, uint64_t dict, uint32_t *freq, uint64_t *outliers, hipStream_t st) {
  auto *ds = DS<T>(h);
  const int nlev = h->L + 1;
  TRY(ld_pack<T>(h, coeff, in, false, st));
  std::vector<QRow> rows;
  for (int k = 0; k < ntol; k++) rows.push_back({kTabRqz, tols[k]});
  rows.push_back({kTabQvol, 0});
  QuantMeta qm;
  TRY(upload_level_rows<T>(h, ebtype, s, norm, rows, &ds->qh_tab, &ds->qh_tab_elems, qm, st));
  HIP_TRY(hipMemsetAsync(freq, 0, (size_t)ntol * dict * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(outliers, 0, (size_t)ntol * sizeof(uint64_t), st));
  const T *vol = ds->qh_tab + (size_t)ntol * nlev;
  for (int k0 = 0; k0 < ntol;) {
    const int kk = qhist_per_launch(dict, ntol - k0);
    if (kk < 1) return fail(MGH_ERR_INVALID_ARGUMENT, "quantize_histograms: dict_size");
    TRY((with_value<1, 2, 3, 4, 5, 6, 7, 8>(kk, [&](auto K) {
      return qhist_launch<T, decltype(K)::value>(h, qm, coeff, ds->qh_tab + (size_t)k0 * nlev, vol, dict,
                                                 freq + (size_t)k0 * dict, outliers + k0, st);
    })));
    k0 += kk;
  }
  return MGH_SUCCESS;
}

// The table of mgh_quantize (upload_quantizers, reciprocal) and the table of mgh_dequantize
// (upload_quantizers, not reciprocal) side by side in ds->qr_tab, in the order of QTab: what the kernels
// that quantize and dequantize in one pass read (k_quantize_roundtrip, k_quantize_symbols_residual).
template <typename T>
int upload_roundtrip_tables(mgh_hierarchy *h, const Bound &b, double norm, QuantMeta &qm, hipStream_t st) {
  auto *ds = DS<T>(h);
  const std::vector<QRow> rows{{kTabRqz, b.tol}, {kTabQvol, b.tol}, {kTabQz, b.tol}, {kTabDvol, b.tol}};
  return upload_level_rows<T>(h, b.ebtype, b.s, norm, rows, &ds->qr_tab, &ds->qr_tab_elems, qm, st);
}

// mgh_quantize_roundtrip: the four tables, then one streaming launch, at most eight workgroups per
// compute unit. The output is dense.
template <typename T>
int quantize_roundtrip_impl(mgh_hierarchy *h, const T *coeff, Layout in, const Bound &b, double norm, T *out,
                            hipStream_t st) {
  auto *ds = DS<T>(h);
  unsigned grid;
  TRY(stream_grid(h, kQrThreads, Vec16<T>::N, 0, 8, &grid));
  TRY(ld_pack<T>(h, coeff, in, false, st));
  QuantMeta qm;
  TRY(upload_roundtrip_tables<T>(h, b, norm, qm, st));
  return launch(h, "quantize_roundtrip", st, [&] {
    k_quantize_roundtrip<T><<<grid, kQrThreads, 0, st>>>(qm, h->total, coeff, ds->marks, ds->qr_tab, h->L + 1, out);
  });
}

// One launch of k_quantize_symbols, or with RES of k_quantize_symbols_residual, on tables that are
// uploaded: eight workgroups per compute unit for the plain stream, as many as the LDS holds beside the
// static tables with the bins. The caller has zeroed the counter and the bins.
template <typename T, bool RES>
int qsym_launch(mgh_hierarchy *h, const QuantMeta &qm, const T *coeff, const T *tab, uint64_t dict, uint16_t *sym,
                uint32_t *freq, const QuantOut &qo, T *residual, hipStream_t st) {
  const size_t lds = freq ? (size_t)dict * 4 : 0;
  unsigned grid;
  TRY(stream_grid(h, kQsThreads, Vec16<T>::N, lds, 8, &grid));
  return with_value<0, 1>(freq ? 1 : 0, [&](auto hist) {
    constexpr bool HIST = decltype(hist)::value != 0;
    auto count = (unsigned long long *)qo.ocount;
    const auto cap = (unsigned long long)qo.ocap;
    if constexpr (HIST) {
      static std::atomic<uint64_t> once{0};
      if constexpr (RES)
        TRY(allow_big_lds_once(k_quantize_symbols_residual<T, true>, once, kQsymLdsBytes));
      else
        TRY(allow_big_lds_once(k_quantize_symbols<T, true>, once, kQsymLdsBytes));
    }
    return launch(h, RES ? "quantize_symbols_residual" : "quantize_symbols", st, [&] {
      if constexpr (RES)
        k_quantize_symbols_residual<T, HIST><<<grid, kQsThreads, lds, st>>>(
            qm, h->total, coeff, DS<T>(h)->marks, tab, h->L + 1, (int)dict, sym, freq, count, qo.oidx, qo.oval, cap, residual);
      else
        k_quantize_symbols<T, HIST><<<grid, kQsThreads, lds, st>>>(
            qm, h->total, coeff, DS<T>(h)->marks, tab, h->L + 1, (int)dict, sym, freq, count, qo.oidx, qo.oval, cap);
    });
  });
}

// mgh_quantize_symbols: the table of mgh_quantize by its own upload (upload_quantizers, reciprocal).
template <typename T>
int quantize_symbols_impl(mgh_hierarchy *h, const T *coeff, Layout in, const Bound &b, double norm, uint64_t dict,
                          uint16_t *sym, uint32_t *freq, const QuantOut &qo, hipStream_t st) {
  auto *ds = DS<T>(h);
  TRY(ld_pack<T>(h, coeff, in, false, st));
  TRY(upload_quantizers<T>(h, b.ebtype, b.tol, b.s, norm, true, st));
  return qsym_launch<T, false>(h, ds->qmeta, coeff, ds->qz, dict, sym, freq, qo, nullptr, st);
}

// mgh_quantize_symbols_residual: the four tables of the round trip. The residual is dense.
template <typename T>
int quantize_symbols_residual_impl(mgh_hierarchy *h, const T *coeff, Layout in, const Bound &b, double norm,
                                   uint64_t dict, uint16_t *sym, uint32_t *freq, const QuantOut &qo, T *residual,
                                   hipStream_t st) {
  TRY(ld_pack<T>(h, coeff, in, false, st));
  QuantMeta qm;
  TRY(upload_roundtrip_tables<T>(h, b, norm, qm, st));
  return qsym_launch<T, true>(h, qm, coeff, DS<T>(h)->qr_tab, dict, sym, freq, qo, residual, st);
}

// mgh_dequantize_add: the table of mgh_dequantize by its own upload, the outliers back into the integers
// (dequantize_dense's step), then one streaming launch of k_dequantize_add on the dense accumulator.
template <typename T>
int dequantize_add_impl(mgh_hierarchy *h, int64_t *q, const QuantSpec &qs, bool first, T *acc, hipStream_t st) {
  auto *ds = DS<T>(h);
  unsigned grid;
  TRY(stream_grid(h, kQaThreads, Vec16<T>::N, 0, 8, &grid));
  TRY(upload_quantizers<T>(h, qs.ebtype, qs.tol, qs.s, qs.norm, false, st));
  TRY(outliers_back(h, qs, "outlier_restore", st, k_outlier_restore, q, h->total));
  const size_t total = h->total;
  const int nlev = h->L + 1;
  const int64_t shift = qs.prep_huffman ? (int64_t)qs.dict_size / 2 : 0;
  return launch(h, "dequantize_add", st, [&] {
    if (first)
      k_dequantize_add<T, true><<<grid, kQaThreads, 0, st>>>(ds->qmeta, total, q, ds->marks, ds->qz, nlev, shift, acc);
    else
      k_dequantize_add<T, false><<<grid, kQaThreads, 0, st>>>(ds->qmeta, total, q, ds->marks, ds->qz, nlev, shift, acc);
  });
}

// The norm k_make_qparams left in ds->normval, on the host: one synchronisation.
template <typename T> int read_back_norm(mgh_hierarchy *h, double *out, hipStream_t st) {
  T nv = 0;
  HIP_TRY(hipMemcpyAsync(&nv, DS<T>(h)->normval, sizeof(T), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *out = (double)nv;
  return MGH_SUCCESS;
}

// ---- the decomposition + quantization core --------------------------------------------------------
// Everything behind mgh_decompose_quantize{,_sym16,_dn}: `data` to the integers `qo` within `b`, the
// coefficients to `co` as well if wanted. The route:
//   - no coefficient output, a shape the fused level kernels take, dict_size <= 2^30 (they test the
//     dictionary range in 32 bits): one fused pass;
//   - else staged on dense arrays: the coefficients go to `co` (through a dense copy if it is pitched)
//     or to scratch_full, and the quantizer reads them there.
// The quantizer table: built on the host from a norm the host has (none, or given) for the int64
// output; made on the device by k_make_qparams when the norm is there (computed here, the caller's
// pointer) and for 16-bit symbols (a given norm is uploaded first) -- no host round trip inside the
// call, ns.h_norm_out costs one synchronisation at the END (mgh_norm + mgh_quantize were two round
// trips, 35 us each on the 5-D step).
template <typename T>
int decompose_quantize(mgh_hierarchy *h, const T *data, Layout in, const Bound &b, const NormSource &ns,
                       const QuantOut &qo, const CoeffOut &co, hipStream_t st) {
  auto *ds = DS<T>(h);
  const bool inf = (T)b.s == std::numeric_limits<T>::infinity();
  TRY(outlier_args(qo));
  if (qo.sym16 && (qo.dict_size == 0 || qo.dict_size > 65536))
    return fail(MGH_ERR_INVALID_ARGUMENT, "dict_size must be in 1..65536");
  if (qo.sym16 && !fused_route(h))
    return fail(MGH_ERR_UNSUPPORTED_DIMENSION, "16-bit symbols: only on the fused 3-D / 4-D path");
  if (ns.kind == NormSource::Device && !fused_route(h))
    return fail(MGH_ERR_UNSUPPORTED_DIMENSION, "device-norm entry point needs the fused 3-D / 4-D path");
  const bool fused = !co.coeff && fused_route(h) && qo.dict_size <= ((uint64_t)1 << 30);
  if (ns.kind == NormSource::Device && !fused)
    return fail(MGH_ERR_INVALID_ARGUMENT, "fused path: dict_size must be at most 2^30");
  // mgh_norm_stream_*: the reduction is in the slot already, for a fused call that would reduce by
  // itself. Any other call drops it (fscal_dirty stays set: the next fused call zeroes the slots).
  const bool streamed = ds->norm_streamed && fused && ns.kind == NormSource::Compute;
  ds->norm_streamed = false;
  const bool device_table = ns.kind == NormSource::Compute || ns.kind == NormSource::Device || qo.sym16;
  if (ns.kind != NormSource::Compute && ns.h_norm_out) *ns.h_norm_out = ns.host;  // (given, or none involved)

  if (fused) {
    TRY(ld_pack<T>(h, data, in, true, st));
    QuantParams<T> qp;
    qp.out = qo;
    const T *d_norm = (const T *)ns.device;
    unsigned long long *slot = nullptr, *other = nullptr;
    if (!device_table) {
      if (qo.ocount) HIP_TRY(hipMemsetAsync(qo.ocount, 0, sizeof(uint64_t), st));  // (else k_make_qparams does it)
      host_quant_table<T>(h, b.ebtype, b.tol, b.s, ns.host, qp);
    } else {
      if (ns.kind == NormSource::Host) {
        const T nv = (T)ns.host;
        HIP_TRY(hipMemcpyAsync(ds->normval, &nv, sizeof(T), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        d_norm = ds->normval;
      }
      qp.d_qp = ds->qz;
      // The norm scalar has two slots used alternately: this call reduces into scalar[slot] (zero on
      // entry) and k_make_qparams zeroes the other one for the next call, together with the outlier
      // counter -- two memset launches less per step.
      if (ds->fscal_dirty && !streamed) HIP_TRY(hipMemsetAsync(ds->fscal, 0, 16, st));
      ds->fscal_dirty = true;
      slot = ds->fscal + ds->scalar_slot;
      other = ds->fscal + (1 - ds->scalar_slot);
    }
    if (ns.kind == NormSource::Compute && !streamed) {
      // all but the last MGH_ABSMAX_WARM_MB of the input with nontemporal loads: the level pass
      // re-reads the input from its end, and only what the norm pass read last can still be in
      // the 256 MB memory-side cache (512^3 f32, same box, 60 steps each: absmax 109 -> 93 us,
      // top-level pass 384 -> 397 us, step 0.894 -> 0.889 ms)
      const size_t total = h->total, warm = ((size_t)h->absmax_warm_mb << 20) / sizeof(T);
      if (in.pitched)  // (read in place: row by row)
        TRY(norm_reduce<T>(h, data, b.s, slot, &in.view, 0, st));
      else
        TRY(norm_reduce<T>(h, data, b.s, slot, nullptr, total > warm ? total - warm : 0, st));
    }
    // (issued right in front of the first launch that reads the table)
    auto table = [&]() -> int {
      if (!device_table) return MGH_SUCCESS;
      QParamArgs<T> P;
      TRY(fill_qparam_args<T>(h, d_norm, b.ebtype, b.tol, b.s, ns.decomposed, ns.nsub, qo.ocount, P));
      P.scalar = slot;
      P.zero_next = other;
      TRY(launch(h, "make_qparams", st, [&] { k_make_qparams<T><<<1, 64, 0, st>>>(P); }));
      ds->scalar_slot = 1 - ds->scalar_slot;
      ds->fscal_dirty = false;
      return MGH_SUCCESS;
    };
    TRY((decompose_fused<T, OUT_Q>(h, data, in, nullptr, &qp, st, table)));
  } else {
    TRY(ld_pack<T>(h, data, in, false, st));
    T *coeff = (T *)co.coeff;
    Layout out = co.lay;
    LdOut<T> o;
    TRY(o.begin(h, coeff, out, false));
    if (!coeff) {
      TRY(ensure_scratch<T>(h));
      coeff = ds->scratch_full;
      if (coeff == data) return fail(MGH_ERR_INVALID_ARGUMENT, "aliasing");
    }
    if (device_table) {
      TRY(norm_launch<T>(h, data, in, b.s, st));
      TRY(make_qparams_launch<T>(h, nullptr, b.ebtype, b.tol, b.s, 0, 1, nullptr, st));
      ds->qmeta.calc_vol = inf ? 0 : 1;
    } else {
      TRY(upload_quantizers<T>(h, b.ebtype, b.tol, b.s, ns.host, true, st));
    }
    TRY(decompose_dense<T>(h, data, coeff, st));
    TRY(quantize_launch<T>(h, coeff, qo, st));
    TRY(o.finish(h, st));
  }
  if (ns.kind == NormSource::Compute && ns.h_norm_out) return read_back_norm<T>(h, ns.h_norm_out, st);
  return MGH_SUCCESS;
}

// the level shapes and level marks the linearisation kernels read (kernels_v1.hpp)
const int *lin_meta(mgh_hierarchy *h, mgh::LinMeta &m) {
  const int *marks = nullptr;
  auto fill = [&](auto *hh, auto *ds) {
    m.D = hh->D;
    m.L = hh->L;
    for (int d = 0; d < hh->D; d++) {
      m.shape[d] = (uint32_t)hh->shape[d];
      m.markoff[d] = ds->qmeta.markoff[d];
      for (int l = 0; l <= hh->L; l++) m.lshape[l][d] = (uint32_t)hh->level_shape[l][d];
    }
    marks = ds->marks;
  };
  if (h->dtype == MGH_FLOAT) fill(HH<float>(h), DS<float>(h));
  else fill(HH<double>(h), DS<double>(h));
  return marks;
}

// What box_from_linear and shell_from_linear share: the level shapes, and the strides of the compact
// box of `level` ...
int lin_box_begin(mgh_hierarchy *h, int level, mgh::LinMeta &m, mgh::LinBox &B) {
  if (h->L + 1 > mgh::kLinMaxLevels + 1) return fail(MGH_ERR_INVALID_ARGUMENT, "too many levels");
  (void)lin_meta(h, m);
  B.level = level;
  compact_strides(h->D, m.lshape[level], B.bs);
  return MGH_SUCCESS;
}
// ... and B.unit0[k + 1]: the units (pieces of rows, one wave each) of a box of extents e behind B.unit0[k]
int lin_box_units(const mgh_hierarchy *h, mgh::LinBox &B, int k, const uint32_t *e, bool none = false) {
  const int D = h->D;
  uint64_t rows = 1;
  for (int d = 0; d < D - 1; d++) rows *= e[d];
  const uint64_t units = none ? 0 : rows * ((e[D - 1] + kLevelBoxPiece - 1) / kLevelBoxPiece);
  if (units >= ((uint64_t)1 << 32)) return fail(MGH_ERR_INVALID_ARGUMENT, "level box too large");
  B.unit0[k + 1] = B.unit0[k] + units;
  return MGH_SUCCESS;
}

// The compact corner box of `level` (dense in level_shape(level)) out of the first N_level integers
// of a level-linearised array: k_box_from_linear, one wave per piece of a run of the stream.
// E: int64_t for 8-byte elements (the integers; double coefficients), int32_t for 4-byte ones (float
// coefficients) -- the permutation moves bits.
template <typename E> int box_from_linear(mgh_hierarchy *h, const E *lin, int level, E *box, hipStream_t st) {
  mgh::LinMeta m{};
  mgh::LinBox B{};
  TRY(lin_box_begin(h, level, m, B));
  for (int j = 0; j <= level; j++) TRY(lin_box_units(h, B, j, m.lshape[j]));
  const unsigned grid = (unsigned)std::min<uint64_t>((B.unit0[level + 1] + 3) / 4, 256 * 32);
  return launch(h, "box_from_linear", st, [&] { mgh::k_box_from_linear<E><<<grid, 256, 0, st>>>(m, B, lin, box); });
}

// mgh_recompose_linear_to_level: the compact box of `level` out of the head of a level-linearised
// COEFFICIENT array (ds->lin_box, N_level elements), then the level loops of mgh_recompose_to_level on it
// with the box's own dense strides -- level == l_target: the box is the whole array in array order, and
// the body is mgh_recompose's.
template <typename T>
int recompose_linear_to_level_impl(mgh_hierarchy *h, const T *lin, int level, T *out, hipStream_t st) {
  auto *ds = DS<T>(h);
  using E = std::conditional_t<sizeof(T) == 8, int64_t, int32_t>;
  TRY(grow(h, &ds->lin_box, &ds->lin_box_elems, (size_t)level_elems(h, level)));
  TRY(box_from_linear<E>(h, reinterpret_cast<const E *>(lin), level, reinterpret_cast<E *>(ds->lin_box), st));
  if (level == h->L) return recompose_impl<T>(h, ds->lin_box, dense_layout(h), out, dense_layout(h), st);
  uint64_t ext[MGH_MAX_DIM];
  for (int d = 0; d < h->D; d++) ext[d] = HH<T>(h)->level_shape[level][d];
  return recompose_to_level_impl<T>(h, ds->lin_box, make_layout(h, ext, false), level, out, st);
}

// The shell of the compact box of `level` (dense in level_shape(level)) out of the level's own segment
// [N_{level-1}, N_level) of a level-linearised array: k_shell_from_linear. fill_inner: the inner box
// of level - 1 gets `inner` (the fused node restore loads those positions).
int shell_from_linear(mgh_hierarchy *h, const int64_t *seg, int level, int64_t *box, bool fill_inner, int64_t inner,
                      hipStream_t st) {
  mgh::LinMeta m{};
  mgh::LinBox B{};
  TRY(lin_box_begin(h, level, m, B));
  for (int k = 0; k < 2; k++)  // the runs of the level; the rows of the inner box
    TRY(lin_box_units(h, B, k, m.lshape[level - k], k == 1 && !fill_inner));
  const unsigned grid = (unsigned)std::min<uint64_t>((B.unit0[2] + 3) / 4, 256 * 32);
  return launch(h, "shell_from_linear", st, [&] { mgh::k_shell_from_linear<<<grid, 256, 0, st>>>(m, B, seg, box, inner); });
}

// ---- precision layers in level order -----------------------------------------
// mgh_quantize_residual_linear: the four tables of the round trip, the int64 instance of the symbol
// kernel into ds->qbox (array order, all of the array), then mgh_level_linearize's two kernels: the
// integers into `lin`, the list's indices in place. The residual is dense, in array order.
template <typename T>
int quantize_residual_linear_impl(mgh_hierarchy *h, const T *coeff, Layout in, const Bound &b, double norm, uint64_t dict,
                                  int64_t *lin, const QuantOut &qo, T *residual, hipStream_t st) {
  auto *ds = DS<T>(h);
  if (h->L + 1 > mgh::kLinMaxLevels + 1) return fail(MGH_ERR_INVALID_ARGUMENT, "too many levels");
  unsigned grid;
  TRY(stream_grid(h, kQsThreads, Vec16<T>::N, 0, 8, &grid));
  TRY(ld_pack<T>(h, coeff, in, false, st));
  QuantMeta qm;
  TRY(upload_roundtrip_tables<T>(h, b, norm, qm, st));
  const size_t total = h->total;
  TRY(grow(h, &ds->qbox, &ds->qbox_elems, total));
  HIP_TRY(hipMemsetAsync(qo.ocount, 0, sizeof(uint64_t), st));
  TRY(launch(h, "quantize_residual_int64", st, [&] {
    k_quantize_residual_int64<T><<<grid, kQsThreads, 0, st>>>(qm, total, coeff, ds->marks, ds->qr_tab, h->L + 1, (int)dict,
                                                              ds->qbox, (unsigned long long *)qo.ocount, qo.oidx, qo.oval,
                                                              (unsigned long long)qo.ocap, residual);
  }));
  mgh::LinMeta m{};
  const int *marks = lin_meta(h, m);
  const unsigned g1 = (unsigned)std::min<size_t>((total + 255) / 256, 256 * 32);
  TRY(launch(h, "level_linearize", st, [&] {
    mgh::k_level_linearize<int64_t, false><<<g1, 256, 0, st>>>(m, marks, total, ds->qbox, lin);
  }));
  if (!qo.ocap) return MGH_SUCCESS;
  const unsigned g2 = (unsigned)std::max<size_t>(1, std::min<size_t>((std::min<size_t>(qo.ocap, total) + 255) / 256, 4096));
  return launch(h, "linearize_indices", st, [&] {
    mgh::k_linearize_indices<<<g2, 256, 0, st>>>(m, marks, total, qo.oidx, (const unsigned long long *)qo.ocount, 0ull,
                                                 (unsigned long long)qo.ocap);
  });
}

// mgh_dequantize_add_linear: the table of mgh_dequantize by its own upload, the outliers of the window
// back into it, then one streaming launch of k_dequantize_add_linear over the window.
template <typename T>
int dequantize_add_linear_impl(mgh_hierarchy *h, int64_t *win, uint64_t first, uint64_t count, const QuantSpec &qs,
                               bool store, T *acc, hipStream_t st) {
  auto *ds = DS<T>(h);
  const int nlev = h->L + 1;
  if (nlev > kMaxLevels) return fail(MGH_ERR_INVALID_ARGUMENT, "too many levels");
  LinOffsets off{};
  for (int l = 0; l < nlev; l++) off.n[l] = (uint32_t)level_elems(h, l);
  const size_t per_wg = (size_t)kQaThreads * Vec16<T>::N;
  const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((count + per_wg - 1) / per_wg, 8 * (size_t)h->num_cu));
  TRY(upload_quantizers<T>(h, qs.ebtype, qs.tol, qs.s, qs.norm, false, st));
  TRY(outliers_back(h, qs, "outlier_restore_window", st, k_outlier_restore_window, win, first, first + count));
  const int64_t shift = qs.prep_huffman ? (int64_t)qs.dict_size / 2 : 0;
  const int calc_vol = ds->qmeta.calc_vol;
  return launch(h, "dequantize_add_linear", st, [&] {
    if (store)
      k_dequantize_add_linear<T, true><<<grid, kQaThreads, 0, st>>>(off, nlev, calc_vol, win, (uint32_t)first, (size_t)count,
                                                                     ds->qz, shift, acc);
    else
      k_dequantize_add_linear<T, false><<<grid, kQaThreads, 0, st>>>(off, nlev, calc_vol, win, (uint32_t)first, (size_t)count,
                                                                      ds->qz, shift, acc);
  });
}

// ---- the reconstruction core ---------------------------------------------------------------------
// Everything behind mgh_dequantize_recompose{,_to_level,_linear_to_level,_sym16,_sym16_to_level} and
// mgh_refine_level: integers `src` with the parameters `qs` to the array `tg`. The route:
//   - the fused level loops (3-D, 4-D) read the integers where they are, with the source's strides;
//   - the other shapes, whole array: dequantizer and recomposition in place on the (dense) output;
//   - the other shapes, a stop level or a level step: the box dequantized into a compact
//     floating-point array, then the one-thread-per-element or N-D levels (recompose_box_to_level).
template <typename T>
int reconstruct(mgh_hierarchy *h, QuantSpec qs, IntSource src, const Target &tg, hipStream_t st) {
  auto *ds = DS<T>(h);
  const int D = h->D, L = h->L, stop = tg.stop, start = tg.start;
  const bool fused = fused_route(h);
  T *out = (T *)tg.out;
  Layout lay = tg.lay;
  LdOut<T> o;
  TRY(o.begin(h, out, lay, fused));
  if (src.kind == IntSource::Sym16) {
    TRY(dequantize_recompose_fused16<T>(h, qs, src.sym, out, lay, st, stop));
    return o.finish(h, st);
  }
  if (src.kind == IntSource::Linear) {
    // outliers at their linearised positions (those behind the head, or outside the segment, are
    // skipped), then the compact box of the stop level in ds->qbox: nothing left to restore
    const uint64_t n = level_elems(h, stop);
    if (start) TRY(outliers_back(h, qs, "outlier_restore_window", st, k_outlier_restore_window, src.q,
                                 level_elems(h, stop - 1), n));
    else TRY(outliers_back(h, qs, "outlier_restore", st, k_outlier_restore, src.q, n));
    TRY(grow(h, &ds->qbox, &ds->qbox_elems, n));
    if (start) TRY(shell_from_linear(h, src.q, stop, ds->qbox, fused, dict_half(qs), st));
    else TRY(box_from_linear(h, src.q, stop, ds->qbox, st));
    src = IntSource{IntSource::Box, ds->qbox, nullptr};
    qs.ocount = 0;
  }
  // (the box of l_target is the full array)
  const bool compact = src.kind == IntSource::Box && stop < L;
  LevelBox lb = level_box_of<T>(h, stop, dense_layout(h));  // what is read of src.q
  if (compact) compact_strides(D, lb.m, lb.ss);
  if (fused) {
    if (stop < L) TRY(outliers_back(h, qs, "outlier_restore", st, k_outlier_restore_in_box, src.q, lb));
    else TRY(outliers_back(h, qs, "outlier_restore", st, k_outlier_restore, src.q, h->total));
    if (start) {
      if (D == 4) TRY(ensure_state4<T>(h));
      TRY(coarse_in<T>(h, D == 4 ? ds->nodal4[start - 1] : ds->nodal[start - 1], tg.coarse, start - 1, st));
    }
    RecomposeArgs<T> A{};
    A.q = src.q;
    A.half = dict_half(qs);
    A.dI = ds->full_I;
    A.dJ = ds->full_J;
    const size_t sT = compact ? box_source(A, D, lb.m) : 0;
    TRY((recompose_levels_any<T, int64_t>(h, A, sT, level_quanta<T>(h, qs), out, lay, st, nullptr, 1, stop, start)));
    return o.finish(h, st);
  }
  if (stop == L && !start) {
    TRY(dequantize_dense<T>(h, src.q, qs, out, st));
    TRY(recompose_dense<T>(h, out, out, st));
    return o.finish(h, st);
  }
  TRY(upload_quantizers<T>(h, qs.ebtype, qs.tol, qs.s, qs.norm, false, st));
  TRY(outliers_back(h, qs, "outlier_restore", st, k_outlier_restore_in_box, src.q, lb));
  if (start)  // (k_box_refine_fill: the inner box is the coarse array, the shell is dequantized)
    for (int d = 0; d < D; d++) lb.n[d] = (uint32_t)HH<T>(h)->level_shape[stop - 1][d];
  const uint64_t rows = level_box_rows(lb);
  const T *coarse = (const T *)tg.coarse;
  return recompose_box_to_level<T>(h, stop, out, st, [&](T *dst) {
    if (start)
      return launch(h, "box_refine_fill", st, [&] {
        k_box_refine_fill<T><<<level_box_grid(lb), 256, 0, st>>>(lb, ds->qmeta, src.q, coarse, ds->marks, ds->qz,
                                                                    ds->qz + (L + 1), (int64_t)qs.dict_size,
                                                                    qs.prep_huffman, dst, rows);
      });
    return launch(h, "box_dequantize", st, [&] {
      k_box_dequantize<T><<<level_box_grid(lb), 256, 0, st>>>(lb, ds->qmeta, src.q, ds->marks, ds->qz,
                                                                 ds->qz + (L + 1), (int64_t)qs.dict_size,
                                                                 qs.prep_huffman, dst, rows);
    });
  }, start, tg.coarse);
}

// Norm accumulated over parts of the input (mgh_norm_stream_begin / _add): the same reduction
// kernels on a range, into the slot the next fused call reads.
template <typename T> int norm_stream_begin(mgh_hierarchy *h, hipStream_t st) {
  auto *ds = DS<T>(h);
  if (ds->fscal_dirty) HIP_TRY(hipMemsetAsync(ds->fscal, 0, 16, st));
  ds->fscal_dirty = true;  // (the slot is in use from here on)
  ds->norm_streamed = true;
  return MGH_SUCCESS;
}
template <typename T>
int norm_stream_add(mgh_hierarchy *h, const T *part, size_t count, double s, int cold, hipStream_t st) {
  auto *ds = DS<T>(h);
  if (!ds->norm_streamed) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_norm_stream_add without mgh_norm_stream_begin");
  if (count == 0) return MGH_SUCCESS;
  unsigned long long *slot = ds->fscal + ds->scalar_slot;
  const unsigned grid = (unsigned)std::min<size_t>((count + 1023) / 1024, 256 * 8);
  if ((T)s == std::numeric_limits<T>::infinity())
    return launch(h, "absmax", st, [&] { k_absmax<T><<<grid, 256, 0, st>>>(part, count, slot, cold ? count : 0); });
  return launch(h, "sqsum", st, [&] { k_sqsum<T><<<grid, 256, 0, st>>>(part, count, (double *)slot, cold ? count : 0); });
}

// mgh_norm_stream_end: the accumulated reduction through k_make_qparams -- the conversion the fused
// call would have run -- and back to the host; the slots are left as that call leaves them.
template <typename T> int norm_stream_end(mgh_hierarchy *h, double s, double *out, hipStream_t st) {
  auto *ds = DS<T>(h);
  if (!ds->norm_streamed) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_norm_stream_end without mgh_norm_stream_begin");
  ds->norm_streamed = false;
  QParamArgs<T> P;
  TRY(fill_qparam_args<T>(h, nullptr, MGH_ABS, 1.0, s, 0, 1, nullptr, P));
  P.scalar = ds->fscal + ds->scalar_slot;
  P.zero_next = ds->fscal + (1 - ds->scalar_slot);
  TRY(launch(h, "make_qparams", st, [&] { k_make_qparams<T><<<1, 64, 0, st>>>(P); }));
  ds->scalar_slot = 1 - ds->scalar_slot;
  ds->fscal_dirty = false;
  return read_back_norm<T>(h, out, st);
}

// The switches as set in the environment (validated by env_validate) on a device of `num_cu` CUs.
// MGH_IPK_PLAN_CU: the CU count the planner plans with instead (a plan is a performance choice:
// every value gives the same bits; a small one puts small boxes on the kernels of the big ones).
inline IpkTuning ipk_tuning_from_env(size_t num_cu) {
  IpkTuning t;
  num_cu = (size_t)env_get("MGH_IPK_PLAN_CU", (long)num_cu);
  t.num_cu = num_cu;
  t.stream = (int)env_get("MGH_IPK_STREAM", t.stream);
  t.dma = (int)env_get("MGH_IPK_DMA", t.dma);
  t.dma_min = (size_t)env_get("MGH_IPK_DMA_MIN", (long)(2 * num_cu));
  t.dma_rounds = (int)env_get("MGH_IPK_DMA_ROUNDS", t.dma_rounds);
  t.spec = (int)env_get("MGH_IPK_SPEC", t.spec);
  t.spec_k = (int)env_get("MGH_IPK_SPEC_K", t.spec_k);
  t.spec_long = (int)env_get("MGH_IPK_SPEC_LONG", t.spec_long);
  t.spec_max = (uint32_t)env_get("MGH_IPK_SPEC_MAX", (long)t.spec_max);
  t.chunk = (int)env_get("MGH_IPK_CHUNK", t.chunk);
  t.chunk_k = (int)env_get("MGH_IPK_CHUNK_K", t.chunk_k);
  t.w = (uint32_t)env_get("MGH_IPK_W", t.w);
  t.wpc = (size_t)env_get("MGH_IPK_WPC", (long)t.wpc);
  t.kr16 = (int)env_get("MGH_IPK_KR16", t.kr16);
  t.contig_rounds = (size_t)env_get("MGH_IPK_CONTIG", (long)t.contig_rounds);
  return t;
}

// One body for both element types: f(T()) with the T of the hierarchy.
template <typename F> auto with_type(const mgh_hierarchy *h, F &&f) {
  return h->dtype == MGH_FLOAT ? f(float()) : f(double());
}

} // namespace

extern "C" {

const char *mgh_last_error(void) { return g_last_error.c_str(); }

/* (internal: lets the high-level translation unit report through the same channel) */
void mgh_set_last_error_(const char *msg) { g_last_error = msg ? msg : ""; }

int mgh_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int mgh_hierarchy_create(mgh_hierarchy **out, int D, const uint64_t *shape, int dtype,
                         const void *const *h_coords, int normalize_coordinates,
                         uint64_t max_level, int device) {
  if (!out || !shape) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (D < 1 || D > MGH_MAX_DIM) return fail(MGH_ERR_UNSUPPORTED_DIMENSION, "D must be 1..5");
  if (dtype != MGH_FLOAT && dtype != MGH_DOUBLE) return fail(MGH_ERR_UNSUPPORTED_DTYPE, "dtype");
  if (mgh_device_count() <= device || device < 0)
    return fail(MGH_ERR_NO_DEVICE, "HIP device " + std::to_string(device) + " not available");
  HIP_TRY(hipSetDevice(device));
  {
    const std::string bad = env_validate();
    if (!bad.empty()) return fail(MGH_ERR_INVALID_ARGUMENT, bad);
  }
  auto *h = new mgh_hierarchy();
  {
    h->force_v1_env = (int)env_get("MGH_FORCE_V1", -1);
    h->force_v1 = h->force_v1_env == 1;
    h->force_nd = env_get("MGH_FORCE_ND", 0) != 0;
    h->force_nd_ipk = env_get("MGH_ND_IPK", 0) != 0;
    h->absmax_warm_mb = (int)env_get("MGH_ABSMAX_WARM_MB", h->absmax_warm_mb);
    h->fused.faces = (int)env_get("MGH_FUSED_FACES", h->fused.faces);
    h->fused.xcd = (int)env_get("MGH_FUSED_XCD", h->fused.xcd);
    h->slice_batch = (int)env_get("MGH_SLICE_BATCH", h->slice_batch);
    h->fused.tall = (int)env_get("MGH_FUSED_TALL", h->fused.tall);
    h->fused_fixed = (int)env_get("MGH_FUSED_FIXED", h->fused_fixed);
    h->fused.wide = (int)env_get("MGH_FUSED_WIDE", -1);  // (-1: by data type, below)
    h->fused4 = (int)env_get("MGH_FUSED4", h->fused4);
    h->fused.box = (int)env_get("MGH_BOX", h->fused.box);
    h->sym16_mixed = (int)env_get("MGH_SYM16_MIXED", h->sym16_mixed);
    h->outlier_agg = (int)env_get("MGH_OUTLIER_AGG", h->outlier_agg);
    h->tail_solves = (int)env_get("MGH_TAIL_SOLVES", h->tail_solves);
    h->nd_rows = (int)env_get("MGH_ND_ROWS", h->nd_rows);
    h->fused.cls1 = (size_t)env_get("MGH_CLS1", (long)h->fused.cls1);
    h->fused.cls2 = (size_t)env_get("MGH_CLS2", (long)h->fused.cls2);
    if (const char *e = std::getenv("MGH_RCH"))
      std::sscanf(e, "%d,%d,%d", &h->fused.rch[0], &h->fused.rch[1], &h->fused.rch[2]);
    // (any of the three set: the marches are the classes' constants, whatever the residency)
    h->fused.pinned = std::getenv("MGH_RCH") || std::getenv("MGH_CLS1") || std::getenv("MGH_CLS2");
    h->fused.slots_override = env_get("MGH_FUSED_SLOTS", 0);
    h->ipk_range_mb = (int)env_get("MGH_IPK_RANGE_MB", h->ipk_range_mb);
    h->no_head = env_get("MGH_NO_RECOMPOSE_HEAD", 0) != 0;
    h->debug_sync = env_get("MGH_DEBUG_SYNC", 0) != 0;
    if (h->force_nd) h->force_v1 = true;  // keeps the fused entry points off
  }
  h->dtype = dtype;
  h->device = device;
  // tile shape of the long marches: 4 x 64 for floats, 8 x 32 for doubles -- fine rows of ~512 bytes
  // either way (512^3 f64 non-uniform, three alternating runs on one box: top-level pass
  // 612 -> 593 us, step 1.413 -> 1.384 ms)
  if (h->fused.wide < 0) h->fused.wide = dtype == MGH_FLOAT ? 1 : 0;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
      h->num_cu = (size_t)cus;
  }
  h->ipk = ipk_tuning_from_env(h->num_cu);
  h->D = D;
  bool ok;
  if (dtype == MGH_FLOAT) {
    auto *hh = new HostHierarchy<float>();
    h->host = hh;
    ok = hh->init(D, shape, (const float *const *)h_coords, normalize_coordinates != 0, max_level);
    hh->normalize_coordinates = normalize_coordinates != 0;
    h->L = hh->L;
    h->total = ok ? hh->total() : 0;
  } else {
    auto *hh = new HostHierarchy<double>();
    h->host = hh;
    ok = hh->init(D, shape, (const double *const *)h_coords, normalize_coordinates != 0, max_level);
    hh->normalize_coordinates = normalize_coordinates != 0;
    h->L = hh->L;
    h->total = ok ? hh->total() : 0;
  }
  if (!ok) {
    if (dtype == MGH_FLOAT) delete HH<float>(h); else delete HH<double>(h);
    delete h;
    return fail(MGH_ERR_INVALID_ARGUMENT,
                "invalid shape: every dimension must have at least 3 nodes");
  }
  h->plane_elems = shape[D - 1] * (D >= 2 ? shape[D - 2] : 1);
  for (int d = 0; d < D; d++) h->shape[d] = shape[d];
  // Thin arrays (a long slowest dimension over planes of a few nodes: 1000000 x 5 x 5): the tiled
  // level kernels cover the coarse (c, f) plane with tiles of 8 x 32 nodes and march along r; where
  // the plane fills less than an eighth of its tiles the one-thread-per-element kernels are the
  // faster ones (4194304 x 3 x 3: 82 -> 12.5 ms per mgh_compress; step of 1000000 x 5 x 5 5.0 vs 6.2 ms,
  // of 100000 x 9 x 9 1.15 vs 1.30 ms -- and 300000 x 17 x 17, 16 % of its tiles, 5.6 vs 3.9 ms the
  // other way round since the tiles of a small cross-section reach all XCDs: round 6).
  if (h->force_v1_env < 0 && D == 3) {
    const uint64_t m1 = shape[1] / 2 + 1, m2 = shape[2] / 2 + 1;
    double tiles = (double)((m1 + 7) / 8) * (double)((m2 + 31) / 32);
    // (a short fastest extent under a long middle one: the 64 x 4 tiles -- fused_tall_tiles)
    if (h->fused.tall && m2 <= 16 && m1 >= 48) tiles = (double)((m1 + 63) / 64) * (double)((m2 + 3) / 4);
    if ((double)(m1 * m2) < 0.125 * tiles * 256.0) h->force_v1 = true;
  }
  int rc = with_type(h, [&](auto t) { return build_device_state<decltype(t)>(h); });
  // what the device holds at once of every level-kernel instance this hierarchy can launch: the
  // marches of the levels below the top are planned against it (fused_plan.hpp)
  if (rc == MGH_SUCCESS) rc = with_type(h, [&](auto t) { return fused_residency_init<decltype(t)>(h); });
  if (rc != MGH_SUCCESS) {
    mgh_hierarchy_destroy(h);
    return rc;
  }
  *out = h;
  return MGH_SUCCESS;
}

void mgh_hierarchy_destroy(mgh_hierarchy *h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  for (auto &kv : h->prof)
    for (auto &ev : kv.second.pending) {
      (void)hipEventDestroy(ev.first);
      (void)hipEventDestroy(ev.second);
    }
  with_type(h, [&](auto t) { destroy_state<decltype(t)>(h); return 0; });
  delete h;
}

int mgh_l_target(const mgh_hierarchy *h) { return h ? h->L : MGH_ERR_INVALID_ARGUMENT; }

int mgh_level_shape(const mgh_hierarchy *h, int level, uint64_t *out_shape) {
  if (!h || !out_shape || level < 0 || level > h->L) return fail(MGH_ERR_INVALID_ARGUMENT, "level");
  return with_type(h, [&](auto t) {
    for (int d = 0; d < h->D; d++) out_shape[d] = HH<decltype(t)>(h)->level_shape[level][d];
    return (int)MGH_SUCCESS;
  });
}

uint64_t mgh_total_num_elems(const mgh_hierarchy *h) { return h ? h->total : 0; }
size_t mgh_device_bytes(const mgh_hierarchy *h) { return h ? h->device_bytes : 0; }
const void *mgh_norm_device_ptr(const mgh_hierarchy *h) {
  if (!h) return nullptr;
  return with_type(h, [&](auto t) { return (const void *)DS<decltype(t)>(h)->normval; });
}


int64_t mgh_hierarchy_table(const mgh_hierarchy *h, int kind, int level, int dim, void *h_out,
                            uint64_t cap) {
  if (!h || !h_out) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  return with_type(h, [&](auto t) { return table_impl<decltype(t)>(h, kind, level, dim, h_out, cap); });
}

int mgh_set_ld(mgh_hierarchy *h, int which, const uint64_t *ld) {
  if (!h || (which != MGH_LD_IN && which != MGH_LD_OUT)) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_set_ld: which");
  if (!ld) {
    h->has_ld[which] = false;
    return MGH_SUCCESS;
  }
  bool dense = true;
  for (int d = 1; d < h->D; d++) {
    if (ld[d] < h->shape[d]) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_set_ld: a leading dimension is smaller than the extent");
    dense &= ld[d] == h->shape[d];
  }
  for (int d = 0; d < h->D; d++) h->ld[which][d] = d == 0 ? h->shape[0] : ld[d];
  h->has_ld[which] = !dense;
  return MGH_SUCCESS;
}

// The stage entry points: arguments checked, the layouts of their OWN T arguments taken from the
// setting (caller_layout), one internal template called. The stages reach each other through the
// templates, never through these.
int mgh_norm(mgh_hierarchy *h, const void *d_data, double s, double *h_norm_out, void *stream) {
  if (!h || !d_data || !h_norm_out) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    return norm_impl<T>(h, (const T *)d_data, caller_layout(h, MGH_LD_IN), s, h_norm_out, (hipStream_t)stream);
  });
}

int mgh_decompose(mgh_hierarchy *h, const void *d_data, void *d_coeff, void *stream) {
  if (!h || !d_data || !d_coeff) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    return decompose_impl<T>(h, (const T *)d_data, caller_layout(h, MGH_LD_IN), (T *)d_coeff,
                             caller_layout(h, MGH_LD_OUT), (hipStream_t)stream);
  });
}

int mgh_recompose(mgh_hierarchy *h, const void *d_coeff, void *d_data, void *stream) {
  if (!h || !d_data || !d_coeff) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    return recompose_impl<T>(h, (const T *)d_coeff, caller_layout(h, MGH_LD_IN), (T *)d_data,
                             caller_layout(h, MGH_LD_OUT), (hipStream_t)stream);
  });
}

int mgh_quantize(mgh_hierarchy *h, const void *d_coeff, int ebtype, double tol, double s,
                 double norm, uint64_t dict_size, int prep_huffman, int64_t *d_quantized,
                 uint64_t *d_outlier_count, uint64_t *d_outlier_idx, int64_t *d_outlier_val,
                 uint64_t outlier_capacity, void *stream) {
  if (!h || !d_coeff || !d_quantized) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  const QuantOut qo{dict_size, prep_huffman, d_quantized, nullptr, d_outlier_count, d_outlier_idx, d_outlier_val,
                    outlier_capacity};
  TRY(outlier_args(qo));
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    return quantize_impl<T>(h, (const T *)d_coeff, caller_layout(h, MGH_LD_IN), {ebtype, tol, s}, norm, qo,
                            (hipStream_t)stream);
  });
}

int mgh_dequantize(mgh_hierarchy *h, int64_t *d_quantized, int ebtype, double tol, double s,
                   double norm, uint64_t dict_size, int prep_huffman,
                   const uint64_t *d_outlier_idx, const int64_t *d_outlier_val,
                   uint64_t outlier_count, void *d_coeff, void *stream) {
  if (!h || !d_coeff || !d_quantized) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  const QuantSpec qs{ebtype, tol, s, norm, dict_size, prep_huffman, d_outlier_idx, d_outlier_val, outlier_count};
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    return dequantize_impl<T>(h, d_quantized, qs, (T *)d_coeff, caller_layout(h, MGH_LD_OUT), (hipStream_t)stream);
  });
}

// The body of mgh_decompose_quantize{,_sym16,_dn}: the core in the hierarchy's data type, on its device.
static int decompose_quantize_entry(mgh_hierarchy *h, const void *d_data, const Bound &b, const NormSource &ns,
                                    const QuantOut &qo, void *d_coeff_opt, void *stream) {
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    return decompose_quantize<T>(h, (const T *)d_data, caller_layout(h, MGH_LD_IN), b, ns, qo,
                                 {d_coeff_opt, caller_layout(h, MGH_LD_OUT)}, (hipStream_t)stream);
  });
}
// The norm argument of the host entries: REL with norm > 0 is a given norm, REL without one asks for it.
static NormSource norm_source(int ebtype, double norm, double *h_norm_out) {
  const NormSource::Kind k = ebtype != MGH_REL ? NormSource::None : norm > 0 ? NormSource::Host : NormSource::Compute;
  return {k, norm, nullptr, 0, 1, h_norm_out};
}

int mgh_decompose_quantize_sym16(mgh_hierarchy *h, const void *d_data, int error_bound_type, double tol,
                                 double s, double norm, double *h_norm_out, uint64_t dict_size,
                                 uint16_t *d_symbols, uint64_t *d_outlier_count,
                                 uint64_t *d_outlier_idx, int64_t *d_outlier_val,
                                 uint64_t outlier_capacity, void *stream) {
  if (!h || !d_data || !d_symbols || !d_outlier_count || (outlier_capacity && (!d_outlier_idx || !d_outlier_val)))
    return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  return decompose_quantize_entry(h, d_data, {error_bound_type, tol, s}, norm_source(error_bound_type, norm, h_norm_out),
                                  {dict_size, 1, nullptr, d_symbols, d_outlier_count, d_outlier_idx, d_outlier_val,
                                   outlier_capacity},
                                  nullptr, stream);
}

int mgh_sym16_supported(const mgh_hierarchy *h) { return h && fused_route(h) ? 1 : 0; }

// The body of the reconstruction entry points: the core in the hierarchy's data type, on its device.
static int reconstruct_entry(mgh_hierarchy *h, const QuantSpec &qs, const IntSource &src, const Target &tg, void *stream) {
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) { return reconstruct<decltype(t)>(h, qs, src, tg, (hipStream_t)stream); });
}

int mgh_dequantize_recompose_sym16(mgh_hierarchy *h, const uint16_t *d_symbols, int error_bound_type,
                                   double tol, double s, double norm, uint64_t dict_size,
                                   const uint64_t *d_outlier_idx, const int64_t *d_outlier_val,
                                   uint64_t outlier_count, void *d_data_out, void *stream) {
  if (!h || !d_symbols || !d_data_out || (outlier_count && (!d_outlier_idx || !d_outlier_val)))
    return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (dict_size == 0 || dict_size > 65536) return fail(MGH_ERR_INVALID_ARGUMENT, "dict_size must be in 1..65536");
  if (!mgh_sym16_supported(h))
    return fail(MGH_ERR_UNSUPPORTED_DIMENSION, "16-bit symbols: only on the fused 3-D / 4-D path");
  return reconstruct_entry(h, {error_bound_type, tol, s, norm, dict_size, 1, d_outlier_idx, d_outlier_val, outlier_count},
                           {IntSource::Sym16, nullptr, d_symbols},
                           {h->L, 0, nullptr, d_data_out, caller_layout(h, MGH_LD_OUT)}, stream);
}

int mgh_decompose_quantize(mgh_hierarchy *h, const void *d_data, int error_bound_type, double tol, double s,
                           double norm, double *h_norm_out, uint64_t dict_size, int prep_huffman,
                           int64_t *d_quantized, uint64_t *d_outlier_count,
                           uint64_t *d_outlier_idx, int64_t *d_outlier_val,
                           uint64_t outlier_capacity, void *d_coeff_opt, void *stream) {
  if (!h || !d_data || !d_quantized) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  return decompose_quantize_entry(h, d_data, {error_bound_type, tol, s}, norm_source(error_bound_type, norm, h_norm_out),
                                  {dict_size, prep_huffman, d_quantized, nullptr, d_outlier_count, d_outlier_idx,
                                   d_outlier_val, outlier_capacity},
                                  d_coeff_opt, stream);
}

int mgh_norm_device(mgh_hierarchy *h, const void *d_data, double s, void *d_norm_out,
                    void *stream) {
  if (!h || !d_data || !d_norm_out) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  return with_type(h, [&](auto t) -> int {
    using T = decltype(t);
    TRY(norm_launch<T>(h, (const T *)d_data, caller_layout(h, MGH_LD_IN), s, st));
    // ABS/undecomposed parameters are irrelevant here: only the norm conversion is wanted
    TRY(make_qparams_launch<T>(h, nullptr, MGH_ABS, 1.0, s, 0, 1, nullptr, st));
    HIP_TRY(hipMemcpyAsync(d_norm_out, DS<T>(h)->normval, sizeof(T), hipMemcpyDeviceToDevice, st));
    return MGH_SUCCESS;
  });
}

int mgh_norm_stream_begin(mgh_hierarchy *h, void *stream) {
  if (!h) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (!fused_route(h))
    return fail(MGH_ERR_UNSUPPORTED_DIMENSION, "streamed norm: only in front of the fused 3-D / 4-D path");
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) { return norm_stream_begin<decltype(t)>(h, (hipStream_t)stream); });
}

int mgh_norm_stream_add(mgh_hierarchy *h, const void *d_part, uint64_t count, double s, int cold, void *stream) {
  if (!h || (!d_part && count)) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (h->has_ld[0]) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_norm_stream_add takes parts of a dense array (mgh_set_ld is set)");
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    return norm_stream_add<T>(h, (const T *)d_part, count, s, cold, (hipStream_t)stream);
  });
}

int mgh_norm_stream_end(mgh_hierarchy *h, double s, double *h_norm_out, void *stream) {
  if (!h || !h_norm_out) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) { return norm_stream_end<decltype(t)>(h, s, h_norm_out, (hipStream_t)stream); });
}

int mgh_quantize_histograms(mgh_hierarchy *h, const void *d_coeff, int error_bound_type, int ntol, const double *tols,
                            double s, double norm, uint64_t dict_size, uint32_t *d_freq, uint64_t *d_outliers,
                            void *stream) {
  if (!h || !d_coeff || !tols || !d_freq || !d_outliers) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (const char *bad = qhist_refusal(h->total, ntol, dict_size)) return fail(MGH_ERR_INVALID_ARGUMENT, bad);
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    return quantize_histograms_impl<T>(h, (const T *)d_coeff, caller_layout(h, MGH_LD_IN), error_bound_type, ntol, tols,
                                       s, norm, dict_size, d_freq, d_outliers, (hipStream_t)stream);
  });
}

int mgh_quantize_roundtrip(mgh_hierarchy *h, const void *d_coeff, int error_bound_type, double tol, double s,
                           double norm, void *d_coeff_out, void *stream) {
  if (!h || !d_coeff || !d_coeff_out) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (const char *bad = qround_refusal(h->total)) return fail(MGH_ERR_INVALID_ARGUMENT, bad);
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    return quantize_roundtrip_impl<T>(h, (const T *)d_coeff, caller_layout(h, MGH_LD_IN), {error_bound_type, tol, s},
                                      norm, (T *)d_coeff_out, (hipStream_t)stream);
  });
}

int mgh_quantize_symbols(mgh_hierarchy *h, const void *d_coeff, int error_bound_type, double tol, double s,
                         double norm, uint64_t dict_size, uint16_t *d_symbols, uint32_t *d_freq_or_null,
                         uint64_t *d_outlier_count, uint64_t *d_outlier_idx, int64_t *d_outlier_val,
                         uint64_t outlier_capacity, void *stream) {
  if (!h || !d_coeff || !d_symbols) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  const QuantOut qo{dict_size, 1, nullptr, d_symbols, d_outlier_count, d_outlier_idx, d_outlier_val, outlier_capacity};
  TRY(outlier_args(qo));
  if (const char *bad = qsym_refusal(h->total, dict_size)) return fail(MGH_ERR_INVALID_ARGUMENT, bad);
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    return quantize_symbols_impl<T>(h, (const T *)d_coeff, caller_layout(h, MGH_LD_IN), {error_bound_type, tol, s},
                                    norm, dict_size, d_symbols, d_freq_or_null, qo, (hipStream_t)stream);
  });
}

int mgh_quantize_symbols_residual(mgh_hierarchy *h, const void *d_coeff, int error_bound_type, double tol, double s,
                                  double norm, uint64_t dict_size, uint16_t *d_symbols, uint32_t *d_freq_or_null,
                                  uint64_t *d_outlier_count, uint64_t *d_outlier_idx, int64_t *d_outlier_val,
                                  uint64_t outlier_capacity, void *d_residual_out, void *stream) {
  if (!h || !d_coeff || !d_symbols || !d_residual_out) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  const QuantOut qo{dict_size, 1, nullptr, d_symbols, d_outlier_count, d_outlier_idx, d_outlier_val, outlier_capacity};
  TRY(outlier_args(qo));
  if (const char *bad = qsym_refusal(h->total, dict_size)) return fail(MGH_ERR_INVALID_ARGUMENT, bad);
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    return quantize_symbols_residual_impl<T>(h, (const T *)d_coeff, caller_layout(h, MGH_LD_IN),
                                             {error_bound_type, tol, s}, norm, dict_size, d_symbols, d_freq_or_null, qo,
                                             (T *)d_residual_out, (hipStream_t)stream);
  });
}

int mgh_dequantize_add(mgh_hierarchy *h, int64_t *d_quantized, int error_bound_type, double tol, double s, double norm,
                       uint64_t dict_size, int prep_huffman, const uint64_t *d_outlier_idx,
                       const int64_t *d_outlier_val, uint64_t outlier_count, int first, void *d_coeff_inout,
                       void *stream) {
  if (!h || !d_quantized || !d_coeff_inout) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (prep_huffman && outlier_count && (!d_outlier_idx || !d_outlier_val))
    return fail(MGH_ERR_INVALID_ARGUMENT, "null outlier list");
  if (h->total == 0 || h->total >= ((uint64_t)1 << 32))
    return fail(MGH_ERR_INVALID_ARGUMENT, "dequantize_add: 1 .. 2^32 - 1 elements (32-bit index arithmetic)");
  HIP_TRY(hipSetDevice(h->device));
  const QuantSpec qs{error_bound_type, tol, s, norm, dict_size, prep_huffman, d_outlier_idx, d_outlier_val, outlier_count};
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    return dequantize_add_impl<T>(h, d_quantized, qs, first != 0, (T *)d_coeff_inout, (hipStream_t)stream);
  });
}

int mgh_quantize_residual_linear(mgh_hierarchy *h, const void *d_coeff, int error_bound_type, double tol, double s,
                                 double norm, uint64_t dict_size, int64_t *d_linear_out, uint64_t *d_outlier_count,
                                 uint64_t *d_outlier_idx, int64_t *d_outlier_val, uint64_t outlier_capacity,
                                 void *d_residual_out, void *stream) {
  if (!h || !d_coeff || !d_linear_out || !d_residual_out) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  const QuantOut qo{dict_size, 1, d_linear_out, nullptr, d_outlier_count, d_outlier_idx, d_outlier_val, outlier_capacity};
  TRY(outlier_args(qo));
  if (const char *bad = qsym_refusal(h->total, dict_size)) return fail(MGH_ERR_INVALID_ARGUMENT, bad);
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    return quantize_residual_linear_impl<T>(h, (const T *)d_coeff, caller_layout(h, MGH_LD_IN), {error_bound_type, tol, s},
                                            norm, dict_size, d_linear_out, qo, (T *)d_residual_out, (hipStream_t)stream);
  });
}

int mgh_dequantize_add_linear(mgh_hierarchy *h, int64_t *d_linear_window, uint64_t first, uint64_t count,
                              int error_bound_type, double tol, double s, double norm, uint64_t dict_size,
                              int prep_huffman, const uint64_t *d_outlier_idx, const int64_t *d_outlier_val,
                              uint64_t outlier_count, int store, void *d_acc_linear, void *stream) {
  if (!h || !d_linear_window || !d_acc_linear) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (prep_huffman && outlier_count && (!d_outlier_idx || !d_outlier_val))
    return fail(MGH_ERR_INVALID_ARGUMENT, "null outlier list");
  if (h->total == 0 || h->total >= ((uint64_t)1 << 32))
    return fail(MGH_ERR_INVALID_ARGUMENT, "dequantize_add_linear: 1 .. 2^32 - 1 elements (32-bit index arithmetic)");
  if (count == 0 || first >= h->total || count > h->total - first)
    return fail(MGH_ERR_INVALID_ARGUMENT, "dequantize_add_linear: the window [first, first + count) leaves the array");
  HIP_TRY(hipSetDevice(h->device));
  const QuantSpec qs{error_bound_type, tol, s, norm, dict_size, prep_huffman, d_outlier_idx, d_outlier_val, outlier_count};
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    return dequantize_add_linear_impl<T>(h, d_linear_window, first, count, qs, store != 0, (T *)d_acc_linear,
                                         (hipStream_t)stream);
  });
}

int mgh_decompose_quantize_dn(mgh_hierarchy *h, const void *d_data, int error_bound_type,
                              double tol, double s, const void *d_norm, uint64_t num_subdomains,
                              uint64_t dict_size, int prep_huffman, int64_t *d_quantized,
                              uint64_t *d_outlier_count, uint64_t *d_outlier_idx,
                              int64_t *d_outlier_val, uint64_t outlier_capacity, void *stream) {
  if (!h || !d_data || !d_quantized || !d_norm) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  return decompose_quantize_entry(h, d_data, {error_bound_type, tol, s},
                                  {NormSource::Device, 0, d_norm, 1, num_subdomains, nullptr},
                                  {dict_size, prep_huffman, d_quantized, nullptr, d_outlier_count, d_outlier_idx,
                                   d_outlier_val, outlier_capacity},
                                  nullptr, stream);
}

int mgh_dequantize_recompose(mgh_hierarchy *h, int64_t *d_quantized, int ebtype, double tol,
                             double s, double norm, uint64_t dict_size, int prep_huffman,
                             const uint64_t *d_outlier_idx, const int64_t *d_outlier_val,
                             uint64_t outlier_count, void *d_data, void *stream) {
  if (!h || !d_data || !d_quantized) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  return reconstruct_entry(h, {ebtype, tol, s, norm, dict_size, prep_huffman, d_outlier_idx, d_outlier_val, outlier_count},
                           {IntSource::Full, d_quantized, nullptr},
                           {h->L, 0, nullptr, d_data, caller_layout(h, MGH_LD_OUT)}, stream);
}

int mgh_level_nodes(const mgh_hierarchy *h, int level, int dim, uint64_t *h_idx_out, uint64_t cap) {
  if (!h || !h_idx_out) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (level < 0 || level > h->L) return fail(MGH_ERR_INVALID_ARGUMENT, "level outside 0 .. l_target");
  if (dim < 0 || dim >= h->D) return fail(MGH_ERR_INVALID_ARGUMENT, "dim");
  std::vector<uint64_t> idx;
  level_nodes(h->shape[dim], h->L - level, idx);
  if (idx.size() > cap) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_level_nodes: capacity too small");
  std::copy(idx.begin(), idx.end(), h_idx_out);
  return (int)idx.size();
}

namespace {
int level_arg(const mgh_hierarchy *h, int level) {
  if (level < 0 || level > h->L) return fail(MGH_ERR_INVALID_ARGUMENT, "level outside 0 .. l_target");
  return MGH_SUCCESS;
}
} // namespace

// The output of these calls is the dense array of level_shape(level): MGH_LD_OUT does not apply.
// level == l_target is the body of the call without a level, with a dense layout for the output.
int mgh_recompose_to_level(mgh_hierarchy *h, const void *d_coeff, int level, void *d_out, void *stream) {
  if (!h || !d_out || !d_coeff) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (d_out == d_coeff) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_recompose_to_level: d_out must not be d_coeff");
  TRY(level_arg(h, level));
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    const Layout in = caller_layout(h, MGH_LD_IN);
    if (level == h->L)
      return recompose_impl<T>(h, (const T *)d_coeff, in, (T *)d_out, dense_layout(h), (hipStream_t)stream);
    return recompose_to_level_impl<T>(h, (const T *)d_coeff, in, level, (T *)d_out, (hipStream_t)stream);
  });
}

int mgh_dequantize_recompose_to_level(mgh_hierarchy *h, int64_t *d_quantized, int ebtype, double tol, double s,
                                      double norm, uint64_t dict_size, int prep_huffman,
                                      const uint64_t *d_outlier_idx, const int64_t *d_outlier_val,
                                      uint64_t outlier_count, int level, void *d_out, void *stream) {
  if (!h || !d_out || !d_quantized) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (prep_huffman && outlier_count && (!d_outlier_idx || !d_outlier_val))
    return fail(MGH_ERR_INVALID_ARGUMENT, "null outlier list");
  TRY(level_arg(h, level));
  return reconstruct_entry(h, {ebtype, tol, s, norm, dict_size, prep_huffman, d_outlier_idx, d_outlier_val, outlier_count},
                           {IntSource::Full, d_quantized, nullptr}, {level, 0, nullptr, d_out, dense_layout(h)}, stream);
}

int mgh_level_box_from_linear(mgh_hierarchy *h, const int64_t *d_linear, int level, int64_t *d_box_out, void *stream) {
  if (!h || !d_linear || !d_box_out || d_linear == d_box_out)
    return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_level_box_from_linear: null or aliasing argument");
  TRY(level_arg(h, level));
  HIP_TRY(hipSetDevice(h->device));
  return box_from_linear(h, d_linear, level, d_box_out, (hipStream_t)stream);
}

// The head of a level-linearised array (a reorder = 1 record) to the dense array of `level`: the
// outliers of the head written in place, the compact box of the level made from it (ds->qbox), and
// the level loops of mgh_dequantize_recompose_to_level on that box with the box's own strides.
int mgh_dequantize_recompose_linear_to_level(mgh_hierarchy *h, int64_t *d_linear, int ebtype, double tol, double s,
                                             double norm, uint64_t dict_size, int prep_huffman,
                                             const uint64_t *d_outlier_idx, const int64_t *d_outlier_val,
                                             uint64_t outlier_count, int level, void *d_out, void *stream) {
  if (!h || !d_out || !d_linear) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (prep_huffman && outlier_count && (!d_outlier_idx || !d_outlier_val))
    return fail(MGH_ERR_INVALID_ARGUMENT, "null outlier list");
  TRY(level_arg(h, level));
  return reconstruct_entry(h, {ebtype, tol, s, norm, dict_size, prep_huffman, d_outlier_idx, d_outlier_val, outlier_count},
                           {IntSource::Linear, d_linear, nullptr}, {level, 0, nullptr, d_out, dense_layout(h)}, stream);
}

// The head of a level-linearised COEFFICIENT array (the accumulator of the level-ordered precision
// layers) to the dense array of `level`: what mgh_recompose_to_level gives for the same coefficients
// in array order, from the first N_level of them.
int mgh_recompose_linear_to_level(mgh_hierarchy *h, const void *d_acc_linear, int level, void *d_out, void *stream) {
  if (!h || !d_acc_linear || !d_out) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (d_out == d_acc_linear) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_recompose_linear_to_level: d_out must not be d_acc_linear");
  TRY(level_arg(h, level));
  if (h->total >= ((uint64_t)1 << 32))
    return fail(MGH_ERR_INVALID_ARGUMENT, "recompose_linear_to_level: at most 2^32 - 1 elements");
  if (h->L + 1 > mgh::kLinMaxLevels + 1) return fail(MGH_ERR_INVALID_ARGUMENT, "too many levels");
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    return recompose_linear_to_level_impl<T>(h, (const T *)d_acc_linear, level, (T *)d_out, (hipStream_t)stream);
  });
}

// One level step: the dense nodal array of level - 1 and the level's own segment of a level-linearised
// array to the dense array of `level` -- one pass of the level loop of
// mgh_dequantize_recompose_linear_to_level, with the box of the level made from the segment alone.
int mgh_refine_level(mgh_hierarchy *h, const void *d_coarse, int64_t *d_segment, int ebtype, double tol, double s,
                     double norm, uint64_t dict_size, int prep_huffman, const uint64_t *d_outlier_idx,
                     const int64_t *d_outlier_val, uint64_t outlier_count, int level, void *d_out, void *stream) {
  if (!h || !d_coarse || !d_segment || !d_out) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (prep_huffman && outlier_count && (!d_outlier_idx || !d_outlier_val))
    return fail(MGH_ERR_INVALID_ARGUMENT, "null outlier list");
  if (level < 1 || level > h->L) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_refine_level: level outside 1 .. l_target");
  if (d_out == d_coarse || d_out == (void *)d_segment)
    return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_refine_level: d_out must not alias an input");
  return reconstruct_entry(h, {ebtype, tol, s, norm, dict_size, prep_huffman, d_outlier_idx, d_outlier_val, outlier_count},
                           {IntSource::Linear, d_segment, nullptr}, {level, level, d_coarse, d_out, dense_layout(h)}, stream);
}

// The dense array of `level` prolonged to the full grid: what mgh_recompose gives for the reordered
// array that holds the level in its corner box and zeros everywhere else.
int mgh_prolong(mgh_hierarchy *h, int level, const void *d_level, void *d_out, void *stream) {
  if (!h || !d_level || !d_out) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (d_out == d_level) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_prolong: d_out must not be d_level");
  TRY(level_arg(h, level));
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    return prolong_impl<T>(h, level, (const T *)d_level, (T *)d_out, (hipStream_t)stream);
  });
}

namespace {
int prolong_window_entry(mgh_hierarchy *h, int level, const void *d_level, const uint64_t *lo, const uint64_t *ext,
                         void *d_out, const uint64_t *out_stride, void *stream) {
  if (!h || !d_level || !d_out || !lo || !ext) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (d_out == d_level) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_prolong_window: d_out must not be d_level");
  TRY(level_arg(h, level));
  HIP_TRY(hipSetDevice(h->device));
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    return prolong_window_impl<T>(h, level, (const T *)d_level, lo, ext, (T *)d_out, out_stride, (hipStream_t)stream);
  });
}
} // namespace

int mgh_prolong_window(mgh_hierarchy *h, int level, const void *d_level, const uint64_t *lo, const uint64_t *ext,
                       void *d_out, void *stream) {
  return prolong_window_entry(h, level, d_level, lo, ext, d_out, nullptr, stream);
}

int mgh_prolong_window_strided(mgh_hierarchy *h, int level, const void *d_level, const uint64_t *lo,
                               const uint64_t *ext, void *d_out, const uint64_t *out_stride, void *stream) {
  if (!out_stride) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  return prolong_window_entry(h, level, d_level, lo, ext, d_out, out_stride, stream);
}

int mgh_debug_prolong_window_ranges(const mgh_hierarchy *h, int level, const uint64_t *lo, const uint64_t *ext,
                                    int64_t *out, uint64_t cap) {
  if (!h || !lo || !ext || !out) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  std::vector<int64_t> chain;
  const bool ok = with_type(h, [&](auto t) {
    return prolong_window_chain(HH<decltype(t)>(h)->level_shape, level, lo, ext, chain);
  });
  if (!ok) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_debug_prolong_window_ranges: level or window outside the hierarchy");
  if (cap < chain.size()) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_debug_prolong_window_ranges: out too small");
  std::copy(chain.begin(), chain.end(), out);
  return (int)chain.size();
}

int mgh_debug_prolong_window_plan(const mgh_hierarchy *h, int level, const uint64_t *lo, const uint64_t *ext, int l,
                                  int *out12) {
  if (!h || !lo || !ext || !out12) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (!(fused_route(h) && h->D == 3))
    return fail(MGH_ERR_UNSUPPORTED_DIMENSION, "mgh_prolong_window runs no kernel of its own on this shape");
  if (l <= level || l > h->L) return fail(MGH_ERR_INVALID_ARGUMENT, "step outside level + 1 .. l_target");
  return with_type(h, [&](auto t) {
    using T = decltype(t);
    std::vector<int64_t> chain;
    if (!prolong_window_chain(HH<T>(h)->level_shape, level, lo, ext, chain))
      return fail(MGH_ERR_INVALID_ARGUMENT, "level or window outside the hierarchy");
    int64_t a[3], b[3];
    for (int k = 0; k < 3; k++) {
      a[k] = chain[(size_t)(l - level) * 6 + 2 * k];
      b[k] = chain[(size_t)(l - level) * 6 + 2 * k + 1];
    }
    const ProlongWinPlan w = prolong_window_plan(DS<T>(h)->lt[l].box.n, a, b, h->fused.tall != 0);
    const int v[12] = {w.p.TC, w.p.TF, w.p.gxm, w.p.ntile, w.p.rch, w.p.nchunk, w.J0[0], w.J0[1], w.J0[2],
                       w.nJ[0], w.nJ[1], w.nJ[2]};
    std::copy(v, v + 12, out12);
    return (int)MGH_SUCCESS;
  });
}

int mgh_debug_prolong_plan(const mgh_hierarchy *h, int level, int *out6) {
  if (!h || !out6) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (level < 1 || level > h->L) return fail(MGH_ERR_INVALID_ARGUMENT, "level outside 1 .. l_target");
  if (!(fused_route(h) && h->D == 3)) return fail(MGH_ERR_UNSUPPORTED_DIMENSION, "mgh_prolong runs no kernel of its own on this shape");
  const ProlongPlan p = with_type(h, [&](auto t) { return prolong_plan_of<decltype(t)>(h, level); });
  const int v[6] = {p.TC, p.TF, p.gxm, p.ntile, p.rch, p.nchunk};
  std::copy(v, v + 6, out6);
  return MGH_SUCCESS;
}

int mgh_dequantize_recompose_sym16_to_level(mgh_hierarchy *h, const uint16_t *d_symbols, int error_bound_type,
                                            double tol, double s, double norm, uint64_t dict_size,
                                            const uint64_t *d_outlier_idx, const int64_t *d_outlier_val,
                                            uint64_t outlier_count, int level, void *d_out, void *stream) {
  if (!h || !d_symbols || !d_out || (outlier_count && (!d_outlier_idx || !d_outlier_val)))
    return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  if (dict_size == 0 || dict_size > 65536) return fail(MGH_ERR_INVALID_ARGUMENT, "dict_size must be in 1..65536");
  TRY(level_arg(h, level));
  if (!mgh_sym16_supported(h))
    return fail(MGH_ERR_UNSUPPORTED_DIMENSION, "16-bit symbols: only on the fused 3-D / 4-D path");
  return reconstruct_entry(h, {error_bound_type, tol, s, norm, dict_size, 1, d_outlier_idx, d_outlier_val, outlier_count},
                           {IntSource::Sym16, nullptr, d_symbols}, {level, 0, nullptr, d_out, dense_layout(h)}, stream);
}

#ifdef MGH_PHASE_TIMING
int mgh_debug_tail_read(unsigned long long *out64, int reset) {
  HIP_TRY(hipMemcpyFromSymbol(out64, HIP_SYMBOL(mgh::g_tail), sizeof(unsigned long long) * 64));
  if (reset) {
    unsigned long long z[64] = {0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(mgh::g_tail), z, sizeof z));
  }
  return MGH_SUCCESS;
}
int mgh_debug_phase_read(unsigned long long *out16, int reset) {
  HIP_TRY(hipMemcpyFromSymbol(out16, HIP_SYMBOL(mgh::g_phase), sizeof(unsigned long long) * 16));
  if (reset) {
    unsigned long long z[16] = {0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(mgh::g_phase), z, sizeof z));
  }
  return MGH_SUCCESS;
}
#endif

int mgh_debug_ipk_plans_read(mgh_hierarchy *h, long long *out, int cap, int reset) {
  if (!h || (cap > 0 && !out) || cap < 0) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  const int n = (int)h->ipk_log.size();
  for (int i = 0; i < std::min(n, cap); i++)
    std::copy(h->ipk_log[i].begin(), h->ipk_log[i].end(), out + (size_t)i * MGH_IPK_PLAN_FIELDS);
  if (reset) h->ipk_log.clear();
  return n;
}

int mgh_debug_spec_repairs_read(mgh_hierarchy *h, uint64_t *out, int reset) {
  if (!h || !out) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  *out = 0;
  return with_type(h, [&](auto t) {
    auto *ds = DS<decltype(t)>(h);
    if (!ds->spec_fixed) return (int)MGH_SUCCESS;  // (no solve in verified chunks so far)
    // (the solves ran on a stream of the caller's: wait for the device, as mgh_profile_read does)
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long v = 0;
    HIP_TRY(hipMemcpy(&v, ds->spec_fixed, sizeof v, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(ds->spec_fixed, 0, sizeof v));
    *out = v;
    return (int)MGH_SUCCESS;
  });
}

int mgh_debug_fused_plans_read(mgh_hierarchy *h, long long *out, int cap, int reset) {
  if (!h || (cap > 0 && !out) || cap < 0) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  const int n = (int)h->fused_log.size();
  for (int i = 0; i < std::min(n, cap); i++)
    std::copy(h->fused_log[i].begin(), h->fused_log[i].end(), out + (size_t)i * MGH_FUSED_PLAN_FIELDS);
  if (reset) h->fused_log.clear();
  return n;
}

int mgh_profile_enable(mgh_hierarchy *h, int enable) {
  if (!h) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  h->profiling = enable != 0;
  return MGH_SUCCESS;
}

int mgh_profile_filter(mgh_hierarchy *h, const char *name) {
  if (!h) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  h->prof_filter = name ? name : "";
  return MGH_SUCCESS;
}

int mgh_profile_read(mgh_hierarchy *h, const char **names, double *total_ms, uint64_t *launches,
                     int cap, int reset) {
  if (!h) return fail(MGH_ERR_INVALID_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  int n = 0;
  for (auto &kv : h->prof) {
    ProfileEntry &e = kv.second;
    for (auto &ev : e.pending) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, ev.first, ev.second));
      e.total_ms += ms;
      e.launches++;
      (void)hipEventDestroy(ev.first);
      (void)hipEventDestroy(ev.second);
    }
    e.pending.clear();
    if (n < cap) {
      if (names) names[n] = kv.first.c_str();
      if (total_ms) total_ms[n] = e.total_ms;
      if (launches) launches[n] = e.launches;
    }
    n++;
    if (reset) {
      e.total_ms = 0;
      e.launches = 0;
    }
  }
  return n;
}

int mgh_outlier_restore(int64_t *d_q, uint64_t n, const uint64_t *d_outlier_idx,
                        const int64_t *d_outlier_val, uint64_t outlier_count, void *stream) {
  if (!d_q || (outlier_count && (!d_outlier_idx || !d_outlier_val)))
    return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_outlier_restore: null argument");
  if (!outlier_count) return MGH_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  mgh::k_outlier_restore<<<(unsigned)((outlier_count + 255) / 256), 256, 0, st>>>(d_q, n, d_outlier_idx,
                                                                                 d_outlier_val, outlier_count);
  HIP_TRY(hipGetLastError());
  return MGH_SUCCESS;
}

int mgh_level_linearize(mgh_hierarchy *h, const int64_t *d_in, int64_t *d_out, int inverse,
                        uint64_t *d_outlier_idx, const uint64_t *d_outlier_count, uint64_t outlier_count,
                        uint64_t outlier_capacity, void *stream) {
  if (!h || !d_in || !d_out || d_in == d_out) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_level_linearize: null or aliasing argument");
  if (inverse && d_outlier_idx) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_level_linearize: indices are mapped forward only");
  if (h->L + 1 > mgh::kLinMaxLevels + 1) return fail(MGH_ERR_INVALID_ARGUMENT, "too many levels");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  mgh::LinMeta m{};
  const int *marks = lin_meta(h, m);
  const size_t total = h->total;
  const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 256 * 32);
  TRY(launch(h, "level_linearize", st, [&] {
    if (inverse) mgh::k_level_linearize<int64_t, true><<<grid, 256, 0, st>>>(m, marks, total, d_in, d_out);
    else mgh::k_level_linearize<int64_t, false><<<grid, 256, 0, st>>>(m, marks, total, d_in, d_out);
  }));
  if (d_outlier_idx && (d_outlier_count || outlier_count)) {
    const unsigned long long cap = outlier_capacity ? outlier_capacity : (d_outlier_count ? ~0ull : outlier_count);
    const size_t work = d_outlier_count ? (size_t)std::min<unsigned long long>(cap, total) : (size_t)outlier_count;
    const unsigned g2 = (unsigned)std::max<size_t>(1, std::min<size_t>((work + 255) / 256, 4096));
    TRY(launch(h, "linearize_indices", st, [&] {
      mgh::k_linearize_indices<<<g2, 256, 0, st>>>(m, marks, total, d_outlier_idx,
                                                   (const unsigned long long *)d_outlier_count,
                                                   (unsigned long long)outlier_count, cap);
    }));
  }
  return MGH_SUCCESS;
}

int mgh_stream_calibrate(int dtype, const void *d_in, int64_t *d_out, void *d_side, uint64_t n,
                         int reps, double *ms_out, void *stream) {
  if (!d_in || !d_out || !d_side || !ms_out || n < 8 || reps < 1 || (dtype != MGH_FLOAT && dtype != MGH_DOUBLE)) {
    return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_stream_calibrate: bad argument");
  }
  hipStream_t st = (hipStream_t)stream;
  hipEvent_t a, b;
  HIP_TRY(hipEventCreate(&a));
  HIP_TRY(hipEventCreate(&b));
  auto go = [&] {
    if (dtype == MGH_FLOAT)
      mgh::k_stream_mix<float><<<32768, 256, 0, st>>>((const float *)d_in, d_out, (float *)d_side,
                                                      (float *)d_side + n / 8, (size_t)n);
    else
      mgh::k_stream_mix<double><<<32768, 256, 0, st>>>((const double *)d_in, d_out, (double *)d_side,
                                                       (double *)d_side + n / 8, (size_t)n);
  };
  for (int i = 0; i < 2; i++) go();
  HIP_TRY(hipEventRecord(a, st));
  for (int i = 0; i < reps; i++) go();
  HIP_TRY(hipEventRecord(b, st));
  HIP_TRY(hipEventSynchronize(b));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, a, b));
  HIP_TRY(hipEventDestroy(a));
  HIP_TRY(hipEventDestroy(b));
  HIP_TRY(hipGetLastError());
  *ms_out = (double)ms / reps;
  return MGH_SUCCESS;
}

// ---- mgh_compare ----------------------------------------------------------------------------------
} // extern "C"

namespace {

// Device scratch of the reduction: the result, then one partial per workgroup.
constexpr size_t kCompareScratchBytes = (size_t)(mgh::kCompareMaxGroups + 1) * sizeof(mgh_error_stats);
// A host array travels to the device in slabs of this many bytes at most.
constexpr size_t kCompareStageBytes = (size_t)64 << 20;

// rows and strides of an array of `shape` with the element strides `str` (str[D - 1] == 1)
LdView compare_view(int D, const uint64_t *shape, const uint64_t *str) {
  LdView V{};
  V.rows = 1;
  for (int k = 0; k < MGH_MAX_DIM; k++) {
    const int d = k - (MGH_MAX_DIM - D);
    V.ext[k] = d >= 0 ? (uint32_t)shape[d] : 1u;
    V.stride[k] = d >= 0 ? str[d] : 0;
    if (k < MGH_MAX_DIM - 1) V.rows *= V.ext[k];
  }
  return V;
}

bool compare_is_dense(int D, const uint64_t *shape, const uint64_t *str) {
  if (!str) return true;
  uint64_t run = 1;
  for (int d = D - 1; d >= 0; d--) {
    if (shape[d] != 1 && str[d] != run) return false;
    run *= shape[d];
  }
  return true;
}

template <typename T>
int compare_launch(int D, const uint64_t *shape, const T *a, const uint64_t *str_a, const T *b, const uint64_t *str_b,
                   mgh_error_stats *d_scratch, hipStream_t st) {
  uint64_t n = 1;
  for (int d = 0; d < D; d++) n *= shape[d];
  const ComparePlan p = compare_plan(n, sizeof(T));
  mgh_error_stats *partials = d_scratch + 1;
  if (p.groups) {
    if (compare_is_dense(D, shape, str_a) && compare_is_dense(D, shape, str_b)) {
      k_compare<T><<<(unsigned)p.groups, 256, 0, st>>>(a, b, n, p.slab, partials);
    } else {
      uint64_t dense[MGH_MAX_DIM];
      compact_strides(D, shape, dense);
      const LdView Va = compare_view(D, shape, str_a ? str_a : dense), Vb = compare_view(D, shape, str_b ? str_b : dense);
      k_compare_ld<T><<<(unsigned)p.groups, 256, 0, st>>>(a, Va, b, Vb, n, p.slab, partials);
    }
    HIP_TRY(hipGetLastError());
  }
  k_compare_final<<<1, 256, 0, st>>>(partials, (uint32_t)p.groups, d_scratch);
  HIP_TRY(hipGetLastError());
  return MGH_SUCCESS;
}

// ... with a mask seen through the element strides str_m and bit0 (mgh_compare_masked_): always the row-wise
// kernel, so that its sums are those of mgh_compare with leading dimensions
template <typename T>
int compare_masked_launch(int D, const uint64_t *shape, const T *a, const uint64_t *str_a, const T *b,
                          const uint64_t *str_b, const uint64_t *words, const uint64_t *str_m, uint64_t bit0,
                          mgh_error_stats *d_scratch, hipStream_t st) {
  uint64_t n = 1;
  for (int d = 0; d < D; d++) n *= shape[d];
  const ComparePlan p = compare_plan(n, sizeof(T));
  mgh_error_stats *partials = d_scratch + 1;
  if (p.groups) {
    uint64_t dense[MGH_MAX_DIM];
    compact_strides(D, shape, dense);
    const LdView Va = compare_view(D, shape, str_a ? str_a : dense), Vb = compare_view(D, shape, str_b ? str_b : dense),
                 Vm = compare_view(D, shape, str_m ? str_m : dense);
    k_compare_masked<T><<<(unsigned)p.groups, 256, 0, st>>>(a, Va, b, Vb, (const unsigned long long *)words, Vm, bit0, n,
                                                             p.slab, partials);
    HIP_TRY(hipGetLastError());
  }
  k_compare_final<<<1, 256, 0, st>>>(partials, (uint32_t)p.groups, d_scratch);
  HIP_TRY(hipGetLastError());
  return MGH_SUCCESS;
}

// Scratch of ONE call: taken from a per-device list of idle buffers (allocated when the list is empty)
// and put back when the call returns, so two calls in flight -- on whatever streams and threads --
// never share one, and the library holds as many buffers as calls have ever run at the same time,
// however many threads come and go. Idle buffers stay until mgh_release_cache (release_idle) or the
// end of the process.
struct CompareScratch {
  int device = -1;
  void *p = nullptr;
  hipStream_t st = nullptr;
  bool drained = false;  // the call's last use of the buffer is known to be over
  static std::mutex &lock() {
    static std::mutex m;
    return m;
  }
  static std::map<int, std::vector<void *>> &idle() {
    static auto *m = new std::map<int, std::vector<void *>>();  // (never destroyed: no HIP call at exit)
    return *m;
  }
  int acquire(int dev) {
    device = dev;
    {
      std::lock_guard<std::mutex> g(lock());
      auto &v = idle()[dev];
      if (!v.empty()) {
        p = v.back();
        v.pop_back();
        return MGH_SUCCESS;
      }
    }
    HIP_TRY(hipMalloc(&p, kCompareScratchBytes));
    return MGH_SUCCESS;
  }
  // frees the idle buffers of every device (buffers of calls in flight are not in the list)
  static void release_idle() {
    std::map<int, std::vector<void *>> gone;
    {
      std::lock_guard<std::mutex> g(lock());
      gone.swap(idle());
    }
    for (auto &kv : gone)
      for (void *q : kv.second) (void)hipFree(q);
  }
  ~CompareScratch() {
    if (!p) return;
    if (!drained) (void)hipStreamSynchronize(st);  // (a call that failed half way: nothing may still write to it)
    std::lock_guard<std::mutex> g(lock());
    idle()[device].push_back(p);
  }
};

bool compare_on_device(const void *p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return at.type == hipMemoryTypeDevice;
}

struct CompareStage {
  void *p = nullptr;
  ~CompareStage() {
    if (p) (void)hipFree(p);
  }
};

template <typename T>
int compare_host(uint64_t n, const T *a, bool a_dev, const T *b, bool b_dev, mgh_error_stats *d_scratch,
                 mgh_error_stats *h_out, hipStream_t st) {
  // slabs of whole 16-byte vectors, so that the alignment of every slab is that of the array
  const uint64_t chunk = std::min<uint64_t>(std::max<uint64_t>(n, 1), kCompareStageBytes / sizeof(T));
  CompareStage sa, sb;
  if (!a_dev) HIP_TRY(hipMalloc(&sa.p, chunk * sizeof(T)));
  if (!b_dev) HIP_TRY(hipMalloc(&sb.p, chunk * sizeof(T)));
  mgh_error_stats total{};
  for (uint64_t at = 0; at < n; at += chunk) {
    const uint64_t len = std::min(chunk, n - at);
    const T *pa = a + at, *pb = b + at;
    if (!a_dev) {
      HIP_TRY(hipMemcpyAsync(sa.p, pa, len * sizeof(T), hipMemcpyHostToDevice, st));
      pa = (const T *)sa.p;
    }
    if (!b_dev) {
      HIP_TRY(hipMemcpyAsync(sb.p, pb, len * sizeof(T), hipMemcpyHostToDevice, st));
      pb = (const T *)sb.p;
    }
    TRY(compare_launch<T>(1, &len, pa, nullptr, pb, nullptr, d_scratch, st));
    mgh_error_stats part;
    HIP_TRY(hipMemcpyAsync(&part, d_scratch, sizeof(part), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    merge(total, part, at);
  }
  *h_out = total;
  return MGH_SUCCESS;
}

template <typename T>
int compare_entry(int D, const uint64_t *shape, const void *a, const uint64_t *ld_a, const void *b, const uint64_t *ld_b,
                  mgh_error_stats *h_out, int device, hipStream_t st) {
  CompareScratch scratch;
  TRY(scratch.acquire(device));
  scratch.st = st;
  mgh_error_stats *d_scratch = (mgh_error_stats *)scratch.p;
  const bool a_dev = compare_on_device(a), b_dev = compare_on_device(b);
  uint64_t sa[MGH_MAX_DIM], sb[MGH_MAX_DIM];
  if (ld_a) compact_strides(D, ld_a, sa);
  if (ld_b) compact_strides(D, ld_b, sb);
  const uint64_t *str_a = ld_a ? sa : nullptr, *str_b = ld_b ? sb : nullptr;
  if (!a_dev || !b_dev) {
    if (!compare_is_dense(D, shape, str_a) || !compare_is_dense(D, shape, str_b))
      return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare: with an array in host memory both arrays must be dense");
    uint64_t n = 1;
    for (int d = 0; d < D; d++) n *= shape[d];
    const int rc = compare_host<T>(n, (const T *)a, a_dev, (const T *)b, b_dev, d_scratch, h_out, st);
    scratch.drained = rc == MGH_SUCCESS;  // (its last step is a synchronise)
    return rc;
  }
  TRY(compare_launch<T>(D, shape, (const T *)a, str_a, (const T *)b, str_b, d_scratch, st));
  HIP_TRY(hipMemcpyAsync(h_out, d_scratch, sizeof(*h_out), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  scratch.drained = true;
  return MGH_SUCCESS;
}

}  // namespace

extern "C" {

int mgh_compare(int D, int dtype, const uint64_t *shape, const void *a, const uint64_t *ld_a, const void *b,
                const uint64_t *ld_b, mgh_error_stats *h_out, int device, void *stream) {
  if (D < 1 || D > MGH_MAX_DIM) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare: D must be 1 .. MGH_MAX_DIM");
  if (dtype != MGH_FLOAT && dtype != MGH_DOUBLE) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare: unknown dtype");
  if (!shape || !a || !b || !h_out) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare: NULL argument");
  for (const uint64_t *ld : {ld_a, ld_b})
    for (int d = 1; ld && d < D; d++)
      if (ld[d] < shape[d]) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare: ld[d] < shape[d]");
  for (int d = 0; d < D; d++)
    if (shape[d] > 0xffffffffull && D > 1)
      return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare: an extent of 2^32 or more in an array of more than one dimension");
  if (device < 0 || device >= mgh_device_count()) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare: no such device");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MGH_FLOAT) return compare_entry<float>(D, shape, a, ld_a, b, ld_b, h_out, device, st);
  return compare_entry<double>(D, shape, a, ld_a, b, ld_b, h_out, device, st);
}

// For highlevel.hip (mgh_verify): the same reduction of two DEVICE arrays given by element strides
// (NULL: dense; the fastest stride is 1), ASYNCHRONOUS on `stream`. d_scratch: mgh_compare_scratch_bytes_()
// bytes of the caller's; the result is the mgh_error_stats at its start.
size_t mgh_compare_scratch_bytes_(void) { return kCompareScratchBytes; }
// (mgh_release_cache: the idle scratch buffers of mgh_compare)
void mgh_compare_release_(void) { CompareScratch::release_idle(); }
int mgh_compare_device_(int D, int dtype, const uint64_t *shape, const void *d_a, const uint64_t *stride_a,
                        const void *d_b, const uint64_t *stride_b, void *d_scratch, void *stream) {
  if (D < 1 || D > MGH_MAX_DIM || !shape || !d_a || !d_b || !d_scratch || (dtype != MGH_FLOAT && dtype != MGH_DOUBLE))
    return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare_device_: bad argument");
  for (const uint64_t *str : {stride_a, stride_b})
    if (str && str[D - 1] != 1) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare_device_: the fastest stride must be 1");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MGH_FLOAT)
    return compare_launch<float>(D, shape, (const float *)d_a, stride_a, (const float *)d_b, stride_b,
                                 (mgh_error_stats *)d_scratch, st);
  return compare_launch<double>(D, shape, (const double *)d_a, stride_a, (const double *)d_b, stride_b,
                                (mgh_error_stats *)d_scratch, st);
}

// mgh_compare with a packed mask (k_compare_masked): a position whose bit is set takes part in NOTHING. n is
// the number of positions compared, i.e. the unmasked ones (the masked count is prod(shape) - n); nonfinite keeps
// its meaning among them; argmax stays the flat index in the logical dense array.
// The mask is a bit array seen through a view of its own, as a and b are: element (i_0 ...) of the logical array
// has bit bit0 + sum_d i_d stride_d of `words`, the strides from ld_m in mgh_set_ld's convention (NULL: dense). So
// a box of a larger array is compared against that array's mask with no gather: ld_m = the array's shape, bit0 =
// the flat index of the box's first element. The caller guarantees that every bit of the view lies inside `words`.
// a, b and words are DEVICE pointers (a host pointer is MGH_ERR_INVALID_ARGUMENT: the caller stages it, as
// mgh_verify does); every extent is below 2^32. Determinism is mgh_compare's: no floating-point atomics, slabs
// fixed by prod(shape). The reduction is the row-wise one of mgh_compare with leading dimensions whatever the
// layout: with an all-zero mask every exact field equals mgh_compare's, and the sums equal, bit for bit, those of
// mgh_compare called with leading dimensions. SYNCHRONOUS like mgh_compare.
// INTERNAL for now (trailing underscore, in no public header; the Python layer and the tests call it): the public
// face of the masked compare is mgh_verify_masked.
int mgh_compare_masked_(int D, int dtype, const uint64_t *shape, const void *a, const uint64_t *ld_a, const void *b,
                       const uint64_t *ld_b, const uint64_t *words, const uint64_t *ld_m, uint64_t bit0,
                       mgh_error_stats *h_out, int device, void *stream) {
  if (D < 1 || D > MGH_MAX_DIM) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare_masked_: D must be 1 .. MGH_MAX_DIM");
  if (dtype != MGH_FLOAT && dtype != MGH_DOUBLE) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare_masked_: unknown dtype");
  if (!shape || !a || !b || !words || !h_out) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare_masked_: NULL argument");
  for (const uint64_t *ld : {ld_a, ld_b, ld_m})
    for (int d = 1; ld && d < D; d++)
      if (ld[d] < shape[d]) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare_masked_: ld[d] < shape[d]");
  for (int d = 0; d < D; d++)
    if (shape[d] == 0 || shape[d] > 0xffffffffull)
      return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare_masked_: an extent of 0, or of 2^32 or more");
  if (device < 0 || device >= mgh_device_count()) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare_masked_: no such device");
  HIP_TRY(hipSetDevice(device));
  if (!compare_on_device(a) || !compare_on_device(b) || !compare_on_device(words))
    return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare_masked_: a, b and words must be device pointers (stage a host array first)");
  hipStream_t st = (hipStream_t)stream;
  CompareScratch scratch;
  TRY(scratch.acquire(device));
  scratch.st = st;
  uint64_t sa[MGH_MAX_DIM], sb[MGH_MAX_DIM], sm[MGH_MAX_DIM];
  if (ld_a) compact_strides(D, ld_a, sa);
  if (ld_b) compact_strides(D, ld_b, sb);
  if (ld_m) compact_strides(D, ld_m, sm);
  const uint64_t *str_a = ld_a ? sa : nullptr, *str_b = ld_b ? sb : nullptr, *str_m = ld_m ? sm : nullptr;
  mgh_error_stats *d_scratch = (mgh_error_stats *)scratch.p;
  if (dtype == MGH_FLOAT)
    TRY(compare_masked_launch<float>(D, shape, (const float *)a, str_a, (const float *)b, str_b, words, str_m, bit0, d_scratch, st));
  else
    TRY(compare_masked_launch<double>(D, shape, (const double *)a, str_a, (const double *)b, str_b, words, str_m, bit0, d_scratch, st));
  HIP_TRY(hipMemcpyAsync(h_out, d_scratch, sizeof(*h_out), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  scratch.drained = true;
  return MGH_SUCCESS;
}

// For highlevel.hip (mgh_verify_masked): mgh_compare_device_ with the mask given by element strides and bit0.
int mgh_compare_masked_device_(int D, int dtype, const uint64_t *shape, const void *d_a, const uint64_t *stride_a,
                               const void *d_b, const uint64_t *stride_b, const uint64_t *d_words, const uint64_t *stride_m,
                               uint64_t bit0, void *d_scratch, void *stream) {
  if (D < 1 || D > MGH_MAX_DIM || !shape || !d_a || !d_b || !d_words || !d_scratch || (dtype != MGH_FLOAT && dtype != MGH_DOUBLE))
    return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare_masked_device_: bad argument");
  for (const uint64_t *str : {stride_a, stride_b, stride_m})
    if (str && str[D - 1] != 1) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare_masked_device_: the fastest stride must be 1");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MGH_FLOAT)
    return compare_masked_launch<float>(D, shape, (const float *)d_a, stride_a, (const float *)d_b, stride_b, d_words,
                                        stride_m, bit0, (mgh_error_stats *)d_scratch, st);
  return compare_masked_launch<double>(D, shape, (const double *)d_a, stride_a, (const double *)d_b, stride_b, d_words,
                                       stride_m, bit0, (mgh_error_stats *)d_scratch, st);
}

// ---- missing-value masks (kernels_mask.hpp) -------------------------------------------------------------
namespace {
// D, shape, dtype and the element count the three entries share (32-bit-free, but refused from 2^32 on
// like mgh_quantize_roundtrip: one record of the lossless stage holds the mask)
int mask_args(const char *who, int D, int dtype, const uint64_t *shape, uint64_t *n_out) {
  const std::string w(who);
  if (D < 1 || D > MGH_MAX_DIM) return fail(MGH_ERR_INVALID_ARGUMENT, w + ": D must be 1 .. MGH_MAX_DIM");
  if (dtype != MGH_FLOAT && dtype != MGH_DOUBLE) return fail(MGH_ERR_INVALID_ARGUMENT, w + ": unknown dtype");
  if (!shape) return fail(MGH_ERR_INVALID_ARGUMENT, w + ": NULL argument");
  uint64_t n = 1;
  for (int d = 0; d < D; d++) {
    if (shape[d] == 0 || shape[d] > 0xffffffffull || n * shape[d] > 0xffffffffull)
      return fail(MGH_ERR_INVALID_ARGUMENT, w + ": 1 .. 2^32 - 1 elements");
    n *= shape[d];
  }
  *n_out = n;
  return MGH_SUCCESS;
}
inline unsigned mask_blocks(uint64_t items) {
  return (unsigned)std::min<uint64_t>(std::max<uint64_t>(items, 1), mgh::mask::kMaxBlocks);
}
// The argument block of a sample (mgh_mask_sample_, mgh_pwrel_inverse_sampled_): both shapes within the sizes of the
// mgh_mask_* calls, `pointers` (the call's arrays are there), shapes and lists right-aligned with leading 1s.
int mask_sample_args(const char *who, int D, int dtype, const uint64_t *shape, const uint64_t *out_shape,
                     const uint32_t *const *d_idx, bool pointers, mgh::mask::MaskSampleArgs &A, uint64_t *n, uint64_t *n_out) {
  static_assert(mgh::kMaskMaxDim == MGH_MAX_DIM, "mask_plan.hpp: kMaskMaxDim");
  TRY(mask_args(who, D, dtype, shape, n));
  TRY(mask_args(who, D, dtype, out_shape, n_out));
  if (!pointers) return fail(MGH_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL argument");
  for (int k = 0; k < MGH_MAX_DIM; k++) {
    const int d = k - (MGH_MAX_DIM - D);
    A.shape[k] = d >= 0 ? (uint32_t)shape[d] : 1u;
    A.out_shape[k] = d >= 0 ? (uint32_t)out_shape[d] : 1u;
    A.idx[k] = d >= 0 && d_idx ? d_idx[d] : nullptr;
    if (!A.idx[k] && A.out_shape[k] > A.shape[k])
      return fail(MGH_ERR_INVALID_ARGUMENT, std::string(who) + ": the identity list (NULL) needs out_shape[d] <= shape[d]");
  }
  return MGH_SUCCESS;
}
}  // namespace

int mgh_mask_scan(int D, int dtype, const uint64_t *shape, const void *data, int flags, double fill_value,
                  uint64_t *words, mgh_mask_stats *stats, void *stream) {
  uint64_t n = 0;
  TRY(mask_args("mgh_mask_scan", D, dtype, shape, &n));
  if (!data || !words || !stats) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_mask_scan: NULL argument");
  if (flags == 0 || (flags & ~(MGH_MASK_NONFINITE | MGH_MASK_VALUE)))
    return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_mask_scan: flags must be MGH_MASK_NONFINITE, MGH_MASK_VALUE or both");
  if ((flags & MGH_MASK_VALUE) && std::isnan(fill_value))
    return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_mask_scan: a NaN fill_value (MGH_MASK_NONFINITE masks NaN)");
  hipStream_t st = (hipStream_t)stream;
  const uint64_t nwords = mgh::mask_words(n);
  unsigned long long *s = reinterpret_cast<unsigned long long *>(stats);
  const unsigned blocks = mask_blocks((nwords + mgh::mask::kWaves * mgh::mask::kScanUnroll - 1) /
                                      (mgh::mask::kWaves * mgh::mask::kScanUnroll));
  mgh::mask::k_mask_stats_begin<<<1, 64, 0, st>>>(s);
  if (dtype == MGH_FLOAT)
    mgh::mask::k_mask_scan<float><<<blocks, mgh::mask::kThreads, 0, st>>>(
        (const float *)data, n, nwords, flags, (float)fill_value, (unsigned long long *)words, s);
  else
    mgh::mask::k_mask_scan<double><<<blocks, mgh::mask::kThreads, 0, st>>>(
        (const double *)data, n, nwords, flags, fill_value, (unsigned long long *)words, s);
  mgh::mask::k_mask_stats_end<<<1, 64, 0, st>>>(s, n);
  HIP_TRY(hipGetLastError());
  return MGH_SUCCESS;
}

// (highlevel.hip: the constant as the bits of (T)c, so that what it derived in double is stored as it is)
int mgh_mask_fill_bits_(int D, int dtype, const uint64_t *shape, const void *data, const uint64_t *words, uint64_t c_bits,
                        void *out, void *stream) {
  uint64_t n = 0;
  TRY(mask_args("mgh_mask_fill", D, dtype, shape, &n));
  if (!data || !words || !out) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_mask_fill: NULL argument");
  const mgh::MaskSegments G = mgh::mask_segments(D, shape);
  const unsigned blocks = mask_blocks((G.total + mgh::mask::kWaves - 1) / mgh::mask::kWaves);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MGH_FLOAT)
    mgh::mask::k_mask_fill<uint32_t><<<blocks, mgh::mask::kThreads, 0, st>>>(
        (const uint32_t *)data, (const unsigned long long *)words, mgh::mask_words(n), G, (uint32_t)c_bits, (uint32_t *)out);
  else
    mgh::mask::k_mask_fill<uint64_t><<<blocks, mgh::mask::kThreads, 0, st>>>(
        (const uint64_t *)data, (const unsigned long long *)words, mgh::mask_words(n), G, c_bits, (uint64_t *)out);
  HIP_TRY(hipGetLastError());
  return MGH_SUCCESS;
}

int mgh_mask_fill(int D, int dtype, const uint64_t *shape, const void *data, const uint64_t *words, double c, void *out,
                  void *stream) {
  return mgh_mask_fill_bits_(D, dtype, shape, data, words, mgh::mask_value_bits(dtype == MGH_DOUBLE, c), out, stream);
}

// (highlevel.hip: the footer's restore_bits as they are)
int mgh_mask_restore_bits_(int D, int dtype, const uint64_t *shape, const uint64_t *words, uint64_t value_bits, void *data,
                           void *stream) {
  uint64_t n = 0;
  TRY(mask_args("mgh_mask_restore", D, dtype, shape, &n));
  if (!words || !data) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_mask_restore: NULL argument");
  const unsigned blocks = mask_blocks((n + mgh::mask::kThreads - 1) / mgh::mask::kThreads);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MGH_FLOAT)
    mgh::mask::k_mask_restore<uint32_t><<<blocks, mgh::mask::kThreads, 0, st>>>(
        (const unsigned long long *)words, n, (uint32_t)value_bits, (uint32_t *)data);
  else
    mgh::mask::k_mask_restore<uint64_t><<<blocks, mgh::mask::kThreads, 0, st>>>(
        (const unsigned long long *)words, n, value_bits, (uint64_t *)data);
  HIP_TRY(hipGetLastError());
  return MGH_SUCCESS;
}

int mgh_mask_restore(int D, int dtype, const uint64_t *shape, const uint64_t *words, double value, void *data, void *stream) {
  return mgh_mask_restore_bits_(D, dtype, shape, words, mgh::mask_value_bits(dtype == MGH_DOUBLE, value), data, stream);
}

// The packed mask of a part of the array -- a level or coarsened grid through its node lists, a window through
// lo + i (k_mask_sample). `words`: the packed mask of a dense array of `shape`. out_words: the packed mask of a
// dense array of out_shape, ceil(prod(out_shape) / 64) words in the same bit order, the unused high bits of the
// last word zero: output (i_0 ... i_{D-1}) is set when bit flat(idx_0[i_0], ..., idx_{D-1}[i_{D-1}]) of `words` is
// set. THIS IS SAMPLING: a node is masked when the element of the full array it stands on is masked; masked
// neighbours do not count.
// d_idx: D pointers on the HOST to DEVICE arrays of out_shape[d] uint32 each; d_idx[d] == NULL (or d_idx == NULL,
// for all) is the identity list 0 ... out_shape[d] - 1 and needs out_shape[d] <= shape[d]. An entry >= shape[d]
// is the caller's error: nothing is read for it and its outputs are 0 -- a bad list cannot make the kernel fault.
// d_count (device, may be NULL): the number of set output bits. ASYNCHRONOUS on `stream`, no allocation, no host
// synchronisation; sizes as for the mgh_mask_* calls, for both shapes. Errors: MGH_ERR_INVALID_ARGUMENT with a
// message, nothing launched.
// INTERNAL for now (trailing underscore, in no public header; highlevel.hip, the Python layer and the tests call
// it): the public faces of the sample are the mgh_decompress_masked_* / mgh_decompress_mask_* readers.
int mgh_mask_sample_(int D, const uint64_t *shape, const uint64_t *words, const uint64_t *out_shape,
                     const uint32_t *const *d_idx, uint64_t *out_words, uint64_t *d_count, void *stream) {
  uint64_t n = 0, n_out = 0;
  mgh::mask::MaskSampleArgs A;
  TRY(mask_sample_args("mgh_mask_sample_", D, MGH_FLOAT, shape, out_shape, d_idx, words && out_words, A, &n, &n_out));
  hipStream_t st = (hipStream_t)stream;
  const uint64_t nwords_out = mgh::mask_words(n_out);
  if (d_count) HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
  mgh::mask::k_mask_sample<<<mask_blocks((nwords_out + mgh::mask::kWaves - 1) / mgh::mask::kWaves), mgh::mask::kThreads, 0, st>>>(
      (const unsigned long long *)words, A, n_out, nwords_out, (unsigned long long *)out_words, (unsigned long long *)d_count);
  HIP_TRY(hipGetLastError());
  return MGH_SUCCESS;
}

// ---- pointwise relative error bound (kernels_pwrel.hpp; classes and tolerance: pwrel_plan.hpp) ------------
// The streaming passes of mgh_compress_pwrel and its readers (include/mgard_hip.h describes the first three beside
// mgh_pwrel_stats / mgh_pwrel_compare). Like the mgh_mask_* calls: no hierarchy, dense DEVICE arrays on the current
// device, 1 ... 2^32 - 1 elements, the stream last. INTERNAL for now (trailing underscore, in no public header; the
// Python layer and the tests call them): the public faces are mgh_compress_pwrel, mgh_decompress_pwrel and
// mgh_verify_pwrel.
namespace {
int pwrel_floor_arg(const char *who, double abs_floor) {
  if (!(abs_floor >= 0.0) || std::isinf(abs_floor))
    return fail(MGH_ERR_INVALID_ARGUMENT, std::string(who) + ": abs_floor must be finite and >= 0");
  return MGH_SUCCESS;
}
}  // namespace

// y_out (may be data) = (T)log2((double)|x|) at valid positions, 0 at the others; mask_words / flag_words:
// ceil(n / 64) words each; *stats: a DEVICE mgh_pwrel_stats. ASYNCHRONOUS on `stream`.
int mgh_pwrel_forward_(int D, int dtype, const uint64_t *shape, const void *data, double abs_floor, void *y_out,
                       uint64_t *mask_words, uint64_t *flag_words, mgh_pwrel_stats *stats, void *stream) {
  uint64_t n = 0;
  TRY(mask_args("mgh_pwrel_forward", D, dtype, shape, &n));
  if (!data || !y_out || !mask_words || !flag_words || !stats) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_pwrel_forward: NULL argument");
  TRY(pwrel_floor_arg("mgh_pwrel_forward", abs_floor));
  static_assert(sizeof(mgh_pwrel_stats) == 6 * sizeof(unsigned long long), "kernels_pwrel.hpp: the statistics' six words");
  hipStream_t st = (hipStream_t)stream;
  const uint64_t nwords = mgh::mask_words(n);
  unsigned long long *s = reinterpret_cast<unsigned long long *>(stats);
  const unsigned blocks = mask_blocks((nwords + mgh::mask::kWaves * mgh::mask::kScanUnroll - 1) /
                                      (mgh::mask::kWaves * mgh::mask::kScanUnroll));
  const double floor_eff = mgh::pwrel_floor_eff(dtype == MGH_DOUBLE, abs_floor);
  mgh::pwrel::k_pwrel_stats_begin<<<1, 64, 0, st>>>(s);
  if (dtype == MGH_FLOAT)
    mgh::pwrel::k_pwrel_forward<float><<<blocks, mgh::mask::kThreads, 0, st>>>(
        (const float *)data, n, nwords, floor_eff, (float *)y_out, (unsigned long long *)mask_words,
        (unsigned long long *)flag_words, s);
  else
    mgh::pwrel::k_pwrel_forward<double><<<blocks, mgh::mask::kThreads, 0, st>>>(
        (const double *)data, n, nwords, floor_eff, (double *)y_out, (unsigned long long *)mask_words,
        (unsigned long long *)flag_words, s);
  mgh::pwrel::k_pwrel_stats_end<<<1, 64, 0, st>>>(s, n);
  HIP_TRY(hipGetLastError());
  return MGH_SUCCESS;
}

// In place over the decoded y': quiet NaN / +0.0 at masked positions, +-exp2(y') clamped to the normal range of T
// elsewhere. ASYNCHRONOUS on `stream`.
int mgh_pwrel_inverse_(int D, int dtype, const uint64_t *shape, const uint64_t *mask_words, const uint64_t *flag_words,
                       void *data_inout, void *stream) {
  uint64_t n = 0;
  TRY(mask_args("mgh_pwrel_inverse", D, dtype, shape, &n));
  if (!mask_words || !flag_words || !data_inout) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_pwrel_inverse: NULL argument");
  const unsigned blocks = mask_blocks((n + mgh::mask::kThreads - 1) / mgh::mask::kThreads);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MGH_FLOAT)
    mgh::pwrel::k_pwrel_inverse<float><<<blocks, mgh::mask::kThreads, 0, st>>>(
        (const unsigned long long *)mask_words, (const unsigned long long *)flag_words, n, (float *)data_inout);
  else
    mgh::pwrel::k_pwrel_inverse<double><<<blocks, mgh::mask::kThreads, 0, st>>>(
        (const unsigned long long *)mask_words, (const unsigned long long *)flag_words, n, (double *)data_inout);
  HIP_TRY(hipGetLastError());
  return MGH_SUCCESS;
}

// mgh_pwrel_inverse_ over a VIEW of the array -- a level or coarsened array through its node lists, a window through
// lo + i -- in one pass (k_pwrel_inverse_sampled). data_inout: the dense y' of out_shape; mask_words / flag_words: the
// packed maps of the FULL array of `shape`. Element (i_0 ...) of the view takes both bits from element
// (idx_0[i_0] ...) of the full array: SAMPLING, as mgh_mask_sample_ does it, whose result for each map followed by
// mgh_pwrel_inverse_ this call equals bit for bit, without the two sampled maps in between. d_idx, the sizes of both
// shapes, the identity list and an entry >= shape[d] (nothing read, both bits clear: a valid, positive element) are
// mgh_mask_sample_'s. ASYNCHRONOUS on `stream`, no allocation, no host synchronisation. INTERNAL like the others.
int mgh_pwrel_inverse_sampled_(int D, int dtype, const uint64_t *shape, const uint64_t *mask_words, const uint64_t *flag_words,
                               const uint64_t *out_shape, const uint32_t *const *d_idx, void *data_inout, void *stream) {
  uint64_t n = 0, n_out = 0;
  mgh::mask::MaskSampleArgs A;
  TRY(mask_sample_args("mgh_pwrel_inverse_sampled_", D, dtype, shape, out_shape, d_idx, mask_words && flag_words && data_inout,
                       A, &n, &n_out));
  // a group of 2^lg lanes per row: the whole wave for rows of more than 32 elements, else the smallest that covers one
  const uint32_t nf = A.out_shape[MGH_MAX_DIM - 1], rows = (uint32_t)(n_out / nf);
  int lg = 6;
  while (lg > 0 && (1u << (lg - 1)) >= nf) lg--;
  const uint64_t rows_per_block = (uint64_t)mgh::mask::kWaves << (6 - lg);
  const unsigned blocks = mask_blocks((rows + rows_per_block - 1) / rows_per_block);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MGH_FLOAT)
    mgh::pwrel::k_pwrel_inverse_sampled<float><<<blocks, mgh::mask::kThreads, 0, st>>>(
        (const unsigned long long *)mask_words, (const unsigned long long *)flag_words, A, rows, lg, (float *)data_inout);
  else
    mgh::pwrel::k_pwrel_inverse_sampled<double><<<blocks, mgh::mask::kThreads, 0, st>>>(
        (const unsigned long long *)mask_words, (const unsigned long long *)flag_words, A, rows, lg, (double *)data_inout);
  HIP_TRY(hipGetLastError());
  return MGH_SUCCESS;
}

// mgh_pwrel_compare of an original against a reconstruction, both dense DEVICE arrays of the current device.
// SYNCHRONOUS like mgh_compare: *out (host) is filled when the call returns; the scratch is mgh_compare's.
int mgh_compare_pwrel_(int D, int dtype, const uint64_t *shape, const void *original, const void *reconstructed,
                       double abs_floor, mgh_pwrel_compare *out, void *stream) {
  uint64_t n = 0;
  TRY(mask_args("mgh_compare_pwrel", D, dtype, shape, &n));
  if (!original || !reconstructed || !out) return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare_pwrel: NULL argument");
  TRY(pwrel_floor_arg("mgh_compare_pwrel", abs_floor));
  if (!compare_on_device(original) || !compare_on_device(reconstructed))
    return fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compare_pwrel: both arrays must be device pointers (stage a host array first)");
  static_assert(sizeof(mgh_pwrel_compare) <= sizeof(mgh_error_stats), "the scratch of mgh_compare holds the partials");
  int device = 0;
  HIP_TRY(hipGetDevice(&device));
  hipStream_t st = (hipStream_t)stream;
  CompareScratch scratch;
  TRY(scratch.acquire(device));
  scratch.st = st;
  mgh_pwrel_compare *d_out = (mgh_pwrel_compare *)scratch.p, *partials = d_out + 1;
  const size_t esz = dtype == MGH_DOUBLE ? 8 : 4;
  const mgh::ComparePlan p = mgh::compare_plan(n, esz);
  const double floor_eff = mgh::pwrel_floor_eff(dtype == MGH_DOUBLE, abs_floor);
  if (dtype == MGH_FLOAT)
    mgh::pwrel::k_compare_pwrel<float><<<(unsigned)p.groups, 256, 0, st>>>((const float *)original, (const float *)reconstructed,
                                                                          n, p.slab, floor_eff, partials);
  else
    mgh::pwrel::k_compare_pwrel<double><<<(unsigned)p.groups, 256, 0, st>>>((const double *)original,
                                                                           (const double *)reconstructed, n, p.slab, floor_eff,
                                                                           partials);
  HIP_TRY(hipGetLastError());
  mgh::pwrel::k_compare_pwrel_final<<<1, 256, 0, st>>>(partials, (uint32_t)p.groups, d_out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, d_out, sizeof(*out), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  scratch.drained = true;
  return MGH_SUCCESS;
}

} // extern "C"

// ---- region of interest (kernels_roi.hpp; the scheme and the bound: roi_plan.hpp) ---------------------------
// The two streaming passes of mgh_compress_roi and mgh_decompress_roi over a box (lo, ext) of a dense DEVICE array
// of `shape` on the current device, 1 ... 2^32 - 1 elements, every extent of the box at least 1. ASYNCHRONOUS on
// `stream`, no allocation, no host synchronisation. INTERNAL for now (trailing underscore, in no public header;
// highlevel.hip, the Python layer and the tests call them): the public faces are mgh_compress_roi, mgh_decompress_roi
// and mgh_verify_roi.
namespace {
struct BoxLaunch {
  mgh::LdView V;
  uint64_t offset = 0;  // of the box's first element in the array
  uint32_t nf = 1;
  int lg = 6;
  unsigned blocks = 1;
};
int box_args(const char *who, int D, int dtype, const uint64_t *shape, const uint64_t *lo, const uint64_t *ext, bool pointers,
             BoxLaunch &B) {
  const std::string w(who);
  if (D < 1 || D > MGH_MAX_DIM) return fail(MGH_ERR_INVALID_ARGUMENT, w + ": D must be 1 .. MGH_MAX_DIM");
  if (dtype != MGH_FLOAT && dtype != MGH_DOUBLE) return fail(MGH_ERR_INVALID_ARGUMENT, w + ": unknown dtype");
  if (!shape || !lo || !ext || !pointers) return fail(MGH_ERR_INVALID_ARGUMENT, w + ": NULL argument");
  uint64_t n = 1;
  for (int d = 0; d < D; d++) {
    if (shape[d] == 0 || shape[d] > 0xffffffffull || n * shape[d] > 0xffffffffull)
      return fail(MGH_ERR_INVALID_ARGUMENT, w + ": 1 .. 2^32 - 1 elements");
    n *= shape[d];
    if (ext[d] == 0 || lo[d] >= shape[d] || ext[d] > shape[d] - lo[d])
      return fail(MGH_ERR_INVALID_ARGUMENT, w + ": the box leaves the array");
  }
  uint64_t stride = 1;
  B.V.rows = 1;
  for (int k = MGH_MAX_DIM - 1; k >= 0; k--) {
    const int d = k - (MGH_MAX_DIM - D);
    B.V.ext[k] = d >= 0 ? (uint32_t)ext[d] : 1u;
    B.V.stride[k] = d >= 0 ? stride : 0;
    if (d >= 0) {
      B.offset += lo[d] * stride;
      stride *= shape[d];
    }
    if (k < MGH_MAX_DIM - 1) B.V.rows *= B.V.ext[k];
  }
  // a group of 2^lg lanes per row: the whole wave for rows of more than 32 elements, else the smallest that covers one
  B.nf = B.V.ext[MGH_MAX_DIM - 1];
  B.lg = 6;
  while (B.lg > 0 && (1u << (B.lg - 1)) >= B.nf) B.lg--;
  const uint64_t rows_per_block = (uint64_t)mgh::roi::kWaves << (6 - B.lg);
  B.blocks = (unsigned)std::min<uint64_t>((B.V.rows + rows_per_block - 1) / rows_per_block, mgh::roi::kMaxBlocks);
  return MGH_SUCCESS;
}
}  // namespace

extern "C" {

// the scratch of mgh_box_residual_: the statistics at its start, the workgroups' partials behind them
size_t mgh_box_scratch_bytes_(void) { return (1 + (size_t)mgh::roi::kMaxBlocks) * sizeof(mgh::roi::BoxStats); }

// r_out (dense, prod(ext) elements) = fl_T(x[box] - b[box]); d_scratch: mgh_box_scratch_bytes_() bytes of DEVICE
// memory, at whose start the call leaves {double max |r|, double max |x|, u64 positions whose x or r is not finite,
// u64 0}, the maxima over the finite values of the box. Deterministic: maxima and counts, no atomics.
int mgh_box_residual_(int D, int dtype, const uint64_t *shape, const uint64_t *lo, const uint64_t *ext, const void *x,
                      const void *b, void *r_out, void *d_scratch, void *stream) {
  BoxLaunch B;
  TRY(box_args("mgh_box_residual_", D, dtype, shape, lo, ext, x && b && r_out && d_scratch, B));
  static_assert(sizeof(mgh::roi::BoxStats) == 32, "kernels_roi.hpp: the statistics' four words");
  hipStream_t st = (hipStream_t)stream;
  mgh::roi::BoxStats *out = (mgh::roi::BoxStats *)d_scratch, *partials = out + 1;
  if (dtype == MGH_FLOAT)
    mgh::roi::k_box_residual<float><<<B.blocks, mgh::roi::kThreads, 0, st>>>(
        (const float *)x + B.offset, (const float *)b + B.offset, B.V, B.nf, B.lg, (float *)r_out, partials);
  else
    mgh::roi::k_box_residual<double><<<B.blocks, mgh::roi::kThreads, 0, st>>>(
        (const double *)x + B.offset, (const double *)b + B.offset, B.V, B.nf, B.lg, (double *)r_out, partials);
  HIP_TRY(hipGetLastError());
  mgh::roi::k_box_stats_final<<<1, mgh::roi::kThreads, 0, st>>>(partials, B.blocks, out);
  HIP_TRY(hipGetLastError());
  return MGH_SUCCESS;
}

// data_inout[box] = fl_T(data_inout[box] + r), r dense of prod(ext) elements; nothing outside the box is touched.
int mgh_box_add_(int D, int dtype, const uint64_t *shape, const uint64_t *lo, const uint64_t *ext, const void *r,
                 void *data_inout, void *stream) {
  BoxLaunch B;
  TRY(box_args("mgh_box_add_", D, dtype, shape, lo, ext, r && data_inout, B));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MGH_FLOAT)
    mgh::roi::k_box_add<float><<<B.blocks, mgh::roi::kThreads, 0, st>>>((float *)data_inout + B.offset, B.V, B.nf, B.lg,
                                                                        (const float *)r);
  else
    mgh::roi::k_box_add<double><<<B.blocks, mgh::roi::kThreads, 0, st>>>((double *)data_inout + B.offset, B.V, B.nf, B.lg,
                                                                         (const double *)r);
  HIP_TRY(hipGetLastError());
  return MGH_SUCCESS;
}

} // extern "C"
