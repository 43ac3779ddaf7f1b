// TEST INFRASTRUCTURE -- a C ABI over the reference MGARD-X's own SERIAL code path.
//
// This file is ours; it only #includes the reference's headers. oracle/build_ref.py compiles it
// once per (dimension, type) against a reference checkout, with
//   -DMGXR_D=<1..5> -DMGXR_T=<float|double> -DMGXR_SFX=<3d_f32 ...>
// and links it with the reference's explicit-instantiation units (generated from its *.cpp.in
// files at build time) into oracle/_ref/libmgx_ref.so. oracle/ref.py binds the result.
//
// Exposed per (D, T), every name suffixed _<D>d_<f32|f64>:
//   mgxr_hier_create(shape, coords|NULL, normalize_coordinates, max_level) -> handle
//   mgxr_hier_destroy, mgxr_l_target, mgxr_level_shape
//   mgxr_decompose / mgxr_recompose      data_refactoring::DataRefactor (Config default: MultiDim)
//   mgxr_quantize / mgxr_dequantize      LinearQuantizer<D, T, QUANTIZED_INT, SERIAL>
//   mgxr_norm                            norm_calculator
// Every array is a dense row-major host buffer (SERIAL "device" memory is host memory).
//
// The Huffman stage is not instantiated (it would pull in zstd): LinearQuantizer::Quantize and
// Dequantize are templated on the lossless type and only touch huffman.outlier_count and the
// outlier buffers of huffman.workspace, which the stub below carries.

#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "mgard-x/RuntimeX/RuntimeX.h"
#include "mgard-x/Config/Config.h"
#include "mgard-x/Hierarchy/Hierarchy.h"
#include "mgard-x/DataRefactoring/DataRefactor.hpp"
#include "mgard-x/Quantization/LinearQuantization.hpp"
#include "mgard-x/CompressionLowLevel/NormCalculator.hpp"

#if !defined(MGXR_D) || !defined(MGXR_T) || !defined(MGXR_SFX)
#error "compile with -DMGXR_D=<dims> -DMGXR_T=<float|double> -DMGXR_SFX=<suffix>"
#endif

#define MGXR_CAT2(a, b) a##_##b
#define MGXR_CAT(a, b) MGXR_CAT2(a, b)
#define MGXR(name) MGXR_CAT(name, MGXR_SFX)

namespace {

using namespace mgard_x;
using Dev = SERIAL;
constexpr DIM D = MGXR_D;
using T = MGXR_T;

struct StubWorkspace {
  Array<1, ATOMIC_IDX, Dev> outlier_count_array;
  Array<1, ATOMIC_IDX, Dev> outlier_idx_array;
  Array<1, QUANTIZED_INT, Dev> outlier_array;
  SubArray<1, ATOMIC_IDX, Dev> outlier_count_subarray;
  SubArray<1, ATOMIC_IDX, Dev> outlier_idx_subarray;
  SubArray<1, QUANTIZED_INT, Dev> outlier_subarray;

  explicit StubWorkspace(SIZE cap)
      : outlier_count_array({1}), outlier_idx_array({cap}), outlier_array({cap}) {
    outlier_count_array.memset(0);
    outlier_count_subarray = SubArray<1, ATOMIC_IDX, Dev>(outlier_count_array);
    outlier_idx_subarray = SubArray<1, ATOMIC_IDX, Dev>(outlier_idx_array);
    outlier_subarray = SubArray<1, QUANTIZED_INT, Dev>(outlier_array);
  }
};

struct StubHuffman {
  ATOMIC_IDX outlier_count = 0;
  StubWorkspace workspace;
  explicit StubHuffman(SIZE cap) : workspace(cap) {}
};

struct StubLossless {
  StubHuffman huffman;
  explicit StubLossless(SIZE cap) : huffman(cap) {}
};

struct Handle {
  Config config;
  Hierarchy<D, T, Dev> *hierarchy;
};

void init_runtime() {
  static bool done = false;
  if (!done) {
    DeviceRuntime<Dev>::Initialize();
    done = true;
  }
}

std::vector<SIZE> to_shape(const uint64_t *shape) {
  return std::vector<SIZE>(shape, shape + D);
}

SIZE total(Hierarchy<D, T, Dev> &h) { return h.total_num_elems(); }

Config quantizer_config(uint64_t dict_size, int prep_huffman) {
  Config config;
  config.huff_dict_size = (SIZE)dict_size;
  // LinearQuantizer: prep_huffman = (config.lossless != lossless_type::CPU_Lossless)
  config.lossless = prep_huffman ? lossless_type::Huffman : lossless_type::CPU_Lossless;
  config.apply();
  return config;
}

} // namespace

extern "C" {

void *MGXR(mgxr_hier_create)(const uint64_t *shape, T *const *coords, int normalize_coordinates,
                             uint64_t max_level) {
  init_runtime();
  Handle *hd = new Handle();
  hd->config.normalize_coordinates = normalize_coordinates != 0;
  hd->config.max_larget_level = (SIZE)max_level;
  hd->config.apply();
  std::vector<SIZE> shp = to_shape(shape);
  for (DIM d = 0; d < D; d++)
    if (shp[d] < 3) {
      delete hd;
      return nullptr;
    }
  if (coords) {
    std::vector<T *> c(coords, coords + D);
    hd->hierarchy = new Hierarchy<D, T, Dev>(shp, c, hd->config);
  } else {
    hd->hierarchy = new Hierarchy<D, T, Dev>(shp, hd->config);
  }
  return hd;
}

void MGXR(mgxr_hier_destroy)(void *h) {
  Handle *hd = (Handle *)h;
  delete hd->hierarchy;
  delete hd;
}

int MGXR(mgxr_l_target)(void *h) { return (int)((Handle *)h)->hierarchy->l_target(); }

void MGXR(mgxr_level_shape)(void *h, int l, uint64_t *out) {
  std::vector<SIZE> s = ((Handle *)h)->hierarchy->level_shape((SIZE)l);
  for (DIM d = 0; d < D; d++)
    out[d] = s[d];
}

// In place on a dense array of the hierarchy's shape.
void MGXR(mgxr_decompose)(void *h, T *data) {
  Handle *hd = (Handle *)h;
  Hierarchy<D, T, Dev> &hier = *hd->hierarchy;
  data_refactoring::DataRefactor<D, T, Dev> refactor(hier, hd->config);
  Array<D, T, Dev> a(hier.level_shape(hier.l_target()), data);
  refactor.Decompose(SubArray<D, T, Dev>(a), 0);
  DeviceRuntime<Dev>::SyncQueue(0);
}

void MGXR(mgxr_recompose)(void *h, T *data) {
  Handle *hd = (Handle *)h;
  Hierarchy<D, T, Dev> &hier = *hd->hierarchy;
  data_refactoring::DataRefactor<D, T, Dev> refactor(hier, hd->config);
  Array<D, T, Dev> a(hier.level_shape(hier.l_target()), data);
  refactor.Recompose(SubArray<D, T, Dev>(a), 0);
  DeviceRuntime<Dev>::SyncQueue(0);
}

// Returns the outlier count; at most `cap` (index, value) pairs are written.
uint64_t MGXR(mgxr_quantize)(void *h, T *coeffs, int ebtype, T tol, T s, T norm,
                             uint64_t dict_size, int prep_huffman, int64_t *q,
                             uint64_t *outlier_idx, int64_t *outlier_val, uint64_t cap) {
  Handle *hd = (Handle *)h;
  Hierarchy<D, T, Dev> &hier = *hd->hierarchy;
  Config config = quantizer_config(dict_size, prep_huffman);
  config.normalize_coordinates = hd->config.normalize_coordinates;
  config.max_larget_level = hd->config.max_larget_level;
  LinearQuantizer<D, T, QUANTIZED_INT, Dev> quantizer(hier, config);
  std::vector<SIZE> shp = hier.level_shape(hier.l_target());
  Array<D, T, Dev> in(shp, coeffs);
  Array<D, QUANTIZED_INT, Dev> out(shp, (QUANTIZED_INT *)q);
  StubLossless lossless(std::max<SIZE>(total(hier), 1));
  quantizer.Quantize(SubArray<D, T, Dev>(in), (error_bound_type)ebtype, tol, s, norm,
                     SubArray<D, QUANTIZED_INT, Dev>(out), lossless, 0);
  DeviceRuntime<Dev>::SyncQueue(0);
  uint64_t n = lossless.huffman.outlier_count;
  uint64_t k = n < cap ? n : cap;
  ATOMIC_IDX *idx = lossless.huffman.workspace.outlier_idx_subarray.data();
  QUANTIZED_INT *val = lossless.huffman.workspace.outlier_subarray.data();
  for (uint64_t i = 0; i < k; i++) {
    outlier_idx[i] = (uint64_t)idx[i];
    outlier_val[i] = (int64_t)val[i];
  }
  return n;
}

void MGXR(mgxr_dequantize)(void *h, const int64_t *q, int ebtype, T tol, T s, T norm,
                           uint64_t dict_size, int prep_huffman, const uint64_t *outlier_idx,
                           const int64_t *outlier_val, uint64_t n_outliers, T *out) {
  Handle *hd = (Handle *)h;
  Hierarchy<D, T, Dev> &hier = *hd->hierarchy;
  Config config = quantizer_config(dict_size, prep_huffman);
  config.normalize_coordinates = hd->config.normalize_coordinates;
  config.max_larget_level = hd->config.max_larget_level;
  LinearQuantizer<D, T, QUANTIZED_INT, Dev> quantizer(hier, config);
  std::vector<SIZE> shp = hier.level_shape(hier.l_target());
  SIZE n = total(hier);
  // Dequantize restores the outliers into the quantized array: work on a copy of it.
  std::vector<QUANTIZED_INT> qcopy(q, q + n);
  Array<D, QUANTIZED_INT, Dev> qa(shp, qcopy.data());
  Array<D, T, Dev> oa(shp, out);
  StubLossless lossless(std::max<SIZE>((SIZE)n_outliers, 1));
  ATOMIC_IDX *idx = lossless.huffman.workspace.outlier_idx_subarray.data();
  QUANTIZED_INT *val = lossless.huffman.workspace.outlier_subarray.data();
  for (uint64_t i = 0; i < n_outliers; i++) {
    idx[i] = (ATOMIC_IDX)outlier_idx[i];
    val[i] = (QUANTIZED_INT)outlier_val[i];
  }
  lossless.huffman.outlier_count = (ATOMIC_IDX)n_outliers;
  quantizer.Dequantize(SubArray<D, T, Dev>(oa), (error_bound_type)ebtype, tol, s, norm,
                       SubArray<D, QUANTIZED_INT, Dev>(qa), lossless, 0);
  DeviceRuntime<Dev>::SyncQueue(0);
}

// norm_calculator on a dense array of the given shape (L-inf for s = inf, else L2).
T MGXR(mgxr_norm)(const uint64_t *shape, T *data, T s, int normalize_coordinates) {
  init_runtime();
  Config config;
  config.apply();
  std::vector<SIZE> shp = to_shape(shape);
  SIZE n = 1;
  for (DIM d = 0; d < D; d++)
    n *= shp[d];
  Array<D, T, Dev> a(shp, data);
  Array<1, T, Dev> workspace({n});
  Array<1, T, Dev> norm_array({1});
  T norm = norm_calculator(a, SubArray<1, T, Dev>(workspace), SubArray<1, T, Dev>(norm_array),
                           s, normalize_coordinates != 0);
  return norm;
}

} // extern "C"
