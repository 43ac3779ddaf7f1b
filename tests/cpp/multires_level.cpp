// Reconstruction at a coarser level through the C++ mirrors (extensions: decompress_level,
// infer_level_shape, Compressor::RecomposeToLevel) against the C ABI they wrap: a level
// l_target - 1 call must return the shape and the bits of mgh_decompress_level /
// mgh_recompose_to_level.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime.h>

#include "compress_hip.hpp"
#include "compress_x_hip.hpp"

static void *dalloc(size_t n) {
  void *p = nullptr;
  return hipMalloc(&p, n) == hipSuccess ? p : nullptr;
}
static void dfree(void *p) { (void)hipFree(p); }

int main() {
  const mgard_hip::SIZE n1 = 70, n2 = 65, n3 = 129;
  std::vector<mgard_hip::SIZE> shape{n1, n2, n3};
  const size_t n = n1 * n2 * n3;
  std::vector<float> in(n);
  for (size_t i = 0; i < n1; i++)
    for (size_t j = 0; j < n2; j++)
      for (size_t k = 0; k < n3; k++)
        in[(i * n2 + j) * n3 + k] = std::sin(0.05f * i) * std::cos(0.07f * j) + 0.3f * std::sin(0.04f * k);
  mgard_hip::HighLevelConfig config;
  void *compressed = nullptr;
  size_t compressed_size = 0;
  auto st = mgard_hip::compress(3, mgard_hip::data_type::Float, shape, 1e-3, std::numeric_limits<double>::infinity(),
                                mgard_hip::error_bound_type::REL, in.data(), compressed, compressed_size, config, false);
  if (st != mgard_hip::compress_status_type::Success) {
    std::printf("compress failed: %s\n", mgh_last_error());
    return 1;
  }
  // ---- high level: shape and bits of the C ABI
  int lt = -1;
  std::vector<mgard_hip::SIZE> ls;
  if (mgard_hip::infer_level_shape(compressed, compressed_size, -1, config, ls, lt) !=
          mgard_hip::compress_status_type::Success || !ls.empty() || lt < 2) {
    std::printf("infer_level_shape(-1): l_target %d\n", lt);
    return 1;
  }
  const int level = lt - 1;
  if (mgard_hip::infer_level_shape(compressed, compressed_size, level, config, ls, lt) !=
          mgard_hip::compress_status_type::Success ||
      mgard_hip::infer_level_shape(compressed, compressed_size, lt + 1, config, ls, lt) ==
          mgard_hip::compress_status_type::Success || !ls.empty()) {
    std::printf("infer_level_shape: status\n");
    return 1;
  }
  (void)mgard_hip::infer_level_shape(compressed, compressed_size, level, config, ls, lt);
  mgh_config c;
  mgh_config_default(&c);
  int D = 0, lt2 = 0;
  uint64_t shp[MGH_MAX_DIM];
  if (mgh_infer_level_shape(compressed, compressed_size, &c, level, &D, shp, &lt2) != MGH_SUCCESS || D != 3 ||
      lt2 != lt || ls != std::vector<mgard_hip::SIZE>(shp, shp + 3) ||
      ls != std::vector<mgard_hip::SIZE>{n1 / 2 + 1, n2 / 2 + 1, n3 / 2 + 1}) {
    std::printf("level shape mismatch\n");
    return 1;
  }
  const size_t m = ls[0] * ls[1] * ls[2];
  void *a = nullptr, *b = nullptr, *x = nullptr;
  st = mgard_hip::decompress_level(compressed, compressed_size, level, a, config, false);
  auto stx = mgard_x::decompress_level(compressed, compressed_size, level, x, mgard_x::Config(), false);
  if (st != mgard_hip::compress_status_type::Success || stx != mgard_x::compress_status_type::Success ||
      mgh_decompress_level(compressed, compressed_size, level, &b, &c, 0) != MGH_SUCCESS) {
    std::printf("decompress_level failed: %s\n", mgh_last_error());
    return 1;
  }
  if (std::memcmp(a, b, m * sizeof(float)) != 0 || std::memcmp(x, b, m * sizeof(float)) != 0) {
    std::printf("decompress_level: the mirrors and the C ABI disagree\n");
    return 1;
  }
  void *bad = nullptr;
  if (mgard_hip::decompress_level(compressed, compressed_size, lt + 1, bad, config, false) ==
      mgard_hip::compress_status_type::Success) {
    std::printf("a level above l_target was accepted\n");
    return 1;
  }
  // ---- low level: Compressor::RecomposeToLevel against mgh_recompose_to_level
  {
    using namespace mgard_hip;
    Hierarchy<3, float> hierarchy(shape, config);
    Compressor<3, float> compressor(hierarchy, config, DeviceAllocator{dalloc, dfree});
    float *d = (float *)dalloc(n * sizeof(float)), *o1 = (float *)dalloc(m * sizeof(float)),
          *o2 = (float *)dalloc(m * sizeof(float));
    (void)hipMemcpy(d, in.data(), n * sizeof(float), hipMemcpyHostToDevice);
    compressor.Decompose(d);
    compressor.RecomposeToLevel(d, level, o1);
    if (mgh_recompose_to_level(hierarchy.handle(), d, level, o2, nullptr) != MGH_SUCCESS) return 1;
    std::vector<float> h1(m), h2(m);
    (void)hipMemcpy(h1.data(), o1, m * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipMemcpy(h2.data(), o2, m * sizeof(float), hipMemcpyDeviceToHost);
    if (std::memcmp(h1.data(), h2.data(), m * sizeof(float)) != 0) {
      std::printf("RecomposeToLevel: the mirror and the C ABI disagree\n");
      return 1;
    }
    // (the level's nodes are every second node of the data and the last: smooth data stays close)
    double err = 0;
    for (size_t i = 0; i < ls[0]; i++) {
      const size_t I = i + 1 < ls[0] ? 2 * i : n1 - 1;
      err = std::fmax(err, std::fabs((double)h1[(i * ls[1]) * ls[2]] - (double)in[(I * n2) * n3]));
    }
    std::printf("level %d of %d: shape %llu x %llu x %llu, |level - data| at the shared nodes <= %.3e\n", level, lt,
                (unsigned long long)ls[0], (unsigned long long)ls[1], (unsigned long long)ls[2], err);
    dfree(d);
    dfree(o1);
    dfree(o2);
  }
  std::free(a);
  std::free(b);
  std::free(x);
  std::free(compressed);
  std::printf("OK\n");
  return 0;
}
