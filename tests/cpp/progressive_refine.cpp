// The progressive reader through the C++ mirror (mgard_hip::ProgressiveReader): open, two refines,
// close -- each result against the bytes of mgh_decompress_level at the same level.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "compress_hip.hpp"

int main() {
  const mgard_hip::SIZE n1 = 70, n2 = 65, n3 = 129;
  std::vector<mgard_hip::SIZE> shape{n1, n2, n3};
  std::vector<float> in(n1 * n2 * n3);
  for (size_t i = 0; i < n1; i++)
    for (size_t j = 0; j < n2; j++)
      for (size_t k = 0; k < n3; k++)
        in[(i * n2 + j) * n3 + k] = std::sin(0.05f * i) * std::cos(0.07f * j) + 0.3f * std::sin(0.04f * k);
  mgard_hip::HighLevelConfig config;
  config.reorder = 1;
  void *compressed = nullptr;
  size_t compressed_size = 0;
  if (mgard_hip::compress(3, mgard_hip::data_type::Float, shape, 1e-3, std::numeric_limits<double>::infinity(),
                          mgard_hip::error_bound_type::REL, in.data(), compressed, compressed_size, config,
                          false) != mgard_hip::compress_status_type::Success) {
    std::printf("compress failed: %s\n", mgh_last_error());
    return 1;
  }
  int lt = -1;
  std::vector<mgard_hip::SIZE> ls;
  if (mgard_hip::infer_level_shape(compressed, compressed_size, -1, config, ls, lt) !=
          mgard_hip::compress_status_type::Success || lt < 2) {
    std::printf("infer_level_shape: l_target %d\n", lt);
    return 1;
  }
  try {
    mgard_hip::ProgressiveReader reader(compressed, compressed_size, config);
    if (reader.level() != -1) return 1;
    const int levels[2] = {lt - 2, lt};
    for (int to : levels) {
      void *got = nullptr, *want = nullptr;
      if (reader.refine(to, got, false) != mgard_hip::compress_status_type::Success || reader.level() != to ||
          mgard_hip::decompress_level(compressed, compressed_size, to, want, config, false) !=
              mgard_hip::compress_status_type::Success ||
          mgard_hip::infer_level_shape(compressed, compressed_size, to, config, ls, lt) !=
              mgard_hip::compress_status_type::Success) {
        std::printf("refine(%d) failed: %s\n", to, mgh_last_error());
        return 1;
      }
      const size_t m = ls[0] * ls[1] * ls[2];
      if (std::memcmp(got, want, m * sizeof(float)) != 0) {
        std::printf("refine(%d): the reader and mgh_decompress_level disagree\n", to);
        return 1;
      }
      std::free(got);
      std::free(want);
    }
    void *again = nullptr;
    if (reader.refine(lt, again, false) == mgard_hip::compress_status_type::Success) {
      std::printf("a level that is not above the current one was accepted\n");
      return 1;
    }
    mgard_hip::SIZE fe = 0, ne = 0, fc = 0, nc = 0;
    if (mgard_hip::infer_level_range(compressed, compressed_size, lt, config, fe, ne, fc, nc) !=
            mgard_hip::compress_status_type::Success || fe + ne != n1 * n2 * n3) {
      std::printf("infer_level_range\n");
      return 1;
    }
  } catch (const std::exception &e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  std::free(compressed);
  std::printf("progressive ok\n");
  return 0;
}
