// mgh_compress_level_layers and its readers through the C++ mirror of compress_hip.hpp alone. Driven by
// tests/test_gpu_cpp_level_layers.py.
//   level_layers_consumer <original f32 file> <n0> <n1> <n2> <level> <file prefix>
// Compresses the array into three level-ordered precision layers in one call, writes layer k to <prefix><k>.bin,
// reads layers 0 .. k at <level> with the one-shot call and with LevelLayersReader and says whether the two
// agree bit for bit; then takes layer 0 to the full level, prints the depths, writes the full-level array of
// layer 0 to <prefix>out.bin, and hands the reader a level it refuses.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "compress_hip.hpp"

int main(int argc, char **argv) {
  using namespace mgard_hip;
  if (argc < 7) return 2;
  const std::vector<SIZE> shape{(SIZE)std::atoll(argv[2]), (SIZE)std::atoll(argv[3]), (SIZE)std::atoll(argv[4])};
  const int level = std::atoi(argv[5]);
  const size_t n = shape[0] * shape[1] * shape[2];
  std::vector<float> x(n);
  FILE *f = std::fopen(argv[1], "rb");
  if (!f || std::fread(x.data(), sizeof(float), n, f) != n) return 2;
  std::fclose(f);
  const double inf = std::numeric_limits<double>::infinity();
  HighLevelConfig cfg;
  cfg.huff_dict_size = 1024;

  const std::vector<double> tols{1e-1, 1e-2, 1e-3};
  std::vector<void *> layers;
  std::vector<size_t> sizes;
  if (compress_level_layers(3, data_type::Float, shape, tols, inf, error_bound_type::REL, x.data(), layers, sizes, {}, cfg,
                            false) != compress_status_type::Success)
    return 3;
  mgh_compress_stats st{};
  if (mgh_last_compress_stats(&st) != 0) return 3;
  std::printf("stats %llu %llu %llu\n", (unsigned long long)st.decompositions, (unsigned long long)st.records,
              (unsigned long long)st.raw_records);
  int D = 0, L = 0;
  uint64_t lshape[MGH_MAX_DIM];
  const mgh_config c = detail::to_c(cfg);
  if (mgh_infer_level_shape(layers[0], sizes[0], &c, level, &D, lshape, &L) != 0 || D != 3) return 3;
  const size_t nl = lshape[0] * lshape[1] * lshape[2];
  std::vector<float> out(nl), full(n);
  {
    LevelLayersReader reader(layers[0], sizes[0], level, cfg);
    for (size_t k = 0; k < tols.size(); k++) {
      f = std::fopen((std::string(argv[6]) + std::to_string(k) + ".bin").c_str(), "wb");
      if (!f || std::fwrite(layers[k], 1, sizes[k], f) != sizes[k]) return 2;
      std::fclose(f);
      if (k && reader.add(layers[k], sizes[k], level) != compress_status_type::Success) return 4;
      void *stateful = out.data();
      if (reader.data(level, stateful, true) != compress_status_type::Success) return 4;
      void *oneshot = nullptr;
      const std::vector<const void *> upto(layers.begin(), layers.begin() + k + 1);
      const std::vector<size_t> upto_size(sizes.begin(), sizes.begin() + k + 1);
      if (decompress_level_layers(upto, upto_size, level, oneshot, cfg, false) != compress_status_type::Success) return 5;
      std::printf("layer %a %zu %d %d %d %a\n", tols[k], sizes[k], std::memcmp(oneshot, out.data(), nl * sizeof(float)) == 0,
                  reader.count(), reader.depth((int)k), reader.tolerance((int)k));
      std::free(oneshot);
    }
    // layer 1 may not go deeper than layer 0; layer 0 may
    std::printf("too_deep %d\n", reader.extend(1, layers[1], sizes[1], L) == compress_status_type::Failure ? 1 : 0);
    if (reader.extend(0, layers[0], sizes[0], L) != compress_status_type::Success) return 6;
    void *p = full.data();
    if (reader.data(L, p, true) != compress_status_type::Success) return 6;
    std::printf("depths %d %d %d\n", reader.depth(0), reader.depth(1), reader.depth(2));
  }
  f = std::fopen((std::string(argv[6]) + "out.bin").c_str(), "wb");
  if (!f || std::fwrite(full.data(), sizeof(float), n, f) != n) return 2;
  std::fclose(f);
  for (void *p : layers) std::free(p);
  release_cache();
  std::printf("OK\n");
  return 0;
}
