// mgh_compress_layers and its readers through the C++ mirror of compress_hip.hpp alone. Driven by
// tests/test_gpu_cpp_layers.py.
//   layers_consumer <original f32 file> <n0> <n1> <n2> <file prefix>
// Compresses the array into four precision layers in one call, writes layer k to <prefix><k>.bin, reads the
// layers back with the one-shot call (layers 0 .. k, for every k) and with LayersReader, prints every
// step's largest error and whether the two readers agree bit for bit, writes the last reconstruction to
// <prefix>out.bin; then hands the writer tolerances it refuses and says what came back.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "compress_hip.hpp"

int main(int argc, char **argv) {
  using namespace mgard_hip;
  if (argc < 6) return 2;
  const std::vector<SIZE> shape{(SIZE)std::atoll(argv[2]), (SIZE)std::atoll(argv[3]), (SIZE)std::atoll(argv[4])};
  const size_t n = shape[0] * shape[1] * shape[2];
  std::vector<float> x(n);
  FILE *f = std::fopen(argv[1], "rb");
  if (!f || std::fread(x.data(), sizeof(float), n, f) != n) return 2;
  std::fclose(f);
  const double inf = std::numeric_limits<double>::infinity();
  HighLevelConfig cfg;
  cfg.huff_dict_size = 1024;

  const std::vector<double> tols{1e-1, 1e-2, 1e-3, 1e-4};
  std::vector<void *> layers;
  std::vector<size_t> sizes;
  if (compress_layers(3, data_type::Float, shape, tols, inf, error_bound_type::REL, x.data(), layers, sizes, {}, cfg, false) !=
      compress_status_type::Success)
    return 3;
  if (layers.size() != tols.size() || sizes.size() != tols.size()) return 3;
  mgh_compress_stats st{};
  if (mgh_last_compress_stats(&st) != 0) return 3;
  std::printf("stats %llu %llu %llu\n", (unsigned long long)st.decompositions, (unsigned long long)st.records,
              (unsigned long long)st.raw_records);
  std::vector<float> out(n);
  {
    LayersReader reader(layers[0], sizes[0], cfg);
    for (size_t k = 0; k < tols.size(); k++) {
      f = std::fopen((std::string(argv[5]) + std::to_string(k) + ".bin").c_str(), "wb");
      if (!f || std::fwrite(layers[k], 1, sizes[k], f) != sizes[k]) return 2;
      std::fclose(f);
      if (k && reader.add(layers[k], sizes[k]) != compress_status_type::Success) return 4;
      void *stateful = out.data();
      if (reader.data(stateful, true) != compress_status_type::Success) return 4;
      void *oneshot = nullptr;
      const std::vector<const void *> upto(layers.begin(), layers.begin() + k + 1);
      const std::vector<size_t> upto_size(sizes.begin(), sizes.begin() + k + 1);
      if (decompress_layers(upto, upto_size, oneshot, cfg, false) != compress_status_type::Success) return 5;
      double err = 0;
      for (size_t i = 0; i < n; i++) err = std::fmax(err, std::fabs((double)out[i] - (double)x[i]));
      std::printf("layer %a %zu %a %d %d %a\n", tols[k], sizes[k], err, std::memcmp(oneshot, out.data(), n * sizeof(float)) == 0,
                  reader.count(), reader.tolerance());
      std::free(oneshot);
    }
    // a layer out of order is refused and the reader stays where it is
    std::printf("out_of_order %d %d\n", reader.add(layers[1], sizes[1]) == compress_status_type::Failure ? 1 : 0,
                reader.count());
  }
  f = std::fopen((std::string(argv[5]) + "out.bin").c_str(), "wb");
  if (!f || std::fwrite(out.data(), sizeof(float), n, f) != n) return 2;
  std::fclose(f);
  for (void *p : layers) std::free(p);

  std::vector<void *> none;
  std::vector<size_t> none_size;
  const compress_status_type bad = compress_layers(3, data_type::Float, shape, {1e-2, 1e-2}, inf, error_bound_type::REL,
                                                   x.data(), none, none_size, {}, cfg, false);
  std::printf("refused %d %d\n", bad == compress_status_type::Failure ? 1 : 0,
              none.size() == 2 && !none[0] && !none[1] ? 1 : 0);
  release_cache();
  std::printf("OK\n");
  return 0;
}
