// mgh_compress_ladder through the C++ mirror of compress_hip.hpp alone. Driven by
// tests/test_gpu_cpp_ladder.py.
//   ladder_consumer <original f32 file> <n0> <n1> <n2> <container file prefix>
// Compresses the array at four tolerances in one call, prints every tier's size, writes it to
// <prefix><k>.bin, decompresses it here, checks its bound with verify and prints the largest error; then
// hands the call a tolerance it refuses and says what came back.
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

  const std::vector<double> tols{5e-2, 1e-1, 5e-1, 2e0};
  std::vector<void *> tiers;
  std::vector<size_t> sizes;
  if (compress_ladder(3, data_type::Float, shape, tols, inf, error_bound_type::REL, x.data(), tiers, sizes, {}, cfg, false) !=
      compress_status_type::Success)
    return 3;
  if (tiers.size() != tols.size() || sizes.size() != tols.size()) return 3;
  mgh_compress_stats st{};
  if (mgh_last_compress_stats(&st) != 0) return 3;
  std::printf("stats %llu %llu %llu\n", (unsigned long long)st.decompositions, (unsigned long long)st.records,
              (unsigned long long)st.raw_records);
  for (size_t k = 0; k < tols.size(); k++) {
    f = std::fopen((std::string(argv[5]) + std::to_string(k) + ".bin").c_str(), "wb");
    if (!f || std::fwrite(tiers[k], 1, sizes[k], f) != sizes[k]) return 2;
    std::fclose(f);
    void *dec = nullptr;
    if (decompress(tiers[k], sizes[k], dec, cfg, false) != compress_status_type::Success) return 4;
    double err = 0;
    for (size_t i = 0; i < n; i++) err = std::fmax(err, std::fabs((double)((const float *)dec)[i] - (double)x[i]));
    std::free(dec);
    mgh_verify_result r{};
    if (verify(tiers[k], sizes[k], x.data(), n * sizeof(float), data_type::Float, 0, cfg, r) != compress_status_type::Success)
      return 5;
    std::printf("tier %a %zu %a %a %a %d\n", tols[k], sizes[k], err, r.stats.max_abs_err, r.bound, r.within);
    std::free(tiers[k]);
  }

  std::vector<void *> none;
  std::vector<size_t> none_size;
  const compress_status_type bad = compress_ladder(3, data_type::Float, shape, {1e-2, -1.0}, inf, error_bound_type::REL,
                                                   x.data(), none, none_size, {}, cfg, false);
  std::printf("refused %d %d\n", bad == compress_status_type::Failure ? 1 : 0,
              none.size() == 2 && !none[0] && !none[1] ? 1 : 0);
  release_cache();
  std::printf("OK\n");
  return 0;
}
