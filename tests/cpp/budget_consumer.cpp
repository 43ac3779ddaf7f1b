// mgh_estimate_sizes and mgh_compress_budget through the C++ mirrors of compress_hip.hpp alone. Driven by
// tests/test_gpu_cpp_budget.py.
//   budget_consumer <original f32 file> <n0> <n1> <n2> <max_bytes> <container out file>
// Prints the estimates of three tolerances, compresses to the budget (tolerances 1e-4 .. 1e2, four rounds),
// writes the container, decompresses it here and prints the largest error; then asks for a budget nothing
// fits and says what came back.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "compress_hip.hpp"

int main(int argc, char **argv) {
  using namespace mgard_hip;
  if (argc < 7) return 2;
  const std::vector<SIZE> shape{(SIZE)std::atoll(argv[2]), (SIZE)std::atoll(argv[3]), (SIZE)std::atoll(argv[4])};
  const size_t n = shape[0] * shape[1] * shape[2], max_bytes = (size_t)std::atoll(argv[5]);
  std::vector<float> x(n);
  FILE *f = std::fopen(argv[1], "rb");
  if (!f || std::fread(x.data(), sizeof(float), n, f) != n) return 2;
  std::fclose(f);
  const double inf = std::numeric_limits<double>::infinity();
  HighLevelConfig cfg;
  cfg.huff_dict_size = 256;

  std::vector<mgh_size_estimate> est;
  if (estimate_sizes(3, data_type::Float, shape, {1e-3, 1e-2, 1e-1}, inf, error_bound_type::REL, x.data(), {}, cfg, est) !=
      compress_status_type::Success)
    return 3;
  for (const mgh_size_estimate &e : est)
    std::printf("estimate %a %llu %llu %llu %llu %d\n", e.tol, (unsigned long long)e.bytes_min,
                (unsigned long long)e.bytes_max, (unsigned long long)e.outliers, (unsigned long long)e.code_bits, e.raw);

  void *cbuf = nullptr, *dec = nullptr;
  size_t csize = 0;
  double tol_used = 0;
  mgh_size_estimate used{};
  if (compress_budget(3, data_type::Float, shape, max_bytes, 1e-4, 1e2, 4, inf, error_bound_type::REL, x.data(), cbuf, csize,
                      {}, cfg, false, tol_used, &used) != compress_status_type::Success)
    return 4;
  std::printf("budget %a %zu %llu %llu\n", tol_used, csize, (unsigned long long)used.bytes_min,
              (unsigned long long)used.bytes_max);
  f = std::fopen(argv[6], "wb");
  if (!f || std::fwrite(cbuf, 1, csize, f) != csize) return 2;
  std::fclose(f);
  if (decompress(cbuf, csize, dec, cfg, false) != compress_status_type::Success) return 5;
  double err = 0;
  for (size_t i = 0; i < n; i++) err = std::fmax(err, std::fabs((double)((const float *)dec)[i] - (double)x[i]));
  std::printf("error %a\n", err);
  std::free(dec);
  std::free(cbuf);

  void *none = nullptr;
  size_t none_size = 0;
  const compress_status_type st = compress_budget(3, data_type::Float, shape, 1000, 1e-4, 1e2, 4, inf, error_bound_type::REL,
                                                  x.data(), none, none_size, {}, cfg, false, tol_used);
  std::printf("too_small %d %d\n", st == compress_status_type::OutputTooLargeFailure ? 1 : 0, none == nullptr ? 1 : 0);
  release_cache();
  std::printf("OK\n");
  return 0;
}
