// mgh_achieved_errors and mgh_compress_target through the C++ mirrors of compress_hip.hpp alone. Driven by
// tests/test_gpu_cpp_target.py.
//   target_consumer <original f32 file> <n0> <n1> <n2> <metric> <target> <container out file>
// Prints the statistics of three tolerances, compresses to the target (tolerances 5e-2 .. 5, six rounds),
// writes the container and prints the tolerance, the candidates and the statistics; then asks for a target
// nothing meets and says what came back.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "compress_hip.hpp"

static void print_stats(const char *tag, double tol, const mgh_error_stats &e) {
  std::printf("%s %a %llu %llu %a %llu %a %a %a %a %a\n", tag, tol, (unsigned long long)e.n, (unsigned long long)e.nonfinite,
              e.max_abs_err, (unsigned long long)e.argmax, e.sum_sq_err, e.ref_min, e.ref_max, e.ref_abs_max, e.ref_sum_sq);
}

int main(int argc, char **argv) {
  using namespace mgard_hip;
  if (argc < 8) return 2;
  const std::vector<SIZE> shape{(SIZE)std::atoll(argv[2]), (SIZE)std::atoll(argv[3]), (SIZE)std::atoll(argv[4])};
  const size_t n = shape[0] * shape[1] * shape[2];
  const target_metric metric = (target_metric)std::atoi(argv[5]);
  const double target = std::strtod(argv[6], nullptr);
  std::vector<float> x(n);
  FILE *f = std::fopen(argv[1], "rb");
  if (!f || std::fread(x.data(), sizeof(float), n, f) != n) return 2;
  std::fclose(f);
  const double inf = std::numeric_limits<double>::infinity();
  HighLevelConfig cfg;
  cfg.huff_dict_size = 1024;

  const std::vector<double> tols{1e-1, 3e-1, 1e0};
  std::vector<mgh_error_stats> stats;
  if (achieved_errors(3, data_type::Float, shape, tols, inf, error_bound_type::REL, x.data(), {}, cfg, stats) !=
      compress_status_type::Success)
    return 3;
  for (size_t k = 0; k < stats.size(); k++) print_stats("achieved", tols[k], stats[k]);

  void *cbuf = nullptr;
  size_t csize = 0;
  double tol_used = 0;
  mgh_error_stats used{};
  int candidates = 0;
  if (compress_target(3, data_type::Float, shape, metric, target, 5e-2, 5e0, 6, inf, error_bound_type::REL, x.data(), cbuf,
                      csize, {}, cfg, false, tol_used, &used, &candidates) != compress_status_type::Success)
    return 4;
  std::printf("target %d %zu\n", candidates, csize);
  print_stats("used", tol_used, used);
  f = std::fopen(argv[7], "wb");
  if (!f || std::fwrite(cbuf, 1, csize, f) != csize) return 2;
  std::fclose(f);
  std::free(cbuf);

  void *none = nullptr;
  size_t none_size = 0;
  const compress_status_type st = compress_target(3, data_type::Float, shape, target_metric::MaxAbs, 0.0, 5e-2, 5e0, 6, inf,
                                                  error_bound_type::REL, x.data(), none, none_size, {}, cfg, false, tol_used);
  std::printf("not_met %d %d\n", st == compress_status_type::Failure ? 1 : 0, none == nullptr ? 1 : 0);
  release_cache();
  std::printf("OK\n");
  return 0;
}
