// mgh_compress_pwrel and its readers through the C++ mirror of compress_hip.hpp alone. Driven by
// tests/test_gpu_cpp_pwrel.py.
//   pwrel_example <original f32 file> <n0> <n1> <n2> <eps> <abs_floor> <file prefix>
// Compresses the array under the pointwise relative bound (the library allocates the buffer), writes the buffer to
// <prefix>buf.bin, asks what it is, reads it back into its own array, writes that to <prefix>out.bin, verifies it
// against the original and prints the largest relative error as the library and as this program see it. Then hands
// the masked part to decompress_pwrel and says what came back.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "compress_hip.hpp"

int main(int argc, char **argv) {
  using namespace mgard_hip;
  if (argc < 8) return 2;
  const std::vector<SIZE> shape{(SIZE)std::atoll(argv[2]), (SIZE)std::atoll(argv[3]), (SIZE)std::atoll(argv[4])};
  const double eps = std::strtod(argv[5], nullptr), floor = std::strtod(argv[6], nullptr);
  const size_t n = shape[0] * shape[1] * shape[2];
  std::vector<float> x(n);
  FILE *f = std::fopen(argv[1], "rb");
  if (!f || std::fread(x.data(), sizeof(float), n, f) != n) return 2;
  std::fclose(f);
  HighLevelConfig cfg;
  cfg.huff_dict_size = 1024;

  void *buf = nullptr;
  size_t size = 0;
  if (compress_pwrel(3, data_type::Float, shape, eps, floor, x.data(), buf, size, {}, cfg, false) != compress_status_type::Success)
    return 3;
  f = std::fopen((std::string(argv[7]) + "buf.bin").c_str(), "wb");
  if (!f || std::fwrite(buf, 1, size, f) != size) return 2;
  std::fclose(f);

  bool pwrel = false;
  struct mgh_pwrel_info info {};
  if (pwrel_info(buf, size, pwrel, info) != compress_status_type::Success || !pwrel) return 4;
  std::printf("info %zu %llu %llu %llu %llu %a %a %a\n", size, (unsigned long long)info.masked_size,
              (unsigned long long)info.flag_record_size, (unsigned long long)info.n_masked, (unsigned long long)info.n_flag,
              info.eps, info.abs_floor, info.delta);

  std::vector<float> out(n);
  void *dst = out.data();
  if (decompress_pwrel(buf, size, dst, cfg, true) != compress_status_type::Success) return 5;
  f = std::fopen((std::string(argv[7]) + "out.bin").c_str(), "wb");
  if (!f || std::fwrite(out.data(), sizeof(float), n, f) != n) return 2;
  std::fclose(f);

  mgh_pwrel_compare r{};
  bool within = false;
  if (verify_pwrel(buf, size, x.data(), n * sizeof(float), data_type::Float, cfg, r, within) != compress_status_type::Success)
    return 6;
  double worst = 0;
  for (size_t i = 0; i < n; i++)
    if (std::isfinite(x[i]) && std::fabs((double)x[i]) >= std::fmax(floor, 1.1754943508222875e-38))
      worst = std::fmax(worst, std::fabs((double)out[i] - (double)x[i]) / std::fabs((double)x[i]));
  std::printf("verify %d %a %a %llu %llu %llu\n", within ? 1 : 0, r.max_rel_err, worst, (unsigned long long)r.n_valid,
              (unsigned long long)r.n_class_mismatch, (unsigned long long)r.n_sign_mismatch);

  // the masked part alone is no such buffer: pwrel = false, and decompress_pwrel refuses it
  bool part = true;
  const compress_status_type q = pwrel_info(buf, (size_t)info.masked_size, part, info);
  void *none = nullptr;
  const compress_status_type s = decompress_pwrel(buf, (size_t)info.masked_size, none, cfg, false);
  std::printf("masked %d %d %d %d\n", q == compress_status_type::Success, part, s != compress_status_type::Success, none == nullptr);
  std::free(buf);
  std::printf("OK\n");
  return 0;
}
