// mgh_compress_masked and its readers through the C++ mirror of compress_hip.hpp alone. Driven by
// tests/test_gpu_cpp_masked.py.
//   masked_example <original f32 file> <n0> <n1> <n2> <file prefix>
// The file holds an array whose missing values are NaN. Compresses it with a REL bound of 3e-2 (the library
// allocates the buffer), writes the buffer to <prefix>buf.bin, asks what it is, reads it back into its own array
// and writes that to <prefix>out.bin; prints the footer's fields, how many positions came back as the restore
// value, and the largest error at the valid positions beside tol times their absmax. Then hands the plain
// container part to decompress_masked and says what came back.
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
  const double inf = std::numeric_limits<double>::infinity(), tol = 3e-2, restore = -9999.0;
  HighLevelConfig cfg;
  cfg.huff_dict_size = 1024;

  const mgh_mask_spec spec{MGH_MASK_NONFINITE, 0.0, restore};
  void *buf = nullptr;
  size_t size = 0;
  if (compress_masked(3, data_type::Float, shape, tol, inf, error_bound_type::REL, x.data(), spec, buf, size, {}, cfg, false) !=
      compress_status_type::Success)
    return 3;
  f = std::fopen((std::string(argv[5]) + "buf.bin").c_str(), "wb");
  if (!f || std::fwrite(buf, 1, size, f) != size) return 2;
  std::fclose(f);

  bool masked = false;
  struct mgh_masked_info info {};
  if (masked_info(buf, size, masked, info) != compress_status_type::Success || !masked) return 4;
  std::printf("info %zu %llu %llu %llu %d %a\n", size, (unsigned long long)info.container_size,
              (unsigned long long)info.record_size, (unsigned long long)info.n_masked, info.kind, info.restore_value);

  std::vector<float> out(n);
  void *dst = out.data();
  if (decompress_masked(buf, size, dst, cfg, true) != compress_status_type::Success) return 5;
  f = std::fopen((std::string(argv[5]) + "out.bin").c_str(), "wb");
  if (!f || std::fwrite(out.data(), sizeof(float), n, f) != n) return 2;
  std::fclose(f);
  size_t restored = 0, wrong = 0;
  double err = 0, absmax = 0;
  for (size_t i = 0; i < n; i++) {
    if (std::isfinite(x[i])) {
      err = std::fmax(err, std::fabs((double)out[i] - (double)x[i]));
      absmax = std::fmax(absmax, std::fabs((double)x[i]));
    } else if (out[i] == (float)restore) {
      restored++;
    } else {
      wrong++;
    }
  }
  std::printf("restored %zu %zu\n", restored, wrong);
  std::printf("error %a %a\n", err, tol * absmax);

  // the container part alone is a plain container: masked = false, and decompress_masked refuses it
  bool plain_masked = true;
  const compress_status_type q = masked_info(buf, (size_t)info.container_size, plain_masked, info);
  void *none = nullptr;
  const compress_status_type r = decompress_masked(buf, (size_t)info.container_size, none, cfg, false);
  std::printf("plain %d %d %d %d\n", q == compress_status_type::Success, plain_masked, r != compress_status_type::Success,
              none == nullptr);
  std::free(buf);
  std::printf("OK\n");
  return 0;
}
