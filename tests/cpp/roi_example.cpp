// mgh_compress_roi and its readers through the C++ mirror of compress_hip.hpp alone. Driven by
// tests/test_gpu_cpp_roi.py.
//   roi_example <original f32 file> <n0> <n1> <n2> <tol> <lo0> <lo1> <lo2> <e0> <e1> <e2> <tol_i> <file prefix>
// Compresses the array (REL, s = inf) with one box at tol_i (the library allocates the buffer), writes the buffer to
// <prefix>buf.bin, asks what it is, reads it back into its own array, writes that to <prefix>out.bin, verifies it
// against the original and prints the largest errors as the library and as this program see them. Then hands the
// container part to decompress_roi and says what came back.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "compress_hip.hpp"

int main(int argc, char **argv) {
  using namespace mgard_hip;
  if (argc < 14) return 2;
  const std::vector<SIZE> shape{(SIZE)std::atoll(argv[2]), (SIZE)std::atoll(argv[3]), (SIZE)std::atoll(argv[4])};
  const double tol = std::strtod(argv[5], nullptr), tol_i = std::strtod(argv[12], nullptr);
  mgh_roi_box box{};
  for (int d = 0; d < 3; d++) {
    box.lo[d] = (uint64_t)std::atoll(argv[6 + d]);
    box.ext[d] = (uint64_t)std::atoll(argv[9 + d]);
  }
  box.tol = tol_i;
  const size_t n = shape[0] * shape[1] * shape[2];
  std::vector<float> x(n);
  FILE *f = std::fopen(argv[1], "rb");
  if (!f || std::fread(x.data(), sizeof(float), n, f) != n) return 2;
  std::fclose(f);
  HighLevelConfig cfg;
  cfg.huff_dict_size = 1024;

  void *buf = nullptr;
  size_t size = 0;
  if (compress_roi(3, data_type::Float, shape, tol, std::numeric_limits<double>::infinity(), error_bound_type::REL, x.data(),
                   {box}, buf, size, {}, cfg, false) != compress_status_type::Success)
    return 3;
  f = std::fopen((std::string(argv[13]) + "buf.bin").c_str(), "wb");
  if (!f || std::fwrite(buf, 1, size, f) != size) return 2;
  std::fclose(f);

  bool roi = false;
  struct mgh_roi_info info {};
  if (roi_info(buf, size, roi, info) != compress_status_type::Success || !roi) return 4;
  std::printf("info %zu %llu %d %d %a %a %llu\n", size, (unsigned long long)info.container_size, info.nbox, info.D,
              info.box[0].tol, info.box[0].tolres, (unsigned long long)info.box[0].record_size);

  std::vector<float> out(n);
  void *dst = out.data();
  if (decompress_roi(buf, size, dst, cfg, true) != compress_status_type::Success) return 5;
  f = std::fopen((std::string(argv[13]) + "out.bin").c_str(), "wb");
  if (!f || std::fwrite(out.data(), sizeof(float), n, f) != n) return 2;
  std::fclose(f);

  mgh_verify_result whole{};
  std::vector<mgh_verify_result> per_box;
  if (verify_roi(buf, size, x.data(), n * sizeof(float), data_type::Float, cfg, whole, per_box) != compress_status_type::Success ||
      per_box.size() != 1)
    return 6;
  double worst = 0, worst_box = 0;
  for (size_t i = 0; i < n; i++) {
    const size_t i0 = i / (shape[1] * shape[2]), i1 = i / shape[2] % shape[1], i2 = i % shape[2];
    const double e = std::fabs((double)out[i] - (double)x[i]);
    worst = std::fmax(worst, e);
    if (i0 - box.lo[0] < box.ext[0] && i1 - box.lo[1] < box.ext[1] && i2 - box.lo[2] < box.ext[2]) worst_box = std::fmax(worst_box, e);
  }
  std::printf("verify %d %a %a %a %d %a %a %a\n", whole.within, whole.bound, whole.stats.max_abs_err, worst, per_box[0].within,
              per_box[0].bound, per_box[0].stats.max_abs_err, worst_box);

  // the container part alone is no such buffer: roi = false, and decompress_roi refuses it
  bool part = true;
  const compress_status_type q = roi_info(buf, (size_t)info.container_size, part, info);
  void *none = nullptr;
  const compress_status_type s = decompress_roi(buf, (size_t)info.container_size, none, cfg, false);
  std::printf("container %d %d %d %d\n", q == compress_status_type::Success, part, s != compress_status_type::Success, none == nullptr);
  std::free(buf);
  std::printf("OK\n");
  return 0;
}
