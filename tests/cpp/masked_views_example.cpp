// A masked buffer in the coarsened reader, the preview window and verify_masked, through the C++ mirror of
// compress_hip.hpp. Driven by tests/test_gpu_cpp_masked_views.py.
//   masked_views_example <original f32 file> <n0> <n1> <n2> <file prefix>
// The file holds an array whose missing values are NaN. Compresses it with a REL bound of 3e-2 and a restore value
// of -9999, then writes: <prefix>coarse.bin, the array after one halving (its shape printed), <prefix>cmask.bin, the
// sampled mask of that array, <prefix>win.bin, the window lo = (3, 0, 31), ext = (5, 33, 1) of the preview after
// one halving; prints what verify_masked says against the array with its NaN.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "compress_hip.hpp"

template <typename T> static bool dump(const std::string &path, const std::vector<T> &v) {
  FILE *f = std::fopen(path.c_str(), "wb");
  const bool ok = f && std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
  if (f) std::fclose(f);
  return ok;
}

int main(int argc, char **argv) {
  using namespace mgard_hip;
  if (argc < 6) return 2;
  const std::vector<SIZE> shape{(SIZE)std::atoll(argv[2]), (SIZE)std::atoll(argv[3]), (SIZE)std::atoll(argv[4])};
  const size_t n = shape[0] * shape[1] * shape[2];
  std::vector<float> x(n);
  FILE *f = std::fopen(argv[1], "rb");
  if (!f || std::fread(x.data(), sizeof(float), n, f) != n) return 2;
  std::fclose(f);
  const std::string prefix(argv[5]);
  const double inf = std::numeric_limits<double>::infinity(), tol = 3e-2, restore = -9999.0;
  HighLevelConfig cfg;
  cfg.huff_dict_size = 1024;
  const mgh_config c = detail::to_c(cfg);

  const mgh_mask_spec spec{MGH_MASK_NONFINITE, 0.0, restore};
  void *buf = nullptr;
  size_t size = 0;
  if (compress_masked(3, data_type::Float, shape, tol, inf, error_bound_type::REL, x.data(), spec, buf, size, {}, cfg, false) !=
      compress_status_type::Success)
    return 3;
  bool masked = false;
  struct mgh_masked_info info {};
  if (masked_info(buf, size, masked, info) != compress_status_type::Success || !masked) return 4;

  // one halving: the shape from the container part, the array and its sampled mask from the whole buffer
  int D = 0, K = 0;
  uint64_t cs[MGH_MAX_DIM];
  if (mgh_infer_coarsened_shape(buf, (size_t)info.container_size, &c, 1, &D, cs, &K) != MGH_SUCCESS || D != 3) return 5;
  std::printf("coarse %llu %llu %llu\n", (unsigned long long)cs[0], (unsigned long long)cs[1], (unsigned long long)cs[2]);
  std::vector<float> coarse(cs[0] * cs[1] * cs[2]);
  std::vector<uint8_t> cmask(coarse.size());
  void *dst = coarse.data();
  if (decompress_masked_coarsened(buf, size, 1, dst, cfg, true) != compress_status_type::Success) return 6;
  if (decompress_mask_coarsened(buf, size, 1, cfg, cmask.data()) != compress_status_type::Success) return 7;
  if (!dump(prefix + "coarse.bin", coarse) || !dump(prefix + "cmask.bin", cmask)) return 2;

  const std::vector<SIZE> lo{3, 0, 31}, ext{5, 33, 1};
  std::vector<float> win(ext[0] * ext[1] * ext[2]);
  dst = win.data();
  if (decompress_masked_preview_window(buf, size, 1, lo, ext, dst, cfg, true) != compress_status_type::Success) return 8;
  if (!dump(prefix + "win.bin", win)) return 2;

  mgh_verify_result r{};
  uint64_t n_masked = 0;
  if (verify_masked(buf, size, x.data(), n * sizeof(float), data_type::Float, 0, cfg, r, n_masked) !=
      compress_status_type::Success)
    return 9;
  std::printf("verify %d %llu %llu %llu %a %a %a\n", r.within, (unsigned long long)r.stats.n, (unsigned long long)n_masked,
              (unsigned long long)r.stats.nonfinite, r.stats.max_abs_err, r.achieved, r.bound);

  // the container part alone is refused
  void *none = nullptr;
  const compress_status_type q = decompress_masked_coarsened(buf, (size_t)info.container_size, 1, none, cfg, false);
  std::printf("plain %d %d\n", q != compress_status_type::Success, none == nullptr);
  std::free(buf);
  std::printf("OK\n");
  return 0;
}
