// A pointwise-relative buffer in the level reader, the coarsened reader and the preview window, through the C++ mirror
// of compress_hip.hpp. Driven by tests/test_gpu_cpp_pwrel_views.py.
//   pwrel_views_example <original f32 file> <n0> <n1> <n2> <file prefix>
// Compresses the array with eps = 1e-1 and abs_floor = 1e-20, then writes: <prefix>buf.bin, the buffer; <prefix>level.bin,
// level 1 of its hierarchy, and <prefix>coarse.bin, the array after one halving (their shapes printed); <prefix>win.bin,
// the window lo = (3, 0, 31), ext = (5, 33, 1) of the preview after one halving. Every output is pre-allocated here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "compress_hip.hpp"

template <typename T> static bool dump(const std::string &path, const T *p, size_t n) {
  FILE *f = std::fopen(path.c_str(), "wb");
  const bool ok = f && std::fwrite(p, sizeof(T), n, f) == n;
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
  HighLevelConfig cfg;
  cfg.huff_dict_size = 1024;
  const mgh_config c = detail::to_c(cfg);

  void *buf = nullptr;
  size_t size = 0;
  if (compress_pwrel(3, data_type::Float, shape, 1e-1, (double)1e-20f, x.data(), buf, size, {}, cfg, false) !=
      compress_status_type::Success)
    return 3;
  bool pwrel = false;
  struct mgh_pwrel_info info {};
  if (pwrel_info(buf, size, pwrel, info) != compress_status_type::Success || !pwrel) return 4;
  if (!dump(prefix + "buf.bin", (const unsigned char *)buf, size)) return 2;

  // the shapes come from the container part, the arrays from the whole buffer
  int D = 0, L = 0, K = 0;
  uint64_t ls[MGH_MAX_DIM], cs[MGH_MAX_DIM];
  if (mgh_infer_level_shape(buf, (size_t)info.container_size, &c, 1, &D, ls, &L) != MGH_SUCCESS || D != 3 || L < 2) return 5;
  std::printf("level %llu %llu %llu\n", (unsigned long long)ls[0], (unsigned long long)ls[1], (unsigned long long)ls[2]);
  std::vector<float> level(ls[0] * ls[1] * ls[2]);
  void *dst = level.data();
  if (decompress_pwrel_level(buf, size, 1, dst, cfg, true) != compress_status_type::Success || dst != level.data()) return 6;
  if (!dump(prefix + "level.bin", level.data(), level.size())) return 2;

  if (mgh_infer_coarsened_shape(buf, (size_t)info.container_size, &c, 1, &D, cs, &K) != MGH_SUCCESS || D != 3) return 5;
  std::printf("coarse %llu %llu %llu\n", (unsigned long long)cs[0], (unsigned long long)cs[1], (unsigned long long)cs[2]);
  std::vector<float> coarse(cs[0] * cs[1] * cs[2]);
  dst = coarse.data();
  if (decompress_pwrel_coarsened(buf, size, 1, dst, cfg, true) != compress_status_type::Success) return 7;
  if (!dump(prefix + "coarse.bin", coarse.data(), coarse.size())) return 2;

  const std::vector<SIZE> lo{3, 0, 31}, ext{5, 33, 1};
  std::vector<float> win(ext[0] * ext[1] * ext[2]);
  dst = win.data();
  if (decompress_pwrel_preview_window(buf, size, 1, lo, ext, dst, cfg, true) != compress_status_type::Success) return 8;
  if (!dump(prefix + "win.bin", win.data(), win.size())) return 2;

  // the preview without halvings is the full reader, and the masked buffer in front is refused
  std::vector<float> full(n), pre(n);
  dst = full.data();
  if (decompress_pwrel(buf, size, dst, cfg, true) != compress_status_type::Success) return 9;
  dst = pre.data();
  if (decompress_pwrel_preview(buf, size, 0, dst, cfg, true) != compress_status_type::Success) return 9;
  int same = 1;
  for (size_t i = 0; i < n; i++) {
    uint32_t a, b;
    std::memcpy(&a, &full[i], 4);
    std::memcpy(&b, &pre[i], 4);
    same &= a == b;
  }
  void *none = nullptr;
  const compress_status_type q = decompress_pwrel_coarsened(buf, (size_t)info.masked_size, 1, none, cfg, false);
  std::printf("preview0 %d\nmasked %d %d\n", same, q != compress_status_type::Success, none == nullptr);
  std::free(buf);
  std::printf("OK\n");
  return 0;
}
