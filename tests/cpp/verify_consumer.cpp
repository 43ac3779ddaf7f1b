// The error figures and mgh_verify through the public headers alone: the reference-named functions of
// compress_x_hip.hpp (mgard_x::L_inf_norm, L_2_norm, L_inf_error, L_2_error, MSE, PSNR) on host and on device
// pointers, their mgard_hip:: counterparts, and verify. Driven by tests/test_gpu_cpp_verify.py, which compares
// the printed figures (C99 hex floats) with NumPy.
//   verify_consumer <original f32 file> <n0> <n1> <n2> <second f32 file> <decompressed out file>
// The first array is compressed here (REL 1e-3, s = inf), decompressed, and measured against its
// reconstruction; the second (all negative, same size) is measured against the first, for PSNR's range rule.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "compress_hip.hpp"
#include "compress_x_hip.hpp"

static std::vector<float> read_floats(const char *path, size_t n) {
  std::vector<float> v(n);
  FILE *f = std::fopen(path, "rb");
  if (!f || std::fread(v.data(), sizeof(float), n, f) != n) std::exit(2);
  std::fclose(f);
  return v;
}

static float *to_device(const std::vector<float> &v) {
  void *p = nullptr;
  if (hipMalloc(&p, v.size() * sizeof(float)) != hipSuccess) std::exit(3);
  if (hipMemcpy(p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) std::exit(3);
  return (float *)p;
}

static void figures(const char *tag, const std::vector<mgard_x::SIZE> &shape, const float *a, const float *b) {
  using namespace mgard_x;
  size_t n = 1;
  for (SIZE e : shape) n *= e;
  std::printf("%s L_inf_norm %a\n", tag, L_inf_norm(n, a));
  std::printf("%s L_2_norm_1 %a\n", tag, L_2_norm(shape, a, true));
  std::printf("%s L_2_norm_0 %a\n", tag, L_2_norm(shape, a, false));
  std::printf("%s L_inf_error_abs %a\n", tag, L_inf_error(n, a, b, error_bound_type::ABS));
  std::printf("%s L_inf_error_rel %a\n", tag, L_inf_error(n, a, b, error_bound_type::REL));
  std::printf("%s L_2_error_abs_1 %a\n", tag, L_2_error(shape, a, b, error_bound_type::ABS, true));
  std::printf("%s L_2_error_rel_1 %a\n", tag, L_2_error(shape, a, b, error_bound_type::REL, true));
  std::printf("%s L_2_error_abs_0 %a\n", tag, L_2_error(shape, a, b, error_bound_type::ABS, false));
  std::printf("%s MSE %a\n", tag, MSE(n, a, b));
  std::printf("%s PSNR %a\n", tag, PSNR(n, a, b));
}

int main(int argc, char **argv) {
  if (argc < 7) return 2;
  const std::vector<mgard_x::SIZE> shape{(mgard_x::SIZE)std::atoll(argv[2]), (mgard_x::SIZE)std::atoll(argv[3]),
                                         (mgard_x::SIZE)std::atoll(argv[4])};
  const size_t n = shape[0] * shape[1] * shape[2];
  const std::vector<float> x = read_floats(argv[1], n), neg = read_floats(argv[5], n);

  void *cbuf = nullptr, *dec = nullptr;
  size_t csize = 0;
  mgard_x::Config cfg;
  if (mgard_x::compress(3, mgard_x::data_type::Float, shape, 1e-3, std::numeric_limits<double>::infinity(),
                        mgard_x::error_bound_type::REL, x.data(), cbuf, csize, cfg, false) !=
      mgard_x::compress_status_type::Success)
    return 4;
  if (mgard_x::decompress(cbuf, csize, dec, cfg, false) != mgard_x::compress_status_type::Success) return 4;
  const std::vector<float> y((const float *)dec, (const float *)dec + n);
  {
    FILE *f = std::fopen(argv[6], "wb");
    if (!f || std::fwrite(y.data(), sizeof(float), n, f) != n || std::fclose(f) != 0) return 2;
  }
  float *dx = to_device(x), *dy = to_device(y), *dneg = to_device(neg);
  figures("host", shape, x.data(), y.data());
  figures("device", shape, dx, dy);
  figures("mixed", shape, x.data(), dy);
  figures("neg-host", shape, neg.data(), x.data());
  figures("neg-device", shape, dneg, dx);
  // the mgard_hip:: counterparts are the same functions under the other namespace
  if (mgard_hip::PSNR(n, dneg, dx) != mgard_x::PSNR(n, dneg, dx) ||
      mgard_hip::L_2_error(shape, x.data(), y.data(), mgard_hip::error_bound_type::REL, true) !=
          mgard_x::L_2_error(shape, x.data(), y.data(), mgard_x::error_bound_type::REL, true) ||
      mgard_hip::L_inf_error(n, dx, dy, mgard_hip::error_bound_type::ABS) !=
          mgard_x::L_inf_error(n, dx, dy, mgard_x::error_bound_type::ABS) ||
      mgard_hip::MSE(n, dx, dy) != mgard_x::MSE(n, dx, dy) || mgard_hip::L_inf_norm(n, dx) != mgard_x::L_inf_norm(n, dx) ||
      mgard_hip::L_2_norm(shape, dx, false) != mgard_x::L_2_norm(shape, dx, false)) {
    std::printf("the mgard_hip:: figures differ from the mgard_x:: ones\n");
    return 5;
  }
  // mgh_verify, the C entry and the two mirrors; host and device original
  mgh_verify_result r{}, rx{}, rh{};
  mgh_config c;
  mgh_config_default(&c);
  if (mgh_verify(cbuf, csize, x.data(), n * sizeof(float), MGH_FLOAT, 0, &c, &r) != MGH_SUCCESS) return 6;
  if (mgard_x::verify(cbuf, csize, dx, n * sizeof(float), mgard_x::data_type::Float, 0, cfg, rx) !=
      mgard_x::compress_status_type::Success)
    return 6;
  if (mgard_hip::verify(cbuf, csize, x.data(), n * sizeof(float), mgard_hip::data_type::Float, 0,
                        mgard_hip::HighLevelConfig(), rh) != mgard_hip::compress_status_type::Success)
    return 6;
  if (mgard_x::verify(cbuf, csize, x.data(), n * sizeof(float) - 4, mgard_x::data_type::Float, 0, cfg, rx) ==
      mgard_x::compress_status_type::Success)
    return 7;  // (a wrong size must be refused)
  for (const mgh_verify_result *q : {&rx, &rh})
    if (q->stats.max_abs_err != r.stats.max_abs_err || q->stats.argmax != r.stats.argmax || q->within != r.within ||
        q->bound != r.bound)
      return 8;
  std::printf("verify n %llu nonfinite %llu argmax %llu\n", (unsigned long long)r.stats.n,
              (unsigned long long)r.stats.nonfinite, (unsigned long long)r.stats.argmax);
  std::printf("verify max_abs_err %a\nverify sum_sq_err %a\nverify bound %a\nverify achieved %a\n", r.stats.max_abs_err,
              r.stats.sum_sq_err, r.bound, r.achieved);
  std::printf("verify bound_kind %d within %d\n", r.bound_kind, r.within);
  (void)hipFree(dx);
  (void)hipFree(dy);
  (void)hipFree(dneg);
  std::free(cbuf);
  std::free(dec);
  mgard_x::release_cache(cfg);
  std::printf("OK\n");
  return 0;
}
