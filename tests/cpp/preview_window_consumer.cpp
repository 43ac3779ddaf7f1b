// Windowed full-grid preview through the C++ mirrors: decompress_preview_window of compress_x_hip.hpp and
// compress_hip.hpp, ProgressiveReader::preview_window and Compressor::ProlongWindow. Reads a one-subdomain
// container a caller made (tests/test_gpu_cpp_preview_window.py; reorder = 1, float, 3-D), takes one window of
// every preview and compares it here with the crop of the full preview.
//   preview_window_consumer <container> <K> <lo0> <lo1> <lo2> <ext0> <ext1> <ext2>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "compress_hip.hpp"
#include "compress_x_hip.hpp"
#include "mgard_hip.hpp"

static void *dalloc(size_t n) {
  void *p = nullptr;
  return hipMalloc(&p, n) == hipSuccess ? p : nullptr;
}
static void dfree(void *p) { (void)hipFree(p); }

int main(int argc, char **argv) {
  if (argc < 9) return 2;
  const int K = std::atoi(argv[2]);
  std::vector<unsigned char> buf;
  {
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    buf.resize((size_t)std::ftell(f));
    std::fseek(f, 0, SEEK_SET);
    if (std::fread(buf.data(), 1, buf.size(), f) != buf.size()) return 2;
    std::fclose(f);
  }
  int D = 0;
  uint64_t shp[MGH_MAX_DIM];
  if (mgh_infer_shape(buf.data(), buf.size(), &D, shp) != MGH_SUCCESS || D != 3) return 2;
  const size_t n = shp[0] * shp[1] * shp[2];
  std::vector<uint64_t> lo(3), ext(3);
  for (int d = 0; d < 3; d++) {
    lo[d] = std::strtoull(argv[3 + d], nullptr, 10);
    ext[d] = std::strtoull(argv[6 + d], nullptr, 10);
  }
  const size_t nw = ext[0] * ext[1] * ext[2];
  // the crop of a full array, dense
  auto crop = [&](const float *full) {
    std::vector<float> w(nw);
    for (uint64_t i = 0; i < ext[0]; i++)
      for (uint64_t j = 0; j < ext[1]; j++)
        std::memcpy(&w[(i * ext[1] + j) * ext[2]], &full[((lo[0] + i) * shp[1] + lo[1] + j) * shp[2] + lo[2]],
                    ext[2] * sizeof(float));
    return w;
  };
  mgard_x::Config xc;
  xc.reorder = 1;
  mgard_hip::HighLevelConfig hc;
  hc.reorder = 1;
  try {
    for (int k = 0; k <= K; k++) {
      void *full = nullptr, *a = nullptr, *b = nullptr;
      if (mgard_hip::decompress_preview(buf.data(), buf.size(), k, full, hc, false) != mgard_hip::compress_status_type::Success ||
          mgard_x::decompress_preview_window(buf.data(), buf.size(), k, lo, ext, a, xc, false) !=
              mgard_x::compress_status_type::Success ||
          mgard_hip::decompress_preview_window(buf.data(), buf.size(), k, lo, ext, b, hc, false) !=
              mgard_hip::compress_status_type::Success) {
        std::printf("k = %d failed: %s\n", k, mgh_last_error());
        return 1;
      }
      const std::vector<float> want = crop((const float *)full);
      if (std::memcmp(a, want.data(), nw * sizeof(float)) != 0 || std::memcmp(b, want.data(), nw * sizeof(float)) != 0) {
        std::printf("k = %d: the window is not the crop of the full preview\n", k);
        return 1;
      }
      std::free(full);
      std::free(a);
      std::free(b);
    }
    void *bad = nullptr;
    std::vector<uint64_t> out_of_range = lo;
    out_of_range[0] = shp[0];
    if (mgard_hip::decompress_preview_window(buf.data(), buf.size(), 0, out_of_range, ext, bad, hc, false) ==
        mgard_hip::compress_status_type::Success) {
      std::printf("a window outside the array was accepted\n");
      return 1;
    }

    mgard_hip::ProgressiveReader reader(buf.data(), buf.size(), hc);
    std::vector<mgard_hip::SIZE> shape{shp[0], shp[1], shp[2]};
    mgard_hip::Hierarchy<3, float> hierarchy(shape, hc);
    mgard_hip::Compressor<3, float> compressor(hierarchy, hc, mgard_hip::DeviceAllocator{dalloc, dfree});
    if ((int)hierarchy.l_target() != K) return 1;
    float *d_win = (float *)dalloc(nw * sizeof(float));
    if (!d_win) return 2;
    for (int level = 0; level <= K; level++) {
      void *lv = nullptr, *pv = nullptr, *wv = nullptr;
      if (reader.refine(level, lv, false) != mgard_hip::compress_status_type::Success ||
          reader.preview(pv, false) != mgard_hip::compress_status_type::Success ||
          reader.preview_window(lo, ext, wv, false) != mgard_hip::compress_status_type::Success || reader.level() != level) {
        std::printf("level %d failed: %s\n", level, mgh_last_error());
        return 1;
      }
      const std::vector<float> want = crop((const float *)pv);
      if (std::memcmp(wv, want.data(), nw * sizeof(float)) != 0) {
        std::printf("level %d: ProgressiveReader::preview_window is not the crop of preview\n", level);
        return 1;
      }
      // Compressor::ProlongWindow of the level the reader handed out is the same window
      const std::vector<mgard_hip::SIZE> ls = hierarchy.level_shape(level);
      const size_t m = ls[0] * ls[1] * ls[2];
      float *d_level = (float *)dalloc(m * sizeof(float));
      std::vector<float> back(nw);
      if (!d_level || hipMemcpy(d_level, lv, m * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return 2;
      compressor.ProlongWindow(d_win, level, d_level, lo, ext);
      if (hipDeviceSynchronize() != hipSuccess ||
          hipMemcpy(back.data(), d_win, nw * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 2;
      dfree(d_level);
      if (std::memcmp(back.data(), want.data(), nw * sizeof(float)) != 0) {
        std::printf("level %d: Compressor::ProlongWindow is not the crop of the preview\n", level);
        return 1;
      }
      std::free(lv);
      std::free(pv);
      std::free(wv);
    }
    dfree(d_win);
  } catch (const std::exception &e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  (void)n;
  std::printf("OK\n");
  return 0;
}
