// Full-grid preview through the C++ mirrors: decompress_preview of compress_x_hip.hpp and compress_hip.hpp,
// ProgressiveReader::preview and Compressor::Prolong. Reads a container a caller made
// (tests/test_gpu_cpp_preview.py), writes every result to a file for the caller to compare, and checks what
// it can on its own: the two mirrors agree, and Compressor::Prolong of a refined level is the reader's preview.
//   preview_consumer <container> <out prefix> <K> block <block size>   -- a Block-decomposed container
//   preview_consumer <container> <out prefix> <K> progressive          -- one subdomain, reorder = 1, float, 3-D
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

static bool write_file(const std::string &path, const void *p, size_t bytes) {
  FILE *f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(p, 1, bytes, f) == bytes;
  return std::fclose(f) == 0 && ok;
}

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  const std::string prefix = argv[2], mode = argv[4];
  const int K = std::atoi(argv[3]);
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

  if (mode == "block") {
    mgard_x::Config xc;
    xc.domain_decomposition = mgard_x::domain_decomposition_type::Block;
    xc.block_size = (mgard_x::SIZE)std::atoi(argv[5]);
    mgard_hip::HighLevelConfig hc;
    hc.domain_decomposition = mgard_hip::domain_decomposition_type::Block;
    hc.block_size = xc.block_size;
    for (int k = 0; k <= K; k++) {
      void *a = nullptr, *b = nullptr;
      if (mgard_x::decompress_preview(buf.data(), buf.size(), k, a, xc, false) != mgard_x::compress_status_type::Success ||
          mgard_hip::decompress_preview(buf.data(), buf.size(), k, b, hc, false) !=
              mgard_hip::compress_status_type::Success) {
        std::printf("decompress_preview(%d) failed: %s\n", k, mgh_last_error());
        return 1;
      }
      if (std::memcmp(a, b, n * sizeof(float)) != 0) {
        std::printf("k = %d: the two mirrors disagree\n", k);
        return 1;
      }
      // ... and into a caller's buffer
      std::vector<float> mine(n, 7.0f);
      void *c = mine.data();
      if (mgard_x::decompress_preview(buf.data(), buf.size(), k, c, xc, true) != mgard_x::compress_status_type::Success ||
          c != (void *)mine.data() || std::memcmp(a, mine.data(), n * sizeof(float)) != 0) {
        std::printf("k = %d: pre-allocated output differs\n", k);
        return 1;
      }
      if (!write_file(prefix + ".k" + std::to_string(k) + ".bin", a, n * sizeof(float))) return 2;
      std::free(a);
      std::free(b);
    }
    void *bad = nullptr;
    if (mgard_x::decompress_preview(buf.data(), buf.size(), K + 1, bad, xc, false) == mgard_x::compress_status_type::Success) {
      std::printf("more halvings than the shallowest block has levels were accepted\n");
      return 1;
    }
    std::printf("OK\n");
    return 0;
  }

  if (mode != "progressive") return 2;
  mgard_hip::HighLevelConfig config;
  config.reorder = 1;
  try {
    mgard_hip::ProgressiveReader reader(buf.data(), buf.size(), config);
    void *none = nullptr;
    if (reader.preview(none, false) == mgard_hip::compress_status_type::Success) {
      std::printf("a preview before the first refine was accepted\n");
      return 1;
    }
    std::vector<mgard_hip::SIZE> shape{shp[0], shp[1], shp[2]};
    mgard_hip::Hierarchy<3, float> hierarchy(shape, config);
    mgard_hip::Compressor<3, float> compressor(hierarchy, config, mgard_hip::DeviceAllocator{dalloc, dfree});
    if ((int)hierarchy.l_target() != K) return 1;
    float *d_full = (float *)dalloc(n * sizeof(float));
    if (!d_full) return 2;
    for (int level = 0; level <= K; level++) {
      void *lv = nullptr, *pv = nullptr;
      if (reader.refine(level, lv, false) != mgard_hip::compress_status_type::Success ||
          reader.preview(pv, false) != mgard_hip::compress_status_type::Success || reader.level() != level) {
        std::printf("level %d failed: %s\n", level, mgh_last_error());
        return 1;
      }
      // Compressor::Prolong of the level the reader handed out is the reader's preview
      const std::vector<mgard_hip::SIZE> ls = hierarchy.level_shape(level);
      const size_t m = ls[0] * ls[1] * ls[2];
      float *d_level = (float *)dalloc(m * sizeof(float));
      std::vector<float> back(n);
      if (!d_level || hipMemcpy(d_level, lv, m * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return 2;
      compressor.Prolong(d_full, level, d_level);
      if (hipDeviceSynchronize() != hipSuccess ||
          hipMemcpy(back.data(), d_full, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 2;
      dfree(d_level);
      if (std::memcmp(back.data(), pv, n * sizeof(float)) != 0) {
        std::printf("level %d: Compressor::Prolong and ProgressiveReader::preview disagree\n", level);
        return 1;
      }
      if (!write_file(prefix + ".p" + std::to_string(level) + ".bin", pv, n * sizeof(float))) return 2;
      std::free(lv);
      std::free(pv);
    }
    dfree(d_full);
  } catch (const std::exception &e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
