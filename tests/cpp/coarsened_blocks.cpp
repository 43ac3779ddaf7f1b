// Reduced resolution of a Block-decomposed container through compress_x_hip.hpp (extensions:
// infer_coarsened_shape, infer_coarsened_nodes, decompress_coarsened). Every block of the stitched result
// must carry the bits of decompress_level(l_target - k) of that block compressed on its own, undecomposed,
// with the same ABS bound and s = inf -- for which the bound of a subdomain is the bound itself.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "compress_hip.hpp"
#include "compress_x_hip.hpp"

using mgard_x::SIZE;

static SIZE halve(SIZE n, int k) {
  for (int i = 0; i < k; i++) n = n / 2 + 1;
  return n;
}

int main() {
  const std::vector<SIZE> shape{66, 45, 37};
  const SIZE bs = 33;
  const double tol = 1e-3, s = std::numeric_limits<double>::infinity();
  const size_t n = shape[0] * shape[1] * shape[2];
  std::vector<float> in(n);
  for (size_t i = 0; i < shape[0]; i++)
    for (size_t j = 0; j < shape[1]; j++)
      for (size_t k = 0; k < shape[2]; k++)
        in[(i * shape[1] + j) * shape[2] + k] = std::sin(0.05f * i) * std::cos(0.07f * j) + 0.3f * std::sin(0.11f * k);
  mgard_x::Config config;
  config.domain_decomposition = mgard_x::domain_decomposition_type::Block;
  config.block_size = bs;
  void *compressed = nullptr;
  size_t compressed_size = 0;
  if (mgard_x::compress(3, mgard_x::data_type::Float, shape, tol, s, mgard_x::error_bound_type::ABS, in.data(),
                        compressed, compressed_size, config, false) != mgard_x::compress_status_type::Success) {
    std::printf("compress failed: %s\n", mgh_last_error());
    return 1;
  }
  // blocks per dimension: (offset, extent)
  std::vector<std::vector<SIZE>> boff(3), bext(3);
  for (int d = 0; d < 3; d++)
    for (SIZE o = 0; o < shape[d]; o += bs) {
      boff[d].push_back(o);
      bext[d].push_back(std::min<SIZE>(bs, shape[d] - o));
    }
  if (bext[0].size() * bext[1].size() * bext[2].size() != 8 || bext[2][1] != 4) return 1;
  int K = -1;
  std::vector<SIZE> cs;
  if (mgard_x::infer_coarsened_shape(compressed, compressed_size, -1, config, cs, K) !=
          mgard_x::compress_status_type::Success || !cs.empty() || K != 2) {  // (4 -> 3 -> 2)
    std::printf("infer_coarsened_shape(-1): K = %d (%s)\n", K, mgh_last_error());
    return 1;
  }
  if (mgard_x::infer_coarsened_shape(compressed, compressed_size, K + 1, config, cs, K) ==
      mgard_x::compress_status_type::Success) {
    std::printf("more halvings than the shallowest block has levels were accepted\n");
    return 1;
  }
  for (int k = 0; k <= K; k++) {
    int K2 = -1;
    std::vector<mgard_hip::SIZE> cs2;
    if (mgard_x::infer_coarsened_shape(compressed, compressed_size, k, config, cs, K2) !=
            mgard_x::compress_status_type::Success || K2 != K ||
        mgard_hip::infer_coarsened_shape(compressed, compressed_size, k, mgard_hip::HighLevelConfig(), cs2, K2) !=
            mgard_hip::compress_status_type::Success || cs2 != cs) {
      std::printf("infer_coarsened_shape(%d) failed: %s\n", k, mgh_last_error());
      return 1;
    }
    // stitched offsets and node lists by the rule
    std::vector<std::vector<SIZE>> soff(3);
    for (int d = 0; d < 3; d++) {
      SIZE at = 0;
      std::vector<SIZE> want;
      for (size_t j = 0; j < bext[d].size(); j++) {
        soff[d].push_back(at);
        at += halve(bext[d][j], k);
        std::vector<SIZE> idx(bext[d][j]);
        for (SIZE i = 0; i < idx.size(); i++) idx[i] = i;
        for (int h = 0; h < k; h++) {
          std::vector<SIZE> nx;
          for (size_t i = 0; i < idx.size(); i += 2) nx.push_back(idx[i]);
          if (nx.back() != idx.back()) nx.push_back(idx.back());
          idx = nx;
        }
        for (SIZE i : idx) want.push_back(boff[d][j] + i);
      }
      std::vector<SIZE> nodes;
      if (at != cs[d] || mgard_x::infer_coarsened_nodes(compressed, compressed_size, k, d, config, nodes) !=
                             mgard_x::compress_status_type::Success || nodes != want) {
        std::printf("k = %d, dimension %d: shape or nodes differ from the rule\n", k, d);
        return 1;
      }
    }
    void *out = nullptr, *out2 = nullptr;
    if (mgard_x::decompress_coarsened(compressed, compressed_size, k, out, config, false) !=
            mgard_x::compress_status_type::Success ||
        mgard_hip::decompress_coarsened(compressed, compressed_size, k, out2, mgard_hip::HighLevelConfig(), false) !=
            mgard_hip::compress_status_type::Success) {
      std::printf("decompress_coarsened(%d) failed: %s\n", k, mgh_last_error());
      return 1;
    }
    const size_t m = cs[0] * cs[1] * cs[2];
    if (std::memcmp(out, out2, m * sizeof(float)) != 0) {
      std::printf("k = %d: the two mirrors disagree\n", k);
      return 1;
    }
    const float *o = (const float *)out;
    // every block on its own
    for (size_t a = 0; a < bext[0].size(); a++)
      for (size_t b = 0; b < bext[1].size(); b++)
        for (size_t c = 0; c < bext[2].size(); c++) {
          const std::vector<SIZE> bsh{bext[0][a], bext[1][b], bext[2][c]};
          std::vector<float> blk(bsh[0] * bsh[1] * bsh[2]);
          for (SIZE i = 0; i < bsh[0]; i++)
            for (SIZE j = 0; j < bsh[1]; j++)
              std::memcpy(&blk[(i * bsh[1] + j) * bsh[2]],
                          &in[((boff[0][a] + i) * shape[1] + boff[1][b] + j) * shape[2] + boff[2][c]],
                          bsh[2] * sizeof(float));
          void *bc = nullptr, *lv = nullptr;
          size_t bcs = 0;
          int lt = -1;
          std::vector<mgard_hip::SIZE> ls;
          if (mgard_x::compress(3, mgard_x::data_type::Float, bsh, tol, s, mgard_x::error_bound_type::ABS, blk.data(), bc,
                                bcs, mgard_x::Config(), false) != mgard_x::compress_status_type::Success ||
              mgard_hip::infer_level_shape(bc, bcs, -1, mgard_hip::HighLevelConfig(), ls, lt) !=
                  mgard_hip::compress_status_type::Success || lt < K ||
              mgard_x::decompress_level(bc, bcs, lt - k, lv, mgard_x::Config(), false) !=
                  mgard_x::compress_status_type::Success) {
            std::printf("block (%zu, %zu, %zu): %s\n", a, b, c, mgh_last_error());
            return 1;
          }
          const SIZE e0 = halve(bsh[0], k), e1 = halve(bsh[1], k), e2 = halve(bsh[2], k);
          const float *l = (const float *)lv;
          for (SIZE i = 0; i < e0; i++)
            for (SIZE j = 0; j < e1; j++)
              if (std::memcmp(&l[(i * e1 + j) * e2],
                              &o[((soff[0][a] + i) * cs[1] + soff[1][b] + j) * cs[2] + soff[2][c]],
                              e2 * sizeof(float)) != 0) {
                std::printf("k = %d, block (%zu, %zu, %zu), row (%llu, %llu): differs from the block's own level\n", k,
                            a, b, c, (unsigned long long)i, (unsigned long long)j);
                return 1;
              }
          std::free(bc);
          std::free(lv);
        }
    std::printf("k = %d: %llu x %llu x %llu, 8 blocks bit-equal to their own decompress_level\n", k,
                (unsigned long long)cs[0], (unsigned long long)cs[1], (unsigned long long)cs[2]);
    std::free(out);
    std::free(out2);
  }
  std::free(compressed);
  std::printf("OK\n");
  return 0;
}
