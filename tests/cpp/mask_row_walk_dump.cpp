// The row walk of mgh_pwrel_inverse_sampled_ (mgard_amd/csrc/mask_plan.hpp: mask_row_count, mask_row_begin,
// mask_row_source) run on the host as the kernel k_pwrel_inverse_sampled runs it -- shapes and lists right-aligned
// in kMaskMaxDim dimensions with leading 1s, one mask_row_begin per row, one mask_row_source per element -- beside
// mask_sample_source, the per-element arithmetic of mgh_mask_sample_, in the case's own D dimensions.
// One case per line of standard input (the format of mask_sample_dump.cpp):
//   D  shape[D]  out_shape[D]  then per dimension: -1 (the identity list) or out_shape[d] entries
// Two lines of output per case: the source bit of every output element, in order, by the row walk and by
// mask_sample_source; -1 where a list leads outside the source (the kernel reads nothing there).
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <vector>

#include "mask_plan.hpp"

int main() {
  int D;
  while (std::cin >> D) {
    if (D < 1 || D > mgh::kMaskMaxDim) return 2;
    std::vector<uint32_t> shape(D), out_shape(D);
    for (auto &e : shape) std::cin >> e;
    for (auto &e : out_shape) std::cin >> e;
    std::vector<std::vector<uint32_t>> lists(D);
    std::vector<const uint32_t *> ptr(D, nullptr);
    uint64_t n_out = 1;
    for (int d = 0; d < D; d++) {
      n_out *= out_shape[d];
      long long first;
      std::cin >> first;
      if (first < 0) continue;
      lists[d].resize(out_shape[d]);
      lists[d][0] = (uint32_t)first;
      for (uint32_t i = 1; i < out_shape[d]; i++) std::cin >> lists[d][i];
      ptr[d] = lists[d].data();
    }
    if (!std::cin) return 3;
    // the kernel's argument block
    constexpr int M = mgh::kMaskMaxDim;
    uint32_t a_shape[M], a_out[M];
    const uint32_t *a_idx[M];
    for (int k = 0; k < M; k++) {
      const int d = k - (M - D);
      a_shape[k] = d >= 0 ? shape[d] : 1u;
      a_out[k] = d >= 0 ? out_shape[d] : 1u;
      a_idx[k] = d >= 0 ? ptr[d] : nullptr;
    }
    const uint32_t rows = mgh::mask_row_count(M, a_out), nf = a_out[M - 1];
    if ((uint64_t)rows * nf != n_out) return 4;
    for (uint32_t row = 0; row < rows; row++) {
      const mgh::MaskRow r = mgh::mask_row_begin(M, a_shape, a_out, a_idx, row);
      for (uint32_t j = 0; j < nf; j++) {
        uint64_t flat = 0;
        if (mgh::mask_row_source(r, a_shape[M - 1], a_idx[M - 1], j, flat)) std::printf("%" PRIu64 " ", flat);
        else std::printf("-1 ");
      }
    }
    std::printf("\n");
    for (uint64_t e = 0; e < n_out; e++) {
      uint64_t flat = 0;
      if (mgh::mask_sample_source(D, shape.data(), out_shape.data(), ptr.data(), (uint32_t)e, flat)) std::printf("%" PRIu64 " ", flat);
      else std::printf("-1 ");
    }
    std::printf("\n");
  }
  return 0;
}
