// The index arithmetic of mgh_mask_sample_ (mgard_amd/csrc/mask_plan.hpp: mask_unravel, mask_flat_index,
// mask_sample_source) run on the host for every output element, as the kernel's lanes run it.
// One case per line of standard input:
//   D  shape[D]  out_shape[D]  then per dimension: -1 (the identity list) or out_shape[d] entries
// One line of output per case: the source bit of every output element, in order; -1 where a list leads outside
// the source (the kernel reads nothing there).
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
    for (uint64_t e = 0; e < n_out; e++) {
      uint64_t flat = 0;
      const bool inside = mgh::mask_sample_source(D, shape.data(), out_shape.data(), ptr.data(), (uint32_t)e, flat);
      if (inside) std::printf("%" PRIu64 " ", flat);
      else std::printf("-1 ");
    }
    std::printf("\n");
  }
  return 0;
}
