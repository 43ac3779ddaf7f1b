// Prints the Thomas-solve plan (mgard_amd/csrc/ipk_plan.hpp) of every solve it reads from stdin
// (tests/test_ipk_plan_cpu.py). One solve per line, as ipk_launch sees it:
//   elem_size axis m0 m1 m2 nbatch batch_stride add [switch=value ...]
// `add`: 0 = no add-to pass, +1 / -1 = its sign (it picks a kernel variant, not a family);
// switches: members of IpkTuning by name, over num_cu = 256 and the defaults.
// Output per solve: a `plan` line with the launch parameters and one `dispatch` line per kernel
// launch -- name with template arguments, grid, workgroup size, dynamic LDS bytes -- which are the
// four fields a kernel trace shows.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "ipk_plan.hpp"

using namespace mgh;

static bool set_switch(IpkTuning &t, const std::string &key, long v) {
#define SW(name, type) if (key == #name) { t.name = (type)v; return true; }
  SW(num_cu, size_t) SW(stream, int) SW(dma, int) SW(dma_min, size_t) SW(dma_rounds, int) SW(spec, int)
  SW(spec_k, int) SW(spec_long, int) SW(spec_max, uint32_t) SW(chunk, int) SW(chunk_k, int)
  SW(chunk_need, int) SW(w, uint32_t) SW(wpc, size_t) SW(kr16, int) SW(contig_rounds, size_t)
#undef SW
  return false;
}

static const char *family(IpkKernel k) {
  switch (k) {
  case IpkKernel::Spec: return "Spec";
  case IpkKernel::LdsContigChunked: return "LdsContigChunked";
  case IpkKernel::Dma: return "Dma";
  case IpkKernel::Stream: return "Stream";
  case IpkKernel::LdsContig: return "LdsContig";
  case IpkKernel::LdsStrided: return "LdsStrided";
  case IpkKernel::Thread: return "Thread";
  }
  return "?";
}

static void dispatch(const std::string &name, unsigned long grid, unsigned block, size_t lds) {
  std::printf("dispatch\t%s\t%lu\t%u\t%zu\n", name.c_str(), grid, block, lds);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    size_t elem, bstride;
    int axis, add;
    uint32_t m[3], nbatch;
    if (!(in >> elem >> axis >> m[0] >> m[1] >> m[2] >> nbatch >> bstride >> add)) return 2;
    IpkTuning t;
    t.num_cu = 256;
    t.dma_min = 2 * t.num_cu;
    std::string kv;
    while (in >> kv) {
      const size_t eq = kv.find('=');
      if (eq == std::string::npos || !set_switch(t, kv.substr(0, eq), std::atol(kv.c_str() + eq + 1))) return 3;
    }
    // (what ipk_launch does with batches that get one thread per pencil: one call per box)
    IpkPlan p = ipk_plan(t, elem, axis, m, nbatch, bstride);
    const bool per_batch = p.per_batch;
    if (per_batch) p = ipk_plan(t, elem, axis, m, 1, 0);
    std::printf("plan\tfam=%s\tW=%u\tn_glob=%u\tK=%u\tKR=%u\tP=%u\tS=%u\tnchunk=%u\tpad=%u\tmagic=%u\tlds_attr=%zu\t"
                "per_batch=%d\tnpencil=%u\n", family(p.kernel), p.W, p.n_glob, p.K, p.KR, p.P, p.S, p.nchunk, p.pad,
                p.magic, p.lds_attr, (int)per_batch, p.geom.npencil);
    const std::string T = elem == 4 ? "float" : "double", U = std::to_string(64 / elem);
    const unsigned long grid = (unsigned long)p.grid * p.grid_y;
    switch (p.kernel) {
    case IpkKernel::Spec:
      for (const char *sweep : {"fwd", "bwd"}) {
        dispatch("k_ipk_spec_" + std::string(sweep) + "<" + T + ">", p.grid, 64, 0);
        dispatch("k_ipk_spec_check<" + T + ">", p.check_grid, 256, 0);
        dispatch("k_ipk_spec_fix<" + T + ">", p.fix_grid, 64, 0);
      }
      if (add) dispatch("k_ipk_spec_apply<" + T + ">", p.apply_grid, 256, 0);
      break;
    case IpkKernel::LdsContigChunked: dispatch("k_ipk_lds_contig<" + T + ", true>", grid, p.block, p.lds); break;
    case IpkKernel::LdsContig: dispatch("k_ipk_lds_contig<" + T + ", false>", grid, p.block, p.lds); break;
    case IpkKernel::Dma:
      dispatch("k_ipk_dma<" + T + ", " + U + ", " + std::to_string(p.KR) + ", " + std::to_string(add) + ", true>", grid,
               p.block, p.lds);
      break;
    case IpkKernel::Stream:
      dispatch("k_ipk_stream<" + T + ", " + U + ", " + std::to_string(p.KR) + ", 1, " + (axis == 2 ? "true" : "false") +
                   ", false>", grid, p.block, p.lds);
      break;
    case IpkKernel::LdsStrided:
      dispatch("k_ipk_lds_strided<" + T + ", " + std::to_string(p.W) + ">", grid, p.block, p.lds);
      break;
    case IpkKernel::Thread:
      for (uint32_t b = 0; b < (per_batch ? nbatch : 1); b++)
        dispatch("k_ipk<" + T + ", " + std::to_string(axis) + ">", grid, p.block, 0);
      break;
    }
    std::puts("end");
  }
  return 0;
}
