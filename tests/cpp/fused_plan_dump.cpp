// Prints what mgard_amd/csrc/fused_plan.hpp plans for the level boxes on stdin
// (tests/test_fused_plan_cpu.py). One box per line:
//   m0 m1 m2 nz_class nlaunch nz0 nz1 slots0 slots1 [switch=value ...]
// switches: wide, faces, tall, xcd, box, cls1, cls2, rch0, rch1, rch2, pinned, slots_override, S
// (S: the start-up of the march model, every tile shape). Output: one line of key=value pairs per
// box, `planes` = the coarse planes of the r-chunks in order.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "fused_plan.hpp"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    uint32_t m[3];
    size_t nzc, nz[2];
    int nlaunch;
    long long slots[2];
    in >> m[0] >> m[1] >> m[2] >> nzc >> nlaunch >> nz[0] >> nz[1] >> slots[0] >> slots[1];
    mgh::FusedTuning t;
    std::string kv;
    while (in >> kv) {
      const size_t eq = kv.find('=');
      const std::string k = kv.substr(0, eq);
      const double v = std::atof(kv.c_str() + eq + 1);
      if (k == "wide") t.wide = (int)v;
      else if (k == "faces") t.faces = (int)v;
      else if (k == "tall") t.tall = (int)v;
      else if (k == "xcd") t.xcd = (int)v;
      else if (k == "box") t.box = (int)v;
      else if (k == "cls1") t.cls1 = (size_t)v;
      else if (k == "cls2") t.cls2 = (size_t)v;
      else if (k == "rch0") t.rch[0] = (int)v;
      else if (k == "rch1") t.rch[1] = (int)v;
      else if (k == "rch2") t.rch[2] = (int)v;
      else if (k == "pinned") t.pinned = v != 0;
      else if (k == "slots_override") t.slots_override = (long)v;
      else if (k == "S") t.startup[0] = t.startup[1] = t.startup[2] = v;
      else {
        std::fprintf(stderr, "unknown switch %s\n", k.c_str());
        return 2;
      }
    }
    mgh::FusedPlan p = mgh::fused_plan_tiles(t, m, nzc);
    mgh::fused_plan_march(p, t, (int)m[0], nlaunch, nz, slots);
    std::printf("cls=%d TC=%d TF=%d gxm=%d n_main=%d ff_F0=%d n_ff=%d cf_C0=%d n_cf=%d faces=%d ntile=%d "
                "xcd_ranges=%d grid_x=%u rch=%d nchunk=%d by_policy=%d wg0=%lld wg1=%lld rounds0=%lld rounds1=%lld "
                "box_kernel=%d planes=",
                p.cls, p.TC, p.TF, p.gxm, p.n_main, p.ff_F0, p.n_ff, p.cf_C0, p.n_cf, (int)p.faces, p.ntile,
                p.xcd_ranges, p.grid_x, p.rch, p.nchunk, (int)p.by_policy, p.workgroups[0], p.workgroups[1],
                p.rounds[0], p.rounds[1], (int)(p.cls < t.box));
    for (int k = 0; k < p.nchunk; k++)
      std::printf("%s%d", k ? "," : "", mgh::fused_chunk_planes((int)m[0], p.rch, p.nchunk, k));
    std::printf("\n");
  }
  return 0;
}
