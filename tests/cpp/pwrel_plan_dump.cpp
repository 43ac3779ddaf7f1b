// Driver of mgard_amd/csrc/pwrel_plan.hpp for tests/test_pwrel_plan_cpu.py: one command per line on stdin, one
// line of answer each. Built with g++ against the header alone.
//   ser M n_flag EPS FLOOR kind HEXRECORD   (hex floats)  -> the 56 footer bytes in hex ("-" is the empty record)
//   open n HEXBUFFER                        -> none | bad MESSAGE | ok M S n_flag EPS FLOOR kind
//   tol is_double EPS YBOUND  (hex floats)  -> ok DELTA (hex float) | bad MESSAGE   (refused: eps outside (0, 1), or
//                                              DELTA below kPwrelMinUlps ulps of YBOUND or half of log2(1 + EPS))
//   cls is_double FLOOR X     (hex floats)  -> 0 valid | 1 zeroed | 2 nonfinite
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "pwrel_plan.hpp"

static std::vector<uint8_t> unhex(const std::string &h) {
  std::vector<uint8_t> out;
  if (h == "-") return out;
  for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)std::strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return out;
}

static double num(const std::string &s) { return std::strtod(s.c_str(), nullptr); }

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "ser") {
      mgh::PwrelFooter f;
      std::string eps, floor, hex;
      in >> f.masked >> f.n_flag >> eps >> floor >> f.kind >> hex;
      f.eps = num(eps);
      f.abs_floor = num(floor);
      const std::vector<uint8_t> rec = unhex(hex);
      f.record = rec.size();
      f.crc = mgh::fmt::crc32(rec.data(), rec.size());
      uint8_t out[mgh::kPwrelFooterBytes];
      mgh::pwrel_footer_serialize(f, out);
      for (uint8_t b : out) std::printf("%02x", b);
      std::printf("\n");
    } else if (cmd == "open") {
      uint64_t n;
      std::string hex;
      in >> n >> hex;
      const std::vector<uint8_t> buf = unhex(hex);
      const size_t have = buf.size() < mgh::kPwrelFooterBytes ? buf.size() : mgh::kPwrelFooterBytes;
      const uint8_t *tail = buf.data() + (buf.size() - have);
      mgh::PwrelFooter f;
      if (!mgh::pwrel_footer_present(tail, buf.size())) {
        std::printf("none\n");
        continue;
      }
      const char *bad = mgh::pwrel_footer_parse(tail, buf.size(), f);
      if (!bad) bad = mgh::pwrel_footer_check_n(f, n);
      if (!bad) bad = mgh::pwrel_record_check_crc(f, buf.data() + f.masked);
      if (bad) std::printf("bad %s\n", bad);
      else
        std::printf("ok %" PRIu64 " %" PRIu64 " %" PRIu64 " %a %a %u\n", f.masked, f.record, f.n_flag, f.eps, f.abs_floor, f.kind);
    } else if (cmd == "tol") {
      int is_double;
      std::string eps, yb;
      in >> is_double >> eps >> yb;
      double delta = 0;
      const char *bad = mgh::pwrel_abs_tolerance(is_double != 0, num(eps), num(yb), &delta);
      if (bad) std::printf("bad %s\n", bad);
      else std::printf("ok %a\n", delta);
    } else if (cmd == "cls") {
      int is_double;
      std::string floor, x;
      in >> is_double >> floor >> x;
      std::printf("%d\n", mgh::pwrel_classify(num(x), mgh::pwrel_floor_eff(is_double != 0, num(floor))));
    } else {
      std::printf("unknown\n");
    }
  }
  return 0;
}
