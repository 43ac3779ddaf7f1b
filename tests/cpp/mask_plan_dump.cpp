// Driver of mgard_amd/csrc/mask_plan.hpp for tests/test_mask_plan_cpu.py: one command per line on stdin, one
// line of answer each. Built with g++ against the header alone.
//   ser C n_masked restore_bits kind HEXRECORD    -> the 48 footer bytes in hex ("-" is the empty record)
//   open n is_double HEXBUFFER                   -> none | bad MESSAGE | ok C R n_masked restore_bits kind
//   seg D shape...                               -> total, then start:len:first_word:shift:nwords per segment
//   kind n n_masked coded_bytes                  -> 0 | 1 | 2
//   codable chunk                                -> 0 | 1
//   c VMIN VMAX  (hex floats)                    -> the constant as a hex float
//   bits is_double VALUE (hex float)             -> restore bits, and the value they give back as a hex float
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mask_plan.hpp"

static std::vector<uint8_t> unhex(const std::string &h) {
  std::vector<uint8_t> out;
  if (h == "-") return out;
  for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)std::strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return out;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "ser") {
      mgh::MaskFooter f;
      std::string hex;
      in >> f.container >> f.n_masked >> f.restore_bits >> f.kind >> hex;
      const std::vector<uint8_t> rec = unhex(hex);
      f.record = rec.size();
      f.crc = mgh::fmt::crc32(rec.data(), rec.size());
      uint8_t out[mgh::kMaskFooterBytes];
      mgh::mask_footer_serialize(f, out);
      for (uint8_t b : out) std::printf("%02x", b);
      std::printf("\n");
    } else if (cmd == "open") {
      uint64_t n;
      int is_double;
      std::string hex;
      in >> n >> is_double >> hex;
      const std::vector<uint8_t> buf = unhex(hex);
      const size_t have = buf.size() < mgh::kMaskFooterBytes ? buf.size() : mgh::kMaskFooterBytes;
      const uint8_t *tail = buf.data() + (buf.size() - have);
      mgh::MaskFooter f;
      if (!mgh::mask_footer_present(tail, buf.size())) {
        std::printf("none\n");
        continue;
      }
      const char *bad = mgh::mask_footer_parse(tail, buf.size(), f);
      if (!bad) bad = mgh::mask_footer_check_n(f, n, is_double != 0);
      if (!bad) bad = mgh::mask_record_check_crc(f, buf.data() + f.container);
      if (bad) std::printf("bad %s\n", bad);
      else
        std::printf("ok %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u\n", f.container, f.record, f.n_masked,
                    f.restore_bits, f.kind);
    } else if (cmd == "seg") {
      int D;
      in >> D;
      std::vector<uint64_t> shape(D);
      for (auto &e : shape) in >> e;
      const mgh::MaskSegments g = mgh::mask_segments(D, shape.data());
      std::printf("%" PRIu64, g.total);
      for (uint64_t s = 0; s < g.total; s++) {
        uint64_t start, len, first;
        int shift, nw;
        mgh::mask_segment(g, s, start, len);
        mgh::mask_segment_words(start, len, first, shift, nw);
        std::printf(" %" PRIu64 ":%" PRIu64 ":%" PRIu64 ":%d:%d", start, len, first, shift, nw);
      }
      std::printf("\n");
    } else if (cmd == "kind") {
      uint64_t n, nm, coded;
      in >> n >> nm >> coded;
      std::printf("%u\n", mgh::mask_record_kind(n, nm, coded));
    } else if (cmd == "codable") {
      uint64_t chunk;
      in >> chunk;
      std::printf("%d\n", mgh::mask_record_codable(chunk) ? 1 : 0);
    } else if (cmd == "c") {
      std::string a, b;
      in >> a >> b;
      std::printf("%a\n", mgh::mask_fill_constant(std::strtod(a.c_str(), nullptr), std::strtod(b.c_str(), nullptr)));
    } else if (cmd == "bits") {
      int is_double;
      std::string a;
      in >> is_double >> a;
      const uint64_t bits = mgh::mask_value_bits(is_double != 0, std::strtod(a.c_str(), nullptr));
      std::printf("%" PRIu64 " %a\n", bits, mgh::mask_bits_value(is_double != 0, bits));
    } else {
      std::printf("unknown\n");
    }
  }
  return 0;
}
