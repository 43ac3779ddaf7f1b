// Driver of mgard_amd/csrc/roi_plan.hpp for tests/test_roi_plan_cpu.py: one command per line on stdin, one line of
// answer each. Built with g++ against the header alone.
//   chk D SHAPE... TOL S NBOX {LO... EXT... TOL_I}   (hex floats)  -> ok | bad MESSAGE
//   fit ARRAY_BYTES MAX_FOOTPRINT                                    -> ok | bad MESSAGE
//   tol is_double A R M  (hex floats)                                -> ok TOLRES (hex float) | bad MESSAGE
//   ser CONTAINER NBOX {LO*5 EXT*5 TOL TOLRES HEXRECORD}             -> table and footer in hex ("-" is the empty record);
//                                                                       lo and ext right-aligned, the offsets back to back
//   open D SHAPE... HEXBUFFER  -> none | bad MESSAGE | ok CONTAINER NBOX {LO*5 EXT*5 TOL TOLRES OFFSET SIZE}
//   magic HEXBUFFER            -> three digits: the masked, the pointwise-relative and the box footer's "present"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "roi_plan.hpp"

static std::vector<uint8_t> unhex(const std::string &h) {
  std::vector<uint8_t> out;
  if (h == "-") return out;
  for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)std::strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return out;
}

static double num(std::istream &in) {
  std::string s;
  in >> s;
  return std::strtod(s.c_str(), nullptr);
}

static void answer(const char *bad) {
  if (bad) std::printf("bad %s\n", bad);
  else std::printf("ok\n");
}

static const uint8_t *tail_of(const std::vector<uint8_t> &buf, size_t want) {
  const size_t have = buf.size() < want ? buf.size() : want;
  return buf.data() + (buf.size() - have);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "chk") {
      int D = 0;
      in >> D;
      uint64_t shape[mgh::kRoiMaxDim] = {1, 1, 1, 1, 1};
      for (int d = 0; d < D && d < mgh::kRoiMaxDim; d++) in >> shape[d];
      const double tol = num(in), s = num(in);
      long long nbox = 0;
      in >> nbox;
      std::vector<mgh::RoiBox> boxes;
      for (long long i = 0; i < nbox && D >= 1 && D <= mgh::kRoiMaxDim; i++) {
        uint64_t lo[mgh::kRoiMaxDim], ext[mgh::kRoiMaxDim];
        for (int d = 0; d < D; d++) in >> lo[d];
        for (int d = 0; d < D; d++) in >> ext[d];
        boxes.push_back(mgh::roi_box(D, lo, ext, num(in)));
      }
      // (the call sees at most 16 boxes, as the library's entry does)
      if (boxes.size() > (size_t)mgh::kRoiMaxBoxes) boxes.resize(mgh::kRoiMaxBoxes);
      const char *bad = mgh::roi_check_boxes(D, shape, tol, s, nbox, boxes.data());
      answer(bad);
    } else if (cmd == "fit") {
      uint64_t bytes = 0, cap = 0;
      in >> bytes >> cap;
      const char *bad = mgh::roi_check_footprint(bytes, cap);
      answer(bad);
    } else if (cmd == "tol") {
      int is_double = 0;
      in >> is_double;
      const double A = num(in), R = num(in), M = num(in);
      double t = 0;
      const char *bad = mgh::roi_tolres(is_double != 0, A, R, M, &t);
      if (bad) std::printf("bad %s\n", bad);
      else std::printf("ok %a\n", t);
    } else if (cmd == "ser") {
      uint64_t container = 0, nbox = 0;
      in >> container >> nbox;
      std::vector<mgh::RoiBox> boxes((size_t)nbox);
      uint64_t at = container;
      for (mgh::RoiBox &b : boxes) {
        for (int k = 0; k < mgh::kRoiMaxDim; k++) in >> b.lo[k];
        for (int k = 0; k < mgh::kRoiMaxDim; k++) in >> b.ext[k];
        b.tol = num(in);
        b.tolres = num(in);
        std::string hex;
        in >> hex;
        const std::vector<uint8_t> rec = unhex(hex);
        b.offset = at;
        b.size = rec.size();
        b.crc = mgh::fmt::crc32(rec.data(), rec.size());
        at += rec.size();
      }
      for (uint8_t v : mgh::roi_trailer_serialize(container, boxes)) std::printf("%02x", v);
      std::printf("\n");
    } else if (cmd == "open") {
      int D = 0;
      in >> D;
      uint64_t shape[mgh::kRoiMaxDim] = {1, 1, 1, 1, 1};
      for (int d = 0; d < D && d < mgh::kRoiMaxDim; d++) in >> shape[d];
      std::string hex;
      in >> hex;
      const std::vector<uint8_t> buf = unhex(hex);
      const uint8_t *tail = tail_of(buf, mgh::kRoiFooterBytes);
      if (!mgh::roi_footer_present(tail, buf.size())) {
        std::printf("none\n");
        continue;
      }
      mgh::RoiFooter f;
      std::vector<mgh::RoiBox> boxes;
      const char *bad = mgh::roi_footer_parse(tail, buf.size(), f);
      // (the table is read only after the footer placed it inside the buffer)
      if (!bad) bad = mgh::roi_table_parse(f, buf.data() + (buf.size() - mgh::kRoiFooterBytes - f.table_bytes), buf.size(), boxes);
      if (!bad) bad = mgh::roi_table_check_shape(boxes, D, shape);
      for (size_t i = 0; !bad && i < boxes.size(); i++) bad = mgh::roi_record_check_crc(boxes[i], buf.data() + boxes[i].offset);
      if (bad) {
        std::printf("bad %s\n", bad);
        continue;
      }
      std::printf("ok %" PRIu64 " %zu", f.container, boxes.size());
      for (const mgh::RoiBox &b : boxes) {
        for (int k = 0; k < mgh::kRoiMaxDim; k++) std::printf(" %" PRIu64, b.lo[k]);
        for (int k = 0; k < mgh::kRoiMaxDim; k++) std::printf(" %" PRIu64, b.ext[k]);
        std::printf(" %a %a %" PRIu64 " %" PRIu64, b.tol, b.tolres, b.offset, b.size);
      }
      std::printf("\n");
    } else if (cmd == "magic") {
      std::string hex;
      in >> hex;
      const std::vector<uint8_t> buf = unhex(hex);
      std::printf("%d%d%d\n", mgh::mask_footer_present(tail_of(buf, mgh::kMaskFooterBytes), buf.size()) ? 1 : 0,
                  mgh::pwrel_footer_present(tail_of(buf, mgh::kPwrelFooterBytes), buf.size()) ? 1 : 0,
                  mgh::roi_footer_present(tail_of(buf, mgh::kRoiFooterBytes), buf.size()) ? 1 : 0);
    } else {
      std::printf("unknown\n");
    }
  }
  return 0;
}
