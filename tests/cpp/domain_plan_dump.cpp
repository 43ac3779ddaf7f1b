// Stand-alone driver of mgard_amd/csrc/domain_plan.hpp for tests/test_domain_plan_cpu.py: built with the
// host compiler against the header alone (no HIP). One command per line on stdin, one line of output each;
// a refusal is "err CODE MESSAGE". Floating values travel as hexadecimal floats (%a) in both directions.
// METHOD is mgh_domain_decomposition (0 MaxDim, 1 Block, 2 Variable); a header travels as hex digits.
//   geom METHOD D SHAPE.. DIM SIZE NVAR VAR..
//        -> "geom num=N max=ELEMS | shape=a,b off=a,b contig=C lin=OFFSET | ..." (one group per id)
//   footprint D SHAPE.. ELEM RATIO DICT BLOCK PREFETCH                   -> "footprint BYTES"
//   split D SHAPE.. ELEM AVAIL METHOD BLOCK_SIZE VAR_DIM NVAR VAR.. RATIO DICT BLOCK
//        -> "split decomposed=B method=M dim=D size=S num=N"
//   multi N0 NDEV -> "multi SIZE"           dist N0.. -> "dist SIZE"
//   norm INF NORMALIZE TOTAL K (LN COUNT)..                              -> "norm RESULT"
//   tol32 | tol64 EBTYPE NORM TOL S NSUB                                 -> "tol RESULT"
//   fromheader HEX NVAR VAR..   (decomposer_from_header, then check_extents)
//        -> "ok decomposed=B method=M dim=D size=S num=N"
//   slab HEX ID LOCAL_TOL       -> "slab HEX" (slab_header, serialized)
//   frame SIZE AT CS            -> "next AT" (frame_prefix, then frame_next)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "domain_plan.hpp"

using namespace mgh;

static std::vector<uint64_t> list(std::istream &in, size_t n) {
  std::vector<uint64_t> v(n);
  for (uint64_t &x : v) in >> x;
  return v;
}
static double real(std::istream &in) {
  std::string t;
  in >> t;
  return std::strtod(t.c_str(), nullptr);
}
static bool refused(const Refusal &r) {
  if (r.msg) std::printf("err %d %s\n", r.code, r.msg);
  return r.msg != nullptr;
}
static std::string join(const std::vector<uint64_t> &v) {
  std::string s;
  for (uint64_t x : v) s += (s.empty() ? "" : ",") + std::to_string(x);
  return s;
}
// the header in a heap block of exactly its size, so that AddressSanitizer sees a read past it
static bool header(std::istream &in, fmt::Header &hd) {
  std::string hex;
  in >> hex;
  const size_t n = hex.size() / 2;
  std::unique_ptr<uint8_t[]> b(new uint8_t[n]);
  for (size_t i = 0; i < n; i++) b[i] = (uint8_t)std::strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
  try {
    fmt::parse_metadata(b.get(), n, hd);
  } catch (const std::exception &e) {
    std::printf("err %d %s\n", MGH_ERR_FORMAT, e.what());
    return false;
  }
  return true;
}
static void print_dd(const char *tag, const Decomposer &dd) {
  std::printf("%s decomposed=%d method=%d dim=%" PRIu64 " size=%" PRIu64 " num=%" PRIu64 "\n", tag, (int)dd.decomposed,
              dd.method, dd.dim, dd.size, dd.num);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "geom") {
      int method = 0, D = 0;
      in >> method >> D;
      fmt::Header hd;
      hd.shape = list(in, D);
      hd.dd_method = method == MGH_DD_MAXDIM ? fmt::DD_MAX_DIMENSION : method == MGH_DD_BLOCK ? fmt::DD_BLOCK : fmt::DD_VARIABLE;
      size_t nvar = 0;
      in >> hd.dd_dim >> hd.dd_size >> nvar;
      const std::vector<uint64_t> var = list(in, nvar);
      Decomposer dd;
      if (refused(decomposer_from_header(hd, var.data(), var.size(), dd))) continue;
      std::printf("geom num=%" PRIu64 " max=%" PRIu64, dd.num, dd.max_subdomain_elems());
      for (uint64_t id = 0; id < dd.num; id++)
        std::printf(" | shape=%s off=%s contig=%d lin=%" PRIu64, join(dd.subdomain_shape(id)).c_str(),
                    join(dd.subdomain_offset(id)).c_str(), (int)dd.contiguous(id), dd.linear_offset(id));
      std::printf("\n");
    } else if (cmd == "footprint" || cmd == "split") {
      int D = 0;
      in >> D;
      const std::vector<uint64_t> shape = list(in, D);
      size_t elem = 0;
      in >> elem;
      if (cmd == "footprint") {
        const double ratio = real(in);
        uint64_t dict = 0, block = 0;
        int prefetch = 0;
        in >> dict >> block >> prefetch;
        std::printf("footprint %zu\n", estimate_footprint(shape, elem, ratio, dict, block, prefetch != 0));
        continue;
      }
      size_t avail = 0, nvar = 0;
      int method = 0, var_dim = 0;
      uint64_t block_size = 0, dict = 0, block = 0;
      in >> avail >> method >> block_size >> var_dim >> nvar;
      const std::vector<uint64_t> var = list(in, nvar);
      const double ratio = real(in);
      in >> dict >> block;
      Decomposer dd;
      if (refused(split_domain(dd, D, shape.data(), elem, avail, method, block_size, var_dim, nvar ? var.data() : nullptr,
                               nvar, ratio, dict, block)))
        continue;
      print_dd("split", dd);
    } else if (cmd == "multi") {
      uint64_t n0 = 0;
      int ndev = 0;
      in >> n0 >> ndev;
      std::printf("multi %" PRIu64 "\n", multi_slab_size(n0, ndev));
    } else if (cmd == "dist") {
      std::vector<uint64_t> n0;
      for (uint64_t x; in >> x;) n0.push_back(x);
      uint64_t size = 0;
      if (refused({MGH_ERR_INVALID_ARGUMENT, dist_slab_size(n0, &size)})) continue;
      std::printf("dist %" PRIu64 "\n", size);
    } else if (cmd == "norm") {
      NormAccumulator na;
      int inf = 0, normalize = 0;
      uint64_t total = 0, k = 0;
      in >> inf >> normalize >> total >> k;
      na.inf = inf != 0;
      na.normalize = normalize != 0;
      for (uint64_t i = 0; i < k; i++) {
        const double ln = real(in);
        uint64_t count = 0;
        in >> count;
        na.add(ln, count);
      }
      std::printf("norm %a\n", na.result(total));
    } else if (cmd == "tol32" || cmd == "tol64") {
      int eb = 0;
      in >> eb;
      const double norm = real(in), tol = real(in), s = real(in);
      uint64_t nsub = 0;
      in >> nsub;
      if (cmd == "tol32") std::printf("tol %a\n", (double)local_abs_tol<float>(eb, (float)norm, (float)tol, (float)s, nsub));
      else std::printf("tol %a\n", local_abs_tol<double>(eb, norm, tol, s, nsub));
    } else if (cmd == "fromheader" || cmd == "slab") {
      fmt::Header hd;
      if (!header(in, hd)) continue;
      Decomposer dd;
      if (cmd == "slab") {
        uint64_t id = 0;
        in >> id;
        const double local_tol = real(in);
        if (refused(decomposer_from_header(hd, nullptr, 0, dd))) continue;
        if (refused({MGH_ERR_FORMAT, check_extents(dd)})) continue;
        std::printf("slab ");
        for (uint8_t b : fmt::serialize_metadata(slab_header(hd, dd, id, local_tol))) std::printf("%02x", b);
        std::printf("\n");
        continue;
      }
      size_t nvar = 0;
      in >> nvar;
      const std::vector<uint64_t> var = list(in, nvar);
      if (refused(decomposer_from_header(hd, nvar ? var.data() : nullptr, nvar, dd))) continue;
      if (refused({MGH_ERR_FORMAT, check_extents(dd)})) continue;
      print_dd("ok", dd);
    } else if (cmd == "frame") {
      size_t size = 0, at = 0, next = 0;
      uint64_t cs = 0;
      in >> size >> at >> cs;
      const char *bad = frame_prefix(size, at);
      if (!bad) bad = frame_next(size, at, cs, &next);
      if (refused({MGH_ERR_FORMAT, bad})) continue;
      std::printf("next %zu\n", next);
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
