// Stand-alone driver of mgard_amd/csrc/huffman_record.hpp for tests/test_huffman_record_cpu.py: built with
// the host compiler against the header alone (no HIP). One command per line on stdin:
//   layout NCHUNK DICT UNITS NOUTLIER WITH_SYNC     -> "layout key=value ..." (PayloadLayout::compute)
//   parse FILE N N_PREFIX FIRST Q_CAP KEEP ON_DEV SYNC_DECODE
//                                   -> "err MESSAGE" or "ok key=value ..." (record_fixed + record_plan)
//   landed FILE N N_PREFIX FIRST C_DONE HAVE LAST   -> "landed C_HI" (chunks_landed on the record's table)
//   decode DICT CHUNK N UNITS HAS_SYNC BOOK_MAX_LEN NDEC CF SERIAL PAR PAIR TB   (TB = "unset": switch not set)
//                                   -> "decode kind=... sync= pair= tb= rtb= lds=" (decode_plan)
//   decode16 (the same arguments)   -> "decode16 kind=... refused=0|1" (sym16_refusal of that plan: a caller
//                                      whose output holds 16-bit symbols)
// A record is handed to the parser the way lossless_decompress() does it, every span in a heap block
// of exactly its size, so that AddressSanitizer sees a read past any of them: the first 24 bytes (or
// fewer), then the bytes up to the code units, and -- a host record, ON_DEV = 0 -- the whole record.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "huffman_record.hpp"

using namespace mgh;

struct Span {
  std::unique_ptr<uint8_t[]> p;
  size_t len = 0;
  Span(const uint8_t *src, size_t n) : p(new uint8_t[n]), len(n) {
    if (n) std::memcpy(p.get(), src, n);
  }
};

std::vector<uint8_t> read_file(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) {
    std::fprintf(stderr, "cannot read %s\n", path.c_str());
    std::exit(2);
  }
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// record_fixed + record_plan; head_out: the host copy record_plan saw
const char *parse(const std::vector<uint8_t> &file, uint64_t n, const DecodeRange &r, bool keep, bool on_dev,
                  const DecodeSwitches &sw, RecordPlan &R, std::unique_ptr<Span> *head_out = nullptr) {
  const Span rec(file.data(), file.size());
  const Span h24(rec.p.get(), std::min<size_t>(rec.len, 24));
  if (const char *bad = record_fixed(h24.p.get(), h24.len, rec.len, n, r, keep, R)) return bad;
  std::unique_ptr<Span> head(new Span(rec.p.get(), R.L.ddata));
  const char *bad = record_plan(head->p.get(), head->len, on_dev ? nullptr : rec.p.get(), rec.len, sw, R);
  if (head_out) *head_out = std::move(head);
  return bad;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "layout") {
      size_t nchunk = 0, dict = 0, units = 0, nout = 0;
      int with_sync = 0;
      in >> nchunk >> dict >> units >> nout >> with_sync;
      PayloadLayout L;
      L.compute(nchunk, dict, units, nout, with_sync != 0);
      std::printf("layout huffmeta=%zu decodebook_size=%zu decodebook=%zu ddata_size=%zu ddata=%zu outlier_count=%zu "
                  "outlier_idx=%zu outliers=%zu sync_tag=%zu sync=%zu total=%zu sync_bytes=%zu\n",
                  L.huffmeta, L.decodebook_size, L.decodebook, L.ddata_size, L.ddata, L.outlier_count, L.outlier_idx,
                  L.outliers, L.sync_tag, L.sync, L.total, PayloadLayout::sync_bytes(nchunk));
    } else if (cmd == "parse" || cmd == "landed") {
      std::string path;
      uint64_t n = 0;
      DecodeRange r;
      in >> path >> n >> r.n_prefix >> r.first;
      const std::vector<uint8_t> file = read_file(path);
      RecordPlan R;
      if (cmd == "landed") {
        size_t c_done = 0;
        uint64_t have = 0;
        int last = 0;
        in >> c_done >> have >> last;
        std::unique_ptr<Span> head;
        if (const char *bad = parse(file, n, r, false, false, DecodeSwitches(), R, &head)) {
          std::printf("err %s\n", bad);
          continue;
        }
        std::vector<uint64_t> table(2 * R.nchunk);
        std::memcpy(table.data(), head->p.get() + R.L.huffmeta, 16 * R.nchunk);
        std::printf("landed %zu\n", chunks_landed(R, table.data(), table.data() + R.nchunk, c_done, have, last != 0));
        continue;
      }
      int keep = 0, on_dev = 0, sync_decode = 1;
      in >> r.q_cap >> keep >> on_dev >> sync_decode;
      DecodeSwitches sw;
      sw.sync_decode = sync_decode != 0;
      if (const char *bad = parse(file, n, r, keep != 0, on_dev != 0, sw, R)) {
        std::printf("err %s\n", bad);
        continue;
      }
      std::printf("ok dict=%d chunk=%d nchunk=%zu huffmeta=%zu decodebook=%zu ddata=%zu ndec=%zu cf=%zu n_dec=%zu tb0=%zu "
                  "tb_cnt=%zu dbsize=%" PRIu64 " units=%" PRIu64 " ocount=%" PRIu64 " o_oc=%zu o_oidx=%zu o_oval=%zu "
                  "o_sync=%zu has_sync=%d units_lo=%zu units_need=%zu book_max_len=%d\n",
                  R.dict, R.chunk, R.nchunk, R.L.huffmeta, R.L.decodebook, R.L.ddata, R.ndec, R.cf, R.n_dec, R.tb0, R.tb_cnt,
                  R.dbsize, R.units, R.ocount, R.o_oc, R.o_oidx, R.o_oval, R.o_sync, (int)R.has_sync, R.units_lo,
                  R.units_need, R.book_max_len);
    } else if (cmd == "decode" || cmd == "decode16") {
      RecordPlan R;
      uint64_t n = 0;
      int has_sync = 0, serial = 0, par = 0;
      DecodeSwitches sw;
      in >> R.dict >> R.chunk >> n >> R.units >> has_sync >> R.book_max_len >> R.ndec >> R.cf >> serial >> par >> sw.pair;
      std::string tb;
      in >> tb;
      if (tb != "unset") sw.tb = std::strtol(tb.c_str(), nullptr, 10);
      R.has_sync = has_sync != 0;
      sw.serial = serial != 0;
      sw.par = par != 0;
      const DecodePlan D = decode_plan(R, n, sw);
      static const char *const kinds[] = {"none", "ring", "par", "serial"};
      if (cmd == "decode16") {
        std::printf("decode16 kind=%s refused=%d\n", kinds[(int)D.kind], sym16_refusal(D) != nullptr);
        continue;
      }
      std::printf("decode kind=%s sync=%d pair=%d tb=%d rtb=%d lds=%zu\n", kinds[(int)D.kind], (int)D.sync, (int)D.pair, D.tb,
                  D.rtb, D.lds);
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
