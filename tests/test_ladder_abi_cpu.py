"""CPU tests of the surface of the tolerance ladder: the built library exports
mgh_quantize_symbols, mgh_compress_ladder and mgh_last_compress_stats (and the histogram call the
measurement script uses), the public headers declare them, the Python bindings carry them, and the
host-only refusal rule of mgh_quantize_symbols (size_plan.hpp) says what the header says."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgard_amd", "csrc")
NEW = {"mgard_hip.h": ["mgh_quantize_symbols"],
       "mgard_hip_compress.h": ["mgh_compress_ladder", "mgh_last_compress_stats", "mgh_histogram_sym16"]}


def _declarations(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): m.group(0) for m in re.finditer(r"\bint\s+(mgh_[a-z_0-9]+)\s*\([^;]*\)\s*;", txt)}


def test_library_exports_and_headers_declare_the_new_calls():
    import mgard_amd
    from mgard_amd import highlevel
    L = mgard_amd.load_library()
    for header, names in NEW.items():
        decl = _declarations(header)
        for name in names:
            assert name in decl, (header, name)
            assert hasattr(L, name), name
    assert "mgh_quantize_symbols" in mgard_amd.SYMBOLS
    assert set(NEW["mgard_hip_compress.h"]) <= set(highlevel.HL_SYMBOLS)
    # the argument lists the issue fixed
    q = _declarations("mgard_hip.h")["mgh_quantize_symbols"]
    assert re.sub(r"\s+", " ", q) == (
        "int mgh_quantize_symbols(mgh_hierarchy *h, const void *d_coeff, int error_bound_type, double tol, double s, "
        "double norm, uint64_t dict_size, uint16_t *d_symbols, uint32_t *d_freq_or_null, uint64_t *d_outlier_count, "
        "uint64_t *d_outlier_idx, int64_t *d_outlier_val, uint64_t outlier_capacity, void *stream);")
    lad = re.sub(r"\s+", " ", _declarations("mgard_hip_compress.h")["mgh_compress_ladder"])
    assert lad.startswith("int mgh_compress_ladder(int D, int dtype, const uint64_t *shape, int ntol, const double *tols, "
                          "double s, int error_bound_type, const void *original_data, void **compressed_data")
    assert lad.endswith("const void *const *coords, const mgh_config *config, int output_pre_allocated);")


def test_compress_stats_struct_matches_the_header():
    from mgard_amd import highlevel
    txt = open(os.path.join(ROOT, "include", "mgard_hip_compress.h")).read()
    body = re.search(r"typedef struct mgh_compress_stats \{(.*?)\} mgh_compress_stats;", txt, flags=re.S).group(1)
    fields = re.findall(r"uint64_t\s+([a-z_]+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == ["decompositions", "quantize_passes", "histogram_launches", "records", "raw_records",
                      "outlier_retries"]
    assert [k for k, _ in highlevel.CompressStats._fields_] == fields
    assert C.sizeof(highlevel.CompressStats) == 8 * len(fields)
    # no GPU is needed to read the counters of a thread that has written nothing... nor to refuse NULL
    import mgard_amd
    assert mgard_amd.load_library().mgh_last_compress_stats(None) == -1


def test_quantize_symbols_refusal_rule(tmp_path):
    src = tmp_path / "qsym.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "size_plan.hpp"\n'
                   "int main(int argc, char **argv) {\n"
                   "  for (int i = 1; i + 1 < argc; i += 2)\n"
                   "    std::printf(\"%d\\n\", mgh::qsym_refusal(std::strtoull(argv[i], nullptr, 10),\n"
                   "                                           std::strtoull(argv[i + 1], nullptr, 10)) ? 1 : 0);\n"
                   "  return 0;\n}\n")
    exe = str(tmp_path / "qsym")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe])
    cases = [(1, 2, 0), (1000, 8192, 0), (2 ** 32 - 1, 16384, 0), (2 ** 32, 8192, 1), (2 ** 33, 8192, 1), (0, 8192, 1),
             (1000, 0, 1), (1000, 1, 1), (1000, 3, 1), (1000, 8191, 1), (1000, 16385, 1), (1000, 16386, 1), (1000, 65536, 1)]
    args = [str(x) for c in cases for x in c[:2]]
    out = subprocess.run([exe, *args], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [c[2] for c in cases]
