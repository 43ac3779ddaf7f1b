"""CPU tests of the surface of the precision layers: the built library exports the two
low-level calls, mgh_compress_layers and the reader's calls, the public headers declare them with the argument
lists the design fixes and compile as C, the Python bindings carry them, and the refusals that come before any
device is touched return their statuses."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mgard_hip.h": ["mgh_quantize_symbols_residual", "mgh_dequantize_add"],
       "mgard_hip_compress.h": ["mgh_compress_layers", "mgh_layers_open", "mgh_layers_add", "mgh_layers_count",
                                "mgh_layers_data", "mgh_decompress_layers"]}
MGH_ERR_INVALID_ARGUMENT = -1


def _declarations(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): m.group(0) for m in re.finditer(r"\bint\s+(mgh_[a-z_0-9]+)\s*\([^;]*\)\s*;", txt)}


def _flat(decl):
    return re.sub(r"\s+", " ", decl)


def test_library_exports_and_headers_declare_the_new_calls():
    import mgard_amd
    from mgard_amd import highlevel
    L = mgard_amd.load_library()
    for header, names in NEW.items():
        decl = _declarations(header)
        for name in names:
            assert name in decl, (header, name)
            assert hasattr(L, name), name
    for name in ("mgh_layers_tolerance", "mgh_layers_close"):  # (not `int`: the regular expression does not see them)
        assert hasattr(L, name) and name in open(os.path.join(ROOT, "include", "mgard_hip_compress.h")).read()
    assert set(NEW["mgard_hip.h"]) <= set(mgard_amd.SYMBOLS)
    assert set(NEW["mgard_hip_compress.h"]) | {"mgh_layers_tolerance", "mgh_layers_close"} <= set(highlevel.HL_SYMBOLS)
    low = _declarations("mgard_hip.h")
    assert _flat(low["mgh_quantize_symbols_residual"]) == (
        "int mgh_quantize_symbols_residual(mgh_hierarchy *h, const void *d_coeff, int error_bound_type, double tol, "
        "double s, double norm, uint64_t dict_size, uint16_t *d_symbols, uint32_t *d_freq_or_null, "
        "uint64_t *d_outlier_count, uint64_t *d_outlier_idx, int64_t *d_outlier_val, uint64_t outlier_capacity, "
        "void *d_residual_out, void *stream);")
    assert _flat(low["mgh_dequantize_add"]) == (
        "int mgh_dequantize_add(mgh_hierarchy *h, int64_t *d_quantized, int error_bound_type, double tol, double s, "
        "double norm, uint64_t dict_size, int prep_huffman, const uint64_t *d_outlier_idx, "
        "const int64_t *d_outlier_val, uint64_t outlier_count, int first, void *d_coeff_inout, void *stream);")
    high = _declarations("mgard_hip_compress.h")
    # the arguments are mgh_compress_ladder's
    assert _flat(high["mgh_compress_layers"]) == _flat(high["mgh_compress_ladder"]).replace("mgh_compress_ladder",
                                                                                          "mgh_compress_layers")


def test_headers_compile_as_c(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "mgard_hip.h"\n#include "mgard_hip_compress.h"\n'
                   "int main(void) {\n"
                   "  int (*a)(mgh_hierarchy *, const void *, int, double, double, double, uint64_t, uint16_t *, uint32_t *,\n"
                   "           uint64_t *, uint64_t *, int64_t *, uint64_t, void *, void *) = mgh_quantize_symbols_residual;\n"
                   "  int (*b)(mgh_hierarchy *, int64_t *, int, double, double, double, uint64_t, int, const uint64_t *,\n"
                   "           const int64_t *, uint64_t, int, void *, void *) = mgh_dequantize_add;\n"
                   "  int (*c)(mgh_layers **, const void *, size_t, const mgh_config *) = mgh_layers_open;\n"
                   "  int (*d)(mgh_layers *, const void *, size_t) = mgh_layers_add;\n"
                   "  int (*e)(const mgh_layers *) = mgh_layers_count;\n"
                   "  double (*f)(const mgh_layers *) = mgh_layers_tolerance;\n"
                   "  int (*g)(mgh_layers *, void **, int) = mgh_layers_data;\n"
                   "  void (*h)(mgh_layers *) = mgh_layers_close;\n"
                   "  int (*i)(int, const void *const *, const size_t *, const mgh_config *, void **, int) = mgh_decompress_layers;\n"
                   "  int (*j)(int, int, const uint64_t *, int, const double *, double, int, const void *, void **, size_t *,\n"
                   "           const void *const *, const mgh_config *, int) = mgh_compress_layers;\n"
                   "  return !(a && b && c && d && e && f && g && h && i && j);\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])


def test_refusals_that_need_no_device():
    import mgard_amd
    from mgard_amd import highlevel as hl
    L = hl._hl()
    err = lambda: L.mgh_last_error()
    shape = (C.c_uint64 * 3)(9, 9, 9)
    data = (C.c_float * 729)()
    cfg = hl.Config()

    def layers(tols, data_ptr=data, outs=True, sizes=True):
        k = len(tols)
        ptrs, szs = (C.c_void_p * max(k, 1))(*([0xdead0] * max(k, 1))), (C.c_size_t * max(k, 1))()
        rc = L.mgh_compress_layers(3, 0, shape, k, (C.c_double * max(k, 1))(*tols) if tols is not None else None, float("inf"),
                                   1, data_ptr, ptrs if outs else None, szs if sizes else None, None, C.byref(cfg), 0)
        assert all(ptrs[i] == 0xdead0 for i in range(max(k, 1)))  # nothing allocated, nothing cleared
        return rc

    for tols, msg in (([], b"ntol must be in 1..64"), ([10.0 ** -(k / 16) for k in range(65)], b"ntol must be in 1..64"),
                      ([1e-2, 0.0], b"positive and finite"), ([-1.0], b"positive and finite"),
                      ([float("inf")], b"positive and finite"), ([1e-2, float("nan")], b"positive and finite"),
                      ([1e-2, 1e-2], b"strictly decreasing"), ([1e-3, 1e-2], b"strictly decreasing"),
                      ([1e-1, 1e-2, 2e-2], b"strictly decreasing")):
        assert layers(tols) == MGH_ERR_INVALID_ARGUMENT and b"compress_layers: " in err() and msg in err(), (tols, err())
    assert layers([1e-2], outs=False) == MGH_ERR_INVALID_ARGUMENT and b"NULL" in err()
    assert layers([1e-2], sizes=False) == MGH_ERR_INVALID_ARGUMENT and b"NULL" in err()
    k1 = (C.c_void_p * 1)(0xdead0)
    assert L.mgh_compress_layers(3, 0, shape, 1, None, float("inf"), 1, data, k1, (C.c_size_t * 1)(), None, C.byref(cfg),
                                 0) == MGH_ERR_INVALID_ARGUMENT
    # the reader
    p = C.c_void_p(0xdead0)
    assert L.mgh_layers_open(None, data, 8, None) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_layers_open(C.byref(p), None, 8, None) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_layers_add(None, data, 8) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_layers_data(None, C.byref(p), 0) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_layers_count(None) == -1 and L.mgh_layers_tolerance(None) == 0.0
    L.mgh_layers_close(None)
    out = C.c_void_p()
    one, size = (C.c_void_p * 1)(C.addressof(data)), (C.c_size_t * 1)(8)
    for k in (0, -1, 65):
        assert L.mgh_decompress_layers(k, one, size, None, C.byref(out), 0) == MGH_ERR_INVALID_ARGUMENT and b"nlayers" in err()
    assert L.mgh_decompress_layers(1, None, size, None, C.byref(out), 0) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_decompress_layers(1, one, None, None, C.byref(out), 0) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_decompress_layers(1, one, size, None, None, 0) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_decompress_layers(1, (C.c_void_p * 1)(), size, None, C.byref(out), 0) == MGH_ERR_INVALID_ARGUMENT
    # the low-level calls: NULL handle
    assert mgard_amd.load_library().mgh_quantize_symbols_residual(None, None, 0, 1e-3, 0.0, 1.0, 1024, None, None, None, None,
                                                                  None, 0, None, None) == MGH_ERR_INVALID_ARGUMENT
    assert mgard_amd.load_library().mgh_dequantize_add(None, None, 0, 1e-3, 0.0, 1.0, 1024, 1, None, None, 0, 1, None,
                                                       None) == MGH_ERR_INVALID_ARGUMENT
