"""CPU tests of the surface of the precision layers in level order, in the way of
tests/test_layers_abi_cpu.py: the built library exports the new calls, the public headers declare them with the
argument lists the design fixes and compile as C, the Python bindings carry them, every stream-taking call of
include/mgard_hip_level_layers.h has a stream-order case, and the refusals that come before any device is touched
return their statuses."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOW = ["mgh_quantize_residual_linear", "mgh_dequantize_add_linear", "mgh_recompose_linear_to_level"]
HIGH = ["mgh_compress_level_layers", "mgh_level_layers_open", "mgh_level_layers_add", "mgh_level_layers_extend",
        "mgh_level_layers_count", "mgh_level_layers_depth", "mgh_level_layers_data", "mgh_decompress_level_layers",
        "mgh_layers_data_level"]
NOT_INT = ["mgh_level_layers_tolerance", "mgh_level_layers_close"]
MGH_ERR_INVALID_ARGUMENT = -1


def _text(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def _declarations(header):
    return {m.group(1): re.sub(r"\s+", " ", m.group(0))
            for m in re.finditer(r"\bint\s+(mgh_[a-z_0-9]+)\s*\([^;]*\)\s*;", _text(header))}


def test_library_exports_and_headers_declare_the_new_calls():
    import mgard_amd
    from mgard_amd import highlevel
    L = mgard_amd.load_library()
    low, high = _declarations("mgard_hip_level_layers.h"), _declarations("mgard_hip_compress.h")
    assert sorted(low) == sorted(LOW)
    for name in LOW + HIGH + NOT_INT:
        assert hasattr(L, name), name
    for name in HIGH:
        assert name in high, name
    for name in NOT_INT:
        assert name in _text("mgard_hip_compress.h")
    assert mgard_amd.LEVEL_LAYERS_SYMBOLS == LOW and set(HIGH + NOT_INT) <= set(highlevel.HL_SYMBOLS)
    assert low["mgh_quantize_residual_linear"] == (
        "int mgh_quantize_residual_linear(mgh_hierarchy *h, const void *d_coeff, int error_bound_type, double tol, "
        "double s, double norm, uint64_t dict_size, int64_t *d_linear_out, uint64_t *d_outlier_count, "
        "uint64_t *d_outlier_idx, int64_t *d_outlier_val, uint64_t outlier_capacity, void *d_residual_out, void *stream);")
    assert low["mgh_dequantize_add_linear"] == (
        "int mgh_dequantize_add_linear(mgh_hierarchy *h, int64_t *d_linear_window, uint64_t first, uint64_t count, "
        "int error_bound_type, double tol, double s, double norm, uint64_t dict_size, int prep_huffman, "
        "const uint64_t *d_outlier_idx, const int64_t *d_outlier_val, uint64_t outlier_count, int store, "
        "void *d_acc_linear, void *stream);")
    assert low["mgh_recompose_linear_to_level"] == (
        "int mgh_recompose_linear_to_level(mgh_hierarchy *h, const void *d_acc_linear, int level, void *d_out, "
        "void *stream);")
    # the writer's arguments are mgh_compress_layers'
    assert high["mgh_compress_level_layers"] == high["mgh_compress_layers"].replace("mgh_compress_layers",
                                                                                    "mgh_compress_level_layers")


def test_python_wrappers_exist():
    import mgard_amd
    from mgard_amd import highlevel as hl
    for name in ("quantize_residual_linear", "dequantize_add_linear", "recompose_linear_to_level"):
        assert callable(getattr(mgard_amd.Hierarchy, name)), name
    for name in ("compress_level_layers", "decompress_level_layers"):
        assert callable(getattr(hl, name)), name
    for name in ("add", "extend", "data", "depth", "tolerance", "close"):
        assert callable(getattr(hl.LevelLayers, name)), name
    import inspect
    assert "level" in inspect.signature(hl.Layers.data).parameters


def test_every_stream_call_of_the_header_has_a_stream_case():
    """tests/test_stream_cases_cpu.py for include/mgard_hip_level_layers.h and tests/test_gpu_stream_level_layers.py."""
    import tests.test_gpu_stream_level_layers as m
    with_stream = {name for name, params in re.findall(r"\b(mgh_[a-z_0-9]+)\s*\(([^;{}]*?)\)\s*;",
                                                        _text("mgard_hip_level_layers.h"), flags=re.S)
                   if re.search(r"\bvoid\s*\*\s*stream\b", params)}
    assert with_stream == set(LOW)
    entries = [e for _, es, _ in m.CASE_TABLE for e in es]
    assert sorted(entries) == sorted(with_stream)
    for name, _, routes in m.CASE_TABLE:
        assert callable(getattr(m, "_case_" + name, None)) and "fused3" in routes, name


def test_headers_compile_as_c(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "mgard_hip_level_layers.h"\n#include "mgard_hip_compress.h"\n'
                   "int main(void) {\n"
                   "  int (*a)(mgh_hierarchy *, const void *, int, double, double, double, uint64_t, int64_t *, uint64_t *,\n"
                   "           uint64_t *, int64_t *, uint64_t, void *, void *) = mgh_quantize_residual_linear;\n"
                   "  int (*b)(mgh_hierarchy *, int64_t *, uint64_t, uint64_t, int, double, double, double, uint64_t, int,\n"
                   "           const uint64_t *, const int64_t *, uint64_t, int, void *, void *) = mgh_dequantize_add_linear;\n"
                   "  int (*c)(mgh_hierarchy *, const void *, int, void *, void *) = mgh_recompose_linear_to_level;\n"
                   "  int (*d)(mgh_level_layers **, const void *, size_t, const mgh_config *, int) = mgh_level_layers_open;\n"
                   "  int (*e)(mgh_level_layers *, const void *, size_t, int) = mgh_level_layers_add;\n"
                   "  int (*f)(mgh_level_layers *, int, const void *, size_t, int) = mgh_level_layers_extend;\n"
                   "  int (*g)(const mgh_level_layers *) = mgh_level_layers_count;\n"
                   "  int (*h)(const mgh_level_layers *, int) = mgh_level_layers_depth;\n"
                   "  double (*i)(const mgh_level_layers *, int) = mgh_level_layers_tolerance;\n"
                   "  int (*j)(mgh_level_layers *, int, void **, int) = mgh_level_layers_data;\n"
                   "  void (*k)(mgh_level_layers *) = mgh_level_layers_close;\n"
                   "  int (*l)(int, const void *const *, const size_t *, int, const mgh_config *, void **, int) =\n"
                   "      mgh_decompress_level_layers;\n"
                   "  int (*m)(int, int, const uint64_t *, int, const double *, double, int, const void *, void **, size_t *,\n"
                   "           const void *const *, const mgh_config *, int) = mgh_compress_level_layers;\n"
                   "  int (*n)(mgh_layers *, int, void **, int) = mgh_layers_data_level;\n"
                   "  return !(a && b && c && d && e && f && g && h && i && j && k && l && m && n);\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])


def test_cpp_mirror_compiles_on_host():
    src = ('#include "compress_hip.hpp"\n'
           'int main() { float a[27] = {}; std::vector<void *> out; std::vector<size_t> n; void *d = nullptr;\n'
           '  auto v = mgard_hip::compress_level_layers(3, mgard_hip::data_type::Float, {3, 3, 3}, {1e-2, 1e-3}, 0.0,\n'
           '                                            mgard_hip::error_bound_type::ABS, a, out, n, {},\n'
           '                                            mgard_hip::HighLevelConfig(), false);\n'
           '  std::vector<const void *> in(out.begin(), out.end());\n'
           '  auto w = mgard_hip::decompress_level_layers(in, n, 0, d, mgard_hip::HighLevelConfig(), false);\n'
           '  mgard_hip::LevelLayersReader r(in[0], n[0], 0);\n'
           '  mgard_hip::LayersReader p(in[0], n[0]);\n'
           '  return (int)v + (int)w + (int)r.add(in[1], n[1], 0) + (int)r.extend(0, in[0], n[0], 1) + (int)r.data(0, d, false) +\n'
           '         r.count() + r.depth(0) + (int)r.tolerance(0) + (int)p.data(0, d, false); }\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-x", "c++", "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr


def test_refusals_that_need_no_device():
    import mgard_amd
    from mgard_amd import highlevel as hl
    L = hl._hl()
    err = lambda: L.mgh_last_error()
    shape = (C.c_uint64 * 3)(9, 9, 9)
    data = (C.c_float * 729)()
    cfg = hl.Config()

    def layers(tols):
        k = len(tols)
        ptrs, szs = (C.c_void_p * max(k, 1))(*([0xdead0] * max(k, 1))), (C.c_size_t * max(k, 1))()
        rc = L.mgh_compress_level_layers(3, 0, shape, k, (C.c_double * max(k, 1))(*tols), float("inf"), 1, data, ptrs, szs,
                                         None, C.byref(cfg), 0)
        assert all(ptrs[i] == 0xdead0 for i in range(max(k, 1)))  # nothing allocated, nothing cleared
        return rc

    for tols, msg in (([], b"ntol must be in 1..64"), ([10.0 ** -(k / 16) for k in range(65)], b"ntol must be in 1..64"),
                      ([1e-2, 0.0], b"positive and finite"), ([1e-2, 1e-2], b"strictly decreasing"),
                      ([1e-3, 1e-2], b"strictly decreasing")):
        assert layers(tols) == MGH_ERR_INVALID_ARGUMENT and b"compress_level_layers: " in err() and msg in err(), (tols, err())
    p = C.c_void_p(0xdead0)
    assert L.mgh_level_layers_open(None, data, 8, None, 0) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_level_layers_open(C.byref(p), None, 8, None, 0) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_level_layers_add(None, data, 8, 0) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_level_layers_extend(None, 0, data, 8, 0) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_level_layers_data(None, 0, C.byref(p), 0) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_layers_data_level(None, 0, C.byref(p), 0) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_level_layers_count(None) == -1 and L.mgh_level_layers_depth(None, 0) == -1
    assert L.mgh_level_layers_tolerance(None, 0) == 0.0
    L.mgh_level_layers_close(None)
    out = C.c_void_p()
    one, size = (C.c_void_p * 1)(C.addressof(data)), (C.c_size_t * 1)(8)
    for k in (0, -1, 65):
        assert L.mgh_decompress_level_layers(k, one, size, 0, None, C.byref(out), 0) == MGH_ERR_INVALID_ARGUMENT
        assert b"nlayers" in err()
    assert L.mgh_decompress_level_layers(1, None, size, 0, None, C.byref(out), 0) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_decompress_level_layers(1, one, size, 0, None, None, 0) == MGH_ERR_INVALID_ARGUMENT
    low = mgard_amd.load_library()
    assert low.mgh_quantize_residual_linear(None, None, 0, 1e-3, 0.0, 1.0, 1024, None, None, None, None, 0, None,
                                            None) == MGH_ERR_INVALID_ARGUMENT
    assert low.mgh_dequantize_add_linear(None, None, 0, 1, 0, 1e-3, 0.0, 1.0, 1024, 1, None, None, 0, 1, None,
                                         None) == MGH_ERR_INVALID_ARGUMENT
    assert low.mgh_recompose_linear_to_level(None, None, 0, None, None) == MGH_ERR_INVALID_ARGUMENT
