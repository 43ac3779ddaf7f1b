"""The C++ mirrors of the error statistics driven by a C++ consumer (tests/cpp/verify_consumer.cpp), built with
hipcc against the public headers and libmgard_hip.so the way tests/test_gpu_cpp_preview.py builds its own: the
reference-named mgard_x::L_inf_norm, L_2_norm, L_inf_error, L_2_error, MSE and PSNR on host and on device
pointers, and mgh_verify. The consumer prints its figures; here they are held against NumPy restatements of
include/mgard-x/Utilities/ErrorCalculator.h:22-121 -- maxima exactly, everything made of a sum within the
tolerance of that sum (compare_ref.sum_tolerance) -- including PSNR's range max(max, 0) - min on an
all-negative array (:112-119: the maximum starts at 0)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.compare_ref import ref_stats, sum_tolerance
from tests.util import smooth_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)
SHAPE = (129, 64, 65)  # (large and smooth enough to become a Huffman record: the reconstruction has an error)


@pytest.fixture(scope="module")
def consumer(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("cpp_verify") / "verify_consumer")
    lib = os.path.join(ROOT, "mgard_amd", "libmgard_hip.so")
    assert os.path.exists(lib), "libmgard_hip.so is not built"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "verify_consumer.cpp"),
                           "-L", os.path.dirname(lib), "-lmgard_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    return exe


def error_calculator(a, b):
    """The figures of ErrorCalculator.h for original a and reconstruction b (no non-finite values)."""
    s = ref_stats(a, b)
    n = a.size
    linf = s["ref_abs_max"] or EPS
    l2 = lambda sq, norm: math.sqrt((sq or EPS) / n) if norm else math.sqrt(sq or EPS)  # noqa: E731
    mse = s["sum_sq_err"] / n
    return {"L_inf_norm": linf, "L_2_norm_1": l2(s["ref_sum_sq"], True), "L_2_norm_0": l2(s["ref_sum_sq"], False),
            "L_inf_error_abs": s["max_abs_err"], "L_inf_error_rel": s["max_abs_err"] / linf,
            "L_2_error_abs_1": l2(s["sum_sq_err"], True), "L_2_error_rel_1": l2(s["sum_sq_err"], True) / l2(s["ref_sum_sq"], True),
            "L_2_error_abs_0": l2(s["sum_sq_err"], False), "MSE": mse,
            "PSNR": 20 * math.log10((max(s["ref_max"], 0.0) - s["ref_min"]) / math.sqrt(mse))}


@pytest.mark.gpu
def test_cpp_error_figures_and_verify(consumer, tmp_path):
    x = smooth_field(SHAPE, np.float32)
    neg = (-np.abs(x) - np.float32(0.5)).astype(np.float32)
    assert neg.max() < 0
    x.tofile(str(tmp_path / "x.bin"))
    neg.tofile(str(tmp_path / "neg.bin"))
    out = subprocess.run([consumer, str(tmp_path / "x.bin"), *map(str, SHAPE), str(tmp_path / "neg.bin"),
                          str(tmp_path / "y.bin")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "OK" in out.stdout, (out.returncode, out.stdout, out.stderr)
    y = np.fromfile(str(tmp_path / "y.bin"), dtype=np.float32).reshape(SHAPE)
    got = {}
    for line in out.stdout.splitlines():
        f = line.split()
        if len(f) == 3 and f[0] != "verify":
            got[(f[0], f[1])] = float.fromhex(f[2])
    n = x.size
    assert ref_stats(x, y)["max_abs_err"] > 0
    tol = 2 * sum_tolerance(n) + 8 * EPS  # (a quotient of two sums, a root and a logarithm on top of the sums' own bound)
    want = {"host": error_calculator(x, y), "neg-host": error_calculator(neg, x)}
    want["device"] = want["mixed"] = want["host"]
    want["neg-device"] = want["neg-host"]
    # the range rule: not ref_max - ref_min
    s = ref_stats(neg, x)
    assert want["neg-host"]["PSNR"] == 20 * math.log10(-s["ref_min"] / math.sqrt(s["sum_sq_err"] / n))
    assert abs(want["neg-host"]["PSNR"] - 20 * math.log10((s["ref_max"] - s["ref_min"]) / math.sqrt(s["sum_sq_err"] / n))) > 1
    for tag, figs in want.items():
        for name, w in figs.items():
            g = got[(tag, name)]
            if name in ("L_inf_norm", "L_inf_error_abs", "L_inf_error_rel"):
                assert g == w, (tag, name, g, w)
            elif name == "PSNR":
                assert abs(g - w) <= 20 / math.log(10) * tol + 4 * EPS * abs(w), (tag, name, g, w)
            else:
                assert abs(g - w) <= tol * w, (tag, name, g, w)
    # mgh_verify against the same arrays
    v = {}
    for line in out.stdout.splitlines():
        f = line.split()
        if f and f[0] == "verify":
            v.update(zip(f[1::2], f[2::2]))
    e = ref_stats(x, y)
    assert int(v["n"]) == n and int(v["nonfinite"]) == 0 and int(v["argmax"]) == e["argmax"]
    assert float.fromhex(v["max_abs_err"]) == e["max_abs_err"] == float.fromhex(v["achieved"])
    assert abs(float.fromhex(v["sum_sq_err"]) - e["sum_sq_err"]) <= sum_tolerance(n) * e["sum_sq_err"]
    assert float.fromhex(v["bound"]) == 1e-3 * float(np.max(np.abs(x)))
    assert int(v["bound_kind"]) == 0 and int(v["within"]) == 1


def test_cpp_error_mirrors_compile_on_host():
    """No GPU needed: the new wrappers of the header-only mirrors compile as plain C++17."""
    src = ('#include "compress_hip.hpp"\n#include "compress_x_hip.hpp"\n'
           'int main() { float a[2] = {1, 2}; mgh_verify_result r;\n'
           '  auto v = mgard_hip::verify(nullptr, 0, a, 8, mgard_hip::data_type::Float, 0, mgard_hip::HighLevelConfig(), r);\n'
           '  auto w = mgard_x::verify(nullptr, 0, a, 8, mgard_x::data_type::Float, 0, mgard_x::Config(), r);\n'
           '  double s = mgard_x::L_inf_norm(2, a) + mgard_x::L_2_norm<float>({2}, a, true) +\n'
           '             mgard_x::L_inf_error(2, a, a, mgard_x::error_bound_type::REL) +\n'
           '             mgard_x::L_2_error<float>({2}, a, a, mgard_x::error_bound_type::ABS, false) +\n'
           '             mgard_x::MSE(2, a, a) + mgard_x::PSNR(2, a, a) + mgard_hip::PSNR(2, a, a, 0);\n'
           '  return (int)v + (int)w + (int)s; }\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-x", "c++", "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr
