"""mgh_estimate_sizes and mgh_compress_budget driven by a C++ consumer (tests/cpp/budget_consumer.cpp), built
with hipcc against the public headers and libmgard_hip.so the way tests/test_gpu_cpp_verify.py builds its own.
The consumer prints what the mirrors of compress_hip.hpp returned; here that is held against the Python
binding on the same array: the same estimates, the same tolerance, a container of the same size and content."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.util import smooth_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (34, 33, 32)
INF = float("inf")


@pytest.fixture(scope="module")
def consumer(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("cpp_budget") / "budget_consumer")
    lib = os.path.join(ROOT, "mgard_amd", "libmgard_hip.so")
    assert os.path.exists(lib), "libmgard_hip.so is not built"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "budget_consumer.cpp"),
                           "-L", os.path.dirname(lib), "-lmgard_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    return exe


@pytest.mark.gpu
def test_cpp_estimates_and_budget(consumer, tmp_path):
    import mgard_amd
    from mgard_amd import highlevel as hl
    x = smooth_field(SHAPE, np.float32)
    x.tofile(str(tmp_path / "x.bin"))
    budget = x.nbytes // 4
    out = subprocess.run([consumer, str(tmp_path / "x.bin"), *map(str, SHAPE), str(budget), str(tmp_path / "c.bin")],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "OK" in out.stdout, (out.returncode, out.stdout, out.stderr)
    lines = [l.split() for l in out.stdout.splitlines()]
    cfg = hl.Config(huff_dict_size=256)
    want = hl.estimate_sizes(x, [1e-3, 1e-2, 1e-1], INF, mgard_amd.REL, config=cfg)
    got = [l[1:] for l in lines if l[0] == "estimate"]
    assert [(float.fromhex(g[0]), *map(int, g[1:])) for g in got] == \
        [(e.tol, e.bytes_min, e.bytes_max, e.outliers, e.code_bits, e.raw) for e in want]
    buf, tol_used, est = hl.compress_budget(x, budget, 1e-4, 1e2, rounds=4, s=INF, mode=mgard_amd.REL, config=cfg)
    (b,) = [l for l in lines if l[0] == "budget"]
    container = np.fromfile(str(tmp_path / "c.bin"), dtype=np.uint8)
    assert float.fromhex(b[1]) == tol_used and int(b[2]) == container.size == buf.size <= budget
    assert (int(b[3]), int(b[4])) == (est.bytes_min, est.bytes_max)
    # (the same container up to the order of its outlier lists, which two runs of the quantizer do not share)
    meta = hl.metadata_parse(bytes(buf))["metadata_size"]
    assert np.array_equal(container[:meta], buf[:meta])
    assert np.array_equal(hl.decompress(container, config=cfg), hl.decompress(buf, config=cfg))
    (e,) = [l for l in lines if l[0] == "error"]
    assert 0 < float.fromhex(e[1]) <= tol_used * float(np.max(np.abs(x)))
    assert [l[1:] for l in lines if l[0] == "too_small"] == [["1", "1"]]


def test_cpp_budget_mirrors_compile_on_host():
    """No GPU needed: the new wrappers of the header-only mirror compile as plain C++17."""
    src = ('#include "compress_hip.hpp"\n'
           'int main() { float a[27] = {}; void *out = nullptr; size_t n = 0; double tol = 0;\n'
           '  std::vector<mgh_size_estimate> est; mgh_size_estimate used;\n'
           '  auto v = mgard_hip::estimate_sizes(3, mgard_hip::data_type::Float, {3, 3, 3}, {1e-3}, 0.0,\n'
           '                                     mgard_hip::error_bound_type::ABS, a, {}, mgard_hip::HighLevelConfig(), est);\n'
           '  auto w = mgard_hip::compress_budget(3, mgard_hip::data_type::Float, {3, 3, 3}, 100, 1e-3, 1.0, 4, 0.0,\n'
           '                                      mgard_hip::error_bound_type::ABS, a, out, n, {}, mgard_hip::HighLevelConfig(),\n'
           '                                      false, tol, &used);\n'
           '  return (int)v + (int)w; }\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-x", "c++", "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr
