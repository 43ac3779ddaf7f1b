"""mgh_compress_ladder driven by a C++ consumer (tests/cpp/ladder_consumer.cpp), built with hipcc against the
public headers and libmgard_hip.so the way tests/test_gpu_cpp_budget.py builds its own. The consumer prints
what the mirror of compress_hip.hpp returned; here that is held against the Python binding on the same array:
containers of the same size and content, every tier within its bound."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.util import smooth_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (34, 33, 32)
TOLS = [5e-2, 1e-1, 5e-1, 2e0]
INF = float("inf")


@pytest.fixture(scope="module")
def consumer(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("cpp_ladder") / "ladder_consumer")
    lib = os.path.join(ROOT, "mgard_amd", "libmgard_hip.so")
    assert os.path.exists(lib), "libmgard_hip.so is not built"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ladder_consumer.cpp"),
                           "-L", os.path.dirname(lib), "-lmgard_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    return exe


@pytest.mark.gpu
def test_cpp_ladder(consumer, tmp_path):
    import mgard_amd
    from mgard_amd import highlevel as hl
    x = smooth_field(SHAPE, np.float32)
    x.tofile(str(tmp_path / "x.bin"))
    out = subprocess.run([consumer, str(tmp_path / "x.bin"), *map(str, SHAPE), str(tmp_path / "tier")],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "OK" in out.stdout, (out.returncode, out.stdout, out.stderr)
    lines = [l.split() for l in out.stdout.splitlines()]
    cfg = hl.Config(huff_dict_size=1024)
    want = hl.compress_ladder(x, TOLS, INF, mgard_amd.REL, config=cfg)
    tiers = [l[1:] for l in lines if l[0] == "tier"]
    assert len(tiers) == len(TOLS)
    assert [l[1:] for l in lines if l[0] == "stats"] == [["1", str(len(TOLS)), "0"]]
    norm = float(np.max(np.abs(x)))
    for k, (t, buf) in enumerate(zip(tiers, want)):
        container = np.fromfile(str(tmp_path / ("tier%d.bin" % k)), dtype=np.uint8)
        assert float.fromhex(t[0]) == TOLS[k] and int(t[1]) == container.size == buf.size
        # (the same container up to the order of its outlier lists, which two runs of the quantizer do not share)
        meta = hl.metadata_parse(bytes(buf))["metadata_size"]
        assert np.array_equal(container[:meta], buf[:meta])
        assert np.array_equal(hl.decompress(container, config=cfg), hl.decompress(buf, config=cfg))
        err, vmax, bound, within = float.fromhex(t[2]), float.fromhex(t[3]), float.fromhex(t[4]), int(t[5])
        assert within == 1 and 0 < err == vmax <= bound and abs(bound - TOLS[k] * norm) <= 1e-6 * bound
    assert [l[1:] for l in lines if l[0] == "refused"] == [["1", "1"]]


def test_cpp_ladder_mirror_compiles_on_host():
    """No GPU needed: the new wrapper of the header-only mirror compiles as plain C++17."""
    src = ('#include "compress_hip.hpp"\n'
           'int main() { float a[27] = {}; std::vector<void *> out; std::vector<size_t> n; mgh_compress_stats st;\n'
           '  auto v = mgard_hip::compress_ladder(3, mgard_hip::data_type::Float, {3, 3, 3}, {1e-3, 1e-2}, 0.0,\n'
           '                                      mgard_hip::error_bound_type::ABS, a, out, n, {}, mgard_hip::HighLevelConfig(),\n'
           '                                      false);\n'
           '  return (int)v + mgh_last_compress_stats(&st); }\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-x", "c++", "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr
