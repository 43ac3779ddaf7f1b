"""mgh_achieved_errors and mgh_compress_target driven by a C++ consumer (tests/cpp/target_consumer.cpp), built
with hipcc against the public headers and libmgard_hip.so the way tests/test_gpu_cpp_budget.py builds its own.
The consumer prints what the mirrors of compress_hip.hpp returned; here that is held against the Python
binding on the same array: the same statistics, the same tolerance and candidates, the same container."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.util import smooth_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (34, 33, 32)
INF = float("inf")
EXACT = ("n", "nonfinite", "max_abs_err", "argmax", "ref_min", "ref_max", "ref_abs_max")


@pytest.fixture(scope="module")
def consumer(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("cpp_target") / "target_consumer")
    lib = os.path.join(ROOT, "mgard_amd", "libmgard_hip.so")
    assert os.path.exists(lib), "libmgard_hip.so is not built"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "target_consumer.cpp"),
                           "-L", os.path.dirname(lib), "-lmgard_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    return exe


def _stats(words):
    """(tol, {field: value}) of a line the consumer printed"""
    names = ("n", "nonfinite", "max_abs_err", "argmax", "sum_sq_err", "ref_min", "ref_max", "ref_abs_max", "ref_sum_sq")
    vals = [int(w) if k in ("n", "nonfinite", "argmax") else float.fromhex(w) for k, w in zip(names, words[1:])]
    return float.fromhex(words[0]), dict(zip(names, vals))


@pytest.mark.gpu
def test_cpp_achieved_errors_and_target(consumer, tmp_path):
    import mgard_amd
    from mgard_amd import highlevel as hl
    x = smooth_field(SHAPE, np.float32)
    x.tofile(str(tmp_path / "x.bin"))
    cfg = hl.Config(huff_dict_size=1024)
    tols = [1e-1, 3e-1, 1e0]  # (Huffman records at this dictionary: tests/test_gpu_target.py)
    want = hl.achieved_errors(x, tols, INF, mgard_amd.REL, config=cfg)
    target = float(np.sqrt(want[0].rmse * want[2].rmse))  # (between the two: the search has to search)
    out = subprocess.run([consumer, str(tmp_path / "x.bin"), *map(str, SHAPE), str(hl.TARGET_RMSE), float(target).hex(),
                          str(tmp_path / "c.bin")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "OK" in out.stdout, (out.returncode, out.stdout, out.stderr)
    lines = [l.split() for l in out.stdout.splitlines()]
    got = [_stats(l[1:]) for l in lines if l[0] == "achieved"]
    assert [g[0] for g in got] == tols
    for (_, g), w in zip(got, want):
        # (a host array: the exact fields; the sums are those of the same call on the same array, too)
        assert all(g[k] == getattr(w, k) for k in g), (g, w)
    buf, tol_used, stats, candidates = hl.compress_target(x, hl.TARGET_RMSE, target, 5e-2, 5e0, rounds=6, s=INF,
                                                          mode=mgard_amd.REL, config=cfg)
    (t,) = [l for l in lines if l[0] == "target"]
    (u,) = [l for l in lines if l[0] == "used"]
    container = np.fromfile(str(tmp_path / "c.bin"), dtype=np.uint8)
    utol, ustats = _stats(u[1:])
    assert int(t[1]) == candidates == 8 and int(t[2]) == container.size == buf.size
    assert utol == tol_used and 5e-2 < tol_used < 5e0
    assert all(ustats[k] == getattr(stats, k) for k in ustats), (ustats, stats)
    assert stats.rmse <= target
    # (the same container up to the order of its outlier lists, which two runs of the quantizer do not share)
    meta = hl.metadata_parse(bytes(buf))["metadata_size"]
    assert np.array_equal(container[:meta], buf[:meta])
    assert np.array_equal(hl.decompress(container, config=cfg), hl.decompress(buf, config=cfg))
    r = hl.verify(container, x, config=cfg)
    assert all(getattr(r.stats, k) == ustats[k] for k in EXACT)
    assert [l[1:] for l in lines if l[0] == "not_met"] == [["1", "1"]]


def test_cpp_target_mirrors_compile_on_host():
    """No GPU needed: the new wrappers of the header-only mirror compile as plain C++17."""
    src = ('#include "compress_hip.hpp"\n'
           'int main() { float a[27] = {}; void *out = nullptr; size_t n = 0; double tol = 0; int cand = 0;\n'
           '  std::vector<mgh_error_stats> st; mgh_error_stats used;\n'
           '  auto v = mgard_hip::achieved_errors(3, mgard_hip::data_type::Float, {3, 3, 3}, {1e-3}, 0.0,\n'
           '                                      mgard_hip::error_bound_type::ABS, a, {}, mgard_hip::HighLevelConfig(), st);\n'
           '  auto w = mgard_hip::compress_target(3, mgard_hip::data_type::Float, {3, 3, 3}, mgard_hip::target_metric::PSNR,\n'
           '                                      80.0, 1e-3, 1.0, 8, 0.0, mgard_hip::error_bound_type::ABS, a, out, n, {},\n'
           '                                      mgard_hip::HighLevelConfig(), false, tol, &used, &cand);\n'
           '  return (int)v + (int)w; }\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-x", "c++", "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr
    # and the mgard_x mirror knows the new status
    src = ('#include "compress_x_hip.hpp"\n'
           'int main() { return mgard_x::detail::status(MGH_ERR_TARGET_NOT_MET) == mgard_x::compress_status_type::Failure ? 0 : 1; }\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-x", "c++", "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr
