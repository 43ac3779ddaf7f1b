"""The C++ mirrors of the full-grid preview (compress_x_hip.hpp / compress_hip.hpp: decompress_preview;
ProgressiveReader::preview; mgard_hip.hpp: Compressor::Prolong) driven by a C++ consumer, built with hipcc against
libmgard_hip.so the way tests/test_gpu_cpp_coarsened.py builds its own. The consumer reads containers made here
and writes its results to files; they must carry the bits of the Python preview."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.util import smooth_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def consumer(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("cpp_preview") / "preview_consumer")
    lib = os.path.join(ROOT, "mgard_amd", "libmgard_hip.so")
    assert os.path.exists(lib), "libmgard_hip.so is not built"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "preview_consumer.cpp"),
                           "-L", os.path.dirname(lib), "-lmgard_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    return exe


def _run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "OK" in out.stdout, (out.returncode, out.stdout, out.stderr)


@pytest.mark.gpu
def test_cpp_decompress_preview_of_blocks(consumer, tmp_path):
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    shape, bs, K = (66, 45, 37), 33, 2  # (blocks of 33, 12 and 4 nodes: 4 -> 3 -> 2)
    u = smooth_field(shape, np.float32)
    cfg = hl.Config(domain_decomposition=hl.DD_BLOCK, block_size=bs)
    buf = hl.compress(u, 1e-3, np.inf, mg.ABS, config=cfg)
    assert hl.infer_coarsened(buf, None, cfg) == (None, K)
    path = str(tmp_path / "blocks.mgard")
    np.asarray(buf).tofile(path)
    _run(consumer, path, str(tmp_path / "out"), K, "block", bs)
    for k in range(K + 1):
        got = np.fromfile(str(tmp_path / ("out.k%d.bin" % k)), dtype=np.float32).reshape(shape)
        want = hl.decompress_preview(buf, k, config=cfg)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "k = %d" % k
    assert np.array_equal(np.fromfile(str(tmp_path / "out.k0.bin"), dtype=np.float32).reshape(shape),
                          hl.decompress(buf, config=cfg))


@pytest.mark.gpu
def test_cpp_progressive_preview_and_prolong(consumer, tmp_path):
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    shape = (33, 40, 34)
    u = smooth_field(shape, np.float32)
    cfg = hl.Config(reorder=1)
    buf = hl.compress(u, 1e-3, np.inf, mg.REL, config=cfg)
    _, L = hl.infer_level(buf, None, cfg)
    path = str(tmp_path / "one.mgard")
    np.asarray(buf).tofile(path)
    _run(consumer, path, str(tmp_path / "out"), L, "progressive")
    for level in range(L + 1):
        got = np.fromfile(str(tmp_path / ("out.p%d.bin" % level)), dtype=np.float32).reshape(shape)
        want = hl.decompress_preview(buf, L - level, config=cfg)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "level %d" % level


def test_cpp_preview_mirrors_compile_on_host():
    """No GPU needed: the new wrappers of the header-only mirrors compile as plain C++17."""
    src = ('#include "compress_hip.hpp"\n#include "compress_x_hip.hpp"\n#include "mgard_hip.hpp"\n'
           'int main() { void *p = nullptr;\n'
           '  auto a = mgard_hip::decompress_preview(nullptr, 0, 0, p, mgard_hip::HighLevelConfig(), false);\n'
           '  auto b = mgard_x::decompress_preview(nullptr, 0, 0, p, mgard_x::Config(), false);\n'
           '  auto c = &mgard_hip::ProgressiveReader::preview;\n'
           '  auto d = &mgard_hip::Compressor<3, float>::Prolong;\n'
           '  return (int)a + (int)b + (c != nullptr) + (d != nullptr); }\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c++", "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr
