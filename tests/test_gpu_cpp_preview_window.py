"""The C++ mirrors of the windowed full-grid preview (compress_x_hip.hpp / compress_hip.hpp:
decompress_preview_window; ProgressiveReader::preview_window; mgard_hip.hpp: Compressor::ProlongWindow) driven by a
C++ consumer, built with hipcc against libmgard_hip.so the way tests/test_gpu_cpp_preview.py builds its own. The
consumer reads a one-subdomain container made here, takes one window of every preview and compares it, in the
program, with the crop of the full preview."""
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
    exe = str(tmp_path_factory.mktemp("cpp_preview_window") / "preview_window_consumer")
    lib = os.path.join(ROOT, "mgard_amd", "libmgard_hip.so")
    assert os.path.exists(lib), "libmgard_hip.so is not built"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "preview_window_consumer.cpp"),
                           "-L", os.path.dirname(lib), "-lmgard_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    return exe


@pytest.mark.gpu
def test_cpp_window_of_a_one_subdomain_container(consumer, tmp_path):
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    shape = (33, 40, 34)
    u = smooth_field(shape, np.float32)
    cfg = hl.Config(reorder=1)
    buf = hl.compress(u, 1e-3, np.inf, mg.REL, config=cfg)
    _, L = hl.infer_level(buf, None, cfg)
    path = str(tmp_path / "one.mgard")
    np.asarray(buf).tofile(path)
    out = subprocess.run([consumer, path, str(L), "5", "39", "11", "17", "1", "23"], capture_output=True, text=True,
                         timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "OK" in out.stdout, (out.returncode, out.stdout, out.stderr)


def test_cpp_window_mirrors_compile_on_host():
    """No GPU needed: the new wrappers of the header-only mirrors compile as plain C++17."""
    src = ('#include "compress_hip.hpp"\n#include "compress_x_hip.hpp"\n#include "mgard_hip.hpp"\n'
           'int main() { void *p = nullptr;\n'
           '  std::vector<uint64_t> lo(3, 0), ext(3, 1);\n'
           '  auto a = mgard_hip::decompress_preview_window(nullptr, 0, 0, lo, ext, p, mgard_hip::HighLevelConfig(), false);\n'
           '  auto b = mgard_x::decompress_preview_window(nullptr, 0, 0, lo, ext, p, mgard_x::Config(), false);\n'
           '  auto c = &mgard_hip::ProgressiveReader::preview_window;\n'
           '  auto d = &mgard_hip::Compressor<3, float>::ProlongWindow;\n'
           '  return (int)a + (int)b + (c != nullptr) + (d != nullptr); }\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c++", "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr
