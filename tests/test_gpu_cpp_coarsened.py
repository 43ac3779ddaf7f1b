"""The C++ mirrors of the reduced resolution of decomposed containers (compress_hip.hpp, compress_x_hip.hpp:
decompress_coarsened, infer_coarsened_shape, infer_coarsened_nodes) driven by a C++ program, built with hipcc
against libmgard_hip.so and run on the GPU the way tests/test_gpu_cpp_multires.py drives its own: a
Block-decomposed container, every block of the stitched result against decompress_level of that block compressed
on its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_coarsened_blocks(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "coarsened_blocks")
    lib = os.path.join(ROOT, "mgard_amd", "libmgard_hip.so")
    assert os.path.exists(lib), "libmgard_hip.so is not built"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "coarsened_blocks.cpp"),
                           "-L", os.path.dirname(lib), "-lmgard_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "OK" in out.stdout


def test_cpp_coarsened_mirrors_compile_on_host():
    """No GPU needed: the extensions of the header-only mirrors compile as plain C++17."""
    src = ('#include "compress_hip.hpp"\n#include "compress_x_hip.hpp"\n'
           'int main() { void *p = nullptr; int K = 0;\n'
           '  std::vector<mgard_hip::SIZE> s;\n'
           '  std::vector<mgard_x::SIZE> t;\n'
           '  auto a = mgard_hip::infer_coarsened_shape(nullptr, 0, -1, mgard_hip::HighLevelConfig(), s, K);\n'
           '  auto b = mgard_hip::infer_coarsened_nodes(nullptr, 0, 0, 0, mgard_hip::HighLevelConfig(), s);\n'
           '  auto c = mgard_hip::decompress_coarsened(nullptr, 0, 0, p, mgard_hip::HighLevelConfig(), false);\n'
           '  auto d = mgard_x::infer_coarsened_shape(nullptr, 0, -1, mgard_x::Config(), t, K);\n'
           '  auto e = mgard_x::infer_coarsened_nodes(nullptr, 0, 0, 0, mgard_x::Config(), t);\n'
           '  auto f = mgard_x::decompress_coarsened(nullptr, 0, 0, p, mgard_x::Config(), false);\n'
           '  return (int)s.size() + (int)t.size() + (int)a + (int)b + (int)c + (int)d + (int)e + (int)f; }\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c++", "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr
