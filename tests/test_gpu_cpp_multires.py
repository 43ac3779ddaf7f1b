"""The C++ mirrors of the reconstruction at a coarser level (include/mgard_hip.hpp, compress_hip.hpp,
compress_x_hip.hpp: extensions) driven by a C++ program, built with hipcc against libmgard_hip.so and run on
the GPU the way tests/test_gpu_cpp_api.py drives its own: a level l_target - 1 call returns the shape and the
bits of the C ABI."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_multires_level(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "multires_level")
    lib = os.path.join(ROOT, "mgard_amd", "libmgard_hip.so")
    assert os.path.exists(lib), "libmgard_hip.so is not built"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "multires_level.cpp"),
                           "-L", os.path.dirname(lib), "-lmgard_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "OK" in out.stdout


def test_cpp_level_mirrors_compile_on_host():
    """No GPU needed: the extensions of the header-only mirrors compile as plain C++17."""
    src = ('#include "compress_hip.hpp"\n#include "compress_x_hip.hpp"\n'
           'int main() { void *p = nullptr; int lt = 0;\n'
           '  std::vector<mgard_hip::SIZE> s;\n'
           '  auto i = mgard_hip::infer_level_shape(nullptr, 0, -1, mgard_hip::HighLevelConfig(), s, lt);\n'
           '  auto a = mgard_hip::decompress_level(nullptr, 0, 0, p, mgard_hip::HighLevelConfig(), false);\n'
           '  auto b = mgard_x::decompress_level(nullptr, 0, 0, p, mgard_x::Config(), false);\n'
           '  auto f = &mgard_hip::Compressor<3, float>::RecomposeToLevel;\n'
           '  auto g = &mgard_hip::Compressor<3, double>::DequantizeRecomposeToLevel;\n'
           '  auto k = &mgard_hip::Compressor<3, float>::DequantizeRecomposeSym16ToLevel;\n'
           '  return (int)s.size() + (int)i + (int)a + (int)b + (f && g && k ? 0 : 1); }\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c++", "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr
