"""mgh_compress_masked and its readers driven by a C++ consumer (tests/cpp/masked_example.cpp), built with hipcc against
the public headers and libmgard_hip.so the way tests/test_gpu_cpp_layers.py builds its own. The consumer prints what the
mirror of compress_hip.hpp returned; here that is held against the NumPy mask and the writer's bound: the restore
value at every masked position, and at the valid ones an error within tol times their absmax."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import mask_model as mm
from tests.util import inside_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (34, 33, 32)
TOL = 3e-2


@pytest.fixture(scope="module")
def consumer(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("cpp_masked") / "masked_example")
    lib = os.path.join(ROOT, "mgard_amd", "libmgard_hip.so")
    assert os.path.exists(lib), "libmgard_hip.so is not built"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "masked_example.cpp"),
                           "-L", os.path.dirname(lib), "-lmgard_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    return exe


@pytest.mark.gpu
def test_cpp_masked(consumer, tmp_path):
    x = inside_field(SHAPE, np.float32)
    g = np.meshgrid(*[np.arange(e) - (e - 1) / 2 for e in SHAPE], indexing="ij")
    mask = sum((a / (0.3 * e)) ** 2 for a, e in zip(g, SHAPE)) < 1.0
    x[mask] = np.nan
    x.tofile(str(tmp_path / "x.bin"))
    out = subprocess.run([consumer, str(tmp_path / "x.bin"), *map(str, SHAPE), str(tmp_path / "m")],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "OK" in out.stdout, (out.returncode, out.stdout, out.stderr)
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines() if l.strip()}
    buf = np.fromfile(str(tmp_path / "mbuf.bin"), dtype=np.uint8)
    size, C, R, nm, kind, restore = lines["info"]
    foot = mm.parse_footer(buf)
    assert int(size) == buf.size == int(C) + int(R) + mm.FOOTER_BYTES
    assert (int(C), int(R), int(nm), int(kind)) == (foot["container"], foot["record"], foot["n_masked"], foot["kind"])
    assert int(nm) == int(mask.sum()) and float.fromhex(restore) == -9999.0
    assert foot["restore_bits"] == mm.value_bits(np.float32, -9999.0)
    # (d) the restore value at every masked position
    assert lines["restored"] == [str(int(mask.sum())), "0"]
    got = np.fromfile(str(tmp_path / "mout.bin"), dtype=np.float32).reshape(SHAPE)
    assert np.all(got[mask] == np.float32(-9999.0))
    # (e) the bound at the valid positions: tol times their absmax, as the consumer and as NumPy see it
    bound = TOL * float(np.max(np.abs(x[~mask])))
    err, cbound = (float.fromhex(v) for v in lines["error"])
    assert cbound == bound and 0 < err <= bound
    assert float(np.max(np.abs(got[~mask].astype(np.float64) - x[~mask].astype(np.float64)))) == err
    assert lines["plain"] == ["1", "0", "1", "1"]


def test_cpp_masked_mirror_compiles_on_host():
    """No GPU needed: the new wrappers of the header-only mirror compile as plain C++17."""
    src = ('#include "compress_hip.hpp"\n'
           'int main() { float a[27] = {}; void *buf = nullptr, *d = nullptr; size_t n = 0; bool m = false;\n'
           '  const mgh_mask_spec spec{MGH_MASK_NONFINITE | MGH_MASK_VALUE, 1e20, 0.0};\n'
           '  struct mgh_masked_info info {};\n'
           '  auto v = mgard_hip::compress_masked(3, mgard_hip::data_type::Float, {3, 3, 3}, 1e-2, 0.0,\n'
           '                                      mgard_hip::error_bound_type::ABS, a, spec, buf, n, {},\n'
           '                                      mgard_hip::HighLevelConfig(), false);\n'
           '  auto w = mgard_hip::masked_info(buf, n, m, info);\n'
           '  auto r = mgard_hip::decompress_masked(buf, n, d, mgard_hip::HighLevelConfig(), false);\n'
           '  return (int)v + (int)w + (int)r + (int)m + info.kind; }\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-x", "c++", "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr
