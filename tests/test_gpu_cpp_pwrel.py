"""mgh_compress_pwrel and its readers driven by a C++ consumer (tests/cpp/pwrel_example.cpp), built with hipcc against
the public headers and libmgard_hip.so the way tests/test_gpu_cpp_masked.py builds its own. The consumer prints what the
mirror of compress_hip.hpp returned; here its output array is held against the pointwise bound in float64 NumPy."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import mask_model as mm
from tests import pwrel_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (34, 33, 32)
EPS = 1e-3
FLOOR = float(np.float32(1e-20))


@pytest.fixture(scope="module")
def consumer(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("cpp_pwrel") / "pwrel_example")
    lib = os.path.join(ROOT, "mgard_amd", "libmgard_hip.so")
    assert os.path.exists(lib), "libmgard_hip.so is not built"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pwrel_example.cpp"),
                           "-L", os.path.dirname(lib), "-lmgard_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    return exe


@pytest.mark.gpu
def test_cpp_pwrel(consumer, tmp_path):
    x = pm.smooth_field(SHAPE, np.float32, abs_floor=FLOOR)
    x.tofile(str(tmp_path / "x.bin"))
    out = subprocess.run([consumer, str(tmp_path / "x.bin"), *map(str, SHAPE), float(EPS).hex(), float(FLOOR).hex(),
                          str(tmp_path / "p")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "OK" in out.stdout, (out.returncode, out.stdout, out.stderr)
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines() if l.strip()}
    buf = np.fromfile(str(tmp_path / "pbuf.bin"), dtype=np.uint8)
    mask, flag = pm.bitmaps(x, FLOOR)
    size, M, S, nm, nf = (int(v) for v in lines["info"][:5])
    eps, floor, delta = (float.fromhex(v) for v in lines["info"][5:])
    foot = pm.parse_footer(buf)
    assert size == buf.size == M + S + pm.FOOTER_BYTES and (foot["masked"], foot["record"]) == (M, S)
    assert (nm, nf, eps, floor) == (int(mask.sum()), int(flag.sum()), EPS, FLOOR) and 0 < delta < pm.log2_1p(EPS)
    got = np.fromfile(str(tmp_path / "pout.bin"), dtype=np.float32).reshape(SHAPE)
    valid = ~mask
    assert np.all(mm.int_view(got)[mask & ~flag] == 0) and np.isnan(got[mask & flag]).all()
    assert np.array_equal(np.signbit(got[valid]), np.signbit(x[valid]))
    xd, gd = x[valid].astype(np.float64), got[valid].astype(np.float64)
    assert np.all(np.abs(gd - xd) <= EPS * np.abs(xd))
    worst = float(np.max(np.abs(gd - xd) / np.abs(xd)))
    assert lines["verify"][0] == "1" and float.fromhex(lines["verify"][1]) == float.fromhex(lines["verify"][2]) == worst
    assert [int(v) for v in lines["verify"][3:]] == [int(valid.sum()), 0, 0]
    assert lines["masked"] == ["1", "0", "1", "1"]


def test_cpp_pwrel_mirror_compiles_on_host():
    """No GPU needed: the new wrappers of the header-only mirror compile as plain C++17."""
    src = ('#include "compress_hip.hpp"\n'
           'int main() { float a[27] = {}; void *buf = nullptr, *d = nullptr; size_t n = 0; bool p = false, w = false;\n'
           '  struct mgh_pwrel_info info {};\n'
           '  mgh_pwrel_compare r{};\n'
           '  auto v = mgard_hip::compress_pwrel(3, mgard_hip::data_type::Float, {3, 3, 3}, 1e-2, 0.0, a, buf, n, {},\n'
           '                                     mgard_hip::HighLevelConfig(), false);\n'
           '  auto i = mgard_hip::pwrel_info(buf, n, p, info);\n'
           '  auto q = mgard_hip::decompress_pwrel(buf, n, d, mgard_hip::HighLevelConfig(), false);\n'
           '  auto s = mgard_hip::verify_pwrel(buf, n, a, sizeof(a), mgard_hip::data_type::Float,\n'
           '                                   mgard_hip::HighLevelConfig(), r, w);\n'
           '  return (int)v + (int)i + (int)q + (int)s + (int)p + (int)w + info.flag_kind + (int)r.n; }\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-x", "c++", "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr
