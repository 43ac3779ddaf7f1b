"""The readers of pointwise-relative buffers at reduced resolution driven by a C++ consumer
(tests/cpp/pwrel_views_example.cpp), built with hipcc against the public headers and libmgard_hip.so the way
tests/test_gpu_cpp_masked_views.py builds its own. What the mirror of compress_hip.hpp wrote for one level, one
coarsened view and one window is what the Python calls give for the consumer's buffer, byte for byte."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import mask_model as mm
from tests import pwrel_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (34, 33, 32)
LO, EXT = (3, 0, 31), (5, 33, 1)


@pytest.fixture(scope="module")
def consumer(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("cpp_pwrel_views") / "pwrel_views_example")
    lib = os.path.join(ROOT, "mgard_amd", "libmgard_hip.so")
    assert os.path.exists(lib), "libmgard_hip.so is not built"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pwrel_views_example.cpp"),
                           "-L", os.path.dirname(lib), "-lmgard_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    return exe


@pytest.mark.gpu
def test_cpp_pwrel_views(consumer, tmp_path):
    from mgard_amd import highlevel as hl
    fl = float(np.float32(1e-20))
    x = pm.smooth_field(SHAPE, np.float32, abs_floor=fl, planted=True)
    x[0, 0, 0] = np.nan
    x[-1, -1, -1] = 0.0
    x.tofile(str(tmp_path / "x.bin"))
    out = subprocess.run([consumer, str(tmp_path / "x.bin"), *map(str, SHAPE), str(tmp_path / "p")],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "OK" in out.stdout, (out.returncode, out.stdout, out.stderr)
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines() if l.strip()}
    cfg = hl.Config(huff_dict_size=1024)
    buf = np.fromfile(str(tmp_path / "pbuf.bin"), dtype=np.uint8)
    info = hl.pwrel_info(buf)
    assert info is not None and (info.eps, info.abs_floor) == (1e-1, fl)
    # one level, one coarsened view, one window: the Python calls on the consumer's buffer
    for key, want in (("level", hl.decompress_pwrel(buf, config=cfg, level=1)),
                      ("coarse", hl.decompress_pwrel(buf, config=cfg, coarsen=1)),
                      ("win", hl.decompress_pwrel_preview(buf, 1, config=cfg, window=(LO, EXT)))):
        got = np.fromfile(str(tmp_path / ("p%s.bin" % key)), dtype=np.float32)
        if key != "win":
            assert tuple(int(v) for v in lines[key]) == want.shape
        assert got.size == want.size and got.tobytes() == want.tobytes(), key
    # the corner nodes carry their classes into the coarse arrays
    level = np.fromfile(str(tmp_path / "plevel.bin"), dtype=np.float32)
    assert np.isnan(level[0]) and mm.int_view(level)[-1] == 0
    assert lines["preview0"] == ["1"] and lines["masked"] == ["1", "1"]
