"""mgh_compress_roi and its readers driven by a C++ consumer (tests/cpp/roi_example.cpp), built with hipcc against the
public headers and libmgard_hip.so the way tests/test_gpu_cpp_pwrel.py builds its own. The consumer prints what the
mirror of compress_hip.hpp returned; here its buffer and its output array are held against the Python layer's and
against both bounds in float64 NumPy."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import roi_model as rm
from tests.test_gpu_roi import BOX, SHAPE, TOL, TOL_BOX, field, same_buffers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def consumer(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("cpp_roi") / "roi_example")
    lib = os.path.join(ROOT, "mgard_amd", "libmgard_hip.so")
    assert os.path.exists(lib), "libmgard_hip.so is not built"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "roi_example.cpp"),
                           "-L", os.path.dirname(lib), "-lmgard_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    return exe


@pytest.mark.gpu
def test_cpp_roi(consumer, tmp_path):
    import mgard_amd
    from mgard_amd import highlevel as hl
    x = field(SHAPE, np.float32)
    x.tofile(str(tmp_path / "x.bin"))
    out = subprocess.run([consumer, str(tmp_path / "x.bin"), *map(str, SHAPE), float(TOL).hex(), *map(str, BOX[0]),
                          *map(str, BOX[1]), float(TOL_BOX).hex(), str(tmp_path / "r")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "OK" in out.stdout, (out.returncode, out.stdout, out.stderr)
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines() if l.strip()}
    buf = np.fromfile(str(tmp_path / "rbuf.bin"), dtype=np.uint8)
    cfg = hl.Config(huff_dict_size=1024)
    same_buffers(buf, hl.compress_roi(x, TOL, [(BOX[0], BOX[1], TOL_BOX)], mode=mgard_amd.REL, config=cfg), x, cfg)
    model = rm.parse(buf)
    size, container, nbox, D = (int(v) for v in lines["info"][:4])
    tol_i, tolres = (float.fromhex(v) for v in lines["info"][4:6])
    assert size == buf.size and container == model["container"] and (nbox, D) == (1, 3)
    b = model["boxes"][0]
    assert (tol_i, tolres, int(lines["info"][6])) == (TOL_BOX, b["tolres"], b["size"]) and b["offset"] == container
    assert size == container + b["size"] + rm.ENTRY_BYTES + rm.FOOTER_BYTES
    got = np.fromfile(str(tmp_path / "rout.bin"), dtype=np.float32).reshape(SHAPE)
    norm = float(np.max(np.abs(x.astype(np.float64))))
    err = np.abs(got.astype(np.float64) - x.astype(np.float64))
    sl = tuple(slice(a, a + e) for a, e in zip(*BOX))
    assert err.max() <= TOL * norm and err[sl].max() <= TOL_BOX * norm
    v = lines["verify"]
    assert (v[0], v[4]) == ("1", "1")
    assert [float.fromhex(w) for w in v[1:4]] == [TOL * norm, err.max(), err.max()]
    assert [float.fromhex(w) for w in v[5:8]] == [TOL_BOX * norm, err[sl].max(), err[sl].max()]
    assert lines["container"] == ["1", "0", "1", "1"]
