"""The masked readers at reduced resolution and verify_masked driven by a C++ consumer
(tests/cpp/masked_views_example.cpp), built with hipcc against the public headers and libmgard_hip.so the way
tests/test_gpu_cpp_masked.py builds its own. What the mirror of compress_hip.hpp wrote is held against the sampled
NumPy mask (tests/mask_view_model.py) and the restore value."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import mask_view_model as mv
from tests.util import inside_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (34, 33, 32)
TOL = 3e-2
LO, EXT = (3, 0, 31), (5, 33, 1)


@pytest.fixture(scope="module")
def consumer(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("cpp_masked_views") / "masked_views_example")
    lib = os.path.join(ROOT, "mgard_amd", "libmgard_hip.so")
    assert os.path.exists(lib), "libmgard_hip.so is not built"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "masked_views_example.cpp"),
                           "-L", os.path.dirname(lib), "-lmgard_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    return exe


@pytest.mark.gpu
def test_cpp_masked_views(consumer, tmp_path):
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
    # one halving: every second node and the last
    lists = [mv.halved_nodes(e, 1) for e in SHAPE]
    cshape = tuple(int(v) for v in lines["coarse"])
    assert cshape == tuple(len(l) for l in lists)
    smask = mv.sample(mask, lists)
    coarse = np.fromfile(str(tmp_path / "mcoarse.bin"), dtype=np.float32).reshape(cshape)
    cmask = np.fromfile(str(tmp_path / "mcmask.bin"), dtype=np.uint8).reshape(cshape)
    assert np.array_equal(cmask, smask.astype(np.uint8)) and 0 < smask.sum() < smask.size
    assert np.all(coarse[smask] == np.float32(-9999.0)) and np.isfinite(coarse[~smask]).all()
    assert not np.any(coarse[~smask] == np.float32(-9999.0))
    # the window of the preview
    wmask = mv.sample(mask, mv.window_lists(LO, EXT))
    win = np.fromfile(str(tmp_path / "mwin.bin"), dtype=np.float32).reshape(EXT)
    assert np.all(win[wmask] == np.float32(-9999.0)) and not np.any(win[~wmask] == np.float32(-9999.0))
    # verify_masked against the array with its NaN
    within, n, n_masked, nonfinite = (int(v) for v in lines["verify"][:4])
    max_abs_err, achieved, bound = (float.fromhex(v) for v in lines["verify"][4:])
    assert within == 1 and n_masked == int(mask.sum()) and n == x.size - n_masked and nonfinite == 0
    assert bound == TOL * float(np.max(np.abs(x[~mask]))) and 0 < max_abs_err == achieved <= bound
    assert lines["plain"] == ["1", "1"]


def test_cpp_masked_views_mirror_compiles_on_host():
    """No GPU needed: the new wrappers of the header-only mirror compile as plain C++17."""
    src = ('#include "compress_hip.hpp"\n'
           'int main() { using namespace mgard_hip; void *buf = nullptr, *d = nullptr; size_t n = 0; uint8_t m[8];\n'
           '  float a[27] = {}; mgh_verify_result r{}; uint64_t nm = 0; HighLevelConfig c;\n'
           '  int s = (int)decompress_masked_level(buf, n, 0, d, c, false) + (int)decompress_masked_coarsened(buf, n, 1, d, c, false)\n'
           '    + (int)decompress_masked_preview(buf, n, 1, d, c, false)\n'
           '    + (int)decompress_masked_preview_window(buf, n, 1, {0, 0, 0}, {1, 1, 1}, d, c, false)\n'
           '    + (int)decompress_mask_level(buf, n, 0, c, m) + (int)decompress_mask_coarsened(buf, n, 1, c, m)\n'
           '    + (int)decompress_mask_window(buf, n, {0, 0, 0}, {1, 1, 1}, c, m)\n'
           '    + (int)verify_masked(buf, n, a, sizeof(a), data_type::Float, 0, c, r, nm);\n'
           '  return s + (int)nm; }\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-x", "c++", "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr
