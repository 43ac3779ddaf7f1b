"""mgh_compress_level_layers and its readers driven by a C++ consumer (tests/cpp/level_layers_consumer.cpp), built
with hipcc against the public headers and libmgard_hip.so the way tests/test_gpu_cpp_layers.py builds its own. The
consumer prints what the mirror of compress_hip.hpp returned; here that is held against the Python binding on the
same array."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.util import smooth_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (34, 33, 32)
TOLS = [1e-1, 1e-2, 1e-3]
INF = float("inf")


@pytest.fixture(scope="module")
def consumer(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("cpp_level_layers") / "level_layers_consumer")
    lib = os.path.join(ROOT, "mgard_amd", "libmgard_hip.so")
    assert os.path.exists(lib), "libmgard_hip.so is not built"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "level_layers_consumer.cpp"),
                           "-L", os.path.dirname(lib), "-lmgard_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    return exe


@pytest.mark.gpu
def test_cpp_level_layers(consumer, tmp_path):
    import mgard_amd
    from mgard_amd import highlevel as hl
    x = smooth_field(SHAPE, np.float32)
    x.tofile(str(tmp_path / "x.bin"))
    cfg = hl.Config(huff_dict_size=1024)
    want = hl.compress_level_layers(x, TOLS, INF, mgard_amd.REL, config=cfg)
    L = hl.infer_level(want[0], None, cfg)[1]
    level = L - 1
    out = subprocess.run([consumer, str(tmp_path / "x.bin"), *map(str, SHAPE), str(level), str(tmp_path / "layer")],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "OK" in out.stdout, (out.returncode, out.stdout, out.stderr)
    lines = [l.split() for l in out.stdout.splitlines()]
    assert [l[1:] for l in lines if l[0] == "stats"] == [["1", str(len(TOLS)), "0"]]
    got = [l[1:] for l in lines if l[0] == "layer"]
    assert len(got) == len(TOLS)
    for k, (t, buf) in enumerate(zip(got, want)):
        container = np.fromfile(str(tmp_path / ("layer%d.bin" % k)), dtype=np.uint8)
        assert float.fromhex(t[0]) == TOLS[k] and int(t[1]) == container.size == buf.size
        meta = hl.metadata_parse(bytes(buf))
        assert meta["reorder"] and np.array_equal(container[:meta["metadata_size"]], buf[:meta["metadata_size"]])
        assert np.array_equal(hl.decompress(container, config=cfg), hl.decompress(buf, config=cfg))
        # the two readers agree; count, depth and tolerance of the layer just added
        assert t[2] == "1" and int(t[3]) == k + 1 and int(t[4]) == level and float.fromhex(t[5]) == TOLS[k]
    assert [l[1:] for l in lines if l[0] == "too_deep"] == [["1"]]
    assert [l[1:] for l in lines if l[0] == "depths"] == [[str(L), str(level), str(level)]]
    # layer 0 at the full level, layers 1 and 2 below it: what the Python reader gives for the same walk
    with hl.LevelLayers(want[0], level, config=cfg) as r:
        r.add(want[1], level).add(want[2], level).extend(0, want[0], L)
        ref = r.data(L)
    last = np.fromfile(str(tmp_path / "layerout.bin"), dtype=np.float32).reshape(SHAPE)
    assert np.array_equal(last.view(np.int32), ref.view(np.int32))
