"""mgh_compress_layers and its readers driven by a C++ consumer (tests/cpp/layers_consumer.cpp), built with hipcc
against the public headers and libmgard_hip.so the way tests/test_gpu_cpp_ladder.py builds its own. The consumer
prints what the mirror of compress_hip.hpp returned; here that is held against the Python binding on the same
array: layers of the same size and content, the same reconstruction bit for bit, every step within its bound."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.util import smooth_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (34, 33, 32)
TOLS = [1e-1, 1e-2, 1e-3, 1e-4]
INF = float("inf")


@pytest.fixture(scope="module")
def consumer(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("cpp_layers") / "layers_consumer")
    lib = os.path.join(ROOT, "mgard_amd", "libmgard_hip.so")
    assert os.path.exists(lib), "libmgard_hip.so is not built"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "layers_consumer.cpp"),
                           "-L", os.path.dirname(lib), "-lmgard_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    return exe


@pytest.mark.gpu
def test_cpp_layers(consumer, tmp_path):
    import mgard_amd
    from mgard_amd import highlevel as hl
    x = smooth_field(SHAPE, np.float32)
    x.tofile(str(tmp_path / "x.bin"))
    out = subprocess.run([consumer, str(tmp_path / "x.bin"), *map(str, SHAPE), str(tmp_path / "layer")],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "OK" in out.stdout, (out.returncode, out.stdout, out.stderr)
    lines = [l.split() for l in out.stdout.splitlines()]
    cfg = hl.Config(huff_dict_size=1024)
    want = hl.compress_layers(x, TOLS, INF, mgard_amd.REL, config=cfg)
    got = [l[1:] for l in lines if l[0] == "layer"]
    assert len(got) == len(TOLS)
    assert [l[1:] for l in lines if l[0] == "stats"] == [["1", str(len(TOLS)), "0"]]
    norm = float(np.max(np.abs(x)))
    for k, (t, buf) in enumerate(zip(got, want)):
        container = np.fromfile(str(tmp_path / ("layer%d.bin" % k)), dtype=np.uint8)
        assert float.fromhex(t[0]) == TOLS[k] and int(t[1]) == container.size == buf.size
        # (the same container up to the order of its outlier lists, which two runs of the quantizer do not share)
        meta = hl.metadata_parse(bytes(buf))["metadata_size"]
        assert np.array_equal(container[:meta], buf[:meta])
        assert np.array_equal(hl.decompress(container, config=cfg), hl.decompress(buf, config=cfg))
        assert 0 < float.fromhex(t[2]) <= TOLS[k] * norm                      # within the bound of its last layer
        assert t[3] == "1" and int(t[4]) == k + 1 and float.fromhex(t[5]) == TOLS[k]   # the two readers agree
    last = np.fromfile(str(tmp_path / "layerout.bin"), dtype=np.float32).reshape(SHAPE)
    assert np.array_equal(last.view(np.int32), hl.decompress_layers(want, config=cfg).view(np.int32))
    assert [l[1:] for l in lines if l[0] == "out_of_order"] == [["1", str(len(TOLS))]]
    assert [l[1:] for l in lines if l[0] == "refused"] == [["1", "1"]]


def test_cpp_layers_mirror_compiles_on_host():
    """No GPU needed: the new wrappers of the header-only mirror compile as plain C++17."""
    src = ('#include "compress_hip.hpp"\n'
           'int main() { float a[27] = {}; std::vector<void *> out; std::vector<size_t> n; void *d = nullptr;\n'
           '  auto v = mgard_hip::compress_layers(3, mgard_hip::data_type::Float, {3, 3, 3}, {1e-2, 1e-3}, 0.0,\n'
           '                                      mgard_hip::error_bound_type::ABS, a, out, n, {}, mgard_hip::HighLevelConfig(),\n'
           '                                      false);\n'
           '  std::vector<const void *> in(out.begin(), out.end());\n'
           '  auto w = mgard_hip::decompress_layers(in, n, d, mgard_hip::HighLevelConfig(), false);\n'
           '  mgard_hip::LayersReader r(in[0], n[0]);\n'
           '  return (int)v + (int)w + (int)r.add(in[1], n[1]) + (int)r.data(d, false) + r.count() + (int)r.tolerance(); }\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-x", "c++", "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr
