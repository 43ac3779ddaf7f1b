"""CPU test of what the reduced-resolution and preview readers of pointwise-relative buffers add: the four public
entry points are declared, exported and bound; the fused inverse pass mgh_pwrel_inverse_sampled_ is exported and bound
and declared in no header; and the row walk the kernel k_pwrel_inverse_sampled runs (mgard_amd/csrc/mask_plan.hpp:
mask_row_count, mask_row_begin, mask_row_source) finds, for every output element, the source index that
mask_sample_source -- the per-element arithmetic of mgh_mask_sample_ -- finds.

tests/cpp/mask_row_walk_dump.cpp is compiled with g++ against the header alone (no HIP) and once more with
-fsanitize=address,undefined as a stand-alone binary, the way tests/test_mask_sample_cpu.py builds its own."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mask_view_model as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgard_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "mask_row_walk_dump.cpp")
HIGH = ["mgh_decompress_pwrel_level", "mgh_decompress_pwrel_coarsened", "mgh_decompress_pwrel_preview",
        "mgh_decompress_pwrel_preview_window"]
LOW = ["mgh_pwrel_inverse_sampled_"]


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_new_symbols_are_declared_exported_and_bound():
    import mgard_amd
    from mgard_amd import highlevel
    L = mgard_amd.load_library()
    for name in HIGH + LOW:
        assert hasattr(L, name), name
    declared = set(re.findall(r"\b(mgh_[a-z_0-9]+)\s*\(", _header("mgard_hip_compress.h")))
    assert set(HIGH) <= declared and set(HIGH) <= set(highlevel.HL_SYMBOLS)
    # (the fused pass is internal: exported and bound, declared in no public header)
    assert mgard_amd.PWREL_VIEW_INTERNAL_SYMBOLS == LOW
    assert not set(LOW) & (set(mgard_amd.SYMBOLS) | set(highlevel.HL_SYMBOLS) | set(mgard_amd.INTERNAL_SYMBOLS))
    for h in os.listdir(os.path.join(ROOT, "include")):
        assert LOW[0] not in _header(h), h
    assert callable(mgard_amd.pwrel_inverse_sampled)
    for fn in ("decompress_pwrel", "decompress_pwrel_preview"):
        assert callable(getattr(highlevel, fn))


def test_cpp_mirror_compiles_on_host():
    """No GPU needed: the new wrappers of the header-only mirror compile as plain C++17."""
    src = ('#include "compress_hip.hpp"\n'
           'int main() { using namespace mgard_hip; void *buf = nullptr, *d = nullptr; size_t n = 0; HighLevelConfig c;\n'
           '  return (int)decompress_pwrel_level(buf, n, 0, d, c, false) + (int)decompress_pwrel_coarsened(buf, n, 1, d, c, false)\n'
           '    + (int)decompress_pwrel_preview(buf, n, 1, d, c, false)\n'
           '    + (int)decompress_pwrel_preview_window(buf, n, 1, {0, 0, 0}, {1, 1, 1}, d, c, false); }\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-x", "c++", "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr


# ---- the row walk -------------------------------------------------------------------------------------------------
def walk_cases():
    """[(id, shape of the source, one list or None per dimension)]"""
    cases = []
    # (a) the level lists of (34, 33, 32) at every level: level l keeps the nodes of l_target - l halvings
    shape = (34, 33, 32)
    steps = 0
    while True:
        lists = [mv.halved_nodes(e, steps) for e in shape]
        cases.append(("level-lists-%d-halvings" % steps, shape, lists))
        if min(len(l) for l in lists) <= 2:
            break
        steps += 1
    assert steps >= 4
    # (b) a window
    cases.append(("window", shape, [list(range(a, a + e)) for a, e in zip((3, 0, 31), (5, 33, 1))]))
    # (c) five dimensions, identity and strided lists mixed
    cases.append(("5d-mixed", (3, 2, 5, 4, 7), [[0, 2], None, [0, 2, 4], None, [0, 3, 6]]))
    cases.append(("5d-last-identity", (3, 2, 5, 4, 7), [None, [1], [4, 0], [0, 3], None]))
    # (d) one dimension, one output
    cases.append(("1d-one-output", (1000,), [[999]]))
    cases.append(("1d-every-seventh", (1000,), [list(range(0, 1000, 7))]))
    # (e) entries past the shape, in a slow dimension and in the last one
    cases.append(("2d-out-of-range", (17, 130), [[0, 5, 17, 16], [0, 200, 129, 3, 130, 2 ** 32 - 1]]))
    return cases


def _build(tmp_path_factory, name, extra=()):
    exe = str(tmp_path_factory.mktemp(name) / "mask_row_walk_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", CSRC, SRC, "-o", exe])
    return exe


def _line(shape, lists):
    out_shape = [shape[d] if l is None else len(l) for d, l in enumerate(lists)]
    parts = [str(len(shape))] + [str(e) for e in shape] + [str(e) for e in out_shape]
    for l in lists:
        parts += ["-1"] if l is None else [str(int(i)) for i in l]
    return " ".join(parts) + "\n"


def _expected(shape, lists):
    """Source index of every output element by NumPy, -1 where a list leads outside the array."""
    full = [np.arange(e, dtype=np.int64) if l is None else np.asarray(l, dtype=np.int64) for l, e in zip(lists, shape)]
    grid = np.meshgrid(*full, indexing="ij")
    inside = np.ones(grid[0].shape, dtype=bool)
    for g, e in zip(grid, shape):
        inside &= g < e
    flat = np.ravel_multi_index([np.minimum(g, e - 1) for g, e in zip(grid, shape)], shape)
    return np.where(inside, flat, -1).reshape(-1)


def _text():
    return "".join(_line(shape, lists) for _, shape, lists in walk_cases())


def test_level_lists_are_the_halved_nodes():
    """(a) rests on it: the nodes of a level are every second node and the last, halving by halving (mgh::level_nodes,
    which tests/test_multires_cpu.py pins), so the cases above are the lists the level reader uploads."""
    assert mv.halved_nodes(34, 1) == list(range(0, 33, 2)) + [33] and mv.halved_nodes(33, 5) == [0, 32]


def test_row_walk_is_mask_sample_source(tmp_path_factory):
    exe = _build(tmp_path_factory, "mask_row_walk")
    out = subprocess.run([exe], input=_text(), capture_output=True, text=True, check=True, timeout=300).stdout.splitlines()
    cases = walk_cases()
    assert len(out) == 2 * len(cases)
    kinds = set()
    for k, (name, shape, lists) in enumerate(cases):
        walk = np.array(out[2 * k].split(), dtype=np.int64)
        per_element = np.array(out[2 * k + 1].split(), dtype=np.int64)
        want = _expected(shape, lists)
        assert walk.shape == want.shape and np.array_equal(walk, per_element), name
        assert np.array_equal(walk, want), name
        kinds |= {bool(v) for v in (want < 0)}
    assert kinds == {False, True}        # outputs of both kinds were met


def test_program_is_clean_under_address_and_undefined_sanitizers(tmp_path_factory):
    exe = _build(tmp_path_factory, "mask_row_walk_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    p = subprocess.run([exe], input=_text(), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-4000:]
    assert len(p.stdout.splitlines()) == 2 * len(walk_cases())
