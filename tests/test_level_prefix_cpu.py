"""Reduced resolution from the head of a reorder = 1 record, the part that needs no GPU: the library
exports the entry points, and the two properties of the level linearisation that k_box_from_linear
and mgh_decompress_level rely on hold in the oracle."""
import ctypes
import os

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["mgh_level_box_from_linear", "mgh_dequantize_recompose_linear_to_level",
               "mgh_lossless_decompress_prefix", "mgh_last_decompress_stats"]

# the shapes the design was checked on, 1-D to 5-D, dyadic and not
SHAPES = [(5,), (8,), (33,), (100,), (9, 6), (17, 17), (9, 10, 17), (5, 9, 17), (6, 8, 10), (33, 20, 17),
          (5, 5, 5, 5), (3, 4, 5, 6, 7)]


def _random_shapes():
    rng = np.random.default_rng(20240607)
    out = []
    for D in range(1, 6):
        for _ in range(3):
            hi = {1: 400, 2: 60, 3: 24, 4: 12, 5: 8}[D]
            out.append(tuple(int(x) for x in rng.integers(3, hi + 1, size=D)))
    return out


def test_library_exports_the_entry_points():
    lib = os.path.join(ROOT, "mgard_amd", "libmgard_hip.so")
    assert os.path.exists(lib), "libmgard_hip.so is not built"
    L = ctypes.CDLL(lib)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    import mgard_amd
    from mgard_amd import highlevel
    for name in NEW_SYMBOLS:
        assert name in mgard_amd.SYMBOLS + highlevel.HL_SYMBOLS, name
    assert callable(mgard_amd.Hierarchy.level_box_from_linear)
    assert callable(mgard_amd.Hierarchy.dequantize_recompose_linear)
    assert callable(highlevel.last_decompress_stats)


@pytest.mark.parametrize("shape", SHAPES + _random_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_head_of_the_linearised_array_is_the_box_of_the_level(shape):
    """1. level_linearize(q)[:N_l] is a permutation of q[0:m_0, ..., 0:m_{D-1}], m = level_shape(l).
    2. Where a hierarchy of shape level_shape(l) exists (extents >= 3), that head equals the linearisation of
    the box by that smaller hierarchy, whose l_target is l."""
    o = oracle.Hierarchy(shape, np.float64)
    n = int(np.prod(shape))
    q = np.arange(n, dtype=np.int64).reshape(shape)  # value = reordered linear index: all distinct
    lin = o.level_linearize(q).reshape(-1)
    assert lin.shape == (n,)
    for level in range(o.l_target + 1):
        m = o.level_shape(level)
        n_l = int(np.prod(m))
        box = q[tuple(slice(0, e) for e in m)]
        assert np.array_equal(np.sort(lin[:n_l]), np.sort(box.reshape(-1))), (shape, level)
        if min(m) >= 3:
            small = oracle.Hierarchy(m, np.float64)
            assert small.l_target == level, (shape, level, m)
            assert np.array_equal(small.level_linearize(np.ascontiguousarray(box)).reshape(-1), lin[:n_l]), \
                (shape, level)
        else:
            assert level == 0, (shape, level, m)
    # the last level: the whole array
    assert np.array_equal(o.level_linearize(lin.reshape(shape), inverse=True).reshape(-1), q.reshape(-1))


def test_rows_of_a_level_are_runs_of_the_stream():
    """9 x 10 x 17, the finest level: a natural row whose slow indices include a level node is ONE contiguous run
    (coarse-f and odd-f nodes interleaved); a row whose slow indices are all coarse keeps its odd-f nodes as one
    run. What the row-wise kernel streams."""
    shape = (9, 10, 17)
    o = oracle.Hierarchy(shape, np.float64)
    L = o.l_target
    n = int(np.prod(shape))
    pos = np.empty(n, dtype=np.int64)  # stream position of every reordered index
    lin = o.level_linearize(np.arange(n, dtype=np.int64).reshape(shape)).reshape(-1)
    pos[lin] = np.arange(n)
    pos = pos.reshape(shape)
    m = o.level_shape(L - 1)
    # reordered row (i, j): slow index i >= m[0] is a level-L node along dim 0
    row = pos[m[0], 0, :]
    nat = np.empty(shape[2], dtype=np.int64)  # natural order along f: coarse 0..m-1 -> 0, 2, ...; odd -> 1, 3, ...
    nat[0::2] = row[:m[2]]
    nat[1::2] = row[m[2]:]
    assert np.array_equal(nat, nat[0] + np.arange(shape[2]))
    # all slow indices coarse: only the odd-f half belongs to level L, one run
    row = pos[0, 0, m[2]:]
    assert np.array_equal(row, row[0] + np.arange(shape[2] - m[2]))
    assert row[0] >= int(np.prod(m))
