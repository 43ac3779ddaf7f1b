"""CPU tests of the reduced resolution of domain-decomposed containers (mgh_infer_coarsened_shape,
mgh_infer_coarsened_nodes): no GPU, containers are headers written by metadata_serialize(dd=...).

The rule, restated here in plain Python and independent of the library:

  * one halving turns an extent n into n // 2 + 1 -- every second node and always the last one;
  * subdomain i has l_target_i = min over its dimensions of the halvings that bring the extent to 2,
    cut by max_larget_level; K = min_i l_target_i, and k > K is refused;
  * along dimension d the stitched grid is the concatenation, over the blocks j of the decomposition
    grid, of offset_j + (the nodes block j keeps after k halvings), offset_j in the FULL array.

The geometry of the three decompositions (MaxDim, Block, Variable) is restated too (blocks()).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.util import MAXDIM, BLOCK, VARIABLE, blocks, nonuniform_coords

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def keep(n, k):
    """Indices a dimension of n nodes keeps after k halvings."""
    idx = list(range(n))
    for _ in range(k):
        nxt = idx[0::2]
        if nxt[-1] != idx[-1]:
            nxt.append(idx[-1])
        assert len(nxt) == len(idx) // 2 + 1
        idx = nxt
    return idx


def steps_to_two(n):
    k = 0
    while n > 2:
        n = n // 2 + 1
        k += 1
    return k


def expected(shape, dd, sizes, max_level):
    """K, and per k the stitched shape and node lists."""
    grid = blocks(shape, dd, sizes)
    # every subdomain is one choice of a block per dimension; l_target is a min over dimensions, so the min over
    # the subdomains is the min over every block of every dimension
    K = min(steps_to_two(e) for per_dim in grid for _, e in per_dim)
    if max_level is not None:
        K = min(K, max_level)
    per_k = []
    for k in range(K + 1):
        nodes = [[o + i for o, e in per_dim for i in keep(e, k)] for per_dim in grid]
        per_k.append((tuple(len(x) for x in nodes), nodes))
    return K, per_k


def _container(shape, dt="f32", nonuniform=False, dd=None):
    from mgard_amd import highlevel as hl
    npdt = np.float64 if dt == "f64" else np.float32
    coords = [c.astype(np.float64).tolist() for c in nonuniform_coords(shape, npdt)] if nonuniform else None
    return np.frombuffer(hl.metadata_serialize(hl.DOUBLE if dt == "f64" else hl.FLOAT, list(shape), hl.REL, 1e-3,
                                               float("inf"), norm=1.0, coords=coords, dd=dd), dtype=np.uint8).copy()


def _config(sizes=None, max_level=None, dim=0):
    from mgard_amd import highlevel as hl
    kw = {}
    if sizes is not None:
        kw.update(domain_decomposition=hl.DD_VARIABLE, domain_decomposition_dim=dim, domain_decomposition_sizes=sizes)
    cfg = hl.Config(**kw)
    if max_level is not None:
        cfg.max_larget_level = max_level
    return cfg


def test_hand_checked_anchor():
    from mgard_amd import highlevel as hl
    buf = _container((129, 40, 40), dd=(MAXDIM, 0, 65))  # blocks of 65 and 64 planes
    assert hl.infer_coarsened(buf, None) == (None, 6)
    assert hl.infer_coarsened(buf, -1) == (None, 6)
    assert hl.infer_coarsened(buf, 1) == ((66, 21, 21), 6)
    want = list(range(0, 65, 2)) + list(range(65, 128, 2)) + [128]
    assert len(want) == 66
    assert hl.infer_coarsened_nodes(buf, 1, 0).tolist() == want
    assert hl.infer_coarsened_nodes(buf, 1, 1).tolist() == list(range(0, 39, 2)) + [39]
    assert hl.infer_coarsened(buf, 0) == ((129, 40, 40), 6)
    assert hl.infer_coarsened_nodes(buf, 0, 0).tolist() == list(range(129))


# (shape, dtype, non-uniform, dd, Variable sizes, max_larget_level, K worked out by hand)
GEOMETRY = [
    ((129, 40, 40), "f32", False, (MAXDIM, 0, 65), None, None, 6),
    ((40, 130, 33), "f32", False, (MAXDIM, 1, 65), None, None, 5),   # 33 -> 17 9 5 3 2
    ((70, 45, 37), "f32", False, (BLOCK, 0, 33), None, None, 2),     # remainder blocks of 4, 12 and 4: 4 -> 3 -> 2
    ((3001,), "f32", False, (VARIABLE, 0, 1000), [1000, 1500, 501], None, 9),  # 501 -> 251 126 64 33 17 9 5 3 2
    ((9, 8, 10, 34), "f32", False, (VARIABLE, 3, 17), [17, 17], None, 3),      # 8 -> 5 3 2
    ((129, 40, 40), "f32", False, (MAXDIM, 0, 65), None, 1, 1),
    ((65, 70, 129), "f64", True, (VARIABLE, 2, 65), [65, 64], None, 6),
    ((65, 70, 129), "f64", True, (MAXDIM, 2, 65), None, 2, 2),
]


@pytest.mark.parametrize("case", GEOMETRY, ids=lambda c: "x".join(map(str, c[0])) + "-dd%d-ml%s" % (c[3][0], c[5]))
def test_shape_and_nodes_equal_the_restated_rule(case):
    from mgard_amd import highlevel as hl
    shape, dt, nonuniform, dd, sizes, ml, K_hand = case
    buf = _container(shape, dt, nonuniform, dd)
    cfg = _config(sizes, ml, dd[1])
    K, per_k = expected(shape, dd, sizes, ml)
    assert K == K_hand
    assert hl.infer_coarsened(buf, None, cfg) == (None, K)
    for k in range(K + 1):
        eshape, enodes = per_k[k]
        assert hl.infer_coarsened(buf, k, cfg) == (eshape, K), k
        for d in range(len(shape)):
            got = hl.infer_coarsened_nodes(buf, k, d, cfg)
            assert got.tolist() == enodes[d], (k, d)
            assert np.all(np.diff(got) > 0) and got[0] == 0 and got[-1] == shape[d] - 1
    assert per_k[0][0] == tuple(shape)
    for bad in (K + 1, K + 5):
        with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
            hl.infer_coarsened(buf, bad, cfg)
        with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
            hl.infer_coarsened_nodes(buf, bad, 0, cfg)


def test_block_remainders_limit_the_halvings():
    """70 x 45 x 37 in blocks of 33: 3 x 2 x 2 = 12 subdomains, remainders of 4, 12 and 4 nodes."""
    grid = blocks((70, 45, 37), (BLOCK, 0, 33))
    assert [[e for _, e in g] for g in grid] == [[33, 33, 4], [33, 12], [33, 4]]
    from mgard_amd import highlevel as hl
    buf = _container((70, 45, 37), dd=(BLOCK, 0, 33))
    assert hl.infer_coarsened(buf, 2) == ((9 + 9 + 2, 9 + 4, 9 + 2), 2)
    with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
        hl.infer_coarsened(buf, 3)


def test_refusals_leave_the_library_usable():
    import mgard_amd
    from mgard_amd import highlevel as hl
    buf = _container((129, 40, 40), dd=(MAXDIM, 0, 65))
    L = mgard_amd.load_library()
    cfg = hl.Config()
    p = C.c_void_p(buf.ctypes.data)
    out = (C.c_uint64 * 129)()
    D, K = C.c_int(-7), C.c_int(-7)
    shp = (C.c_uint64 * hl.MAX_DIM)(*([99] * hl.MAX_DIM))
    hl.infer_coarsened(buf, None)  # (declares the argument types)
    assert L.mgh_infer_coarsened_shape(p, buf.size, C.byref(cfg), 7, C.byref(D), shp, C.byref(K)) == -1
    assert L.mgh_infer_coarsened_nodes(p, buf.size, C.byref(cfg), 7, 0, out, 129) == -1
    for bad_dim in (-1, 3, 5):
        assert L.mgh_infer_coarsened_nodes(p, buf.size, C.byref(cfg), 1, bad_dim, out, 129) == -1
    assert L.mgh_infer_coarsened_nodes(p, buf.size, C.byref(cfg), 1, 0, out, 10) == -1  # capacity
    # halvings < 0: only K; D_out and shape_out stay untouched; _nodes returns K
    D.value = -7
    assert L.mgh_infer_coarsened_shape(p, buf.size, C.byref(cfg), -1, C.byref(D), shp, C.byref(K)) == 0
    assert (D.value, K.value, list(shp)) == (-7, 6, [99] * hl.MAX_DIM)
    assert L.mgh_infer_coarsened_nodes(p, buf.size, C.byref(cfg), -1, 0, None, 0) == 6
    # a Variable decomposition whose sizes the config does not carry
    var = _container((3001,), dd=(VARIABLE, 0, 1000))
    with pytest.raises(hl.MgardHipError, match=r"error -1\b.*sizes"):
        hl.infer_coarsened(var, 1)
    with pytest.raises(hl.MgardHipError, match=r"error -1\b.*sizes"):
        hl.infer_coarsened_nodes(var, 1, 0)
    with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
        hl.infer_coarsened(var, 1, _config([1000, 1500, 500]))  # (do not add up)
    # afterwards
    assert hl.infer_coarsened(buf, 1) == ((66, 21, 21), 6)
    assert hl.infer_coarsened(var, 9, _config([1000, 1500, 501])) == ((3 + 4 + 2,), 9)


ONE_SUBDOMAIN = [((3001,), "f32", False, None), ((50, 20, 31), "f32", True, None), ((129, 130, 257), "f32", False, 3),
                 ((4, 3, 20, 5, 31), "f64", True, None), ((5, 6, 7, 8, 9), "f32", False, 0)]


@pytest.mark.parametrize("case", ONE_SUBDOMAIN, ids=lambda c: "x".join(map(str, c[0])))
def test_one_subdomain_is_infer_level(case):
    from mgard_amd import highlevel as hl
    shape, dt, nonuniform, ml = case
    buf = _container(shape, dt, nonuniform)
    cfg = _config(max_level=ml)
    _, L = hl.infer_level(buf, None, cfg)
    assert hl.infer_coarsened(buf, None, cfg) == (None, L)
    for k in range(L + 1):
        assert hl.infer_coarsened(buf, k, cfg) == hl.infer_level(buf, L - k, cfg)
        for d in range(len(shape)):
            assert np.array_equal(hl.infer_coarsened_nodes(buf, k, d, cfg), hl.infer_level_nodes(buf, L - k, d, cfg))
    with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
        hl.infer_coarsened(buf, L + 1, cfg)


SIGNATURES = [
    "int mgh_infer_coarsened_shape(const void *compressed_data, size_t compressed_size, const mgh_config *config, "
    "int halvings, int *D_out, uint64_t *shape_out , int *max_halvings_out);",
    "int mgh_infer_coarsened_nodes(const void *compressed_data, size_t compressed_size, const mgh_config *config, "
    "int halvings, int dim, uint64_t *h_idx_out, uint64_t cap);",
    "int mgh_decompress_coarsened(const void *compressed_data, size_t compressed_size, int halvings, "
    "void **decompressed_data, const mgh_config *config, int output_pre_allocated);",
]


def test_declarations():
    import inspect
    import mgard_amd
    from mgard_amd import highlevel as hl
    txt = open(os.path.join(ROOT, "include", "mgard_hip_compress.h")).read()
    txt = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    L = mgard_amd.load_library()
    for sig in SIGNATURES:
        name = re.search(r"(mgh_[a-z_0-9]+)\(", sig).group(1)
        assert hasattr(L, name), name
        assert name in hl.HL_SYMBOLS, name
        assert sig in txt, "declaration of %s differs from the documented one" % name
    hl.infer_coarsened(_container((20, 31)), None)
    for name in ("mgh_infer_coarsened_shape", "mgh_infer_coarsened_nodes", "mgh_decompress_coarsened"):
        assert getattr(L, name).argtypes is not None, name
    p = inspect.signature(hl.decompress).parameters
    assert list(p) == ["buf", "config", "out", "level", "coarsen"] and p["coarsen"].default is None
    assert list(inspect.signature(hl.infer_coarsened).parameters) == ["buf", "halvings", "config"]
    assert list(inspect.signature(hl.infer_coarsened_nodes).parameters) == ["buf", "halvings", "dim", "config"]
    for header in ("compress_hip.hpp", "compress_x_hip.hpp"):
        src = open(os.path.join(ROOT, "include", header)).read()
        for fn in ("decompress_coarsened", "infer_coarsened_shape", "infer_coarsened_nodes"):
            assert re.search(r"\b%s\(" % fn, src), (header, fn)


def test_level_and_coarsen_exclude_each_other():
    from mgard_amd import highlevel as hl
    with pytest.raises(ValueError, match="level.*coarsen"):
        hl.decompress(_container((20, 31)), level=1, coarsen=1)
