"""CPU tests of the reconstruction at a coarser level of the hierarchy (reduced resolution).

No GPU: the new symbols and their signatures, mgh_infer_level_shape / mgh_infer_level_nodes on
containers written by metadata_serialize against oracle.Hierarchy, and the identity the GPU tests
(tests/test_gpu_multires.py) take their expected values from:

    expected(L) = recompose(z_L)[nodes of level L],  z_L = the coefficients with everything outside
                  the corner box level_shape(L) set to zero,

checked here against an INDEPENDENT hierarchy of shape level_shape(L) built from the sub-sampled
coordinates (normalize_coordinates = False) that recomposes the box on its own, bit for bit.
(Uniform grids only: a hierarchy built from sub-sampled NON-uniform coordinates takes its spacings as
differences of coordinates, the full hierarchy's coarse levels as sums of the fine spacings -- two
roundings of the same number, so that pair agrees to rounding only and pins nothing bit for bit.)
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
from tests.util import nonuniform_coords

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGH_ERR_INVALID_ARGUMENT = -1


def keep_rule(n, steps):
    """Indices in the finest grid after `steps` coarsenings: every second node and always the last."""
    idx = np.arange(n)
    for _ in range(steps):
        keep = list(range(0, len(idx), 2))
        if keep[-1] != len(idx) - 1:
            keep.append(len(idx) - 1)
        idx = idx[keep]
    return idx


def expected_level(H, coeff, level):
    """The yardstick: full recomposition of the coefficients zeroed outside the box, at the nodes of `level`."""
    ls = H.level_shape(level)
    z = np.zeros_like(coeff)
    sl = tuple(slice(0, m) for m in ls)
    z[sl] = coeff[sl]
    ix = np.ix_(*[keep_rule(n, H.l_target - level) for n in coeff.shape])
    return np.ascontiguousarray(H.recompose(z)[ix])


def _header_text(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


SIGNATURES = {
    "mgard_hip.h": [
        "int mgh_recompose_to_level(mgh_hierarchy *h, const void *d_coeff, int level, void *d_out, void *stream);",
        "int mgh_dequantize_recompose_to_level(mgh_hierarchy *h, int64_t *d_quantized, int error_bound_type, "
        "double tol, double s, double norm, uint64_t dict_size, int prep_huffman, const uint64_t *d_outlier_idx, "
        "const int64_t *d_outlier_val, uint64_t outlier_count, int level, void *d_out, void *stream);",
        "int mgh_dequantize_recompose_sym16_to_level(mgh_hierarchy *h, const uint16_t *d_symbols, "
        "int error_bound_type, double tol, double s, double norm, uint64_t dict_size, "
        "const uint64_t *d_outlier_idx, const int64_t *d_outlier_val, uint64_t outlier_count, int level, "
        "void *d_out, void *stream);",
        "int mgh_level_nodes(const mgh_hierarchy *h, int level, int dim, uint64_t *h_idx_out, uint64_t cap);",
    ],
    "mgard_hip_compress.h": [
        "int mgh_infer_level_shape(const void *compressed_data, size_t compressed_size, const mgh_config *config, "
        "int level, int *D_out, uint64_t *shape_out , int *l_target_out);",
        "int mgh_infer_level_nodes(const void *compressed_data, size_t compressed_size, const mgh_config *config, "
        "int level, int dim, uint64_t *h_idx_out, uint64_t cap);",
        "int mgh_decompress_level(const void *compressed_data, size_t compressed_size, int level, "
        "void **decompressed_data, const mgh_config *config, int output_pre_allocated);",
    ],
}


def test_symbols_and_signatures():
    import mgard_amd
    from mgard_amd import highlevel
    L = mgard_amd.load_library()
    for header, sigs in SIGNATURES.items():
        txt = _header_text(header)
        for sig in sigs:
            name = re.search(r"(mgh_[a-z_0-9]+)\(", sig).group(1)
            assert hasattr(L, name), name
            assert name in mgard_amd.SYMBOLS + highlevel.HL_SYMBOLS, name
            assert sig in txt, "declaration of %s differs from the documented one" % name


def test_python_keywords():
    import inspect
    import mgard_amd
    from mgard_amd import highlevel
    for fn in (mgard_amd.Hierarchy.recompose, mgard_amd.Hierarchy.dequantize_recompose,
               mgard_amd.Hierarchy.dequantize_recompose_sym16, highlevel.decompress):
        p = inspect.signature(fn).parameters
        assert "level" in p and p["level"].default is None, fn
    assert list(inspect.signature(mgard_amd.Hierarchy.level_nodes).parameters)[1:] == ["level", "dim"]
    assert list(inspect.signature(highlevel.infer_level).parameters) == ["buf", "level", "config"]


# (shape, dtype, non-uniform, max_larget_level or None)
HEADERS = [
    ((3001,), "f32", False, None),
    ((20, 31), "f64", False, None),
    ((50, 20, 31), "f32", True, None),
    ((129, 130, 257), "f32", False, 3),
    ((9, 8, 10, 17), "f32", False, None),
    ((4, 3, 20, 5, 31), "f64", True, None),
    ((5, 6, 7, 8, 9), "f32", False, 0),
    ((65, 70, 129), "f64", True, 2),
]


def _container(shape, dt, nonuniform, dd=None):
    from mgard_amd import highlevel as hl
    npdt = np.float64 if dt == "f64" else np.float32
    coords = [c.astype(np.float64).tolist() for c in nonuniform_coords(shape, npdt)] if nonuniform else None
    return np.frombuffer(hl.metadata_serialize(hl.DOUBLE if dt == "f64" else hl.FLOAT, list(shape), hl.REL, 1e-3,
                                               float("inf"), norm=1.0, coords=coords, dd=dd), dtype=np.uint8).copy()


@pytest.mark.parametrize("case", HEADERS, ids=lambda c: "x".join(map(str, c[0])) + "-" + c[1])
def test_infer_level_shape_and_nodes(case):
    from mgard_amd import highlevel as hl
    shape, dt, nonuniform, ml = case
    buf = _container(shape, dt, nonuniform)
    cfg = hl.Config()
    if ml is not None:
        cfg.max_larget_level = ml
    H = oracle.Hierarchy(shape, np.float64 if dt == "f64" else np.float32,
                         **({} if ml is None else dict(max_level=ml)))
    assert hl.infer_level(buf, None, cfg) == (None, H.l_target)
    assert hl.infer_level(buf, -1, cfg) == (None, H.l_target)
    for level in range(H.l_target + 1):
        assert hl.infer_level(buf, level, cfg) == (H.level_shape(level), H.l_target)
        for d, n in enumerate(shape):
            got = hl.infer_level_nodes(buf, level, d, cfg)
            assert np.array_equal(got, keep_rule(n, H.l_target - level)), (level, d)
            assert got.size == H.level_shape(level)[d]
            # the level marks of the oracle say the same: in the reordered layout the nodes of levels
            # <= `level` are the first level_shape(level)[d] positions
            assert int(np.sum(np.asarray(H.marks(d)) <= level)) == got.size
    for bad in (H.l_target + 1, H.l_target + 7):
        with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
            hl.infer_level(buf, bad, cfg)
        with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
            hl.infer_level_nodes(buf, bad, 0, cfg)


def test_infer_level_nodes_returns_l_target_for_negative_level():
    import mgard_amd
    from mgard_amd import highlevel as hl
    buf = _container((20, 31), "f32", False)
    hl.infer_level(buf, None)  # (declares the argument types)
    L = mgard_amd.load_library()
    cfg = hl.Config()
    rc = L.mgh_infer_level_nodes(C.c_void_p(buf.ctypes.data), buf.size, C.byref(cfg), -1, 0, None, 0)
    assert rc == oracle.Hierarchy((20, 31), np.float32).l_target


def test_decomposed_container_is_refused():
    import mgard_amd
    from mgard_amd import highlevel as hl
    buf = _container((129, 40, 40), "f32", False, dd=(0, 0, 65))  # MaxDim along dimension 0, 65 nodes a piece
    assert hl.infer(buf)[0] == (129, 40, 40)
    with pytest.raises(hl.MgardHipError, match=r"error -1\b.*domain-decomposed"):
        hl.infer_level(buf, 1)
    with pytest.raises(hl.MgardHipError, match=r"error -1\b.*domain-decomposed"):
        hl.infer_level(buf, None)
    with pytest.raises(hl.MgardHipError, match=r"error -1\b.*domain-decomposed"):
        hl.infer_level_nodes(buf, 0, 0)
    # the library is usable afterwards
    assert hl.infer_level(_container((20, 31), "f32", False), 0)[0] == oracle.Hierarchy((20, 31)).level_shape(0)
    assert MGH_ERR_INVALID_ARGUMENT == -1 and mgard_amd.load_library() is not None


IDENTITY = [
    ((17, 12, 9), np.float32, True, False),
    ((33, 33, 33), np.float64, True, False),
    ((20, 31), np.float32, True, False),
    ((6, 7, 9, 11), np.float64, False, False),
    ((50,), np.float32, True, False),
    ((5, 6, 7, 8, 9), np.float32, True, False),
]


@pytest.mark.parametrize("case", IDENTITY, ids=lambda c: "x".join(map(str, c[0])) + "-" + np.dtype(c[1]).name)
def test_zero_outside_the_box_identity(case):
    shape, dt, normalize, nonuniform = case
    if nonuniform:
        coords = nonuniform_coords(shape, dt)
    elif normalize:
        coords = [np.arange(n, dtype=dt) / dt(n - 1) for n in shape]  # (Hierarchy.hpp:695-703, in T)
    else:
        coords = [np.arange(n).astype(dt) for n in shape]
    H = oracle.Hierarchy(shape, dt, coords=coords if nonuniform else None, normalize_coordinates=normalize)
    u = np.random.default_rng(0).standard_normal(shape).astype(dt)
    c = H.decompose(u)
    assert np.array_equal(expected_level(H, c, H.l_target).view(np.uint8), H.recompose(c).view(np.uint8))
    ran = 0
    for level in range(1, H.l_target + 1):
        ls = H.level_shape(level)
        sub_coords = [x[keep_rule(n, H.l_target - level)] for x, n in zip(coords, shape)]
        Hs = oracle.Hierarchy(ls, dt, coords=sub_coords, normalize_coordinates=False)
        assert Hs.l_target == level
        box = np.ascontiguousarray(c[tuple(slice(0, m) for m in ls)])
        got, want = Hs.recompose(box), expected_level(H, c, level)
        assert got.shape == want.shape == ls
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), level
        ran += 1
    assert ran == H.l_target
    # level 0: no pass at all -- the head of the coefficient array
    l0 = H.level_shape(0)
    assert np.array_equal(expected_level(H, c, 0).view(np.uint8),
                          np.ascontiguousarray(c[tuple(slice(0, m) for m in l0)]).view(np.uint8))
