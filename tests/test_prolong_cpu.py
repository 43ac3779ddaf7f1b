"""Full-grid preview on the CPU: the contract of mgh_prolong is what its kernel is described to compute.

The contract: the dense array of level L0 prolonged to the full grid equals
H.recompose(z), z the reordered coefficient array with everything outside the corner box of L0 zero.
The kernel is described as the interpolation f, then c, then r of every level above L0, `lerp_ref` per
value, every interpolated node (T)0 + interpolant, coarse nodes copied. This module restates that
level step in NumPy (in the data type, ratios from the oracle hierarchy) and holds it against
oracle.Hierarchy.recompose and ref.Hierarchy.recompose bit for bit.

The cases and fields are shared with tests/test_gpu_prolong.py.
"""
import os

import numpy as np
import pytest

import oracle
from oracle import ref
from tests.test_multires_cpu import keep_rule
from tests.util import nonuniform_coords, smooth_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (shape, dtypes, hierarchy options, runs the prolongation kernel?, what it is there for)
CASES_3D = {
    "5": ((5, 5, 5), (np.float32, np.float64), {}, False,
          "smallest hierarchy (a thin shape for the library: it runs the fallback there)"),
    "16": ((16, 16, 16), (np.float32, np.float64), {}, True, "even at every level"),
    "33": ((33, 33, 33), (np.float32, np.float64), {}, True, "dyadic"),
    "34x21x18": ((34, 21, 18), (np.float32, np.float64), {}, True,
                 "ghost nodes in every dimension, different depths per dimension"),
    "65x40x70-nonuniform": ((65, 40, 70), (np.float64,), dict(coords="nonuniform", normalize_coordinates=False), True,
                            "non-uniform coordinates, normalize_coordinates = False"),
    "17x101x18-tall": ((17, 101, 18), (np.float32, np.float64), {}, True,
                       "fastest extent 2^4 + 2; 64 x 4 tiles (coarse f <= 16 under coarse c >= 48)"),
    "9x9x129-wide+1": ((9, 9, 129), (np.float32, np.float64), {}, True,
                       "coarse extents 5 x 65: one more than the 4 x 64 tile in c and in f"),
    "9x129x9-tall+1": ((9, 129, 9), (np.float32, np.float64), {}, True,
                       "coarse extents 65 x 5: one more than the 64 x 4 tile in c and in f"),
    "129x255x33-chunks": ((129, 255, 33), (np.float32,), {}, True,
                          "65 coarse planes under 32 tiles: the march takes chunks of 2 planes and a last one of 1"),
    "33x40x34-maxlevel": ((33, 40, 34), (np.float32, np.float64), dict(max_level="top-1"), True,
                          "max_level = l_target - 1"),
}
FIELDS = ("smooth", "zeros")


def hierarchy_kw(shape, dt, opts, cls=oracle.Hierarchy):
    kw = {}
    if opts.get("coords") == "nonuniform":
        kw["coords"] = nonuniform_coords(shape, dt, seed=sum(shape))
    if "normalize_coordinates" in opts:
        kw["normalize_coordinates"] = opts["normalize_coordinates"]
    if opts.get("max_level") == "top-1":
        kw["max_level"] = cls(shape, dt).l_target - 1
    return kw


def field(shape, dt, which):
    """smooth: a smooth field plus noise. zeros: the same with a block of exact zeros and some -0.0 in it."""
    u = smooth_field(shape, dt, noise=1e-2)
    if which == "zeros":
        blk = tuple(slice(0, max(2, (2 * n) // 3)) for n in shape)
        u[blk] = 0
        flat = u.reshape(-1)
        flat[::7][flat[::7] == 0] = dt(-0.0)
        u[tuple(n - 1 for n in shape)] = dt(-0.0)
    return u


def zeroed(H, coeff, level):
    """The coefficient array with everything outside the corner box of `level` zero."""
    z = np.zeros_like(coeff)
    sl = tuple(slice(0, m) for m in H.level_shape(level))
    z[sl] = coeff[sl]
    return z


def coefficients(H, shape, dt, which):
    """Reordered coefficients of the field; for `zeros`, -0.0 also written straight into the coarsest box (those
    values are nodal values of every level and must come through every level step as they are)."""
    c = H.decompose(field(shape, dt, which))
    if which == "zeros":
        m = H.level_shape(0)
        c[tuple(slice(0, 1) for _ in m)] = dt(-0.0)
        c[tuple(k - 1 for k in m)] = dt(-0.0)
    return c


def level_of(full, H, level):
    ix = np.ix_(*[keep_rule(n, H.l_target - level) for n in full.shape])
    return np.ascontiguousarray(full[ix])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    assert not bad.any(), "%s: %d of %d values differ, first at %r" % (
        what, int(bad.sum()), bad.size, tuple(int(x[0]) for x in np.nonzero(bad)))


# ---- the level step, restated ---------------------------------------------------------------------
def lerp_ref(v0, v1, t):
    dt = v0.dtype.type
    r = v0 + v0 * t * dt(-1)
    return r + t * v1


def _step_dim(a, axis, n, ratio):
    """m -> n nodes along `axis` in padded coordinates: P = 2j is coarse node j (the last one of an even n sits at
    P = n, real index n - 1), P = 2j + 1 the interpolant of j and j + 1 with ratio[2j]; the ghost P = n - 1 of an
    even n has no output."""
    a = np.moveaxis(a, axis, -1)
    m = a.shape[-1]
    assert m == n // 2 + 1
    out = np.empty(a.shape[:-1] + (n,), a.dtype)
    even = np.zeros(n, bool)
    for P in range(2 * m - 1):
        if n % 2 == 0 and P == n - 1:
            continue
        real = min(P, n - 1)
        if P % 2 == 0:
            out[..., real] = a[..., P // 2]
            even[real] = True
        else:
            out[..., real] = lerp_ref(a[..., P // 2], a[..., P // 2 + 1], ratio[P - 1])
    return np.moveaxis(out, -1, axis), even


def prolong_step(coarse, H, l):
    """Level l - 1 -> l: f innermost, then c, then r; every interpolated node 0 + interpolant, coarse nodes copied."""
    dt = coarse.dtype.type
    n = H.level_shape(l)
    a, evens = coarse, [None] * len(n)
    for d in reversed(range(len(n))):
        a, evens[d] = _step_dim(a, d, n[d], H.ratio(l, d).astype(coarse.dtype))
    is_coarse = np.ones(n, bool)
    for d, e in enumerate(evens):
        is_coarse &= e.reshape([-1 if k == d else 1 for k in range(len(n))])
    return np.where(is_coarse, a, dt(0) + a)


def prolong_numpy(level_array, H, level):
    a = level_array
    for l in range(level + 1, H.l_target + 1):
        a = prolong_step(a, H, l)
    return np.ascontiguousarray(a)


# ---- tests ----------------------------------------------------------------------------------------
def test_library_exports_the_new_entries():
    import mgard_amd
    L = mgard_amd.load_library()
    for sym in ("mgh_prolong", "mgh_decompress_preview", "mgh_progressive_preview"):
        assert hasattr(L, sym), sym


def test_headers_declare_the_new_entries():
    import re

    def text(name):
        txt = open(os.path.join(ROOT, "include", name)).read()
        return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    assert ("int mgh_prolong(mgh_hierarchy *h, int level, const void *d_level, void *d_out, void *stream);"
            in text("mgard_hip.h"))
    hl = text("mgard_hip_compress.h")
    assert ("int mgh_decompress_preview(const void *compressed_data, size_t compressed_size, int halvings, "
            "void **decompressed_data, const mgh_config *config, int output_pre_allocated);") in hl
    assert "int mgh_progressive_preview(mgh_progressive *p, void **data, int output_pre_allocated);" in hl


def _check_contract(cls, name, dt, which):
    shape, _, opts, _, _ = CASES_3D[name]
    kw = hierarchy_kw(shape, dt, opts, cls)
    H = cls(shape, dt, **kw)
    O = oracle.Hierarchy(shape, dt, **kw)  # (the ratios; the same tables by tests/test_oracle_vs_reference.py)
    assert O.l_target == H.l_target
    if opts.get("max_level"):
        assert H.l_target == cls(shape, dt).l_target - 1
    c = coefficients(O, shape, dt, which)
    for level in range(H.l_target + 1):
        want = H.recompose(zeroed(O, c, level))
        got = prolong_numpy(level_of(want, O, level), O, level)
        assert_same_bits(got, want, "%s %s %s level %d of %d (%s)" % (cls.__module__, name, np.dtype(dt).name, level,
                                                                     H.l_target, which))


@pytest.mark.parametrize("which", FIELDS)
@pytest.mark.parametrize("name", list(CASES_3D))
def test_level_steps_are_the_oracles_recomposition(name, which):
    for dt in CASES_3D[name][1]:
        _check_contract(oracle.Hierarchy, name, dt, which)


@pytest.mark.skipif(not ref.available(), reason="%s is not built (oracle.build_ref())" % ref.LIB_PATH)
@pytest.mark.parametrize("which", FIELDS)
@pytest.mark.parametrize("name", list(CASES_3D))
def test_level_steps_are_the_references_recomposition(name, which):
    for dt in CASES_3D[name][1]:
        _check_contract(ref.Hierarchy, name, dt, which)


def test_minus_zero_at_a_coarse_node():
    """The one place where a copy is not the recomposition, written down: a -0.0 of the level array. An
    interpolant of -0.0 values is +0.0 on both sides (lerp_ref, and the kept addition). A coarse node is copied by
    the level step, while the recomposition subtracts a zero correction from it, and that zero is -0.0 away from
    the corners of the level: there the recomposition gives +0.0 where the level step keeps -0.0. Nothing but the
    sign of such a zero differs (5 x 5 x 5, every node of level l_target - 1 set to -0.0: 19 of the 27 coarse nodes)."""
    O = oracle.Hierarchy((5, 5, 5), np.float32)
    lvl = np.full(O.level_shape(O.l_target - 1), np.float32(-0.0))
    got = prolong_numpy(lvl, O, O.l_target - 1)
    neg = np.signbit(got)
    assert neg[::2, ::2, ::2].all() and neg.sum() == 27
    z = np.zeros((5, 5, 5), np.float32)
    z[:3, :3, :3] = lvl
    want = O.recompose(z)
    assert np.array_equal(got, want) and not want.any()
    differ = bits(got) != bits(want)
    print("coarse nodes whose zero changes sign in the recomposition: %d of 27" % differ.sum())
    assert not differ[~neg].any()
    corners = np.ix_([0, 4], [0, 4], [0, 4])
    assert np.signbit(want[corners]).all()
