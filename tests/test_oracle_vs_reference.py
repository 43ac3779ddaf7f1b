"""The CPU oracle against a build of the reference itself, bit for bit.

oracle/_ref/libmgx_ref.so is the reference MGARD-X's own SERIAL code path (Hierarchy,
DataRefactor::Decompose/Recompose, LinearQuantizer::Quantize/Dequantize, norm_calculator) behind
the C ABI of oracle/ref_driver.cpp, built by oracle.build_ref() from a reference checkout. These
tests pin what the reference's test vectors do not reach: non-dyadic shapes in 1-5 D (the ghost-node
rule on every class of extent), the level-dependent quantizers (s != inf, the level volumes),
normalize_coordinates = False, non-uniform spacing on non-dyadic grids, and max_level.

Floats compare through their bit patterns, integers exactly, outliers as sorted (index, value) sets.
The L2 norm is not bit-reproducible (sequential vs tree sum): both sides are held
to a float64 math.fsum evaluation instead.
"""
import math

import numpy as np
import pytest

import oracle
from oracle import ref
from tests.util import nonuniform_coords, smooth_field

pytestmark = pytest.mark.skipif(not ref.available(),
                                reason="%s is not built (oracle.build_ref())" % ref.LIB_PATH)

DTYPES = [np.float32, np.float64]

# Every class of extent in 1-5 D: odd and even, 3 and 4, 2^k, 2^k+1, 2^k+2, primes, one extent far
# longer than the others, and the shapes the kernels special-case.
SHAPES = [
    (3,), (4,), (5,), (16,), (31,), (64,), (65,), (66,), (127,), (300001,),
    (3, 4), (4, 3), (16, 17), (18, 33), (13, 7), (66, 64), (257, 5), (3, 130),
    (3, 3, 3), (4, 4, 4), (5, 6, 7), (9, 16, 17), (18, 10, 11), (13, 11, 7), (3, 4, 200),
    (40, 130, 9), (70, 300, 5), (5000, 5, 7), (3000, 17, 17),
    (3, 4, 3, 4), (5, 6, 7, 8), (9, 8, 10, 17), (4, 4, 4, 66), (11, 13, 3, 5),
    (8, 66, 70, 129), (20, 40, 40, 40),
    (3, 3, 3, 3, 3), (4, 4, 4, 4, 4), (9, 5, 3, 17, 4), (3, 3, 4, 5, 33), (6, 7, 5, 3, 10),
    (4, 3, 70, 5, 131),
]
# the full option matrices run on the shapes that stay small
SMALL = [s for s in SHAPES if np.prod(s) <= 40000]
SVALS = [np.inf, 0.0, 1.0, -1.0, 0.5]
DICTS = [64, 8192, 1001]
TOL_OUTLIERS, TOL_ZERO = 1e-6, 1e5


def _id(shape):
    return "x".join(map(str, shape))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_bit_equal(got, want, what=""):
    gb, wb = _bits(got), _bits(want)
    assert gb.shape == wb.shape, (what, gb.shape, wb.shape)
    if not np.array_equal(gb, wb):
        bad = np.argwhere(gb != wb)
        i = tuple(bad[0])
        raise AssertionError("%s: %d/%d elements differ; first at %s: oracle %r reference %r" % (
            what, len(bad), gb.size, i, got[i], want[i]))


def _outliers(idx, val):
    order = np.argsort(idx, kind="stable")
    return list(zip(np.asarray(idx)[order].tolist(), np.asarray(val)[order].tolist()))


def _pair(shape, dt, coords=None, normalize=True, max_level=None):
    kw = dict(coords=coords, normalize_coordinates=normalize)
    o = oracle.Hierarchy(shape, dt, max_level=2**62 if max_level is None else max_level, **kw)
    r = ref.Hierarchy(shape, dt, max_level=2**64 - 1 if max_level is None else max_level, **kw)
    assert o.l_target == r.l_target, (o.l_target, r.l_target)
    for l in range(r.l_target + 1):
        assert o.level_shape(l) == r.level_shape(l), l
    return o, r


def _field(shape, dt):
    return smooth_field(shape, dt, seed=int(np.prod(shape)) % 100003, noise=1e-2)


def _check_decompose(o, r, u, what):
    co, cr = o.decompose(u), r.decompose(u)
    assert_bit_equal(co, cr, what + " decompose")
    assert_bit_equal(o.recompose(cr), r.recompose(cr), what + " recompose")
    return cr


def _check_quantize(o, r, c, dt, ebtype, tol, s, norm, dict_size, prep, what):
    args = (ebtype, dt(tol), dt(s), dt(norm), dict_size, prep)
    qo, oio, ovo, no = o.quantize(c, *args)
    qr, oir, ovr, nr = r.quantize(c, *args)
    assert no == nr, (what, no, nr)
    assert np.array_equal(qo, qr), what + ": quantized values differ at %d places" % int(
        np.sum(qo != qr))
    assert _outliers(oio, ovo) == _outliers(oir, ovr), what + ": outliers differ"
    assert_bit_equal(o.dequantize(qr, *args, outlier_idx=oir, outlier_val=ovr),
                     r.dequantize(qr, *args, outlier_idx=oir, outlier_val=ovr), what + " dequantize")
    return qr, nr


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_decompose_recompose_and_quantizer(shape, dt):
    """Default hierarchy (uniform, normalized coordinates): level shapes, decomposition, the
    recomposition of the reference's coefficients, and quantize/dequantize at s = inf and s = 0."""
    o, r = _pair(shape, dt)
    u = _field(shape, dt)
    c = _check_decompose(o, r, u, "default")
    norm = ref.norm(u, np.inf)
    for s in (np.inf, 0.0):
        _check_quantize(o, r, c, dt, oracle.REL, 1e-3, s, norm, 8192, True, "REL s=%g" % s)


def _hierarchy_variants(shape, dt):
    """(label, kwargs of _pair) over coordinates x normalize_coordinates x max_level."""
    l_target = ref.Hierarchy(shape, dt).l_target
    levels = sorted({None, 0, min(1, l_target), max(l_target - 1, 0)}, key=lambda x: -1 if x is None else x)
    out = []
    for nonuni in (False, True):
        coords = nonuniform_coords(shape, dt, seed=sum(shape)) if nonuni else None
        for normalize in (True, False):
            for ml in levels:
                out.append(("%s norm=%d max_level=%s" % ("nonuniform" if nonuni else "uniform",
                                                         normalize, ml),
                            dict(coords=coords, normalize=normalize, max_level=ml)))
    return out


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [s for s in SHAPES if np.prod(s) <= 300000], ids=_id)
def test_decompose_variants(shape, dt):
    """Uniform and non-uniform coordinates x normalize_coordinates x max_level in {none, 0, 1,
    l_target - 1}: hierarchy, decomposition and recomposition."""
    u = _field(shape, dt)
    for label, kw in _hierarchy_variants(shape, dt):
        o, r = _pair(shape, dt, **kw)
        _check_decompose(o, r, u, label)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", SMALL, ids=_id)
def test_quantizer_matrix(shape, dt):
    """REL/ABS x s in {inf, 0, 1, -1, 0.5} x dict_size in {64, 8192, 1001} x prep_huffman x a
    tolerance with outliers and one that quantizes everything to zero, on the default hierarchy and
    on ones whose level volumes differ (non-uniform coordinates, normalize_coordinates = False,
    max_level = 1). The norm is injected."""
    u = _field(shape, dt)
    variants = [("default", {}), ("normalize=0", dict(normalize=False)),
                ("nonuniform", dict(coords=nonuniform_coords(shape, dt, seed=3))),
                ("max_level=1", dict(max_level=1))]
    saw_outliers = False
    for label, kw in variants:
        o, r = _pair(shape, dt, **kw)
        c = r.decompose(u)
        for s in SVALS:
            norm = ref.norm(u, s, kw.get("normalize", True))
            for ebtype in (oracle.REL, oracle.ABS):
                for dict_size in DICTS:
                    for prep in (True, False):
                        what = "%s eb=%d s=%g dict=%d prep=%d" % (label, ebtype, s, dict_size, prep)
                        _, n = _check_quantize(o, r, c, dt, ebtype, TOL_OUTLIERS, s, norm,
                                               dict_size, prep, what + " tol=small")
                        saw_outliers |= n > 0
                        q, n = _check_quantize(o, r, c, dt, ebtype, TOL_ZERO, s, norm, dict_size,
                                               prep, what + " tol=large")
                        assert n == 0 and np.all(q == (dict_size // 2 if prep else 0)), what
    assert saw_outliers


def _random_cases(n_cases, seed):
    rng = np.random.default_rng(seed)
    cases = []
    budget = {1: 5000, 2: 40000, 3: 150000, 4: 150000, 5: 120000}
    while len(cases) < n_cases:
        D = int(rng.integers(1, 6))
        lo, hi = 3, {1: 3000, 2: 220, 3: 70, 4: 22, 5: 12}[D]
        shape = tuple(int(x) for x in rng.integers(lo, hi + 1, size=D))
        if np.prod(shape) > budget[D]:
            continue
        cases.append((shape, bool(rng.integers(0, 2)), bool(rng.integers(0, 2)),
                      bool(rng.integers(0, 2)), int(rng.integers(-1, 3)),
                      SVALS[int(rng.integers(0, len(SVALS)))], int(rng.integers(0, 2)),
                      DICTS[int(rng.integers(0, len(DICTS)))], bool(rng.integers(0, 2))))
    return cases


@pytest.mark.parametrize("case", _random_cases(40, 20261016), ids=lambda c: _id(c[0]))
def test_random_shapes(case):
    """Seeded draw of ragged 1-5-D shapes with random options: decompose, recompose, quantize,
    dequantize."""
    shape, f64, nonuni, normalize, ml, s, ebtype, dict_size, prep = case
    dt = np.float64 if f64 else np.float32
    coords = nonuniform_coords(shape, dt, seed=sum(shape)) if nonuni else None
    o, r = _pair(shape, dt, coords=coords, normalize=normalize, max_level=None if ml < 0 else ml)
    u = _field(shape, dt)
    c = _check_decompose(o, r, u, "random")
    norm = ref.norm(u, s, normalize)
    _check_quantize(o, r, c, dt, ebtype, 1e-4, s, norm, dict_size, prep, "random")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [(3,), (1000,), (17, 18), (5, 6, 7), (9, 8, 10, 17),
                                   (4, 3, 70, 5, 131), (40, 130, 9)], ids=_id)
def test_norm(shape, dt):
    """L-inf bit for bit; L2 (s != inf) from both sides within n * eps(T) of float64 math.fsum."""
    u = _field(shape, dt) - dt(0.25)
    assert _bits(np.array(ref.norm(u, np.inf), dt)) == _bits(np.array(oracle.norm(u, np.inf), dt))
    n = u.size
    eps = float(np.finfo(dt).eps)
    for normalize in (True, False):
        ss = math.fsum(float(x) * float(x) for x in u.reshape(-1).astype(np.float64))
        want = math.sqrt(ss / n) if normalize else math.sqrt(ss)
        for s in (0.0, 1.0):
            for who, got in (("reference", ref.norm(u, s, normalize)),
                             ("oracle", oracle.norm(u, s, normalize))):
                assert abs(got - want) <= n * eps * want, (who, normalize, got, want)
