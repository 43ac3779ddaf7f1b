"""mgh_compare on the GPU (mgard_amd.compare): the one-pass error statistics of two arrays against the
NumPy restatement of the reference's ErrorCalculator.h in tests/compare_ref.py (difference and fabs in T,
:57-64; squares summed in double, :41-45 and :101-105 -- there with math.fsum).

Exact, as bit patterns: n, nonfinite, max_abs_err, argmax, ref_min, ref_max, ref_abs_max. The two sums differ
from the correctly rounded sum by at most n 2^-52 relative (compare_ref.sum_tolerance: the worst case of
adding n non-negative doubles in any order), and two calls on the same inputs give the same bits.
Shapes: one element up to five dimensions; (257, 129, 65) takes 1053 slabs of 2048 elements (f32) or 1403 of 1536
(f64), and its last slab ends in a tail that is no whole vector."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.compare_ref import EXACT, assert_stats, bits, ref_stats

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (3,), (1025,), (70, 45), (33, 17, 65), (9, 17, 17, 17), (4, 3, 10, 5, 9), (257, 129, 65)]
DTYPES = [np.float32, np.float64]
BIG = (257, 129, 65)


def _pair(shape, dt, seed=0):
    rng = np.random.default_rng(seed + int(np.prod(shape)))
    a = rng.standard_normal(shape).astype(dt)
    b = (a + (rng.standard_normal(shape) * 1e-3).astype(dt)).astype(dt)
    return a, b


_cache = {}


def pair(shape, dt):
    """(a, b, NumPy statistics): computed once per shape and type, never modified."""
    key = (shape, np.dtype(dt).name)
    if key not in _cache:
        a, b = _pair(shape, dt)
        a.setflags(write=False)
        b.setflags(write=False)
        _cache[key] = (a, b, ref_stats(a, b))
    return _cache[key]


def dev(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()  # (a copy: the shared arrays are read-only)


def as_dict(s):
    return {k: getattr(s, k) for k, _ in s._fields_}


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_compare_matches_numpy_and_is_reproducible(shape, dt):
    import mgard_amd as mg
    a, b, want = pair(shape, dt)
    da, db = dev(a), dev(b)
    got = mg.compare(da, db)
    print(shape, np.dtype(dt).name, got)
    assert_stats(got, want)
    again = mg.compare(da, db)
    assert bytes(again) == bytes(got), "two calls on the same inputs differ"
    assert got.mse == got.sum_sq_err / got.n
    if got.ref_max > got.ref_min:
        assert got.psnr == pytest.approx(20 * math.log10((got.ref_max - got.ref_min) / math.sqrt(got.mse)), rel=1e-12)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("which", ["both", "b-only"])
def test_arrays_that_start_off_a_16_byte_boundary(which, dt):
    """Slices that begin one element behind a 16-byte boundary: both arrays (the head of every slab is
    scalar, b is aligned with a), or b alone (the body reads b with its own alignment)."""
    import torch
    import mgard_amd as mg
    a, b, want = pair(BIG, dt)
    n = a.size

    def shifted(x):
        buf = torch.empty(n + 1, dtype=torch.float32 if dt == np.float32 else torch.float64, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[1:] = dev(x.reshape(-1))
        return buf[1:].view(BIG)

    da = shifted(a) if which == "both" else dev(a)
    db = shifted(b)
    assert db.data_ptr() % 16 == a.itemsize and db.is_contiguous() and da.data_ptr() % 16 == (a.itemsize if which == "both" else 0)
    got = mg.compare(da, db)
    assert_stats(got, want)
    # the slabs are those of the aligned call, only the split into head, body and tail moves: exact fields equal
    ref = mg.compare(dev(a), dev(b))
    for k in EXACT:
        assert bits(getattr(got, k)) == bits(getattr(ref, k)), k


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_tie_between_the_first_and_the_last_slab_takes_the_lower_index(dt):
    import mgard_amd as mg
    a, b, _ = pair(BIG, dt)
    a, b = a.copy(), b.copy()
    a.reshape(-1)[0] = a.reshape(-1)[-1] = dt(1)
    b.reshape(-1)[0] = b.reshape(-1)[-1] = dt(-7)
    got = mg.compare(dev(a), dev(b))
    assert got.argmax == 0 and got.max_abs_err == 8.0
    assert_stats(got, ref_stats(a, b))
    # ... and alone at the end it is found there
    b.reshape(-1)[0] = a.reshape(-1)[0]
    got = mg.compare(dev(a), dev(b))
    assert got.argmax == a.size - 1 and got.max_abs_err == 8.0


def _padded(x, pads):
    """A cuda tensor equal to x that is a slice of a larger allocation: dimension d padded by pads[d]."""
    import torch
    src = dev(x)
    big = torch.full([e + p for e, p in zip(x.shape, pads)], float("nan"), dtype=src.dtype, device="cuda")
    view = big[tuple(slice(0, e) for e in x.shape)]
    view.copy_(src)
    return view


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(33, 17, 65), (257, 129, 65), (9, 17, 17, 17), (70, 45)], ids=lambda s: "x".join(map(str, s)))
def test_pitched_arrays_equal_their_dense_copies(shape, dt):
    """The NaN padding is never read; exact fields equal the dense call's bit for bit, sums within the tolerance."""
    import mgard_amd as mg
    a, b, want = pair(shape, dt)
    D = len(shape)
    last, last2 = [0] * (D - 1) + [3], [0] * (D - 1) + [7]
    middle = [0] * D
    middle[D - 2] = 2  # (D = 2: the slowest dimension, which is no padding at all -- a longer allocation)
    both_mid = list(middle)
    both_mid[-1] = 5
    cases = {"a-last": (_padded(a, last), dev(b)), "b-last": (dev(a), _padded(b, last)),
             "both-different": (_padded(a, last), _padded(b, last2)), "middle": (_padded(a, middle), _padded(b, both_mid))}
    dense = mg.compare(dev(a), dev(b))
    for name, (x, y) in cases.items():
        assert name == "middle" and D == 2 or not (x.is_contiguous() and y.is_contiguous())
        got = mg.compare(x, y)
        assert_stats(got, want, what=name)
        assert got.nonfinite == 0
        for k in EXACT:
            assert bits(getattr(got, k)) == bits(getattr(dense, k)), (name, k)
        assert bytes(mg.compare(x, y)) == bytes(got)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_nonfinite_positions_are_counted_and_left_out(dt):
    import mgard_amd as mg
    a, b, _ = pair(BIG, dt)
    a, b = a.copy(), b.copy()
    fa, fb = a.reshape(-1), b.reshape(-1)
    fa[12345] = np.nan
    fb[a.size - 2] = np.inf
    fa[700000] = fb[700000] = np.inf
    got = mg.compare(dev(a), dev(b))
    want = ref_stats(a, b)
    assert want["nonfinite"] == 3 == got.nonfinite
    assert_stats(got, want)
    # a slab of nothing else, and an array of nothing else
    fa[:5000] = np.nan
    assert_stats(mg.compare(dev(a), dev(b)), ref_stats(a, b))
    none = mg.compare(dev(np.full(100, np.nan, dt)), dev(np.zeros(100, dt)))
    assert as_dict(none) == dict(n=100, nonfinite=100, max_abs_err=0.0, argmax=0, sum_sq_err=0.0, ref_min=0.0,
                                 ref_max=0.0, ref_abs_max=0.0, ref_sum_sq=0.0)
    assert none.mse == 0 and none.psnr == math.inf


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_an_array_against_itself_and_signed_zeros(dt):
    import mgard_amd as mg
    a, _, _ = pair((33, 17, 65), dt)
    da = dev(a)
    got = mg.compare(da, da)
    assert got.max_abs_err == 0 and got.sum_sq_err == 0 and got.argmax == 0 and got.nonfinite == 0
    assert got.mse == 0 and got.rmse == 0 and got.psnr == math.inf
    assert_stats(got, ref_stats(a, a))
    z = mg.compare(dev(np.full(1000, -0.0, dt)), dev(np.zeros(1000, dt)))
    assert z.max_abs_err == 0 and z.sum_sq_err == 0 and z.nonfinite == 0 and z.argmax == 0
    assert bits(z.ref_abs_max) == bits(0.0)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_host_arrays_are_staged(dt):
    import mgard_amd as mg
    a, b, want = pair(BIG, dt)
    device = mg.compare(dev(a), dev(b))
    for x, y in ((a, b), (a, dev(b)), (dev(a), b)):
        got = mg.compare(x, y)
        assert_stats(got, want)
        for k in EXACT:
            assert bits(getattr(got, k)) == bits(getattr(device, k)), k


def test_host_arrays_longer_than_one_staging_slab():
    """72 MB of f64 per array: two slabs of the 64 MB staging loop, folded with a non-zero index offset; the
    largest error sits in the second slab, a non-finite position in each. In the mixed calls the
    device-resident side is read at the slab's offset. Staging changes the order of the sums: they are held to
    the tolerance, the exact fields to the device call's bits."""
    import mgard_amd as mg
    n = 9_000_001
    assert n * 8 > 64 << 20
    rng = np.random.default_rng(9)
    a = rng.standard_normal(n)
    b = a + rng.standard_normal(n) * 1e-3
    a[n - 5], b[n - 5] = 1.0, -7.0
    a[17] = np.nan
    b[n - 100] = np.inf
    want = ref_stats(a, b)
    assert want["argmax"] == n - 5 > (64 << 20) // 8 and want["nonfinite"] == 2
    da, db = dev(a), dev(b)
    device = mg.compare(da, db)
    assert_stats(device, want)
    for x, y in ((a, b), (a, db), (da, b)):
        got = mg.compare(x, y)
        assert_stats(got, want)
        for k in EXACT:
            assert bits(getattr(got, k)) == bits(getattr(device, k)), k


def test_release_cache_frees_the_idle_scratch_and_the_next_call_allocates_again():
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    a, b, want = pair((33, 17, 65), np.float32)
    da, db = dev(a), dev(b)
    first = mg.compare(da, db)
    hl.release_cache()
    hl.release_cache()  # (nothing left: harmless)
    assert bytes(mg.compare(da, db)) == bytes(first)
    assert_stats(first, want)


def test_bad_arguments_are_refused_and_the_library_stays_usable():
    import torch
    import mgard_amd as mg
    L = mg.load_library()
    a, b, want = pair((33, 17, 65), np.float32)
    da, db = dev(a), dev(b)
    shape = (C.c_uint64 * 3)(33, 17, 65)
    out = mg.ErrorStats()
    pa, pb, po = C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()), C.byref(out)
    short = (C.c_uint64 * 3)(33, 17, 64)
    wide = (C.c_uint64 * 3)(33, 17, 80)

    def call(D=3, dtype=mg.FLOAT, shp=shape, a_=pa, lda=None, b_=pb, ldb=None, o=po, device=0):
        return L.mgh_compare(D, dtype, shp, a_, lda, b_, ldb, o, device, None)

    bad = {"D = 0": dict(D=0), "D = 6": dict(D=6), "dtype": dict(dtype=7), "shape": dict(shp=None), "a": dict(a_=None),
           "b": dict(b_=None), "out": dict(o=None), "ld_a": dict(lda=short), "ld_b": dict(ldb=short),
           "device": dict(device=1000),
           # a pitched array next to a host array
           "pitched host": dict(a_=C.c_void_p(a.ctypes.data), lda=wide)}
    for name, kw in bad.items():
        assert call(**kw) == -1, name  # MGH_ERR_INVALID_ARGUMENT
        assert L.mgh_last_error(), name
        assert call() == 0, "after " + name
        assert_stats(out, want)
    torch.cuda.synchronize()
