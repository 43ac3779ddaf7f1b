"""mgh_compare_masked_ (k_compare_masked) against tests/mask_view_model.masked_stats.

Exact fields (n, nonfinite, max_abs_err, argmax, ref_min, ref_max, ref_abs_max) bit for bit. The two sums are sums of
at most 4 * 10^4 non-negative doubles in another order than NumPy's: they are held to a relative 1e-12 of the model's
float64 sum (worst case n * 2^-53 = 4e-12, far less in practice: the observed value is printed)."""
import numpy as np
import pytest

from tests import mask_model as mm
from tests import mask_view_model as mv
from tests.util import inside_field

CASES = [((34, 33, 32), np.float32), ((17, 130), np.float64)]
IDS = ["34x33x32-f32", "17x130-f64"]
SUM_RTOL = 1e-12


def _pair(shape, dtype):
    a = inside_field(shape, dtype)
    rng = np.random.default_rng(7)
    b = (a + rng.normal(0, 1e-3, shape)).astype(dtype)
    return a, b


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _words(mask):
    return _cuda(mm.packed_words(mask).view(np.int64))


def _bits(x):
    return np.float64(x).view(np.uint64)


def _assert_exact(got, want, what):
    for f in mv.EXACT_FIELDS:
        g, w = getattr(got, f), want[f]
        assert (g == w) if isinstance(w, int) else (_bits(g) == _bits(w)), (what, f, g, w)


def _assert_model(got, want, what):
    _assert_exact(got, want, what)
    for f in mv.SUM_FIELDS:
        g, w = getattr(got, f), want[f]
        rel = abs(g - w) / w if w else abs(g)
        print("%s %s: relative difference to the model's sum %.3e" % (what, f, rel))
        assert rel <= SUM_RTOL, (what, f, g, w)


def _assert_same(got, other, what):
    for f, _ in type(got)._fields_:
        g, w = getattr(got, f), getattr(other, f)
        assert (g == w) if isinstance(g, int) else (_bits(g) == _bits(w)), (what, f, g, w)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dtype", CASES, ids=IDS)
def test_against_the_model(shape, dtype):
    import mgard_amd
    a, b = _pair(shape, dtype)
    mask = np.random.default_rng(len(shape)).random(shape) < 0.3
    b.reshape(-1)[np.flatnonzero(~mask.reshape(-1))[5]] = np.nan        # an unmasked position that is not finite
    got = mgard_amd.compare_masked(_cuda(a), _cuda(b), _words(mask))
    want = mv.masked_stats(a, b, mask)
    assert want["nonfinite"] == 1 and want["n"] == a.size - int(mask.sum())
    _assert_model(got, want, "random mask")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dtype", CASES, ids=IDS)
def test_masked_positions_take_part_in_nothing(shape, dtype):
    """NaN and 1e20 in `a` at the masked positions: nonfinite stays 0 and ref_max the valid maximum."""
    import mgard_amd
    a, b = _pair(shape, dtype)
    mask = np.random.default_rng(5).random(shape) < 0.3
    marked = a.copy()
    idx = np.flatnonzero(mask.reshape(-1))
    marked.reshape(-1)[idx] = np.array([np.nan, 1e20], dtype=dtype)[np.arange(idx.size) % 2]
    got = mgard_amd.compare_masked(_cuda(marked), _cuda(b), _words(mask))
    assert got.nonfinite == 0 and got.n == a.size - idx.size
    assert _bits(got.ref_max) == _bits(float(a[~mask].max()))
    _assert_model(got, mv.masked_stats(marked, b, mask), "marks under the mask")
    # the largest error sits under the mask: it must not be seen
    worst = b.copy()
    worst.reshape(-1)[idx[0]] += dtype(50.0)
    got2 = mgard_amd.compare_masked(_cuda(marked), _cuda(worst), _words(mask))
    _assert_same(got2, got, "an error under the mask")


@pytest.mark.gpu
def test_box_of_a_larger_array_against_the_full_mask():
    """(10, 33, 20) at (7, 0, 5) of (34, 33, 32) through ld_a, ld_m and bit0 equals the dense call on cropped copies,
    sums bit for bit (the same kernel, the same slabs, the same order)."""
    import mgard_amd
    shape, dtype = CASES[0]
    a, b = _pair(shape, dtype)
    mask = np.random.default_rng(9).random(shape) < 0.3
    lo, ext = (7, 0, 5), (10, 33, 20)
    box = tuple(slice(l, l + e) for l, e in zip(lo, ext))
    bit0 = int(np.ravel_multi_index(lo, shape))
    ta, tb = _cuda(a), _cuda(b)
    got = mgard_amd.compare_masked(ta[box], tb[box], _words(mask), ld_m=shape, bit0=bit0)
    dense = mgard_amd.compare_masked(_cuda(a[box]), _cuda(b[box]), _words(mask[box]))
    _assert_same(got, dense, "box")
    _assert_model(got, mv.masked_stats(a[box], b[box], mask[box]), "box")
    assert 0 < got.n < int(np.prod(ext))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dtype", CASES, ids=IDS)
def test_all_zero_mask_is_compare_on_pitched_views(shape, dtype):
    """mgh_compare with leading dimensions runs the same kernel family: all fields bit for bit."""
    import torch
    import mgard_amd
    a, b = _pair(shape, dtype)
    pitched = tuple(shape[:-1]) + (shape[-1] + 3,)
    pa = torch.zeros(pitched, dtype=_cuda(a).dtype, device="cuda")
    pb = torch.zeros_like(pa)
    va, vb = pa[..., :shape[-1]], pb[..., :shape[-1]]
    va.copy_(_cuda(a))
    vb.copy_(_cuda(b))
    zero = _words(np.zeros(shape, dtype=bool))
    got = mgard_amd.compare_masked(va, vb, zero)
    _assert_same(got, mgard_amd.compare(va, vb), "all-zero mask, pitched")
    # dense arrays: mgh_compare takes its 16-byte kernel there, so only the exact fields are its
    dense = mgard_amd.compare_masked(_cuda(a), _cuda(b), zero)
    plain = mgard_amd.compare(_cuda(a), _cuda(b))
    for f in mv.EXACT_FIELDS:
        g, w = getattr(dense, f), getattr(plain, f)
        assert (g == w) if isinstance(g, int) else (_bits(g) == _bits(w)), f
    _assert_same(dense, got, "dense and pitched")
    assert got.n == a.size


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dtype", CASES, ids=IDS)
def test_fully_masked_array(shape, dtype):
    import mgard_amd
    a, b = _pair(shape, dtype)
    got = mgard_amd.compare_masked(_cuda(a), _cuda(b), _words(np.ones(shape, dtype=bool)))
    for f, _ in type(got)._fields_:
        assert getattr(got, f) == 0, f


@pytest.mark.gpu
def test_refusals():
    import mgard_amd
    shape, dtype = CASES[1]
    a, b = _pair(shape, dtype)
    w = _words(np.zeros(shape, dtype=bool))
    with pytest.raises(ValueError):                                    # the view leaves the words
        mgard_amd.compare_masked(_cuda(a), _cuda(b), w, bit0=64)
    with pytest.raises(ValueError):                                    # host arrays are the caller's to stage
        mgard_amd.compare_masked(a, b, w)
    L = mgard_amd.load_library()
    import ctypes as C
    out = mgard_amd.ErrorStats()
    shp = (C.c_uint64 * 2)(*shape)
    rc = L.mgh_compare_masked_(2, mgard_amd.DOUBLE, shp, C.c_void_p(a.ctypes.data), None, C.c_void_p(_cuda(b).data_ptr()), None,
                              C.c_void_p(w.data_ptr()), None, 0, C.byref(out), 0, None)
    assert rc == -1 and b"device pointers" in L.mgh_last_error()
