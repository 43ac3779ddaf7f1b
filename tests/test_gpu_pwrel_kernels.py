"""The three streaming passes of the pointwise relative bound (mgard_amd.pwrel_forward / pwrel_inverse / compare_pwrel)
against tests/pwrel_model.py: bitmaps and counts to the bit, y within one ulp of T (the device log2 of a double is
within 1 ulp of a double, plus one rounding to T), the inverse within 2 eps_T of |x| on the exact y and clamped at the
ends of the range, and the compare against float64 NumPy."""
import numpy as np
import pytest

from tests import mask_model as mm
from tests import pwrel_model as pm

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (63,), (64,), (65,), (1000,), (4097,), (5, 7, 13)]
DTYPES = [np.float32, np.float64]


def _floor(dtype):
    return float(dtype(1e-20))      # (a value of T: "exactly at the floor" exists in both types)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ulps(a, b):
    """distance of two arrays of T in units in the last place (same sign assumed or zero)"""
    ia, ib = mm.int_view(a).astype(np.int64), mm.int_view(b).astype(np.int64)
    lo = np.iinfo(np.int32 if a.dtype == np.float32 else np.int64).min
    ia, ib = np.where(ia < 0, lo - ia, ia), np.where(ib < 0, lo - ib, ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_forward(shape, dtype):
    import mgard_amd
    fl = _floor(dtype)
    x = pm.decades_field(shape, dtype, seed=len(shape) + shape[0], abs_floor=fl)
    n = x.size
    y, mw, fw, st = mgard_amd.pwrel_forward(_dev(x), fl)
    y = y.cpu().numpy()
    mask, flag = pm.bitmaps(x, fl)
    # bitmaps to the bit, the zero high bits of the last word included, and the counts
    assert np.array_equal(mw.cpu().numpy().view(np.uint64), mm.packed_words(mask))
    assert np.array_equal(fw.cpu().numpy().view(np.uint64), mm.packed_words(flag))
    cls = pm.classify(x, fl)
    assert (st.n, st.n_masked, st.n_nonfinite, st.n_flag) == (n, int(mask.sum()), int((cls == pm.NONFINITE).sum()), int(flag.sum()))
    # y within one ulp of T(log2(float64(|x|)))
    want = pm.forward(x, fl)
    valid = ~mask
    if valid.any():
        assert _ulps(y[valid], want[valid]).max() <= 1
        assert (st.ymin, st.ymax) == (float(y[valid].min()), float(y[valid].max()))
    else:
        assert (st.ymin, st.ymax) == (0.0, 0.0)
    # in place gives the same bits
    xi = _dev(x)
    y2, mw2, fw2, _ = mgard_amd.pwrel_forward(xi, fl, out=xi)
    assert y2.data_ptr() == xi.data_ptr()
    assert np.array_equal(mm.int_view(y2.cpu().numpy())[valid], mm.int_view(y)[valid])
    assert np.array_equal(mw2.cpu().numpy(), mw.cpu().numpy()) and np.array_equal(fw2.cpu().numpy(), fw.cpu().numpy())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_inverse(shape, dtype):
    import mgard_amd
    fl = _floor(dtype)
    x = pm.decades_field(shape, dtype, seed=7 + shape[0], abs_floor=fl)
    y, mw, fw, _ = mgard_amd.pwrel_forward(_dev(x), fl)
    out = mgard_amd.pwrel_inverse(y.clone(), mw, fw).cpu().numpy()
    mask, flag = pm.bitmaps(x, fl)
    valid = ~mask
    # the masked / flag rules to the bit: quiet NaN, +0.0
    assert np.isnan(out[mask & flag]).all()
    assert np.all(mm.int_view(out)[mask & ~flag] == 0)
    # signs exact, nothing infinite or denormal
    assert np.array_equal(np.signbit(out[valid]), np.signbit(x[valid]))
    xa, oa = np.abs(x[valid].astype(np.float64)), np.abs(out[valid].astype(np.float64))
    fi = np.finfo(dtype)
    if valid.any():
        assert oa.min() >= float(fi.tiny) and oa.max() <= float(fi.max)
        # the pass itself: within 2 eps_T of 2^y for the y it was given (1 ulp of the device exp2 plus one rounding),
        # clamped like the kernel's
        yv = y.cpu().numpy()[valid].astype(np.float64)
        with np.errstate(over="ignore"):
            exact = np.clip(np.exp2(yv), float(fi.tiny), float(fi.max))
        assert np.max(np.abs(oa - exact) / exact) <= 2 * float(fi.eps)
        # ... and against |x|: y in T is log2|x| within E1 = ulp_T(max |y|), so the ratio lies within 2^E1 (1 + E2)
        e1 = pm.ulp(dtype, float(np.max(np.abs(yv))))
        assert np.max(np.abs(oa - xa) / xa) <= 2.0 ** e1 * (1 + pm.e2(dtype)) - 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_inverse_of_an_exact_y_is_within_two_eps(dtype):
    """Powers of two are the elements whose y = log2|x| is exact in T: they come back within 2 eps_T of |x| (in fact
    exactly), across the whole normal range and with both signs. For any other element y in T is itself rounded, by
    up to ulp_T(y) / 2, which alone moves 2^y by more than 2 eps_T once |y| > 2: test_inverse bounds those."""
    import mgard_amd
    fi = np.finfo(dtype)
    k = np.arange(fi.minexp, fi.maxexp, dtype=np.float64)
    x = (np.exp2(k) * np.where(k.astype(np.int64) % 3 == 0, -1.0, 1.0)).astype(dtype)
    y, mw, fw, st = mgard_amd.pwrel_forward(_dev(x), 0.0)
    assert st.n_masked == 0 and np.array_equal(y.cpu().numpy().astype(np.float64), k)
    out = mgard_amd.pwrel_inverse(y, mw, fw).cpu().numpy()
    xa, oa = np.abs(x.astype(np.float64)), np.abs(out.astype(np.float64))
    assert np.max(np.abs(oa - xa) / xa) <= 2 * float(fi.eps)
    assert np.array_equal(np.signbit(out), np.signbit(x))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_inverse_clamps_at_both_ends(dtype):
    import torch
    import mgard_amd
    fi = np.finfo(dtype)
    top, bottom = (128.5, -127.0) if dtype == np.float32 else (1024.5, -1023.0)
    y = np.array([top, bottom, top, bottom, 0.0, 1.0, -1.0], dtype=dtype)
    flag = np.array([0, 0, 1, 1, 0, 1, 0], dtype=bool)
    zeros = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = mgard_amd.pwrel_inverse(_dev(y), zeros, _dev(mm.packed_words(flag).view(np.int64))).cpu().numpy()
    want = np.array([fi.max, fi.tiny, -fi.max, -fi.tiny, 1.0, -2.0, 0.5], dtype=dtype)
    assert np.array_equal(mm.int_view(out), mm.int_view(want))
    assert np.array_equal(mm.int_view(pm.inverse(y, np.zeros(7, dtype=bool), flag)), mm.int_view(want))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_compare(shape, dtype):
    import mgard_amd
    fl = _floor(dtype)
    x = pm.decades_field(shape, dtype, seed=11 + shape[0], abs_floor=fl)
    mask, flag = pm.bitmaps(x, fl)
    rng = np.random.default_rng(3)
    # a reconstruction that respects every class, with a relative error of up to 1e-3
    r = pm.inverse(pm.forward(x, fl), mask, flag)
    with np.errstate(over="ignore"):                        # (the largest finite value: clipped back below)
        r = (r.astype(np.float64) * (1 + rng.uniform(-1e-3, 1e-3, size=x.shape))).astype(dtype)
    r[~mask] = np.clip(np.abs(r[~mask]), np.finfo(dtype).tiny, np.finfo(dtype).max) * np.where(flag[~mask], -1, 1)
    r[mask & ~flag] = 0.0

    def check(r, sign=0, cls=0):
        got = mgard_amd.compare_pwrel(_dev(x), _dev(r), fl)
        want = pm.compare(x, r, fl)
        for f in ("n", "n_valid", "n_zeroed", "n_nonfinite", "n_class_mismatch", "n_sign_mismatch"):
            assert getattr(got, f) == want[f], f
        assert (got.n_sign_mismatch, got.n_class_mismatch) == (sign, cls)
        assert np.float64(got.max_rel_err).view(np.uint64) == np.float64(want["max_rel_err"]).view(np.uint64)
        assert got.argmax == want["argmax"] or want["rel"][got.argmax] == want["max_rel_err"]
        assert got.max_zeroed_abs == want["max_zeroed_abs"]
        return got

    check(r)
    valid = np.flatnonzero(~mask.reshape(-1))
    if valid.size:
        # a planted sign flip and a planted class mismatch are each counted once
        flipped = r.copy()
        flipped.reshape(-1)[valid[0]] *= -1
        assert check(flipped, sign=1).max_rel_err >= 1.9
        lost = r.copy()
        lost.reshape(-1)[valid[-1]] = 0.0
        check(lost, cls=1)
    zeroed = np.flatnonzero((mask & ~flag).reshape(-1))
    if zeroed.size:
        neg = r.copy()
        neg.reshape(-1)[zeroed[0]] = -0.0                   # -0.0 is not +0.0 to the bit
        check(neg, cls=1)
    nonfin = np.flatnonzero((mask & flag).reshape(-1))
    if nonfin.size:
        inf = r.copy()
        inf.reshape(-1)[nonfin[0]] = np.inf                 # a non-finite position must come back as NaN
        check(inf, cls=1)


def test_refusals():
    import torch
    import mgard_amd
    x = torch.ones(10, dtype=torch.float32, device="cuda")
    for floor in (-1.0, float("nan"), float("inf")):
        with pytest.raises(mgard_amd.MgardHipError, match="error -1"):
            mgard_amd.pwrel_forward(x, floor)
        with pytest.raises(mgard_amd.MgardHipError, match="error -1"):
            mgard_amd.compare_pwrel(x, x, floor)
    y, mw, fw, st = mgard_amd.pwrel_forward(x, 0.0)
    assert (st.n, st.n_masked, st.n_flag, st.ymin, st.ymax) == (10, 0, 0, 0.0, 0.0)
