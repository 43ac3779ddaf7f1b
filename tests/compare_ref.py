"""NumPy restatement of mgh_error_stats (include/mgard_hip.h), shared by the CPU and GPU tests of
mgh_compare / mgh_verify. It follows the reference's include/mgard-x/Utilities/ErrorCalculator.h: the
difference and its absolute value are taken in the arrays' type T (:57-64, :83, :103) and widened to double;
the squares are summed in double (:41-45, :101-105) -- here with math.fsum, the correctly rounded sum, so
that the expectation carries no order of its own. Positions whose difference is not finite are counted and
left out of everything else (the library's rule; the reference has none)."""
import math

import numpy as np

EXACT = ("n", "nonfinite", "max_abs_err", "argmax", "ref_min", "ref_max", "ref_abs_max")
SUMS = ("sum_sq_err", "ref_sum_sq")


def ref_stats(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    assert a.dtype == b.dtype and a.dtype in (np.float32, np.float64) and a.size == b.size
    with np.errstate(all="ignore"):
        d = a - b  # in T
    ok = np.isfinite(d)
    idx = np.flatnonzero(ok)
    e = np.abs(d[ok]).astype(np.float64)
    x = a[ok].astype(np.float64)
    r = {"n": int(a.size), "nonfinite": int(a.size - idx.size)}
    if idx.size:
        r.update(max_abs_err=float(e.max()), argmax=int(idx[int(np.argmax(e))]),  # (argmax: the first of equals)
                 ref_min=float(x.min()), ref_max=float(x.max()), ref_abs_max=float(np.abs(x).max()))
    else:
        r.update(max_abs_err=0.0, argmax=0, ref_min=0.0, ref_max=0.0, ref_abs_max=0.0)
    r["sum_sq_err"] = math.fsum(e * e)
    r["ref_sum_sq"] = math.fsum(x * x)
    return r


def bits(v):
    return np.float64(v).view(np.uint64) if isinstance(v, float) else int(v)


def sum_tolerance(n):
    """Relative error of a sum of n non-negative doubles added in ANY order, against the exact sum: every
    one of the at most n - 1 additions rounds a partial sum that is no larger than the total by at most
    2^-53 of itself, and no cancellation can occur, so (1 + 2^-53)^(n-1) - 1 <= n 2^-52 for every n a test
    can hold in memory. Derived, not measured."""
    return n * 2.0 ** -52


def assert_stats(got, want, n_sum=None, exact_sums=False, what=""):
    """got: anything with the fields as attributes or keys; want: a dict of ref_stats."""
    get = (lambda k: got[k]) if isinstance(got, dict) else (lambda k: getattr(got, k))
    for k in EXACT:
        assert bits(get(k)) == bits(want[k]), "%s %s: got %r, want %r" % (what, k, get(k), want[k])
    tol = sum_tolerance(want["n"] if n_sum is None else n_sum)
    for k in SUMS:
        g, w = float(get(k)), float(want[k])
        if exact_sums:
            assert bits(g) == bits(w), "%s %s: got %r, want %r" % (what, k, g, w)
        elif w == 0:
            assert g == 0, "%s %s: got %r, want 0" % (what, k, g)
        else:
            assert abs(g - w) / w <= tol, "%s %s: got %r, want %r (relative %g > %g)" % (what, k, g, w, abs(g - w) / w, tol)
