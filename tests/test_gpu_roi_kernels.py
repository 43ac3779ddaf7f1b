"""mgh_box_residual_ and mgh_box_add_ (mgard_amd/csrc/kernels_roi.hpp) against NumPy, to the bit: the dense residual
fl(x - b) of a box of two arrays with its statistics, and the in-place addition of a dense box into an array, which
must leave every element outside the box alone. Shapes: one to five dimensions, rows that cross a 64-lane boundary at
an unaligned start, rows shorter than a wave (several rows per wave), more rows than one workgroup holds, and the
whole array as the box."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [
    ("1d-1000", (1000,), (37,), (130,)),
    ("2d-17x130", (17, 130), (2, 1), (9, 129)),
    ("3d-17x19x70-unaligned-rows", (17, 19, 70), (1, 2, 3), (5, 7, 65)),
    ("3d-9x9x9-short-rows", (9, 9, 9), (3, 3, 3), (3, 3, 3)),
    ("5d-5x4x6x7x9", (5, 4, 6, 7, 9), (1, 0, 2, 1, 3), (3, 4, 3, 5, 4)),
    ("3d-whole-array", (17, 19, 70), (0, 0, 0), (17, 19, 70)),
    ("2d-whole-array-one-row-wide", (2100, 3), (0, 0), (2100, 3)),
]
IDS = [c[0] for c in CASES]
DTYPES = [np.float32, np.float64]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _box(lo, ext):
    return tuple(slice(a, a + e) for a, e in zip(lo, ext))


def _ints(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _fields(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(dtype)
    b = (x.astype(np.float64) * (1 + 1e-3 * rng.standard_normal(shape))).astype(dtype)
    return x, b


def _stats(x, r):
    ax, ar = np.abs(x.astype(np.float64)), np.abs(r.astype(np.float64))
    fx, fr = np.isfinite(ax), np.isfinite(ar)
    return (float(ar[fr].max()) if fr.any() else 0.0, float(ax[fx].max()) if fx.any() else 0.0, int((~(fx & fr)).sum()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name,shape,lo,ext", CASES, ids=IDS)
def test_box_residual_is_numpy_to_the_bit(name, shape, lo, ext, dtype):
    import mgard_amd
    x, b = _fields(shape, dtype, 11)
    r, st = mgard_amd.box_residual(_dev(x), _dev(b), lo, ext)
    with np.errstate(all="ignore"):
        want = (x[_box(lo, ext)] - b[_box(lo, ext)]).astype(dtype)
    got = r.cpu().numpy()
    assert got.shape == tuple(ext) and got.dtype == dtype
    assert np.array_equal(_ints(got), _ints(want))
    assert (st.max_abs_r, st.max_abs_x, st.n_nonfinite) == _stats(x[_box(lo, ext)], want)
    assert st.max_abs_r > 0 and st.n_nonfinite == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name,shape,lo,ext", CASES[:5], ids=IDS[:5])
def test_nonfinite_counts_only_inside_the_box(name, shape, lo, ext, dtype):
    import mgard_amd
    x, b = _fields(shape, dtype, 12)
    base = mgard_amd.box_residual(_dev(x), _dev(b), lo, ext)[1]
    inside = tuple(a + e - 1 for a, e in zip(lo, ext))            # the box's last element
    outside = tuple(int(v) for v in np.unravel_index(np.ravel_multi_index(inside, shape) + 1, shape))  # ... the one behind it
    first_out = tuple(lo[:-1]) + (lo[-1] - 1,)                    # ... and the one in front of the box's first
    for site, counted in ((inside, 1), (tuple(lo), 1), (outside, 0), (first_out, 0)):
        for value in (np.nan, np.inf):
            y = x.copy()
            y[site] = value
            r, st = mgard_amd.box_residual(_dev(y), _dev(b), lo, ext)
            with np.errstate(all="ignore"):
                want = (y[_box(lo, ext)] - b[_box(lo, ext)]).astype(dtype)
            assert st.n_nonfinite == counted, (site, value)
            assert (st.max_abs_r, st.max_abs_x, st.n_nonfinite) == _stats(y[_box(lo, ext)], want)
            if not counted:
                assert (st.max_abs_r, st.max_abs_x) == (base.max_abs_r, base.max_abs_x)
    # a NaN in b inside the box makes r non-finite there: counted as well
    c = b.copy()
    c[inside] = np.nan
    assert mgard_amd.box_residual(_dev(x), _dev(c), lo, ext)[1].n_nonfinite == 1


def test_residual_of_equal_arrays_is_zero():
    import mgard_amd
    x, _ = _fields((9, 9, 9), np.float32, 13)
    r, st = mgard_amd.box_residual(_dev(x), _dev(x), (3, 3, 3), (3, 3, 3))
    assert st.max_abs_r == 0.0 and st.n_nonfinite == 0 and not r.cpu().numpy().any()
    assert st.max_abs_x == float(np.abs(x[3:6, 3:6, 3:6]).max())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name,shape,lo,ext", CASES, ids=IDS)
def test_box_add_is_numpy_inside_and_leaves_the_outside_alone(name, shape, lo, ext, dtype):
    import mgard_amd
    x, b = _fields(shape, dtype, 14)
    rng = np.random.default_rng(15)
    r = (1e-2 * rng.standard_normal(ext)).astype(dtype)
    # the outside poisoned with NaNs of distinct payloads: compared as integers
    it = np.uint32 if dtype == np.float32 else np.uint64
    nan = it(0x7fc00000) if dtype == np.float32 else it(0x7ff8000000000000)
    poison = (nan + np.arange(1, x.size + 1, dtype=it)).reshape(shape)
    data = poison.view(dtype).copy()
    data[_box(lo, ext)] = b[_box(lo, ext)]
    before = _ints(data).copy()
    out = mgard_amd.box_add(_dev(data), _dev(r), lo).cpu().numpy()
    want = (b[_box(lo, ext)] + r).astype(dtype)
    assert np.array_equal(_ints(out[_box(lo, ext)]), _ints(want))
    mask = np.ones(shape, dtype=bool)
    mask[_box(lo, ext)] = False
    assert np.array_equal(_ints(out)[mask], before[mask])


def test_argument_refusals_launch_nothing():
    import mgard_amd
    x, b = _fields((9, 9, 9), np.float32, 16)
    dx, db = _dev(x), _dev(b)
    for lo, ext in (((7, 0, 0), (3, 3, 3)), ((0, 0, 9), (3, 3, 1)), ((0, 0, 0), (10, 3, 3))):
        with pytest.raises(mgard_amd.MgardHipError, match="box leaves the array"):
            mgard_amd.box_residual(dx, db, lo, ext)
    import torch
    with pytest.raises(mgard_amd.MgardHipError, match="box leaves the array"):
        mgard_amd.box_add(dx, torch.zeros((3, 3, 3), dtype=torch.float32, device="cuda"), (7, 7, 7))
