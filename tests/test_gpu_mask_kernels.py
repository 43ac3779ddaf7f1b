"""mgh_mask_scan / mgh_mask_fill / mgh_mask_restore against tests/mask_model.py, bit for bit: the packed words
including the zero bits behind the array's end, the statistics, the filled array, the array filled in place, the
restored array. Floats are compared through their integer views, so NaN payloads and -0.0 count.

Shapes: the smallest at which each mechanism can break -- around a wave (64), a segment (1024), two segments and a
tail, rows that do not start on a word of the mask, more rows than a workgroup has waves, and a length that takes
several workgroups of the scan."""
import numpy as np
import pytest

from tests import mask_model as mm

SHAPES = [(1,), (63,), (64,), (65,), (1023,), (1024,), (1025,), (2049,), (5000,),
          (7, 1025), (130, 65), (5, 9, 67), (33, 17, 130), (3, 5, 9, 66)]
NAN = float("nan")


def _patterns(shape, rng):
    """name -> boolean mask"""
    n, nf = int(np.prod(shape)), shape[-1]
    rows = n // nf
    out = {"none": np.zeros(shape, bool), "all": np.ones(shape, bool)}
    first = np.zeros(n, bool)
    first[0] = True
    last = np.zeros(n, bool)
    last[-1] = True
    out["first"], out["last"] = first.reshape(shape), last.reshape(shape)
    whole = np.zeros((rows, nf), bool)
    whole[::2] = True                       # rows 0, 2, ...: the first row and, for odd counts, the last
    out["rows"] = whole.reshape(shape)
    if nf == 2049:
        run = np.zeros((rows, nf), bool)
        run[:, 1000:1100] = True            # straddles the segment boundary at 1024 and wave boundaries
        out["run"] = run.reshape(shape)
    end = np.ones((rows, nf), bool)         # a valid element only at the end of every segment: the right-hand rule
    for a in range(0, nf, mm.SEGMENT):
        end[:, min(a + mm.SEGMENT, nf) - 1] = False
    out["segment_end"] = end.reshape(shape)
    out["random30"] = rng.random(shape) < 0.30
    out["random99"] = rng.random(shape) < 0.99
    if len(shape) == 3:
        g = np.meshgrid(*[np.arange(e) - (e - 1) / 2 for e in shape], indexing="ij")
        out["ball"] = sum((x / (0.4 * e)) ** 2 for x, e in zip(g, shape)) < 1.0
    return out


# how the masked positions are marked, and what the scan is asked to look for
MODES = {
    "nonfinite": dict(marks=[NAN, float("inf"), float("-inf")], nonfinite=True, fill_value=None),
    "fill1e20": dict(marks=[1e20], nonfinite=False, fill_value=1e20),
    "fill-9999": dict(marks=[-9999.0], nonfinite=False, fill_value=-9999.0),
    "both": dict(marks=[NAN, 1e20, float("-inf"), 1e20], nonfinite=True, fill_value=1e20),
}


def _field(shape, dtype, rng):
    x = rng.standard_normal(shape).astype(dtype)
    flat = x.reshape(-1)
    flat[rng.random(flat.size) < 0.05] = 0.0     # zeros of both signs among the valid elements
    flat[rng.random(flat.size) < 0.05] = -0.0
    return x


def _mark(x, mask, marks):
    y = x.copy()
    idx = np.flatnonzero(mask.reshape(-1))
    y.reshape(-1)[idx] = np.array(marks, dtype=x.dtype)[np.arange(idx.size) % len(marks)]
    return y


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scan_fill_restore_bit_for_bit(shape, dtype):
    import torch
    import mgard_amd
    rng = np.random.default_rng([np.dtype(dtype).itemsize, *shape])
    x = _field(shape, dtype, rng)
    n = x.size
    for pname, mask in _patterns(shape, rng).items():
        for mname, mode in MODES.items():
            what = (pname, mname)
            data = _mark(x, mask, mode["marks"])
            assert np.array_equal(mm.classify(data, mode["nonfinite"], mode["fill_value"]), mask), what
            d = torch.from_numpy(data).cuda()
            words, st = mgard_amd.mask_scan(d, nonfinite=mode["nonfinite"], fill_value=mode["fill_value"])
            assert np.array_equal(_u64(words), mm.packed_words(mask)), what
            _, nm, vmin, vmax = mm.stats(data, mask)
            assert (st.n, st.n_masked) == (n, nm), what
            assert np.array_equal(np.array([st.vmin, st.vmax]).view(np.int64), np.array([vmin, vmax]).view(np.int64)), what
            c = mm.fill_constant(data, mask)
            want = mm.fill(data, mask, c)
            assert np.isfinite(want).all() and np.array_equal(mm.int_view(want)[~mask], mm.int_view(data)[~mask]), what
            got = mgard_amd.mask_fill(d, words, float(c))
            assert np.array_equal(mm.int_view(got.cpu().numpy()), mm.int_view(want)), what
            assert np.array_equal(mm.int_view(d.cpu().numpy()), mm.int_view(data)), what      # the input is left alone
            inplace = d.clone()
            assert mgard_amd.mask_fill(inplace, words, float(c), out=inplace) is inplace
            assert np.array_equal(mm.int_view(inplace.cpu().numpy()), mm.int_view(want)), what
            for value in (NAN, -9999.0):
                back = mgard_amd.mask_restore(got.clone(), words, value)
                assert np.array_equal(mm.int_view(back.cpu().numpy()), mm.int_view(mm.restore(want, mask, value))), what


@pytest.mark.gpu
def test_all_masked_array_fills_with_zero_and_fill_takes_any_constant():
    import torch
    import mgard_amd
    data = np.full((3, 70), np.nan, dtype=np.float32)
    d = torch.from_numpy(data).cuda()
    words, st = mgard_amd.mask_scan(d)
    assert (st.n, st.n_masked, st.vmin, st.vmax) == (210, 210, 0.0, 0.0)
    assert np.array_equal(mgard_amd.mask_fill(d, words, 0.0).cpu().numpy(), np.zeros((3, 70), np.float32))
    assert np.array_equal(mgard_amd.mask_fill(d, words, -2.5).cpu().numpy(), np.full((3, 70), -2.5, np.float32))


@pytest.mark.gpu
def test_refusals_leave_the_library_usable():
    import torch
    import mgard_amd
    d = torch.from_numpy(np.arange(100, dtype=np.float32)).cuda()
    with pytest.raises(mgard_amd.MgardHipError, match="flags"):
        mgard_amd.mask_scan(d, nonfinite=False, fill_value=None)          # flags = 0
    with pytest.raises(mgard_amd.MgardHipError, match="NaN fill_value"):
        mgard_amd.mask_scan(d, nonfinite=False, fill_value=NAN)
    with pytest.raises(mgard_amd.MgardHipError, match="NaN fill_value"):
        mgard_amd.mask_scan(d, nonfinite=True, fill_value=NAN)
    words, st = mgard_amd.mask_scan(d, nonfinite=False, fill_value=7.0)
    assert (st.n_masked, st.vmin, st.vmax) == (1, 0.0, 99.0) and int(_u64(words)[0]) == 1 << 7
