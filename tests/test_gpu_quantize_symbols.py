"""GPU tests of mgh_quantize_symbols (k_quantize_symbols, DESIGN.md sections 4 and 8): one pass from a
coefficient array to 16-bit symbols, the outlier list and the histogram of the symbols, held against
mgh_quantize(prep_huffman = 1) on the same coefficients. Every comparison is an equality of integers; the
outlier lists are compared as sets (their order is the order of the quantizer's atomics)."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_budget import _tolerances
from tests.test_gpu_target import FUSED3, SMALL
from tests.util import nonuniform_coords, smooth_field

pytestmark = pytest.mark.gpu

INF = float("inf")
F32, F64 = np.float32, np.float64
MGH_ERR_INVALID_ARGUMENT = -1
DICTS = (64, 1024, 8192)


def _gpu():
    import torch
    import mgard_amd
    return torch, mgard_amd


def _u16(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _pairs(idx, val):
    i, v = idx.cpu().numpy().astype(np.int64), val.cpu().numpy()
    order = np.argsort(i, kind="stable")
    return i[order], v[order]


def _check_against_quantize(h, what, got, ref, dict_size):
    """got: quantize_symbols' (symbols, freq, idx, val); ref: quantize's (q, idx, val, count)."""
    sym, freq, oi, ov = got
    q, roi, rov, rn = ref
    qn = q.cpu().numpy()
    assert qn.min() >= 0 and qn.max() < dict_size, what
    s = _u16(sym)
    assert s.shape == qn.shape and np.array_equal(s, qn.astype(np.uint16)), what
    assert int(oi.numel()) == int(ov.numel()) == rn, (what, int(oi.numel()), rn)   # the counter
    gi, gv = _pairs(oi, ov)
    ri, rv = _pairs(roi, rov)
    assert np.array_equal(gi, ri) and np.array_equal(gv, rv), what
    assert not s.ravel()[gi].any(), what                                           # symbol 0 at the outliers
    if freq is not None:
        f = freq.cpu().numpy()
        assert np.array_equal(f, np.bincount(s.ravel(), minlength=dict_size)), what
    return s, gi, gv


# (shape, non-uniform grid): every branch of the walk -- 1-D, shorter than one vector, rows that are no
# multiple of a vector (vectors run across one row end, across several), the fused shapes, 4-D, 5-D
SHAPES = [
    ((1001,), False),
    ((3,), False),
    ((65, 40), False),
    ((7, 20), False),
    ((9, 5), False),
    (SMALL, False),
    (SMALL, True),
    (FUSED3, False),
    ((5, 9, 9, 17), False),
    ((3, 3, 5, 5, 9), False),
]


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("shape,nonuniform", SHAPES)
def test_symbols_lists_and_histogram_are_the_quantizers(shape, nonuniform, dt):
    torch, mg = _gpu()
    h = mg.Hierarchy(shape, dt, coords=nonuniform_coords(shape, dt) if nonuniform else None)
    d = torch.from_numpy(smooth_field(shape, dt)).cuda()
    dense = h.decompose(d)
    n = int(np.prod(shape))
    # the misaligned scalar route: a view that starts one element into an allocation
    store = torch.empty(n + 1, dtype=dense.dtype, device=dense.device)
    off = store[1:].view(shape)
    off.copy_(dense)
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()
    tols = _tolerances(5)
    for rel in (False, True):
        eb = mg.REL if rel else mg.ABS
        for s in (INF, 0.0, 1.0):
            norm = h.norm(d, s) if rel else 1.0
            for k, tol in enumerate(tols):
                for dict_size in DICTS:
                    what = (shape, np.dtype(dt).name, "REL" if rel else "ABS", s, tol, dict_size)
                    ref = h.quantize(dense, eb, tol, s, norm, dict_size=dict_size, prep_huffman=True)
                    got = h.quantize_symbols(dense, eb, tol, s, norm, dict_size=dict_size)
                    sym, gi, gv = _check_against_quantize(h, what, got, ref, dict_size)
                    if k == 0 and dict_size == 64:  # (nearly every value travels through the outlier list)
                        assert len(gi) > 0.9 * n if n >= 40 else len(gi) >= 1, (what, len(gi))
                    if k == len(tols) - 1:          # (everything in the centre bin)
                        assert len(gi) == 0 and np.all(sym == dict_size // 2), what
                    if dict_size == 1024:
                        # the same answer without the histogram, and from the misaligned view
                        for src, hist in ((dense, False), (off, True)):
                            s2, f2, oi2, ov2 = h.quantize_symbols(src, eb, tol, s, norm, dict_size=dict_size,
                                                                  histogram=hist)
                            assert (f2 is None) == (not hist)
                            assert np.array_equal(_u16(s2), sym), (what, hist)
                            i2, v2 = _pairs(oi2, ov2)
                            assert np.array_equal(i2, gi) and np.array_equal(v2, gv), (what, hist)
                            if hist:
                                assert np.array_equal(f2.cpu().numpy(), got[1].cpu().numpy()), what
    # an all-zero array: every symbol is the centre one
    zero = torch.zeros_like(dense)
    for dict_size in DICTS:
        sym, freq, oi, ov = h.quantize_symbols(zero, mg.ABS, 1e-3, INF, 1.0, dict_size=dict_size)
        assert oi.numel() == 0 and np.all(_u16(sym) == dict_size // 2)
        assert int(freq[dict_size // 2]) == n and int(freq.sum()) == n
    h.close()


@pytest.mark.parametrize("dt", [F32, F64])
def test_symbols_are_the_fused_calls_on_the_fused_shape(dt):
    torch, mg = _gpu()
    h = mg.Hierarchy(FUSED3, dt)
    assert h.sym16_supported()
    d = torch.from_numpy(smooth_field(FUSED3, dt)).cuda()
    dense = h.decompose(d)
    for rel, s, tol, dict_size in ((True, INF, 1e-3, 8192), (True, INF, 1e-5, 64), (False, INF, 1e-2, 1024),
                                   (True, 0.0, 1e-3, 1024)):
        eb = mg.REL if rel else mg.ABS
        fsym, foi, fov, fn, fnorm = h.decompose_quantize_sym16(d, eb, tol, s, dict_size=dict_size)
        sym, _, oi, ov = h.quantize_symbols(dense, eb, tol, s, fnorm if rel else 1.0, dict_size=dict_size)
        what = (np.dtype(dt).name, rel, s, tol, dict_size)
        assert np.array_equal(_u16(sym), _u16(fsym)), what
        assert int(oi.numel()) == fn, what
        gi, gv = _pairs(oi, ov)
        ri, rv = _pairs(foi[:fn], fov[:fn])
        assert np.array_equal(gi, ri) and np.array_equal(gv, rv), what
    h.close()


def _raw_call(mg, h, coeff, dict_size, sym, freq, cnt, idx, val, cap, tol=1e-13):
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    return mg.load_library().mgh_quantize_symbols(h._h, p(coeff), mg.ABS, tol, INF, 1.0, dict_size, p(sym), p(freq),
                                                  p(cnt), p(idx), p(val), cap, None)


def test_capacity_below_the_count_reports_the_count_and_writes_nothing_past_it():
    torch, mg = _gpu()
    shape, dict_size, guard, mark = SMALL, 64, 64, -0x5a5a5a5a5a5a5a5b
    h = mg.Hierarchy(shape, F32)
    dense = h.decompose(torch.from_numpy(smooth_field(shape, F32)).cuda())
    n = int(np.prod(shape))
    q, roi, rov, rn = h.quantize(dense, mg.ABS, 1e-13, INF, 1.0, dict_size=dict_size, prep_huffman=True)
    assert rn > 0.9 * n
    ri, rv = _pairs(roi, rov)
    cap = rn // 3
    sym = torch.empty(shape, dtype=torch.uint16, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    idx = torch.full((cap + guard,), mark, dtype=torch.int64, device="cuda")
    val = torch.full((cap + guard,), mark, dtype=torch.int64, device="cuda")
    assert _raw_call(mg, h, dense, dict_size, sym, None, cnt, idx, val, cap) == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == rn                                     # the full count
    assert bool((idx[cap:] == mark).all()) and bool((val[cap:] == mark).all())   # nothing past the capacity
    gi, gv = _pairs(idx[:cap], val[:cap])
    assert len(np.unique(gi)) == cap                                 # `cap` valid pairs
    at = np.searchsorted(ri, gi)
    assert np.array_equal(ri[at], gi) and np.array_equal(rv[at], gv)
    assert np.array_equal(_u16(sym), q.cpu().numpy().astype(np.uint16))
    # a second call with the reported capacity
    cnt.zero_()
    idx = torch.full((rn + guard,), mark, dtype=torch.int64, device="cuda")
    val = torch.full((rn + guard,), mark, dtype=torch.int64, device="cuda")
    assert _raw_call(mg, h, dense, dict_size, sym, None, cnt, idx, val, rn) == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == rn and bool((idx[rn:] == mark).all()) and bool((val[rn:] == mark).all())
    gi, gv = _pairs(idx[:rn], val[:rn])
    assert np.array_equal(gi, ri) and np.array_equal(gv, rv)
    # capacity 0 with NULL lists only counts
    cnt.zero_()
    assert _raw_call(mg, h, dense, dict_size, sym, None, cnt, None, None, 0) == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == rn
    h.close()


def test_refusals_leave_the_library_usable():
    torch, mg = _gpu()
    h = mg.Hierarchy(SMALL, F32)
    dense = h.decompose(torch.from_numpy(smooth_field(SMALL, F32)).cuda())
    sym = torch.empty(SMALL, dtype=torch.uint16, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    idx = torch.empty(16, dtype=torch.int64, device="cuda")
    val = torch.empty(16, dtype=torch.int64, device="cuda")

    def works():
        ref = h.quantize(dense, mg.ABS, 1e-3, INF, 1.0, dict_size=1024, prep_huffman=True)
        _check_against_quantize(h, "after a refusal", h.quantize_symbols(dense, mg.ABS, 1e-3, INF, 1.0, dict_size=1024),
                                ref, 1024)

    for dict_size in (0, 1, 3, 8191, 16386, 65536):
        assert _raw_call(mg, h, dense, dict_size, sym, None, cnt, idx, val, 16) == MGH_ERR_INVALID_ARGUMENT, dict_size
        assert b"dict_size" in mg.load_library().mgh_last_error()
        works()
    for args in ((None, cnt, idx, val, 16), (sym, None, idx, val, 16), (sym, cnt, None, val, 16), (sym, cnt, idx, None, 16)):
        assert _raw_call(mg, h, dense, 1024, args[0], None, *args[1:]) == MGH_ERR_INVALID_ARGUMENT, args
        works()
    assert _raw_call(mg, h, None, 1024, sym, None, cnt, idx, val, 16) == MGH_ERR_INVALID_ARGUMENT
    works()
    for dict_size in (2, 16384):  # the ends of the range are taken
        ref = h.quantize(dense, mg.ABS, 1e-2, INF, 1.0, dict_size=dict_size, prep_huffman=True)
        _check_against_quantize(h, dict_size, h.quantize_symbols(dense, mg.ABS, 1e-2, INF, 1.0, dict_size=dict_size), ref,
                                dict_size)
    h.close()
