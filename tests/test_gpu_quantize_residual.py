"""GPU tests of the two kernels of the precision layers (DESIGN.md sections 4 and 8):
mgh_quantize_symbols_residual (k_quantize_symbols_residual) -- mgh_quantize_symbols with the residual
`coeff - dequantize(integers)` as one more output -- and mgh_dequantize_add (k_dequantize_add), the dequantizer
that stores or adds. Symbols, outlier lists, counter and histogram are held against mgh_quantize(prep_huffman = 1)
the way tests/test_gpu_quantize_symbols.py holds mgh_quantize_symbols; the floating-point outputs are compared
bit for bit with mgh_dequantize and ONE torch subtraction or addition."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_quantize_symbols import SHAPES, _check_against_quantize, _pairs, _u16
from tests.test_gpu_target import FUSED3, SMALL
from tests.util import nonuniform_coords, smooth_field

pytestmark = pytest.mark.gpu

INF = float("inf")
F32, F64 = np.float32, np.float64
MGH_ERR_INVALID_ARGUMENT = -1
DICTS = (64, 1024)  # (outliers exist at 64)


def _gpu():
    import torch
    import mgard_amd
    return torch, mgard_amd


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64).cpu().numpy()


def _offset_view(torch, dense):
    """The misaligned scalar route: a copy that starts one element into an allocation."""
    store = torch.empty(dense.numel() + 1, dtype=dense.dtype, device=dense.device)
    off = store[1:].view(dense.shape)
    off.copy_(dense)
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()
    return off


def _step(h, mg, what, coeff, eb, tol, s, norm, dict_size, histogram=True, out=None):
    """One residual step checked in full: returns (residual as the kernel wrote it, the reference's q + lists).
    The reference is made BEFORE the call, so an in-place call is compared with what it overwrote."""
    ref = h.quantize(coeff, eb, tol, s, norm, dict_size=dict_size, prep_huffman=True)
    q, roi, rov, rn = ref
    back = h.dequantize(q.clone(), eb, tol, s, norm, dict_size=dict_size, outlier_idx=roi, outlier_val=rov)
    want = coeff - back                                               # (one IEEE subtraction per element)
    sym, freq, oi, ov, res = h.quantize_symbols_residual(coeff, eb, tol, s, norm, dict_size=dict_size,
                                                         histogram=histogram, out=out)
    assert (freq is None) == (not histogram), what
    _check_against_quantize(h, what, (sym, freq, oi, ov), ref, dict_size)
    assert out is None or res.data_ptr() == out.data_ptr(), what
    assert np.array_equal(_bits(res), _bits(want)), what
    return res, ref


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("shape,nonuniform", SHAPES)
def test_residual_step_is_the_quantizer_and_the_dequantizer(shape, nonuniform, dt):
    torch, mg = _gpu()
    h = mg.Hierarchy(shape, dt, coords=nonuniform_coords(shape, dt) if nonuniform else None)
    d = torch.from_numpy(smooth_field(shape, dt)).cuda()
    dense = h.decompose(d)
    off = _offset_view(torch, dense)
    outliers = 0
    for rel, s, tol in ((True, INF, 1e-3), (False, INF, 1e-2), (True, 0.0, 1e-3)):
        eb = mg.REL if rel else mg.ABS
        norm = h.norm(d, s) if rel else 1.0
        for dict_size in DICTS:
            what = (shape, np.dtype(dt).name, "REL" if rel else "ABS", s, tol, dict_size)
            res, ref = _step(h, mg, what, dense, eb, tol, s, norm, dict_size)            # out of place, HIST
            outliers += ref[3] if dict_size == 64 else 0
            _step(h, mg, what + ("no histogram",), dense, eb, tol, s, norm, dict_size, histogram=False)
            work = dense.clone()
            got, _ = _step(h, mg, what + ("in place",), work, eb, tol, s, norm, dict_size, out=work)
            assert got.data_ptr() == work.data_ptr() and np.array_equal(_bits(work), _bits(res)), what
            got, _ = _step(h, mg, what + ("misaligned",), off, eb, tol, s, norm, dict_size)
            assert np.array_equal(_bits(got), _bits(res)), what
            # ... and with the residual misaligned as well, in place in the offset view
            work = _offset_view(torch, dense)
            _step(h, mg, what + ("misaligned, in place",), work, eb, tol, s, norm, dict_size, out=work)
            assert np.array_equal(_bits(work), _bits(res)), what
    assert outliers > 0, "the case must send values through the outlier list"
    h.close()


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("shape", [SMALL, FUSED3])
def test_three_chained_tolerances(shape, dt):
    torch, mg = _gpu()
    h = mg.Hierarchy(shape, dt)
    d = torch.from_numpy(smooth_field(shape, dt)).cuda()
    norm = h.norm(d, INF)
    r = h.decompose(d)
    acc = None
    for k, tol in enumerate((1e-2, 1e-3, 1e-4)):
        what = (shape, np.dtype(dt).name, k)
        r_next, (q, oi, ov, n) = _step(h, mg, what, r, mg.REL, tol, INF, norm, 256)
        if k:  # a residual layer: |q| <= ceil(tol_{k-1} / tol_k / 2) = 5, a handful of symbols and no outliers
            qn = q.cpu().numpy() - 128
            assert n == 0 and np.abs(qn).max() <= 5, (what, n, int(np.abs(qn).max()))
        back = h.dequantize(q.clone(), mg.REL, tol, INF, norm, dict_size=256, outlier_idx=oi, outlier_val=ov)
        want = back if acc is None else acc + back
        acc = h.dequantize_add(q.clone(), mg.REL, tol, INF, norm, dict_size=256, outlier_idx=oi, outlier_val=ov, acc=acc)
        assert np.array_equal(_bits(acc), _bits(want)), what
        r = r_next
    # what the reader has after three layers is within the third tolerance of the data
    err = float((h.recompose(acc) - d).abs().max())
    assert err <= 1e-4 * norm, (err, 1e-4 * norm)
    h.close()


def _raw_call(mg, h, coeff, dict_size, sym, freq, cnt, idx, val, cap, res, tol=1e-13):
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    return mg.load_library().mgh_quantize_symbols_residual(h._h, p(coeff), mg.ABS, tol, INF, 1.0, dict_size, p(sym),
                                                           p(freq), p(cnt), p(idx), p(val), cap, p(res), None)


def test_capacity_below_the_count_reports_the_count_and_the_residual_is_complete():
    torch, mg = _gpu()
    shape, dict_size, guard, mark = SMALL, 64, 64, -0x5a5a5a5a5a5a5a5b
    h = mg.Hierarchy(shape, F32)
    dense = h.decompose(torch.from_numpy(smooth_field(shape, F32)).cuda())
    n = int(np.prod(shape))
    q, roi, rov, rn = h.quantize(dense, mg.ABS, 1e-13, INF, 1.0, dict_size=dict_size, prep_huffman=True)
    assert rn > 0.9 * n
    want = dense - h.dequantize(q.clone(), mg.ABS, 1e-13, INF, 1.0, dict_size=dict_size, outlier_idx=roi, outlier_val=rov)
    ri, rv = _pairs(roi, rov)
    cap = rn // 3
    sym = torch.empty(shape, dtype=torch.uint16, device="cuda")
    res = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    idx = torch.full((cap + guard,), mark, dtype=torch.int64, device="cuda")
    val = torch.full((cap + guard,), mark, dtype=torch.int64, device="cuda")
    assert _raw_call(mg, h, dense, dict_size, sym, None, cnt, idx, val, cap, res) == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == rn                                                  # the full count
    assert bool((idx[cap:] == mark).all()) and bool((val[cap:] == mark).all())    # nothing past the capacity
    gi, gv = _pairs(idx[:cap], val[:cap])
    assert len(np.unique(gi)) == cap                                              # `cap` valid pairs
    at = np.searchsorted(ri, gi)
    assert np.array_equal(ri[at], gi) and np.array_equal(rv[at], gv)
    assert np.array_equal(_u16(sym), q.cpu().numpy().astype(np.uint16))
    assert np.array_equal(_bits(res), _bits(want))                                # the residual does not need the list
    # capacity 0 with NULL lists only counts, and still writes the residual
    cnt.zero_()
    res.fill_(float("nan"))
    assert _raw_call(mg, h, dense, dict_size, sym, None, cnt, None, None, 0, res) == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == rn and np.array_equal(_bits(res), _bits(want))
    h.close()


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("shape,nonuniform", SHAPES)
def test_dequantize_add_stores_or_adds_the_dequantizers_value(shape, nonuniform, dt):
    torch, mg = _gpu()
    h = mg.Hierarchy(shape, dt, coords=nonuniform_coords(shape, dt) if nonuniform else None)
    d = torch.from_numpy(smooth_field(shape, dt)).cuda()
    dense = h.decompose(d)
    outliers = 0
    for rel, s, tol in ((True, INF, 1e-3), (False, INF, 1e-2), (True, 0.0, 1e-3)):
        eb = mg.REL if rel else mg.ABS
        norm = h.norm(d, s) if rel else 1.0
        for dict_size in DICTS:
            what = (shape, np.dtype(dt).name, rel, s, tol, dict_size)
            q, oi, ov, n = h.quantize(dense, eb, tol, s, norm, dict_size=dict_size, prep_huffman=True)
            outliers += n if dict_size == 64 else 0
            want = h.dequantize(q.clone(), eb, tol, s, norm, dict_size=dict_size, outlier_idx=oi, outlier_val=ov)
            first = h.dequantize_add(q.clone(), eb, tol, s, norm, dict_size=dict_size, outlier_idx=oi, outlier_val=ov)
            assert np.array_equal(_bits(first), _bits(want)), what
            base = dense * 0.75 - 0.125                                # (any accumulator)
            acc = base.clone()
            got = h.dequantize_add(q.clone(), eb, tol, s, norm, dict_size=dict_size, outlier_idx=oi, outlier_val=ov,
                                   acc=acc)
            assert got.data_ptr() == acc.data_ptr()
            assert np.array_equal(_bits(acc), _bits(base + want)), what
            # the scalar route: an accumulator that starts one element into its allocation
            off = _offset_view(torch, base)
            h.dequantize_add(q.clone(), eb, tol, s, norm, dict_size=dict_size, outlier_idx=oi, outlier_val=ov, acc=off)
            assert np.array_equal(_bits(off), _bits(base + want)), what
            # no dictionary shift
            q0, _, _, _ = h.quantize(dense, eb, tol, s, norm, dict_size=dict_size, prep_huffman=False)
            plain = h.dequantize_add(q0.clone(), eb, tol, s, norm, dict_size=dict_size, prep_huffman=False)
            assert np.array_equal(_bits(plain), _bits(h.dequantize(q0, eb, tol, s, norm, dict_size=dict_size,
                                                                   prep_huffman=False))), what
    assert outliers > 0, "the case must restore values from the outlier list"
    h.close()


def test_refusals_leave_the_library_usable():
    torch, mg = _gpu()
    h = mg.Hierarchy(SMALL, F32)
    dense = h.decompose(torch.from_numpy(smooth_field(SMALL, F32)).cuda())
    sym = torch.empty(SMALL, dtype=torch.uint16, device="cuda")
    res = torch.empty(SMALL, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    idx = torch.empty(16, dtype=torch.int64, device="cuda")
    val = torch.empty(16, dtype=torch.int64, device="cuda")

    def works():
        _step(h, mg, "after a refusal", dense, mg.ABS, 1e-3, INF, 1.0, 1024)

    for dict_size in (0, 1, 3, 8191, 16386, 65536):
        assert _raw_call(mg, h, dense, dict_size, sym, None, cnt, idx, val, 16, res) == MGH_ERR_INVALID_ARGUMENT, dict_size
        assert b"dict_size" in mg.load_library().mgh_last_error()
        works()
    for args in ((None, cnt, idx, val, 16, res), (sym, None, idx, val, 16, res), (sym, cnt, None, val, 16, res),
                 (sym, cnt, idx, None, 16, res), (sym, cnt, idx, val, 16, None)):
        assert _raw_call(mg, h, dense, 1024, args[0], None, *args[1:]) == MGH_ERR_INVALID_ARGUMENT, args
        works()
    assert _raw_call(mg, h, None, 1024, sym, None, cnt, idx, val, 16, res) == MGH_ERR_INVALID_ARGUMENT
    works()
    # mgh_dequantize_add: NULL integers, NULL accumulator, a count without its lists
    L = mg.load_library()
    q, oi, ov, n = h.quantize(dense, mg.ABS, 1e-3, INF, 1.0, dict_size=1024, prep_huffman=True)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    for qq, ii, vv, cc, aa in ((None, None, None, 0, res), (q, None, None, 0, None), (q, None, val, 3, res),
                               (q, idx, None, 3, res)):
        assert L.mgh_dequantize_add(h._h, p(qq), mg.ABS, 1e-3, INF, 1.0, 1024, 1, p(ii), p(vv), cc, 1, p(aa),
                                    None) == MGH_ERR_INVALID_ARGUMENT
        works()
    for dict_size in (2, 16384):  # the ends of the range are taken
        _step(h, mg, dict_size, dense, mg.ABS, 1e-2, INF, 1.0, dict_size)
    h.close()
