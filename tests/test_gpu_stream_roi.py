"""The region of interest on a busy NON-DEFAULT stream, with the harness of tests/stream_order.py as it is: the two
streaming passes over a box (mgh_box_residual_ / mgh_box_add_) and the four container calls (mgh_compress_roi /
mgh_decompress_roi / mgh_roi_info / mgh_verify_roi). The inputs are still being produced on the stream when the call
is made and are overwritten on it right behind the call; the poison is another field, another residual, another
buffer of the same size.

CASE_TABLE has the form of tests/test_gpu_stream_order.CASE_TABLE. The two passes are internal (declared in no public
header), so tests/test_stream_cases_cpu.py does not ask for them."""
import numpy as np
import pytest

from tests import stream_order as so
from tests.test_gpu_roi import BOX, SHAPE, TOL, TOL_BOX, field, same_buffers

pytestmark = pytest.mark.gpu

DTYPE = np.float32
CASE_TABLE = [
    ("box_residual", ("mgh_box_residual_",), ("fused3",)),
    ("box_add", ("mgh_box_add_",), ("fused3",)),
    ("compress_roi", ("mgh_compress_roi",), ("fused3",)),
    ("decompress_roi", ("mgh_decompress_roi", "mgh_roi_info"), ("fused3",)),
    ("verify_roi", ("mgh_verify_roi",), ("fused3",)),
]
BOXES = [(BOX[0], BOX[1], TOL_BOX)]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ints(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _sl():
    return tuple(slice(a, a + e) for a, e in zip(*BOX))


def _field(poison=False):
    x = field(SHAPE, DTYPE)
    return np.ascontiguousarray((-x[::-1, ::-1, ::-1] * DTYPE(3.0)).astype(DTYPE)) if poison else x


def _base(x):
    return (x * DTYPE(1.001)).astype(DTYPE)


def _cfg():
    from mgard_amd import highlevel as hl
    return hl.Config(huff_dict_size=1024)


def _case_box_residual(stream):
    import mgard_amd
    x, p = _field(), _field(True)
    b = _base(x)
    r, st = so.run_ordered(stream, [_dev(x), _dev(b)], [_dev(p), _dev(_base(p) * DTYPE(2))],
                           lambda dx, db: mgard_amd.box_residual(dx, db, *BOX))
    want = x[_sl()] - b[_sl()]
    assert np.array_equal(_ints(r.cpu().numpy()), _ints(want))
    assert (st.max_abs_r, st.max_abs_x, st.n_nonfinite) == (float(np.abs(want).max()), float(np.abs(x[_sl()]).max()), 0)


def _case_box_add(stream):
    import mgard_amd
    x, p = _field(), _field(True)
    r, pr = (x[_sl()] * DTYPE(1e-3)).astype(DTYPE), (p[_sl()] * DTYPE(0.5)).astype(DTYPE)
    out = so.run_ordered(stream, [_dev(x), _dev(r)], [_dev(p), _dev(pr)], lambda d, dr: mgard_amd.box_add(d.clone(), dr, BOX[0]))
    want = x.copy()
    want[_sl()] = x[_sl()] + r
    assert np.array_equal(_ints(out.cpu().numpy()), _ints(want))


def _case_compress_roi(stream):
    from mgard_amd import highlevel as hl
    x = _field()
    buf = so.run_ordered(stream, [_dev(x)], [_dev(_field(True))], lambda d: hl.compress_roi(d, TOL, BOXES, config=_cfg()))
    want = hl.compress_roi(_dev(x), TOL, BOXES, config=_cfg())
    same_buffers(buf.cpu().numpy(), want.cpu().numpy(), x, _cfg())     # (up to the order of the outlier pairs)


def _buffers():
    """(the buffer of the field, as many bytes that begin with the smaller buffer of another field: read in place of
    the real one they decode to other values or fail the footer's checks, and nothing else)"""
    import torch
    from mgard_amd import highlevel as hl
    real = hl.compress_roi(_dev(_field()), TOL, BOXES, config=_cfg())
    poison = torch.zeros_like(real)
    small = hl.compress_roi(_dev(_field(True)), 0.1, [(BOX[0], BOX[1], 0.05)], config=_cfg())
    assert small.numel() <= real.numel()
    poison[:small.numel()] = small
    torch.cuda.synchronize()
    return real, poison


def _case_decompress_roi(stream):
    from mgard_amd import highlevel as hl
    real, poison = _buffers()
    want = hl.decompress_roi(real, config=_cfg()).cpu().numpy()
    out, info = so.run_ordered(stream, [real], [poison], lambda b: (hl.decompress_roi(b, config=_cfg()), hl.roi_info(b)))
    assert np.array_equal(_ints(out.cpu().numpy()), _ints(want))
    assert [(b[0], b[1], b[2]) for b in info.boxes] == [(BOX[0], BOX[1], TOL_BOX)]


def _case_verify_roi(stream):
    from mgard_amd import highlevel as hl
    x = _field()
    real, poison = _buffers()
    want, want_box = hl.verify_roi(real, _dev(x), config=_cfg())
    got, got_box = so.run_ordered(stream, [real, _dev(x)], [poison, _dev(_field(True))],
                                  lambda b, d: hl.verify_roi(b, d, config=_cfg()))
    assert got.within == 1 and got.stats.max_abs_err == want.stats.max_abs_err
    assert got_box[0].within == 1 and got_box[0].stats.max_abs_err == want_box[0].stats.max_abs_err


@pytest.mark.parametrize("name", [n for n, _, _ in CASE_TABLE])
def test_entry_point_in_stream_order(name):
    from tests.test_gpu_stream_order import _side_stream
    globals()["_case_" + name](_side_stream())


@pytest.mark.parametrize("name", [n for n, _, _ in CASE_TABLE])
def test_default_stream_results_unchanged(name):
    """The same cases on the default stream: a failure above that does not show here is the stream's."""
    import torch
    globals()["_case_" + name](torch.cuda.default_stream())
