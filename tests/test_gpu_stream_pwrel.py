"""The pointwise relative bound on a busy NON-DEFAULT stream, with the harness of tests/stream_order.py: the three
streaming passes (mgh_pwrel_forward_ / mgh_pwrel_inverse_ / mgh_compare_pwrel_) and the four container calls
(mgh_compress_pwrel / mgh_decompress_pwrel / mgh_pwrel_info / mgh_verify_pwrel). The inputs are still being produced
on the stream when the call is made and are overwritten on it right behind the call; the poison is another field,
other bitmaps, another buffer of the same size. The expectations are tests/pwrel_model.py's.

CASE_TABLE has the form of tests/test_gpu_stream_order.CASE_TABLE. The three passes are internal (declared in no
public header), so tests/test_stream_cases_cpu.py does not ask for them; when they become public their rows move into
that table."""
import numpy as np
import pytest

from tests import mask_model as mm
from tests import pwrel_model as pm
from tests import stream_order as so

pytestmark = pytest.mark.gpu

SHAPE = (34, 33, 32)
DTYPE = np.float32
FLOOR = float(np.float32(1e-20))
EPS = 1e-3
CASE_TABLE = [
    ("pwrel_forward", ("mgh_pwrel_forward_",), ("fused3",)),
    ("pwrel_inverse", ("mgh_pwrel_inverse_",), ("fused3",)),
    ("compare_pwrel", ("mgh_compare_pwrel_",), ("fused3",)),
    ("compress_pwrel", ("mgh_compress_pwrel",), ("fused3",)),
    ("decompress_pwrel", ("mgh_decompress_pwrel", "mgh_pwrel_info"), ("fused3",)),
    ("verify_pwrel", ("mgh_verify_pwrel",), ("fused3",)),
]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _field(poison=False):
    x = pm.smooth_field(SHAPE, DTYPE, abs_floor=FLOOR)
    if poison:      # another valid field: other magnitudes, other signs, the special values elsewhere
        with np.errstate(over="ignore"):      # (its largest finite values become +-Inf: still a valid input)
            x = np.ascontiguousarray((-x[::-1, ::-1, ::-1] * DTYPE(3.0)).astype(DTYPE))
    return x


def _words(bits):
    return _dev(mm.packed_words(bits).view(np.int64))


def _case_pwrel_forward(stream):
    import mgard_amd
    x = _field()
    y, mw, fw, st = so.run_ordered(stream, [_dev(x)], [_dev(_field(True))], lambda d: mgard_amd.pwrel_forward(d, FLOOR))
    mask, flag = pm.bitmaps(x, FLOOR)
    assert np.array_equal(mw.cpu().numpy().view(np.uint64), mm.packed_words(mask))
    assert np.array_equal(fw.cpu().numpy().view(np.uint64), mm.packed_words(flag))
    assert (st.n_masked, st.n_flag) == (int(mask.sum()), int(flag.sum()))
    want = pm.forward(x, FLOOR)
    assert np.max(np.abs(y.cpu().numpy()[~mask].astype(np.float64) - want[~mask])) <= pm.ulp(DTYPE, 128.0)


def _case_pwrel_inverse(stream):
    import mgard_amd
    x, p = _field(), _field(True)
    (mask, flag), (pmask, pflag) = pm.bitmaps(x, FLOOR), pm.bitmaps(p, FLOOR)
    y, py = pm.forward(x, FLOOR), pm.forward(p, FLOOR)
    out = so.run_ordered(stream, [_dev(y), _words(mask), _words(flag)], [_dev(py), _words(pmask), _words(pflag)],
                         lambda d, m, f: mgard_amd.pwrel_inverse(d.clone(), m, f))
    want = pm.inverse(y, mask, flag)
    out = out.cpu().numpy()
    assert np.array_equal(np.isnan(out), np.isnan(want)) and np.array_equal(np.signbit(out), np.signbit(want))
    ok = ~np.isnan(want) & (want != 0)
    assert np.all(out[mask & ~flag] == 0)
    assert np.max(np.abs(out[ok].astype(np.float64) - want[ok]) / np.abs(want[ok].astype(np.float64))) <= 2 * np.finfo(DTYPE).eps


def _recon(x):
    mask, flag = pm.bitmaps(x, FLOOR)
    r = pm.inverse(pm.forward(x, FLOOR), mask, flag)
    return (r * DTYPE(0.9995)).astype(DTYPE)     # (towards zero: the largest finite value stays finite)


def _case_compare_pwrel(stream):
    import mgard_amd
    x, p = _field(), _field(True)
    r = _recon(x)
    got = so.run_ordered(stream, [_dev(x), _dev(r)], [_dev(p), _dev(_recon(x) * DTYPE(-1))],
                         lambda a, b: mgard_amd.compare_pwrel(a, b, FLOOR))
    want = pm.compare(x, r, FLOOR)
    assert got.max_rel_err == want["max_rel_err"] and (got.n_valid, got.n_zeroed, got.n_nonfinite) == \
        (want["n_valid"], want["n_zeroed"], want["n_nonfinite"])
    assert (got.n_class_mismatch, got.n_sign_mismatch) == (want["n_class_mismatch"], want["n_sign_mismatch"]) == (0, 0)


def _cfg():
    from mgard_amd import highlevel as hl
    return hl.Config(huff_dict_size=1024)


def _case_compress_pwrel(stream):
    from mgard_amd import highlevel as hl
    x = _field()
    buf = so.run_ordered(stream, [_dev(x)], [_dev(_field(True))], lambda d: hl.compress_pwrel(d, EPS, FLOOR, config=_cfg()))
    want = hl.compress_pwrel(_dev(x), EPS, FLOOR, config=_cfg())
    assert np.array_equal(buf.cpu().numpy(), want.cpu().numpy())


def _buffers():
    """(the buffer of the field, as many bytes that begin with the smaller buffer of another field: read in place of
    the real one they decode to other values or fail the footer's checks, and nothing else)"""
    import torch
    from mgard_amd import highlevel as hl
    real = hl.compress_pwrel(_dev(_field()), EPS, FLOOR, config=_cfg())
    poison = torch.empty_like(real)
    hl.compress_pwrel(_dev(_field(True)), 0.5, FLOOR, config=_cfg(), out=poison)
    torch.cuda.synchronize()
    return real, poison


def _case_decompress_pwrel(stream):
    from mgard_amd import highlevel as hl
    real, poison = _buffers()
    want = hl.decompress_pwrel(real, config=_cfg()).cpu().numpy()
    out, info = so.run_ordered(stream, [real], [poison], lambda b: (hl.decompress_pwrel(b, config=_cfg()), hl.pwrel_info(b)))
    assert np.array_equal(mm.int_view(out.cpu().numpy()), mm.int_view(want))
    assert (info.eps, info.abs_floor) == (EPS, FLOOR)


def _case_verify_pwrel(stream):
    from mgard_amd import highlevel as hl
    x = _field()
    real, poison = _buffers()
    want, _ = hl.verify_pwrel(real, _dev(x), config=_cfg())
    got, within = so.run_ordered(stream, [real, _dev(x)], [poison, _dev(_field(True))],
                                 lambda b, d: hl.verify_pwrel(b, d, config=_cfg()))
    assert within == 1 and got.max_rel_err == want.max_rel_err and got.n_valid == want.n_valid


@pytest.mark.parametrize("name", [n for n, _, _ in CASE_TABLE])
def test_entry_point_in_stream_order(name):
    from tests.test_gpu_stream_order import _side_stream
    globals()["_case_" + name](_side_stream())


@pytest.mark.parametrize("name", [n for n, _, _ in CASE_TABLE])
def test_default_stream_results_unchanged(name):
    """The same cases on the default stream: a failure above that does not show here is the stream's."""
    import torch
    globals()["_case_" + name](torch.cuda.default_stream())
