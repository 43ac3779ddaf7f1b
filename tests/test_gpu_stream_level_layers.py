"""The three low-level calls of the precision layers in level order on a busy NON-DEFAULT stream, with the harness
of tests/stream_order.py (as tests/test_gpu_stream_pwrel.py): the inputs are still being produced on the stream when
the call is made and are overwritten on it right behind the call; the poison is another field's coefficients,
integers and accumulator. The expectations come from the stand-alone stages on the default stream.

CASE_TABLE has the form of tests/test_gpu_stream_order.CASE_TABLE. The three calls are declared in
include/mgard_hip_level_layers.h, which tests/test_level_layers_abi_cpu.py holds against this table the way
tests/test_stream_cases_cpu.py holds the two main headers against that one."""
import numpy as np
import pytest

from tests import stream_order as so
from tests.util import smooth_field

pytestmark = pytest.mark.gpu

SHAPE = (34, 33, 32)
DTYPE = np.float32
INF = float("inf")
TOL, DICT = 1e-3, 1024
CASE_TABLE = [
    ("quantize_residual_linear", ("mgh_quantize_residual_linear",), ("fused3",)),
    ("dequantize_add_linear", ("mgh_dequantize_add_linear",), ("fused3",)),
    ("recompose_linear_to_level", ("mgh_recompose_linear_to_level",), ("fused3",)),
]


def _bits(t):
    return t.contiguous().cpu().numpy().view(np.int32)


class _Ref:
    """Hierarchy, the coefficients of the field and of the poison field, the norm -- made on the default stream."""

    def __init__(self):
        import torch
        import mgard_amd as mg
        self.mg = mg
        self.h = mg.Hierarchy(SHAPE, DTYPE)
        u = torch.from_numpy(smooth_field(SHAPE, DTYPE)).cuda()
        p = torch.from_numpy(np.ascontiguousarray(-2.0 * smooth_field(SHAPE, DTYPE)[::-1, ::-1, ::-1])).cuda()
        self.norm = self.h.norm(u, INF)
        self.coeff, self.poison = self.h.decompose(u), self.h.decompose(p)
        self.n = u.numel()
        self.perm = self.h.level_linearize(torch.arange(self.n, dtype=torch.int64, device="cuda").reshape(SHAPE)).reshape(-1)
        torch.cuda.synchronize()

    def integers(self, coeff):
        """(level-linearised integers, linearised outlier indices, values) of mgh_quantize + mgh_level_linearize"""
        q, oi, ov, _ = self.h.quantize(coeff, self.mg.REL, TOL, INF, self.norm, dict_size=DICT, prep_huffman=True)
        lin = self.h.level_linearize(q, outlier_idx=oi).reshape(-1)
        return q, lin, oi, ov


def _case_quantize_residual_linear(stream):
    import torch
    R = _Ref()
    _, want_lin, wi, wv = R.integers(R.coeff)
    want_res = R.h.quantize_symbols_residual(R.coeff, R.mg.REL, TOL, INF, R.norm, dict_size=DICT)[4]
    torch.cuda.synchronize()
    lin, gi, gv, res = so.run_ordered(stream, [R.coeff], [R.poison],
                                      lambda c: R.h.quantize_residual_linear(c, R.mg.REL, TOL, INF, R.norm, dict_size=DICT))
    assert np.array_equal(lin.cpu().numpy(), want_lin.cpu().numpy())
    assert np.array_equal(_bits(res), _bits(want_res))
    a, b = np.argsort(gi.cpu().numpy(), kind="stable"), np.argsort(wi.cpu().numpy(), kind="stable")
    assert np.array_equal(gi.cpu().numpy()[a], wi.cpu().numpy()[b]) and np.array_equal(gv.cpu().numpy()[a], wv.cpu().numpy()[b])
    R.h.close()


def _case_dequantize_add_linear(stream):
    import torch
    R = _Ref()
    q, lin, oi, ov = R.integers(R.coeff)
    _, plin, _, _ = R.integers(R.poison)
    kw = dict(dict_size=DICT, outlier_val=ov)
    base = R.coeff.reshape(-1)[R.perm].contiguous()             # the accumulator so far, level-linearised
    pbase = R.poison.reshape(-1)[R.perm].contiguous()
    oi_arr = torch.empty_like(oi)                                # the same list at array positions
    oi_arr.copy_(R.perm[oi])
    want = R.h.dequantize_add(q.clone(), R.mg.REL, TOL, INF, R.norm, acc=R.coeff.clone(), outlier_idx=oi_arr, **kw)
    want = want.reshape(-1)[R.perm]
    N = [int(np.prod(R.h.level_shape(l))) for l in range(R.h.l_target + 1)]
    first = N[-2] - 3                                            # a window across the last level boundary
    count = R.n - first - 5
    torch.cuda.synchronize()

    def call(w, acc):
        R.h.dequantize_add_linear(w, first, acc, R.mg.REL, TOL, INF, R.norm, outlier_idx=oi, **kw)
        return acc.clone()

    got = so.run_ordered(stream, [lin[first:first + count].clone(), base], [plin[first:first + count].clone(), pbase], call)
    inside = slice(first, first + count)
    assert np.array_equal(_bits(got[inside]), _bits(want[inside]))
    assert np.array_equal(_bits(got[:first]), _bits(base[:first])) and np.array_equal(_bits(got[first + count:]),
                                                                                      _bits(base[first + count:]))
    R.h.close()


def _case_recompose_linear_to_level(stream):
    import torch
    R = _Ref()
    level = R.h.l_target - 1
    want = R.h.recompose(R.coeff, level=level)
    torch.cuda.synchronize()
    got = so.run_ordered(stream, [R.coeff.reshape(-1)[R.perm].contiguous()], [R.poison.reshape(-1)[R.perm].contiguous()],
                         lambda a: R.h.recompose_linear_to_level(a, level))
    assert np.array_equal(_bits(got), _bits(want))
    R.h.close()


@pytest.mark.parametrize("name", [n for n, _, _ in CASE_TABLE])
def test_entry_point_in_stream_order(name):
    from tests.test_gpu_stream_order import _side_stream
    globals()["_case_" + name](_side_stream())


@pytest.mark.parametrize("name", [n for n, _, _ in CASE_TABLE])
def test_default_stream_results_unchanged(name):
    """The same cases on the default stream: a failure above that does not show here is the stream's."""
    import torch
    globals()["_case_" + name](torch.cuda.default_stream())
