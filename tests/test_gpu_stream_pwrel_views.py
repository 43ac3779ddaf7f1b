"""mgh_pwrel_inverse_sampled_ on a busy NON-DEFAULT stream, with the harness of tests/stream_order.py: y' of the view
and the two packed maps of the full array are still being produced on the stream when the call is made and are
overwritten on it right behind the call; the poison is another y' and other maps of the same sizes. The expectation
is the three launches the call stands in for, run on complete inputs.

CASE_TABLE has the form of tests/test_gpu_stream_pwrel.CASE_TABLE. The entry is internal (declared in no public
header), so tests/test_stream_cases_cpu.py does not ask for it; when it becomes public its row moves into that table."""
import numpy as np
import pytest

from tests import mask_model as mm
from tests import mask_view_model as mv

pytestmark = pytest.mark.gpu

SHAPE = (34, 33, 32)
DTYPE = np.float32
LISTS = [mv.halved_nodes(e, 1) for e in SHAPE]      # -> (18, 17, 17)
CASE_TABLE = [
    ("pwrel_inverse_sampled", ("mgh_pwrel_inverse_sampled_",), ("fused3",)),
]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _inputs(seed):
    """(y' of the view, mask words, flag words) on the device, all three classes among the bits"""
    rng = np.random.default_rng(seed)
    y = rng.uniform(-100.0, 100.0, size=[len(l) for l in LISTS]).astype(DTYPE)
    cls = rng.choice(4, size=SHAPE, p=[0.4, 0.3, 0.15, 0.15])      # valid +, valid -, zeroed, non-finite
    words = lambda bits: _dev(mm.packed_words(bits).view(np.int64))
    return [_dev(y), words(cls >= 2), words((cls == 1) | (cls == 3))]


def _case_pwrel_inverse_sampled(stream):
    import torch
    import mgard_amd
    from tests import stream_order as so
    real, poison = _inputs(1), _inputs(2)
    idx = [torch.from_numpy(np.asarray(l, dtype=np.int32)).cuda() for l in LISTS]
    oshape = tuple(len(l) for l in LISTS)
    want = mgard_amd.pwrel_inverse(real[0].clone(), mgard_amd.mask_sample(real[1], SHAPE, idx, out_shape=oshape)[0],
                                   mgard_amd.mask_sample(real[2], SHAPE, idx, out_shape=oshape)[0])
    torch.cuda.synchronize()
    out = so.run_ordered(stream, real, poison, lambda d, m, f: mgard_amd.pwrel_inverse_sampled(d.clone(), m, f, SHAPE, idx))
    assert np.array_equal(mm.int_view(out.cpu().numpy()), mm.int_view(want.cpu().numpy()))
    assert np.isnan(want.cpu().numpy()).any() and (want.cpu().numpy() == 0).any()


@pytest.mark.parametrize("name", [n for n, _, _ in CASE_TABLE])
def test_entry_point_in_stream_order(name):
    from tests.test_gpu_stream_order import _side_stream
    globals()["_case_" + name](_side_stream())


@pytest.mark.parametrize("name", [n for n, _, _ in CASE_TABLE])
def test_default_stream_results_unchanged(name):
    """The same case on the default stream: a failure above that does not show here is the stream's."""
    import torch
    globals()["_case_" + name](torch.cuda.default_stream())
