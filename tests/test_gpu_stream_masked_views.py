"""mgh_mask_sample_ and mgh_compare_masked_ on a busy NON-DEFAULT stream, with the harness of tests/stream_order.py:
the mask, the index lists and the arrays are still being produced on the stream when the call is made and are
overwritten on it right behind the call. The poison is another mask, other lists and other arrays, as
tests/test_gpu_stream_order.py does for the other mgh_mask_* calls; the expectations are tests/mask_view_model.py's.

CASE_TABLE has the form of tests/test_gpu_stream_order.CASE_TABLE. The two entry points are internal (declared in
no public header), so tests/test_stream_cases_cpu.py does not ask for them; when they become public their rows
move into that table."""
import numpy as np
import pytest

from tests import mask_model as mm
from tests import mask_view_model as mv
from tests import stream_order as so
from tests.util import inside_field

pytestmark = pytest.mark.gpu

SHAPE = (34, 33, 32)
# (case, the entry points it runs, routes: these calls need no hierarchy)
CASE_TABLE = [
    ("mask_sample", ("mgh_mask_sample_",), ("fused3",)),
    ("compare_masked", ("mgh_compare_masked_",), ("fused3",)),
]


def _mask(seed):
    return np.random.default_rng(seed).random(SHAPE) < 0.3


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _words(mask):
    return _dev(mm.packed_words(mask).view(np.int64))


def _lists(kind):
    """The node lists of one halving, or (the poison) the first nodes of each dimension: the same lengths."""
    real = [mv.halved_nodes(e, 1) for e in SHAPE]
    return real if kind == "real" else [list(range(len(l))) for l in real]


def _case_mask_sample(stream):
    import mgard_amd
    mask = _mask(1)
    as_dev = lambda ls: [_dev(np.asarray(l, dtype=np.int32)) for l in ls]
    inputs = [_words(mask)] + as_dev(_lists("real"))
    poison = [_words(_mask(2))] + as_dev(_lists("poison"))
    out_words, count = so.run_ordered(stream, inputs, poison, lambda w, *ls: mgard_amd.mask_sample(w, SHAPE, list(ls)))
    want = mv.sample(mask, _lists("real"))
    assert np.array_equal(out_words.cpu().numpy().view(np.uint64), mm.packed_words(want)), "mask_sample"
    assert count == int(want.sum())


def _case_compare_masked(stream):
    import mgard_amd
    a = inside_field(SHAPE, np.float32)
    b = (a + np.random.default_rng(3).normal(0, 1e-3, SHAPE)).astype(np.float32)
    pa = (a * np.float32(1.5) + np.float32(0.25)).astype(np.float32)
    pb = (a - np.float32(0.125)).astype(np.float32)
    mask = _mask(1)
    got = so.run_ordered(stream, [_dev(a), _dev(b), _words(mask)], [_dev(pa), _dev(pb), _words(_mask(2))],
                         lambda x, y, w: mgard_amd.compare_masked(x, y, w))
    want = mv.masked_stats(a, b, mask)
    for f in mv.EXACT_FIELDS:
        g, w = getattr(got, f), want[f]
        assert (g == w) if isinstance(w, int) else (np.float64(g).view(np.uint64) == np.float64(w).view(np.uint64)), f
    for f in mv.SUM_FIELDS:
        assert abs(getattr(got, f) - want[f]) <= 1e-12 * want[f], f


@pytest.mark.parametrize("name", [n for n, _, _ in CASE_TABLE])
def test_entry_point_in_stream_order(name):
    from tests.test_gpu_stream_order import _side_stream
    globals()["_case_" + name](_side_stream())


@pytest.mark.parametrize("name", [n for n, _, _ in CASE_TABLE])
def test_default_stream_results_unchanged(name):
    """The same cases on the default stream: a failure above that does not show here is the stream's."""
    import torch
    globals()["_case_" + name](torch.cuda.default_stream())
