"""NumPy restatement of the masked readers at reduced resolution and of mgh_compare_masked_, on top of
tests/mask_model.py. The rule is sampling: a node of a level or coarsened array is masked when the element of the
full array at that node's index is masked; a position of a window is masked when that position of the array is."""
import numpy as np

from tests import mask_model as mm  # noqa: F401  (the packed words and bit views the tests use beside this)


def sample(mask, idx_lists):
    """The mask of the array whose element (i_0 ...) is element (idx_0[i_0] ...) of the full array."""
    return mask[np.ix_(*[np.asarray(l, dtype=np.int64) for l in idx_lists])]


def sample_any(mask, idx_lists):
    """sample() for lists as mgh_mask_sample_ takes them: None is the identity, and an entry outside the array gives 0
    (nothing is read for it)."""
    lists = [np.arange(e, dtype=np.int64) if l is None else np.asarray(l, dtype=np.int64)
             for l, e in zip(idx_lists, mask.shape)]
    ok = np.ones([len(l) for l in lists], dtype=bool)
    for d, (l, e) in enumerate(zip(lists, mask.shape)):
        ok &= (l < e).reshape([-1 if k == d else 1 for k in range(len(lists))])
    return sample(mask, [np.minimum(l, e - 1) for l, e in zip(lists, mask.shape)]) & ok


def halved_nodes(n, steps):
    """Index in the finest grid of the nodes after `steps` coarsenings n -> n / 2 + 1: every second node, and the last."""
    idx = list(range(n))
    for _ in range(steps):
        idx = idx[:-1:2] + [idx[-1]] if len(idx) % 2 == 0 else idx[::2]
    return idx


def sample_cases():
    """[(id, shape of the source, one list or None per dimension)]: where k_mask_sample can go wrong."""
    h = halved_nodes
    return [
        ("1d-every-second", (1000,), [list(range(0, 1000, 2))]),
        ("1d-one-output", (1000,), [[999]]),                       # a tail word with 63 dead lanes
        ("2d-rows-longer-than-a-wave", (17, 130), [h(17, 1), h(130, 1)]),          # -> (9, 66)
        ("3d-rows-shorter-than-a-wave", (34, 33, 32), [h(34, 1), h(33, 1), h(32, 1)]),  # -> (18, 17, 17)
        ("4d-mixed", (5, 6, 7, 9), [None, [0, 2, 4, 5], None, [0, 2, 4, 6, 8]]),
        ("5d-mixed", (3, 3, 4, 5, 70), [[0, 2], None, [0, 3], None, h(70, 1)]),
        ("3d-window", (34, 33, 32), [list(range(3, 8)), list(range(33)), [31]]),
        ("2d-out-of-range", (17, 130), [[0, 5, 17, 16], [0, 200, 129, 3, 130, 2 ** 32 - 1]]),
    ]


def level_lists(buf, level, config=None):
    from mgard_amd import highlevel as hl
    D = len(hl.infer(buf)[0])
    return [hl.infer_level_nodes(buf, level, d, config) for d in range(D)]


def coarsened_lists(buf, halvings, config=None):
    from mgard_amd import highlevel as hl
    D = len(hl.infer(buf)[0])
    return [hl.infer_coarsened_nodes(buf, halvings, d, config) for d in range(D)]


def window_lists(lo, ext):
    return [np.arange(a, a + e, dtype=np.int64) for a, e in zip(lo, ext)]


def masked_stats(a, b, mask):
    """mgh_error_stats of a (the reference) against b over the positions where `mask` is False, as a dict: the
    difference and its absolute value in the arrays' type, the sums in float64. A position whose difference is not
    finite is counted in `nonfinite` and takes part in nothing else; argmax is the lowest flat index of the logical
    dense array that attains max_abs_err. Everything is 0 where no position is finite."""
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    flat = np.flatnonzero(~np.ascontiguousarray(mask).reshape(-1))
    av, bv = a.reshape(-1)[flat], b.reshape(-1)[flat]
    with np.errstate(invalid="ignore", over="ignore"):
        d = av - bv
    ok = np.isfinite(d)
    out = dict(n=int(flat.size), nonfinite=int((~ok).sum()), max_abs_err=0.0, argmax=0, sum_sq_err=0.0, ref_min=0.0,
               ref_max=0.0, ref_abs_max=0.0, ref_sum_sq=0.0)
    if not ok.any():
        return out
    e = np.abs(d[ok])
    ref = av[ok]
    out["max_abs_err"] = float(e.max())
    out["argmax"] = int(flat[ok][int(np.argmax(e))])  # (argmax: the first of equals)
    out["sum_sq_err"] = float(np.sum(e.astype(np.float64) ** 2))
    out["ref_min"] = float(ref.min())
    out["ref_max"] = float(ref.max())
    out["ref_abs_max"] = float(np.abs(ref).max())
    out["ref_sum_sq"] = float(np.sum(ref.astype(np.float64) ** 2))
    return out


EXACT_FIELDS = ("n", "nonfinite", "max_abs_err", "argmax", "ref_min", "ref_max", "ref_abs_max")
SUM_FIELDS = ("sum_sq_err", "ref_sum_sq")
