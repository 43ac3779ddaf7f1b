"""GPU tests of the three low-level calls of the precision layers in level order:
mgh_quantize_residual_linear, mgh_dequantize_add_linear (k_dequantize_add_linear) and mgh_recompose_linear_to_level.

The reference is built from the stand-alone stages, never from the code under test: mgh_quantize(prep_huffman = 1),
mgh_level_linearize, mgh_quantize_symbols_residual's residual, mgh_dequantize_add, mgh_recompose_to_level and torch
indexing with the permutation mgh_level_linearize gives for arange(n). Every comparison is an equality of integers
or of bits."""
import numpy as np
import pytest

from tests.test_gpu_layers import _bits, _sorted_pairs, _tols
from tests.test_gpu_target import FUSED3, SMALL
from tests.util import nonuniform_coords, smooth_field

pytestmark = pytest.mark.gpu

INF = float("inf")
F32, F64 = np.float32, np.float64
HUFFMAN_ZSTD = 2
# shape, type, REL, s, dictionary, non-uniform, configuration, decades: the rows tests/test_gpu_target.py's ACH_CASES
# has for these shapes (the decades are its), with the options the level-ordered layers are asked to cover
CASES = [
    ((1001,), F64, False, INF, 64, False, {}, (-2.5, -0.5)),        # N_l odd: vectors straddle levels, windows misaligned
    ((65, 40), F32, True, INF, 256, True, {}, (-1.0, 1.0)),
    (SMALL, F32, False, INF, 1024, True, {}, (-1.0, 1.0)),
    (FUSED3, F32, True, INF, 1024, False, {}, (-1.5, 0.5)),          # even extents: the fine / 2 branch of the order
    (FUSED3, F64, False, INF, 1024, False, {}, (-1.5, 0.5)),
    (FUSED3, F32, True, 0.0, 1024, False, {}, (-2.5, -0.5)),
    (FUSED3, F32, True, INF, 1024, False, {"lossless": HUFFMAN_ZSTD}, (-2.5, -0.5)),
    ((5, 9, 9, 17), F32, False, INF, 1024, False, {}, (-0.5, 1.0)),
    ((3, 3, 5, 5, 9), F64, True, INF, 1024, False, {}, (-0.5, 1.0)),
]
IDS = ["x".join(map(str, c[0])) + "-" + np.dtype(c[1]).name + ("-s0" if c[3] == 0.0 else "") + ("-zstd" if c[6] else "")
       for c in CASES]
KERNEL_CASES = [c for c in CASES if not c[6]]   # (the lossless stage is no part of these calls)
KERNEL_IDS = [i for i, c in zip(IDS, CASES) if not c[6]]
GUARD = 12345.678


def _gpu():
    import torch
    import mgard_amd
    return torch, mgard_amd


class Stage:
    """One case: hierarchy, coefficients, norm, the permutation of the level-linearised order, the level offsets."""

    def __init__(self, shape, dt, rel, s, dict_size, nonuniform):
        torch, mg = _gpu()
        self.shape, self.dt, self.s, self.dict = shape, dt, s, dict_size
        self.mode = mg.REL if rel else mg.ABS
        self.h = h = mg.Hierarchy(shape, dt, coords=nonuniform_coords(shape, dt) if nonuniform else None)
        self.n = int(np.prod(shape))
        d = torch.from_numpy(smooth_field(shape, dt)).cuda()
        self.norm = h.norm(d, s) if rel else 1.0
        self.coeff = h.decompose(d)
        # perm[p] = the array-order index of linearised position p
        self.perm = h.level_linearize(torch.arange(self.n, dtype=torch.int64, device="cuda").reshape(shape)).reshape(-1)
        self.L = h.l_target
        self.N = [int(np.prod(h.level_shape(l))) for l in range(self.L + 1)]

    def to_linear(self, a):
        return a.reshape(-1)[self.perm]

    def close(self):
        self.h.close()


@pytest.mark.parametrize("shape,dt,rel,s,dict_size,nonuniform,extra,decades", KERNEL_CASES, ids=KERNEL_IDS)
def test_quantize_residual_linear_is_quantize_linearize_and_the_residual(shape, dt, rel, s, dict_size, nonuniform, extra,
                                                                         decades):
    torch, mg = _gpu()
    S = Stage(shape, dt, rel, s, dict_size, nonuniform)
    h = S.h
    r = S.coeff
    outliers = 0
    for tol in _tols(decades):
        q, oi, ov, n = h.quantize(r, S.mode, tol, s, S.norm, dict_size=dict_size, prep_huffman=True)
        oi_lin = oi.clone()
        want_lin = h.level_linearize(q, outlier_idx=oi_lin).reshape(-1)
        _, _, _, _, want_res = h.quantize_symbols_residual(r, S.mode, tol, s, S.norm, dict_size=dict_size)
        lin, gi, gv, res = h.quantize_residual_linear(r, S.mode, tol, s, S.norm, dict_size=dict_size)
        assert np.array_equal(lin.cpu().numpy(), want_lin.cpu().numpy()), tol
        wi, wv = _sorted_pairs(oi_lin, ov)
        si, sv = _sorted_pairs(gi, gv)
        assert n == gi.numel() and np.array_equal(si, wi) and np.array_equal(sv, wv), tol
        assert np.array_equal(_bits(res), _bits(want_res)), tol
        # in place over the coefficients
        again = r.clone()
        lin2, _, _, res2 = h.quantize_residual_linear(again, S.mode, tol, s, S.norm, dict_size=dict_size, out=again)
        assert res2.data_ptr() == again.data_ptr() and np.array_equal(_bits(again), _bits(want_res)), tol
        assert np.array_equal(lin2.cpu().numpy(), want_lin.cpu().numpy()), tol
        outliers += n
        r = want_res
    if dict_size == 64:
        assert outliers > 0, "the dictionary of 64 sends values through the list"
    S.close()


def _windows(S):
    """(first, count): the whole array, one window per level, a window inside the finest level at odd offsets, and
    one across a level boundary that starts and ends at odd offsets."""
    N, n = S.N, S.n
    w = [(0, n)] + [(N[l - 1] if l else 0, N[l] - (N[l - 1] if l else 0)) for l in range(S.L + 1)]
    lo = N[S.L - 1] + (N[S.L] - N[S.L - 1]) // 3
    lo += 1 - lo % 2
    hi = N[S.L] - 2
    hi -= 1 - hi % 2
    assert lo < hi
    w.append((lo, hi - lo))
    if S.L >= 2:
        a, b = N[S.L - 2] + 1, N[S.L - 1] + 7
        a, b = a + 1 - a % 2, b + 1 - b % 2
        w.append((a, b - a))
    return w


@pytest.mark.parametrize("shape,dt,rel,s,dict_size,nonuniform,extra,decades", KERNEL_CASES, ids=KERNEL_IDS)
def test_dequantize_add_linear_is_dequantize_add_in_the_linear_order(shape, dt, rel, s, dict_size, nonuniform, extra,
                                                                     decades):
    torch, mg = _gpu()
    S = Stage(shape, dt, rel, s, dict_size, nonuniform)
    h = S.h
    tdt = torch.float32 if dt == F32 else torch.float64
    seen_outliers = 0
    # (the first tolerance of the case, and a tight one that sends more values through the list)
    for tol in (_tols(decades)[0], _tols(decades)[3]):
        q, oi, ov, _ = h.quantize(S.coeff, S.mode, tol, s, S.norm, dict_size=dict_size, prep_huffman=True)
        oi_lin = oi.clone()
        lin = h.level_linearize(q, outlier_idx=oi_lin).reshape(-1)
        seen_outliers += int(oi.numel())
        kw = dict(dict_size=dict_size, outlier_idx=oi, outlier_val=ov)
        lkw = dict(dict_size=dict_size, outlier_idx=oi_lin, outlier_val=ov)
        stored = S.to_linear(h.dequantize_add(q.clone(), S.mode, tol, s, S.norm, **kw))
        base = torch.from_numpy(smooth_field(shape, dt)[::-1].copy()).cuda() * 3 + 1
        added = S.to_linear(h.dequantize_add(q.clone(), S.mode, tol, s, S.norm, acc=base.clone(), **kw))
        base_lin = S.to_linear(base)
        for first, count in _windows(S):
            for store, want in ((True, stored), (False, added)):
                start = torch.full((S.n,), GUARD, dtype=tdt, device="cuda") if store else base_lin.clone()
                acc = start.clone()
                # a window of its own allocation, and one that is a view at an odd offset (misaligned integers)
                for pad in (0, 1):
                    acc.copy_(start)
                    buf = torch.zeros(count + pad, dtype=torch.int64, device="cuda")
                    win = buf[pad:]
                    win.copy_(lin[first:first + count])
                    got = h.dequantize_add_linear(win, first, acc, S.mode, tol, s, S.norm, store=store, **lkw)
                    assert got.data_ptr() == acc.data_ptr()
                    inside = slice(first, first + count)
                    assert np.array_equal(_bits(acc[inside]), _bits(want[inside])), (tol, first, count, store, pad)
                    assert np.array_equal(_bits(acc[:first]), _bits(start[:first])), (tol, first, count, store, pad)
                    assert np.array_equal(_bits(acc[first + count:]), _bits(start[first + count:])), (tol, first, count, store)
        # no dictionary shift, no list
        q0, _, _, _ = h.quantize(S.coeff, S.mode, tol, s, S.norm, dict_size=dict_size, prep_huffman=False)
        lin0 = h.level_linearize(q0).reshape(-1)
        want0 = S.to_linear(h.dequantize_add(q0.clone(), S.mode, tol, s, S.norm, dict_size=dict_size, prep_huffman=False))
        acc = torch.empty(S.n, dtype=tdt, device="cuda")
        h.dequantize_add_linear(lin0.clone(), 0, acc, S.mode, tol, s, S.norm, dict_size=dict_size, prep_huffman=False,
                                store=True)
        assert np.array_equal(_bits(acc), _bits(want0)), tol
    if dict_size == 64:
        assert seen_outliers > 0
    # refusals: an empty window, one that leaves the array
    L = mg.load_library()
    import ctypes as C
    acc = torch.zeros(S.n, dtype=tdt, device="cuda")
    win = torch.zeros(8, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    for first, count in ((0, 0), (S.n, 1), (S.n - 4, 5)):
        assert L.mgh_dequantize_add_linear(h._h, p(win), first, count, S.mode, 1e-3, s, S.norm, dict_size, 1, None, None, 0, 1,
                                           p(acc), None) == -1, (first, count)
    assert not acc.any()
    S.close()


@pytest.mark.parametrize("shape,dt,rel,s,dict_size,nonuniform,extra,decades", KERNEL_CASES, ids=KERNEL_IDS)
def test_recompose_linear_to_level_is_recompose_to_level(shape, dt, rel, s, dict_size, nonuniform, extra, decades):
    torch, mg = _gpu()
    S = Stage(shape, dt, rel, s, dict_size, nonuniform)
    h = S.h
    lin = S.to_linear(S.coeff).contiguous()
    keep = lin.clone()
    for level in range(S.L + 1):
        want = h.recompose(S.coeff, level=level)
        # the head alone, in a buffer that ends where the head ends
        head = lin[:S.N[level]].clone()
        got = h.recompose_linear_to_level(head, level)
        assert tuple(got.shape) == tuple(h.level_shape(level))
        assert np.array_equal(_bits(got), _bits(want)), level
        assert np.array_equal(_bits(h.recompose_linear_to_level(lin, level)), _bits(want)), level
    assert np.array_equal(_bits(h.recompose_linear_to_level(lin, S.L)), _bits(h.recompose(S.coeff)))
    assert np.array_equal(_bits(lin), _bits(keep)), "the accumulator is not modified"
    S.close()
