"""Masked buffers in the reduced-resolution, preview and verify readers against tests/mask_view_model.py.

The writer set-up is that of tests/test_gpu_masked.py (inside_field, TOL = 3e-2, huff_dict_size = 1024, (34, 33, 32)
float32 and (17, 130) float64, the `ball` mask as NaN / +-Inf and the `random30` mask as 1e20 restored as -9999: lossy
records), plus the decomposed `block` case of tests/test_gpu_coarsened.py, (70, 45, 37) in blocks of 33, with a
random mask. For every view -- every level, every number of halvings, previews, windows -- the output holds
restore_value's bits where the model's SAMPLED mask is set and the plain reader's bits of buf[:C] everywhere else."""
import numpy as np
import pytest

from tests import mask_model as mm
from tests import mask_view_model as mv
from tests.test_coarsened_cpu import BLOCK
from tests.test_gpu_masked import TOL, _marked
from tests.util import inside_field

INF = float("inf")
# name: (shape, dtype, mask kind, decomposed, windows)
CASES = {
    "34x33x32-f32-ball": ((34, 33, 32), np.float32, "ball", False, [((3, 0, 31), (5, 33, 1))]),
    "34x33x32-f32-random30": ((34, 33, 32), np.float32, "random30", False, [((3, 0, 31), (5, 33, 1))]),
    "17x130-f64-ball": ((17, 130), np.float64, "ball", False, [((2, 60), (9, 70))]),
    "17x130-f64-random30": ((17, 130), np.float64, "random30", False, [((2, 60), (9, 70))]),
    # (the second window crosses the block borders at 33 along the first and the last dimension)
    "block-70x45x37-f32": ((70, 45, 37), np.float32, "random30", True, [((3, 0, 31), (5, 33, 1)), ((30, 10, 30), (8, 20, 7))]),
}
SIZED = [k for k, v in CASES.items() if not v[3]]
_made = {}


def _cfg(name):
    from mgard_amd import highlevel as hl
    if CASES[name][3]:
        return hl.Config(huff_dict_size=1024, domain_decomposition=BLOCK, block_size=33)
    return hl.Config(huff_dict_size=1024)


def _case(name, mode_s="REL-inf"):
    """(data with its marks, mask, keywords, host buffer, C), made once."""
    import mgard_amd
    from mgard_amd import highlevel as hl
    key = (name, mode_s)
    if key not in _made:
        shape, dtype, kind, _, _ = CASES[name]
        data, mask, kw = _marked(shape, dtype, kind)
        mode = mgard_amd.REL if mode_s.startswith("REL") else mgard_amd.ABS
        s = INF if mode_s.endswith("inf") else 0.0
        buf = hl.compress_masked(data, TOL, s, mode, config=_cfg(name), **kw)
        _made[key] = (data, mask, kw, buf, int(hl.masked_info(buf).container_size))
    return _made[key]


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _where(buf, where):
    import torch
    return buf if where == "host" else torch.from_numpy(buf).cuda()


def _assert_view(out, plain, smask, dtype, restore_value, what):
    out, plain = _np(out), _np(plain)
    assert out.dtype == dtype and out.shape == smask.shape == plain.shape, what
    bits = mm.int_view(np.array([restore_value], dtype=dtype))[0]
    assert np.all(mm.int_view(out)[smask] == bits), what
    assert np.array_equal(mm.int_view(out)[~smask], mm.int_view(plain)[~smask]), what


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", list(CASES))
def test_views_hold_restore_bits_at_the_sampled_mask_and_the_plain_reader_elsewhere(name, where):
    import torch
    from mgard_amd import highlevel as hl
    shape, dtype, kind, decomposed, windows = CASES[name]
    data, mask, kw, hbuf, C = _case(name)
    cfg = _cfg(name)
    buf = _where(hbuf, where)
    rv = kw["restore_value"]
    seen_masked = 0
    # every level (containers with one subdomain)
    if not decomposed:
        L = hl.infer_level(hbuf[:C], None, cfg)[1]
        for level in range(L + 1):
            smask = mv.sample(mask, mv.level_lists(hbuf[:C], level, cfg))
            out = hl.decompress_masked(buf, config=cfg, level=level)
            assert isinstance(out, np.ndarray) == (where == "host")
            _assert_view(out, hl.decompress(buf[:C], config=cfg, level=level), smask, dtype, rv, "level %d" % level)
            got = hl.decompress_mask(buf, config=cfg, level=level)
            assert got.dtype in (np.bool_, torch.bool) and np.array_equal(_np(got), smask), "mask of level %d" % level
            seen_masked += int(smask.sum())
    # every number of halvings, as the coarsened array and as the preview
    K = hl.infer_coarsened(hbuf[:C], None, cfg)[1]
    assert K >= 2
    for k in range(K + 1):
        smask = mv.sample(mask, mv.coarsened_lists(hbuf[:C], k, cfg))
        out = hl.decompress_masked(buf, config=cfg, coarsen=k)
        _assert_view(out, hl.decompress(buf[:C], config=cfg, coarsen=k), smask, dtype, rv, "coarsen %d" % k)
        assert np.array_equal(_np(hl.decompress_mask(buf, config=cfg, coarsen=k)), smask), "mask of coarsen %d" % k
        seen_masked += int(smask.sum())
        out = hl.decompress_masked_preview(buf, k, config=cfg)
        _assert_view(out, hl.decompress_preview(buf[:C], k, config=cfg), mask, dtype, rv, "preview %d" % k)
        for lo, ext in windows:
            wmask = mv.sample(mask, mv.window_lists(lo, ext))
            out = hl.decompress_masked_preview(buf, k, config=cfg, window=(lo, ext))
            _assert_view(out, hl.decompress_preview(buf[:C], k, config=cfg, window=(lo, ext)), wmask, dtype, rv,
                         "window %r of preview %d" % ((lo, ext), k))
    for lo, ext in windows:
        wmask = mv.sample(mask, mv.window_lists(lo, ext))
        assert np.array_equal(_np(hl.decompress_mask(buf, config=cfg, window=(lo, ext))), wmask), "mask of window"
    assert seen_masked > 0
    # coarsen = 0 is the full reader, and a pre-allocated output is filled in place
    full = hl.decompress_masked(buf, config=cfg)
    out = torch.empty(shape, dtype=full.dtype, device="cuda") if where == "device" else np.empty(shape, dtype=dtype)
    assert hl.decompress_masked(buf, config=cfg, coarsen=0, out=out) is out
    assert np.array_equal(mm.int_view(_np(out)), mm.int_view(_np(full)))


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("mode_s", ["REL-inf", "REL-0"])
@pytest.mark.parametrize("name", list(CASES))
def test_verify_masked_against_the_original_with_its_marks(name, mode_s, where):
    import torch
    import mgard_amd
    from mgard_amd import highlevel as hl
    shape, dtype, kind, decomposed, _ = CASES[name]
    data, mask, kw, hbuf, C = _case(name, mode_s)
    cfg = _cfg(name)
    buf = _where(hbuf, where)
    original = data if where == "host" else torch.from_numpy(data).cuda()
    v, n_masked = hl.verify_masked(buf, original, config=cfg)
    n = data.size
    print("%s %s: achieved %.3e, bound %.3e, max_abs_err %.3e, n_masked %d" % (name, mode_s, v.achieved, v.bound,
                                                                                 v.stats.max_abs_err, n_masked))
    assert v.within == 1
    assert n_masked == int(mask.sum()) and v.stats.n == n - n_masked and v.stats.nonfinite == 0
    # the statistics are compare_masked's of the original against the masked reconstruction
    back = hl.decompress_masked(torch.from_numpy(hbuf).cuda(), config=cfg)
    words = torch.from_numpy(mm.packed_words(mask).view(np.int64)).cuda()
    ref = mgard_amd.compare_masked(torch.from_numpy(data).cuda(), back, words)
    for f in mv.EXACT_FIELDS:
        g, w = getattr(v.stats, f), getattr(ref, f)
        assert (g == w) if isinstance(g, int) else (np.float64(g).view(np.uint64) == np.float64(w).view(np.uint64)), f
    if not decomposed:
        assert v.stats.max_abs_err > 0          # a lossy record: the verdict is about an error that exists
    if mode_s == "REL-0":
        assert v.bound_kind == 1 and v.achieved == float(np.sqrt(np.float64(v.stats.sum_sq_err) / n))
    else:
        assert v.bound_kind == 0 and v.achieved == v.stats.max_abs_err
    # a preview carries no bound
    vp, nm = hl.verify_masked(buf, original, config=cfg, coarsen=1)
    assert vp.within == -1 and nm == n_masked and vp.stats.n == n - n_masked and vp.stats.nonfinite == 0


@pytest.mark.gpu
def test_plain_verify_cannot_answer_for_the_marked_original():
    """Why the call exists: against the original with 1e20 (and NaN) mgh_verify of the container part fails."""
    from mgard_amd import highlevel as hl
    name = "34x33x32-f32-random30"
    data, mask, kw, buf, C = _case(name)
    v = hl.verify(buf[:C], data, config=_cfg(name))
    assert v.within == 0
    assert v.stats.nonfinite > 0 or v.stats.max_abs_err > 1e19
    vm, _ = hl.verify_masked(buf, data, config=_cfg(name))
    assert vm.within == 1 and vm.stats.ref_max < 1e19


@pytest.mark.gpu
def test_nothing_masked_is_the_plain_reader():
    import mgard_amd
    from mgard_amd import highlevel as hl
    shape, dtype = (34, 33, 32), np.float32
    data = inside_field(shape, dtype)
    cfg = hl.Config(huff_dict_size=1024)
    buf = hl.compress_masked(data, TOL, INF, mgard_amd.REL, config=cfg, fill_value=1e20)
    info = hl.masked_info(buf)
    assert info.kind == mm.NONE
    C = int(info.container_size)
    assert np.array_equal(mm.int_view(hl.decompress_masked(buf, config=cfg, coarsen=1)),
                          mm.int_view(hl.decompress(buf[:C], config=cfg, coarsen=1)))
    assert not hl.decompress_mask(buf, config=cfg, level=0).any()
    v, n_masked = hl.verify_masked(buf, data, config=cfg)
    assert v.within == 1 and n_masked == 0 and v.stats.n == data.size


@pytest.mark.gpu
def test_refusals():
    import mgard_amd
    from mgard_amd import highlevel as hl
    name = "34x33x32-f32-ball"
    data, mask, kw, buf, C = _case(name)
    cfg = _cfg(name)
    plain = buf[:C]
    lo, ext = CASES[name][4][0]
    calls = [lambda b: hl.decompress_masked(b, config=cfg, level=0), lambda b: hl.decompress_masked(b, config=cfg, coarsen=1),
             lambda b: hl.decompress_masked_preview(b, 1, config=cfg),
             lambda b: hl.decompress_masked_preview(b, 1, config=cfg, window=(lo, ext)),
             lambda b: hl.decompress_mask(b, config=cfg, level=0), lambda b: hl.decompress_mask(b, config=cfg, coarsen=1),
             lambda b: hl.decompress_mask(b, config=cfg, window=(lo, ext)), lambda b: hl.verify_masked(b, data, config=cfg)]
    for call in calls:
        with pytest.raises(mgard_amd.MgardHipError, match="error -8"):       # MGH_ERR_FORMAT: no footer
            call(plain)
    # ... through the C interface too, whose refusal the Python layer does not anticipate
    import ctypes as C_
    L = hl._hl()
    out = np.empty(hl.infer_coarsened(plain, 1, cfg)[0], dtype=np.float32)
    optr = C_.c_void_p(out.ctypes.data)
    for fn in (L.mgh_decompress_masked_coarsened, L.mgh_decompress_masked_preview, L.mgh_decompress_masked_level):
        assert fn(C_.c_void_p(plain.ctypes.data), plain.size, 1, C_.byref(optr), C_.byref(cfg), 1) == -8
    # `level` on a decomposed buffer: the refusal of mgh_decompress_level
    bname = "block-70x45x37-f32"
    _, _, _, bbuf, bC = _case(bname)
    with pytest.raises(mgard_amd.MgardHipError, match="domain-decomposed"):
        hl.decompress_masked(bbuf, config=_cfg(bname), level=0)
    with pytest.raises(mgard_amd.MgardHipError, match="domain-decomposed"):
        hl.decompress_mask(bbuf, config=_cfg(bname), level=0)
    # a window that leaves the array, more halvings than there are
    with pytest.raises(mgard_amd.MgardHipError, match="window"):
        hl.decompress_mask(buf, config=cfg, window=((30, 0, 0), (5, 33, 32)))
    K = hl.infer_coarsened(plain, None, cfg)[1]
    with pytest.raises(mgard_amd.MgardHipError, match="halvings"):
        hl.decompress_masked_preview(buf, K + 1, config=cfg)
    # the library is usable afterwards
    assert np.isnan(hl.decompress_masked(buf, config=cfg, coarsen=1)[mv.sample(mask, mv.coarsened_lists(plain, 1, cfg))]).all()
