"""Pointwise-relative buffers in the level, coarsened, preview and windowed-preview readers.

The writer set-up is that of tests/test_gpu_pwrel.py and tests/pwrel_model.py (smooth_field and decades_field with the
special values planted, abs_floor 1e-20, huff_dict_size = 1024): (34, 33, 32) float32 at eps 1e-1, (17, 130) float64 at
eps 1e-2, and the decomposed case of tests/test_gpu_masked_views.py, (70, 45, 37) float32 in blocks of 33. On top of
pwrel_model.plant, which fills the first rows, the test plants a NaN at index (0, ...), a zero at the last index --
nodes of every level -- and a negative value at a node of the coarser levels.

For every view the expectation is built from entry points older than these readers: mgard_amd.pwrel_inverse applied to
what the plain reader gives for buf[:container_size] at that view, with the packed words of pwrel_model.bitmaps(x)
sampled by tests/mask_view_model.py through the view's node lists. The output equals it bit for bit."""
import numpy as np
import pytest

from tests import mask_model as mm
from tests import mask_view_model as mv
from tests import pwrel_model as pm
from tests.test_coarsened_cpu import BLOCK

# name: (shape, dtype, eps, field, decomposed, windows) -- the windows of tests/test_gpu_masked_views.py
CASES = {
    "34x33x32-f32-smooth": ((34, 33, 32), np.float32, 1e-1, "smooth", False, [((3, 0, 31), (5, 33, 1))]),
    "34x33x32-f32-decades": ((34, 33, 32), np.float32, 1e-1, "decades", False, [((3, 0, 31), (5, 33, 1))]),
    "17x130-f64-smooth": ((17, 130), np.float64, 1e-2, "smooth", False, [((2, 60), (9, 70))]),
    "17x130-f64-decades": ((17, 130), np.float64, 1e-2, "decades", False, [((2, 60), (9, 70))]),
    # (the second window crosses the block borders at 33 along the first and the last dimension)
    "block-70x45x37-f32-smooth": ((70, 45, 37), np.float32, 1e-1, "smooth", True,
                                  [((3, 0, 31), (5, 33, 1)), ((30, 10, 30), (8, 20, 7))]),
}
FIELDS = {"smooth": pm.smooth_field, "decades": pm.decades_field}
_made = {}


def _floor(dtype):
    return float(dtype(1e-20))


def _mid_node(shape):
    """A node of every level down to three halvings below the finest: the second one of each dimension there."""
    return tuple(mv.halved_nodes(e, 3)[1] for e in shape)


def _field(name):
    shape, dtype, _, field, _, _ = CASES[name]
    x = FIELDS[field](shape, dtype, abs_floor=_floor(dtype), planted=True)
    x[(0,) * len(shape)] = np.nan
    x[tuple(e - 1 for e in shape)] = 0.0
    x[_mid_node(shape)] = -abs(dtype(3.5))
    return x


def _cfg(name):
    from mgard_amd import highlevel as hl
    if CASES[name][4]:
        return hl.Config(huff_dict_size=1024, domain_decomposition=BLOCK, block_size=33)
    return hl.Config(huff_dict_size=1024)


def _case(name):
    """(x, mask bits, flag bits, host buffer, container size C, masked size M), made once."""
    from mgard_amd import highlevel as hl
    if name not in _made:
        shape, dtype, eps, _, _, _ = CASES[name]
        x = _field(name)
        buf = hl.compress_pwrel(x, eps, _floor(dtype), config=_cfg(name))
        info = hl.pwrel_info(buf)
        mask, flag = pm.bitmaps(x, _floor(dtype))
        _made[name] = (x, mask, flag, buf, int(info.container_size), int(info.masked_size))
    return _made[name]


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _where(buf, where):
    return buf if where == "host" else _dev(buf)


def _words(bits):
    return _dev(mm.packed_words(bits).view(np.int64))


def _assert_view(out, plain, smask, sflag, sneg, dtype, what):
    """out: the reader's output; plain: the plain reader's y' of the container part at the same view; smask / sflag:
    the bitmaps of the full array sampled at the view; sneg: the sign of x at the view's positions."""
    import mgard_amd
    out = _np(out)
    assert out.dtype == dtype and out.shape == smask.shape == _np(plain).shape, what
    want = _np(mgard_amd.pwrel_inverse(_dev(_np(plain)), _words(smask), _words(sflag)))
    assert np.array_equal(mm.int_view(out), mm.int_view(want)), what
    nonfin, zeroed, valid = smask & sflag, smask & ~sflag, ~smask
    assert np.array_equal(np.isnan(out), nonfin), what
    assert np.array_equal(mm.int_view(out) == 0, zeroed), what                # +0.0, sign bit clear, exactly there
    assert np.isfinite(out[valid]).all() and np.all(np.abs(out[valid]) >= np.finfo(dtype).tiny), what
    assert np.array_equal(np.signbit(out[valid]), sneg[valid]), what
    return np.array([nonfin.sum(), zeroed.sum(), (valid & sneg).sum(), (valid & ~sneg).sum()])


def test_planted_classes_stand_on_nodes_of_the_coarse_levels():
    """On the CPU: pwrel_model.plant fills the first rows only, so a coarse level keeps a planted special only where it
    stands on a corner; with the three values planted above every level meets a NaN and a zero, and the levels down to
    three halvings a negative valid value too."""
    for name, (shape, dtype, _, _, _, _) in CASES.items():
        x = _field(name)
        mask, flag = pm.bitmaps(x, _floor(dtype))
        steps = 0
        while min(len(mv.halved_nodes(e, steps)) for e in shape) > 2:
            lists = [mv.halved_nodes(e, steps) for e in shape]
            smask, sflag = mv.sample(mask, lists), mv.sample(flag, lists)
            assert (smask & sflag).any() and (smask & ~sflag).any(), (name, steps)
            if steps <= 3:
                assert (~smask & sflag).any() and (~smask & ~sflag).any(), (name, steps)
            steps += 1
        assert steps >= 4, name


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", list(CASES))
def test_views_are_the_inverse_pass_of_the_plain_reader_with_the_sampled_bits(name, where):
    import torch
    from mgard_amd import highlevel as hl
    shape, dtype, eps, _, decomposed, windows = CASES[name]
    x, mask, flag, hbuf, C, M = _case(name)
    neg = np.signbit(x)
    cfg = _cfg(name)
    buf = _where(hbuf, where)
    full = hl.decompress_pwrel(buf, config=cfg)
    seen = np.zeros(4, dtype=np.int64)      # non-finite, zeroed, negative, positive nodes met by the sampled views
    # every level (containers with one subdomain)
    if not decomposed:
        L = hl.infer_level(hbuf[:C], None, cfg)[1]
        for level in range(L + 1):
            lists = mv.level_lists(hbuf[:C], level, cfg)
            out = hl.decompress_pwrel(buf, config=cfg, level=level)
            assert isinstance(out, np.ndarray) == (where == "host")
            seen += _assert_view(out, hl.decompress(buf[:C], config=cfg, level=level), mv.sample(mask, lists),
                                 mv.sample(flag, lists), mv.sample(neg, lists), dtype, "level %d" % level)
        assert np.array_equal(mm.int_view(_np(out)), mm.int_view(_np(full)))     # level = l_target
    # every number of halvings, as the coarsened array, as the preview and as windows of the preview
    K = hl.infer_coarsened(hbuf[:C], None, cfg)[1]
    assert K >= 2
    for k in range(K + 1):
        lists = mv.coarsened_lists(hbuf[:C], k, cfg)
        out = hl.decompress_pwrel(buf, config=cfg, coarsen=k)
        seen += _assert_view(out, hl.decompress(buf[:C], config=cfg, coarsen=k), mv.sample(mask, lists), mv.sample(flag, lists),
                             mv.sample(neg, lists), dtype, "coarsen %d" % k)
        if k == 0:
            assert np.array_equal(mm.int_view(_np(out)), mm.int_view(_np(full)))
        out = hl.decompress_pwrel_preview(buf, k, config=cfg)
        assert isinstance(out, np.ndarray) == (where == "host")
        _assert_view(out, hl.decompress_preview(buf[:C], k, config=cfg), mask, flag, neg, dtype, "preview %d" % k)
        if k == 0:
            assert np.array_equal(mm.int_view(_np(out)), mm.int_view(_np(full)))
        for lo, ext in windows:
            lists = mv.window_lists(lo, ext)
            out = hl.decompress_pwrel_preview(buf, k, config=cfg, window=(lo, ext))
            seen += _assert_view(out, hl.decompress_preview(buf[:C], k, config=cfg, window=(lo, ext)), mv.sample(mask, lists),
                                 mv.sample(flag, lists), mv.sample(neg, lists), dtype, "window %r of preview %d" % ((lo, ext), k))
    assert np.all(seen > 0), seen       # no class was met by none of the views
    # a pre-allocated output is filled in place and returned
    for kw, oshape in (({"coarsen": 1}, hl.infer_coarsened(hbuf[:C], 1, cfg)[0]), ({"coarsen": 0}, shape)):
        o = torch.empty(tuple(oshape), dtype=full.dtype, device="cuda") if where == "device" else np.empty(tuple(oshape), dtype=dtype)
        assert hl.decompress_pwrel(buf, config=cfg, out=o, **kw) is o
        assert np.array_equal(mm.int_view(_np(o)), mm.int_view(_np(hl.decompress_pwrel(buf, config=cfg, **kw))))
    lo, ext = windows[0]
    o = torch.empty(ext, dtype=full.dtype, device="cuda") if where == "device" else np.empty(ext, dtype=dtype)
    assert hl.decompress_pwrel_preview(buf, 1, config=cfg, out=o, window=(lo, ext)) is o
    o = torch.empty(shape, dtype=full.dtype, device="cuda") if where == "device" else np.empty(shape, dtype=dtype)
    assert hl.decompress_pwrel_preview(buf, 0, config=cfg, out=o) is o
    assert np.array_equal(mm.int_view(_np(o)), mm.int_view(_np(full)))


def _status(fn, buf, *args):
    """The status of a C reader that is handed no output (a refusal comes before anything is allocated)."""
    import ctypes as C_
    from mgard_amd import highlevel as hl
    out = C_.c_void_p()
    rc = fn(C_.c_void_p(buf.ctypes.data), buf.size, *args, C_.byref(out), C_.byref(hl.Config(huff_dict_size=1024)), 0)
    assert rc < 0 and not out.value, (rc, out.value)
    return rc


@pytest.mark.gpu
def test_refusals_are_those_of_the_masked_readers():
    import ctypes as C_
    import mgard_amd
    from mgard_amd import highlevel as hl
    name = "34x33x32-f32-smooth"
    shape, dtype, eps, _, _, windows = CASES[name]
    x, mask, flag, buf, C, M = _case(name)
    cfg = _cfg(name)
    lo, ext = windows[0]
    calls = [lambda b: hl.decompress_pwrel(b, config=cfg, level=0), lambda b: hl.decompress_pwrel(b, config=cfg, coarsen=1),
             lambda b: hl.decompress_pwrel_preview(b, 1, config=cfg),
             lambda b: hl.decompress_pwrel_preview(b, 1, config=cfg, window=(lo, ext))]
    # a plain container and a masked buffer: MGH_ERR_FORMAT, with the existing text under the call's name
    for other in (buf[:C], buf[:M]):
        for call in calls:
            with pytest.raises(mgard_amd.MgardHipError, match="error -8.*no pointwise-relative footer"):
                call(other)
    L = hl._hl()
    u64 = C_.c_uint64 * 3
    for other in (buf[:C], buf[:M]):
        for fn in (L.mgh_decompress_pwrel_level, L.mgh_decompress_pwrel_coarsened, L.mgh_decompress_pwrel_preview):
            assert _status(fn, other, 1) == -8
            assert fn.__name__[4:] + ": no pointwise-relative footer" in L.mgh_last_error().decode()
        assert _status(L.mgh_decompress_pwrel_preview_window, other, 1, u64(*lo), u64(*ext)) == -8
    # every other refusal: the status of the masked reader of the same view on the masked buffer in front
    mbuf = np.ascontiguousarray(buf[:M])
    Lt = hl.infer_level(buf[:C], None, cfg)[1]
    K = hl.infer_coarsened(buf[:C], None, cfg)[1]
    assert _status(L.mgh_decompress_pwrel_level, buf, Lt + 1) == _status(L.mgh_decompress_masked_level, mbuf, Lt + 1)
    assert _status(L.mgh_decompress_pwrel_level, buf, -1) == _status(L.mgh_decompress_masked_level, mbuf, -1)
    assert _status(L.mgh_decompress_pwrel_coarsened, buf, K + 1) == _status(L.mgh_decompress_masked_coarsened, mbuf, K + 1)
    assert _status(L.mgh_decompress_pwrel_preview, buf, K + 1) == _status(L.mgh_decompress_masked_preview, mbuf, K + 1)
    assert _status(L.mgh_decompress_pwrel_preview, buf, -1) == _status(L.mgh_decompress_masked_preview, mbuf, -1)
    out_lo, out_ext = u64(30, 0, 0), u64(5, 33, 32)
    assert _status(L.mgh_decompress_pwrel_preview_window, buf, 1, out_lo, out_ext) == \
        _status(L.mgh_decompress_masked_preview_window, mbuf, 1, out_lo, out_ext)
    assert _status(L.mgh_decompress_pwrel_preview_window, buf, K + 1, u64(*lo), u64(*ext)) == \
        _status(L.mgh_decompress_masked_preview_window, mbuf, K + 1, u64(*lo), u64(*ext))
    with pytest.raises(mgard_amd.MgardHipError, match="level"):
        hl.decompress_pwrel(buf, config=cfg, level=Lt + 1)
    with pytest.raises(mgard_amd.MgardHipError, match="halvings"):
        hl.decompress_pwrel_preview(buf, K + 1, config=cfg)
    with pytest.raises(mgard_amd.MgardHipError, match="halvings"):
        hl.decompress_pwrel(buf, config=cfg, coarsen=K + 1)
    with pytest.raises(mgard_amd.MgardHipError, match="window"):
        hl.decompress_pwrel_preview(buf, 1, config=cfg, window=((30, 0, 0), (5, 33, 32)))
    with pytest.raises(ValueError):
        hl.decompress_pwrel(buf, config=cfg, level=0, coarsen=1)
    # `level` on the decomposed case: the refusal of mgh_decompress_level
    bname = "block-70x45x37-f32-smooth"
    _, _, _, bbuf, bC, bM = _case(bname)
    with pytest.raises(mgard_amd.MgardHipError, match="domain-decomposed"):
        hl.decompress_pwrel(bbuf, config=_cfg(bname), level=0)
    import ctypes
    bcfg = _cfg(bname)
    codes = []
    for fn, b in ((L.mgh_decompress_pwrel_level, bbuf), (L.mgh_decompress_masked_level, np.ascontiguousarray(bbuf[:bM]))):
        out = ctypes.c_void_p()
        codes.append(fn(ctypes.c_void_p(b.ctypes.data), b.size, 0, ctypes.byref(out), ctypes.byref(bcfg), 0))
        assert not out.value
    assert codes[0] == codes[1] < 0
    # the library is usable afterwards
    pm_out = hl.decompress_pwrel(buf, config=cfg)
    assert np.array_equal(np.isnan(pm_out), mask & flag) and np.all(mm.int_view(pm_out)[mask & ~flag] == 0)
    valid = ~mask
    xd, od = x[valid].astype(np.float64), pm_out[valid].astype(np.float64)
    assert np.all(np.abs(od - xd) <= eps * np.abs(xd))
