"""mgh_compress_roi and its readers: a tighter pointwise bound inside boxes of an array. Every bound is evaluated in
float64 NumPy over every element, with no tolerance on the tolerance: at most A_i = tol_i (times the norm for REL)
inside box i, at most A = tol (times the norm) everywhere; outside the boxes the output is the plain decode of the
container part to the bit, and the container part is byte for byte what compress writes.

"Byte for byte" is held the way tests/test_gpu_ladder.py holds it (_same_container): two mgh_compress calls on the
same input do not write the same bytes themselves -- the outlier pairs of a record stand in the order of the
quantizer's atomics, and the length of a Huffman_Zstd frame depends on that order -- so containers are compared byte
for byte up to the order of those pairs (Zstd frames inflated first), and as plain bytes wherever that order has no
freedom. Seen on one MI355X with these fields: three of four cases differed between two mgh_compress calls."""
import numpy as np
import pytest

from tests.test_gpu_ladder import HUFFMAN_ZSTD, _same_container

pytestmark = pytest.mark.gpu

SHAPE = (33, 40, 65)
TOL, TOL_BOX = 1e-2, 1e-4
BOX = ((4, 5, 3), (17, 25, 57))
SEED = 20261021


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cfg(**kw):
    from mgard_amd import highlevel as hl
    return hl.Config(huff_dict_size=1024, **kw)


def _sl(lo, ext):
    return tuple(slice(a, a + e) for a, e in zip(lo, ext))


def _ints(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def field(shape, dtype, seed=SEED, noise=0.01):
    """smooth plus 1 % noise"""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.linspace(0.0, 1.0, e) for e in shape], indexing="ij")
    u = sum(np.sin(2.0 * np.pi * (k + 1) * x / (k + 2.0) + 0.3 * k) for k, x in enumerate(g)) / len(shape) + 1.5
    return (u * (1.0 + noise * rng.standard_normal(shape))).astype(dtype)


def _zstd(cfg):
    return cfg.lossless == HUFFMAN_ZSTD


def same_buffers(a, b, x, cfg):
    """Two buffers with boxes of the array x: the same table up to the records' CRCs, the container parts and the
    records the same containers (_same_container), the same decoded array to the bit."""
    from mgard_amd import highlevel as hl
    ia, ib = hl.roi_info(a), hl.roi_info(b)
    assert ia is not None and ib is not None
    assert [q[:4] for q in ia.boxes] == [q[:4] for q in ib.boxes]
    _same_container(hl, a[:ia.container_size], b[:ib.container_size], x, cfg, _zstd(cfg))
    at_a, at_b = ia.container_size, ib.container_size
    for qa, qb in zip(ia.boxes, ib.boxes):
        assert (qa[4] == 0) == (qb[4] == 0)
        if qa[4]:
            _same_container(hl, a[at_a:at_a + qa[4]], b[at_b:at_b + qb[4]], np.empty(qa[1], dtype=x.dtype), cfg, _zstd(cfg))
        at_a, at_b = at_a + qa[4], at_b + qb[4]
    if not _zstd(cfg):
        assert len(a) == len(b)
    assert np.array_equal(_ints(_np(hl.decompress_roi(a, config=cfg))), _ints(_np(hl.decompress_roi(b, config=cfg))))


def _factor(x, mode):
    import mgard_amd
    return float(np.max(np.abs(x.astype(np.float64)))) if mode == mgard_amd.REL else 1.0


def _err(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64))


def check(x, buf, boxes, tol, mode, cfg):
    """assertions 1 to 5 of a buffer with boxes; returns (decoded, plain decode of the base)"""
    import mgard_amd
    from mgard_amd import highlevel as hl
    info = hl.roi_info(buf)
    assert info is not None and info.nbox == len(boxes)
    assert [(b[0], b[1], b[2]) for b in info.boxes] == [(tuple(lo), tuple(ext), t) for lo, ext, t in boxes]
    out = _np(hl.decompress_roi(buf, config=cfg))
    base = _np(hl.decompress(buf[:info.container_size], config=cfg))
    assert out.shape == x.shape and out.dtype == x.dtype
    f = _factor(x, mode)
    outside = np.ones(x.shape, dtype=bool)
    for (lo, ext, tol_i), ib in zip(boxes, info.boxes):
        e = _err(out[_sl(lo, ext)], x[_sl(lo, ext)])
        print("box", lo, ext, "max error", e.max(), "A_i", tol_i * f, "base error", _err(base[_sl(lo, ext)], x[_sl(lo, ext)]).max(),
              "tolres", ib[3], "record", ib[4])
        assert e.max() <= tol_i * f                                                   # 1
        assert 0.5 * tol_i * f <= ib[3] <= tol_i * f
        outside[_sl(lo, ext)] = False
    print("whole max error", _err(out, x).max(), "A", tol * f, "bytes", len(buf), "container", info.container_size)
    assert _err(out, x).max() <= tol * f                                              # 2
    plain = hl.compress(x if isinstance(buf, np.ndarray) else _dev(x), tol, float("inf"), mode, config=cfg)
    _same_container(hl, buf[:info.container_size], plain, x, cfg, _zstd(cfg))         # 4
    assert np.array_equal(_ints(out)[outside], _ints(base)[outside])                  # 5
    return out, base


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mode", ["REL", "ABS"])
def test_one_box_holds_its_bound(mode, dtype):
    import mgard_amd
    from mgard_amd import highlevel as hl
    mode = getattr(mgard_amd, mode)
    cfg = _cfg()
    x = field(SHAPE, dtype)
    boxes = [(BOX[0], BOX[1], TOL_BOX)]
    buf = hl.compress_roi(x, TOL, boxes, mode=mode, config=cfg)
    out, base = check(x, buf, boxes, TOL, mode, cfg)
    # 3: without the box's record the bound does not hold -- the case shows something
    assert _err(base[_sl(*BOX)], x[_sl(*BOX)]).max() > TOL_BOX * _factor(x, mode)
    # 6: cheaper than the tight bound everywhere
    tight = hl.compress(x, TOL_BOX, float("inf"), mode, config=cfg)
    print("roi bytes", len(buf), "tight-everywhere bytes", len(tight), "loose bytes", hl.roi_info(buf).container_size)
    assert len(buf) < len(tight)
    whole, per_box = hl.verify_roi(buf, x, config=cfg)
    assert whole.within == 1 and [r.within for r in per_box] == [1]
    assert whole.stats.max_abs_err == _err(out, x).max() and whole.bound == TOL * _factor(x, mode)
    assert per_box[0].stats.max_abs_err == _err(out[_sl(*BOX)], x[_sl(*BOX)]).max()
    assert per_box[0].bound == TOL_BOX * _factor(x, mode) and per_box[0].stats.n == int(np.prod(BOX[1]))
    # ... and 0 after one element of the box moved by 2 A_i
    y = x.copy()
    y[10, 12, 30] += dtype(2 * TOL_BOX * _factor(x, mode))
    whole, per_box = hl.verify_roi(buf, y, config=cfg)
    assert whole.within == 1 and per_box[0].within == 0


def test_two_boxes_at_different_tolerances():
    import mgard_amd
    from mgard_amd import highlevel as hl
    cfg = _cfg()
    x = field(SHAPE, np.float32)
    boxes = [((0, 0, 0), (9, 40, 33), 1e-3), ((20, 7, 30), (13, 11, 35), 1e-4)]
    buf = hl.compress_roi(x, TOL, boxes, mode=mgard_amd.REL, config=cfg)
    check(x, buf, boxes, TOL, mgard_amd.REL, cfg)
    whole, per_box = hl.verify_roi(buf, x, config=cfg)
    assert whole.within == 1 and [r.within for r in per_box] == [1, 1]
    for bad in ([boxes[0], ((8, 0, 0), (3, 3, 3), 1e-3)], [boxes[0]] * 2):
        with pytest.raises(mgard_amd.MgardHipError, match="pairwise disjoint"):
            hl.compress_roi(x, TOL, bad, config=cfg)


@pytest.mark.parametrize("shape,box,tol_i,dtype", [((100001,), ((37,), (13000,)), 1e-4, np.float64),
                                                   ((17, 18, 19, 20), ((1, 2, 3, 4), (9, 11, 13, 15)), 1e-5, np.float32)],
                         ids=["1d", "4d"])
def test_one_and_four_dimensions(shape, box, tol_i, dtype):
    """(Fields with 0.1 % noise, and large enough that the writer does not store the array as it is -- a 1000-element
    or 9x10x11x12 field with 1 % noise is stored raw, its base is exact and its box's record empty. In four dimensions
    the base at 1e-2 is already within 5.8e-5 in the box -- the quantum shrinks with the dimension -- so that box asks
    for 1e-5.)"""
    import mgard_amd
    from mgard_amd import highlevel as hl
    cfg = _cfg()
    x = field(shape, dtype, noise=1e-3)
    boxes = [(box[0], box[1], tol_i)]
    buf = hl.compress_roi(x, TOL, boxes, mode=mgard_amd.ABS, config=cfg)
    _, base = check(x, buf, boxes, TOL, mgard_amd.ABS, cfg)
    assert _err(base[_sl(*box)], x[_sl(*box)]).max() > tol_i


def test_constant_field_stores_an_empty_record():
    """R = 0: the base is exact in the box (the constant is 0, which every quantizer keeps), so nothing is stored."""
    import mgard_amd
    from mgard_amd import highlevel as hl
    cfg = _cfg()
    x = np.zeros((17, 18, 19), dtype=np.float32)
    boxes = [((2, 3, 4), (5, 6, 7), 1e-4)]
    buf = hl.compress_roi(x, TOL, boxes, mode=mgard_amd.ABS, config=cfg)
    out, base = check(x, buf, boxes, TOL, mgard_amd.ABS, cfg)
    assert np.array_equal(base, x), "the base of a constant field is expected to be exact"
    info = hl.roi_info(buf)
    assert info.boxes[0][4] == 0 and len(buf) == info.container_size + 120 + 40
    assert np.array_equal(_ints(out), _ints(base))


@pytest.mark.parametrize("value", [1.5, 2.7182817])
def test_nonzero_constant_field(value):
    """A constant other than 0 need not come back exactly from the base (the coarsest nodes are quantized like any
    coefficient), so R = 0 is not assumed: both bounds are held, and the record is empty exactly where the base is
    exact in the box."""
    import mgard_amd
    from mgard_amd import highlevel as hl
    cfg = _cfg()
    x = np.full((17, 18, 19), value, dtype=np.float32)
    boxes = [((2, 3, 4), (5, 6, 7), 1e-4)]
    buf = hl.compress_roi(x, TOL, boxes, mode=mgard_amd.ABS, config=cfg)
    out, base = check(x, buf, boxes, TOL, mgard_amd.ABS, cfg)
    exact = np.array_equal(base[_sl(*boxes[0][:2])], x[_sl(*boxes[0][:2])])
    info = hl.roi_info(buf)
    print("constant", value, "base exact in the box:", exact, "record", info.boxes[0][4])
    assert (info.boxes[0][4] == 0) == exact
    whole, per_box = hl.verify_roi(buf, x, config=cfg)
    assert whole.within == 1 and per_box[0].within == 1


def test_device_buffers_and_preallocated_outputs():
    import torch
    import mgard_amd
    from mgard_amd import highlevel as hl
    cfg = _cfg()
    x = field(SHAPE, np.float32)
    boxes = [(BOX[0], BOX[1], TOL_BOX)]
    host = hl.compress_roi(x, TOL, boxes, config=cfg)
    dbuf = hl.compress_roi(_dev(x), TOL, boxes, config=cfg)
    assert isinstance(dbuf, torch.Tensor) and dbuf.is_cuda
    same_buffers(_np(dbuf), host, x, cfg)
    want = hl.decompress_roi(host, config=cfg)
    dout = hl.decompress_roi(dbuf, config=cfg)
    assert isinstance(dout, torch.Tensor) and dout.is_cuda and np.array_equal(_ints(_np(dout)), _ints(want))
    check(x, dbuf, boxes, TOL, mgard_amd.REL, cfg)
    # pre-allocated outputs of exactly the size, and one byte too small
    exact = np.empty(len(host), dtype=np.uint8)
    same_buffers(hl.compress_roi(x, TOL, boxes, config=cfg, out=exact), host, x, cfg)
    dexact = torch.empty(len(host), dtype=torch.uint8, device="cuda")
    same_buffers(_np(hl.compress_roi(_dev(x), TOL, boxes, config=cfg, out=dexact)), host, x, cfg)
    with pytest.raises(mgard_amd.MgardHipError, match="error -7"):
        hl.compress_roi(x, TOL, boxes, config=cfg, out=np.empty(len(host) - 1, dtype=np.uint8))
    with pytest.raises(mgard_amd.MgardHipError, match="error -7"):
        hl.compress_roi(_dev(x), TOL, boxes, config=cfg, out=torch.empty(len(host) - 1, dtype=torch.uint8, device="cuda"))
    o = np.empty(SHAPE, dtype=np.float32)
    assert hl.decompress_roi(host, config=cfg, out=o) is o and np.array_equal(_ints(o), _ints(want))
    do = torch.empty(SHAPE, dtype=torch.float32, device="cuda")
    assert hl.decompress_roi(dbuf, config=cfg, out=do) is do and np.array_equal(_ints(_np(do)), _ints(want))
    whole, per_box = hl.verify_roi(dbuf, _dev(x), config=cfg)
    assert whole.within == 1 and per_box[0].within == 1


def test_huffman_zstd():
    import mgard_amd
    from mgard_amd import highlevel as hl
    cfg = _cfg(lossless=hl.HUFFMAN_ZSTD)
    x = field(SHAPE, np.float32)
    boxes = [(BOX[0], BOX[1], TOL_BOX)]
    buf = hl.compress_roi(x, TOL, boxes, config=cfg)
    check(x, buf, boxes, TOL, mgard_amd.REL, cfg)


def test_refusals():
    import mgard_amd
    from mgard_amd import highlevel as hl
    cfg = _cfg()
    x = field(SHAPE, np.float32)
    # float32 cannot carry 1e-9 of the norm: refused, never loosened
    with pytest.raises(mgard_amd.MgardHipError, match="cannot carry"):
        hl.compress_roi(x, TOL, [(BOX[0], BOX[1], 1e-9)], mode=mgard_amd.REL, config=cfg)
    y = x.copy()
    y[10, 12, 30] = np.nan
    with pytest.raises(mgard_amd.MgardHipError, match="non-finite"):
        hl.compress_roi(y, TOL, [(BOX[0], BOX[1], TOL_BOX)], mode=mgard_amd.ABS, config=cfg)
    with pytest.raises(mgard_amd.MgardHipError, match="s must be infinite"):
        hl.compress_roi(x, TOL, [(BOX[0], BOX[1], TOL_BOX)], s=0.0, config=cfg)


def test_corrupted_and_truncated_buffers_are_format_errors():
    import mgard_amd
    from mgard_amd import highlevel as hl
    cfg = _cfg()
    x = field(SHAPE, np.float32)
    buf = hl.compress_roi(x, TOL, [(BOX[0], BOX[1], TOL_BOX)], config=cfg)
    info = hl.roi_info(buf)
    table_at = len(buf) - 40 - 120
    for at in (table_at + 3, table_at + 80, len(buf) - 16, info.container_size + 5, len(buf) - 40 - 120 - 1):
        bad = buf.copy()
        bad[at] ^= 0x10                      # the table (lo, tol), the table's CRC, the record's first and last bytes
        with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
            hl.decompress_roi(bad, config=cfg)
        with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
            hl.roi_info(bad)
    for cut in (1, 8, 41, 200):
        part = buf[:len(buf) - cut].copy()
        assert hl.roi_info(part) is None     # (the magic is no longer where a footer ends)
        with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
            hl.decompress_roi(part, config=cfg)
    front = buf[1:].copy()                   # one byte short in front: the sizes do not add up
    with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
        hl.decompress_roi(front, config=cfg)


def test_other_readers_and_other_footers():
    import mgard_amd
    from mgard_amd import highlevel as hl
    cfg = _cfg(reorder=1)                    # (the progressive reader wants a level-ordered record)
    x = field(SHAPE, np.float32)
    buf = hl.compress_roi(x, TOL, [(BOX[0], BOX[1], TOL_BOX)], config=cfg)
    cont = buf[:hl.roi_info(buf).container_size].copy()
    plain = hl.compress(x, TOL, float("inf"), mgard_amd.REL, config=cfg)
    # the existing readers open the container part as the unrefined base
    base = hl.decompress(cont, config=cfg)
    assert np.array_equal(hl.decompress(cont, config=cfg, level=1), hl.decompress(plain, config=cfg, level=1))
    assert np.array_equal(hl.decompress(cont, config=cfg, coarsen=1), hl.decompress(plain, config=cfg, coarsen=1))
    assert np.array_equal(hl.decompress_preview(cont, 1, config=cfg), hl.decompress_preview(plain, 1, config=cfg))
    with hl.Progressive(cont, cfg) as p, hl.Progressive(plain, cfg) as q:
        assert np.array_equal(_np(p.refine(1)), _np(q.refine(1)))
        assert np.array_equal(_np(p.refine(2)), _np(hl.decompress(plain, config=cfg, level=2)))
    assert np.array_equal(hl.decompress(plain, config=cfg), base)
    assert hl.verify(cont, x, config=cfg).within == 1
    # a buffer with boxes is no masked and no pointwise-relative buffer, and the other way round
    assert hl.masked_info(buf) is None and hl.pwrel_info(buf) is None
    with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
        hl.decompress_masked(buf, config=cfg)
    with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
        hl.decompress_pwrel(buf, config=cfg)
    masked = hl.compress_masked(x, TOL, config=cfg)
    pwrel = hl.compress_pwrel(x, 1e-2, config=cfg)
    for other in (masked, pwrel, plain):
        assert hl.roi_info(other) is None
        with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
            hl.decompress_roi(other, config=cfg)
