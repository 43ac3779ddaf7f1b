"""mgh_compress_masked and its readers against tests/mask_model.py and the plain writer.

The buffer is [container][mask record][48-byte footer]. The container part must BE the container of the filled
array (the model's fill, bit for bit), so it is held against highlevel.compress of that array; the readers are held
against the NumPy mask and the restore value's bits; the bound is the writer's own guarantee at the valid
positions, with no measured margin."""
import itertools

import numpy as np
import pytest

from tests import mask_model as mm
from tests.util import inside_field

INF = float("inf")
NAN = float("nan")
TOL = 3e-2
CASES = [((34, 33, 32), np.float32), ((17, 130), np.float64)]


def _ball(shape, radius):
    g = np.meshgrid(*[np.arange(e) - (e - 1) / 2 for e in shape], indexing="ij")
    return sum((x / (radius * e)) ** 2 for x, e in zip(g, shape)) < 1.0


def _mask(kind, shape):
    if kind == "ball":
        return _ball(shape, 0.3)
    return np.random.default_rng(len(shape)).random(shape) < {"random30": 0.30, "random50": 0.50}[kind]


def _marked(shape, dtype, kind):
    """(data, mask, keyword arguments of compress_masked): the ball as NaN / +-Inf, the random mask as a fill value of
    1e20 with a few NaN among it, restored as -9999."""
    x = inside_field(shape, dtype)
    mask = _mask(kind, shape)
    idx = np.flatnonzero(mask.reshape(-1))
    if kind == "ball":
        marks, kw = [NAN, INF, -INF], dict(nonfinite=True, fill_value=None, restore_value=NAN)
    else:
        marks, kw = [1e20, 1e20, NAN], dict(nonfinite=True, fill_value=1e20, restore_value=-9999.0)
    x.reshape(-1)[idx] = np.array(marks, dtype=dtype)[np.arange(idx.size) % len(marks)]
    return x, mask, kw


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _cfg():
    from mgard_amd import highlevel as hl
    return hl.Config(huff_dict_size=1024)


def _filled_reference(data, mask, s, mode):
    """(the model's filled array, its plain container written from device memory, as the masked writer does)"""
    import torch
    from mgard_amd import highlevel as hl
    filled = mm.fill(data, mask, mm.fill_constant(data, mask))
    return filled, hl.compress(torch.from_numpy(filled).cuda(), TOL, s, mode, config=_cfg())


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("kind", ["ball", "random30"])
@pytest.mark.parametrize("mode_s", ["REL-inf", "ABS-inf", "REL-0"])
@pytest.mark.parametrize("shape,dtype", CASES, ids=["34x33x32-f32", "17x130-f64"])
def test_masked_round_trip(shape, dtype, mode_s, kind, where):
    import torch
    import mgard_amd
    from mgard_amd import highlevel as hl
    mode = mgard_amd.REL if mode_s.startswith("REL") else mgard_amd.ABS
    s = INF if mode_s.endswith("inf") else 0.0
    data, mask, kw = _marked(shape, dtype, kind)
    n = data.size
    src = data if where == "host" else torch.from_numpy(data).cuda()
    buf = hl.compress_masked(src, TOL, s, mode, config=_cfg(), **kw)
    assert isinstance(buf, np.ndarray) == (where == "host")
    # (a) the footer, through the library and through the restatement
    info = hl.masked_info(buf)
    foot = mm.parse_footer(_np(buf))
    bits = mm.value_bits(dtype, kw["restore_value"])
    assert info.n_masked == int(mask.sum()) == foot["n_masked"] and foot["restore_bits"] == bits
    assert mm.value_bits(dtype, info.restore_value) == bits
    C, R = int(info.container_size), int(info.record_size)
    assert (C, R, info.kind) == (foot["container"], foot["record"], foot["kind"]) and C + R + mm.FOOTER_BYTES == len(buf)
    assert _np(buf)[-mm.FOOTER_BYTES:].tobytes() == mm.footer(C, _np(buf)[C:C + R].tobytes(), foot["n_masked"], bits, foot["kind"])
    # (b) the mask
    got_mask = hl.decompress_mask(buf)
    assert got_mask.dtype in (np.bool_, torch.bool) and np.array_equal(_np(got_mask), mask)
    # (c) the container part is the plain container of the model's filled array
    filled, ref = _filled_reference(data, mask, s, mode)
    assert C == len(ref)
    assert C < data.nbytes    # (a record, not the array stored raw: the bound below is tested on a lossy container)
    plain = _np(hl.decompress(buf[:C], config=_cfg()))
    assert np.array_equal(mm.int_view(plain), mm.int_view(_np(hl.decompress(ref, config=_cfg()))))
    # (d) restore_value's bits at every masked position, the plain reconstruction everywhere else
    out = hl.decompress_masked(buf, config=_cfg())
    assert isinstance(out, np.ndarray) == (where == "host")
    out = _np(out)
    assert out.dtype == dtype and out.shape == shape
    assert np.all(mm.int_view(out)[mask] == mm.int_view(np.array([kw["restore_value"]], dtype=dtype))[0])
    assert np.array_equal(mm.int_view(out)[~mask], mm.int_view(plain)[~mask])
    # (e) the writer's guarantee at the valid positions
    err = np.abs(out[~mask].astype(np.float64) - data[~mask].astype(np.float64))
    absmax = float(np.max(np.abs(data[~mask])))
    norm = hl.metadata_parse(_np(buf)[:C].tobytes())["norm"]
    if s == INF:
        bound = TOL * absmax if mode == mgard_amd.REL else TOL
        if mode == mgard_amd.REL:
            assert norm == absmax         # fills are copies of valid values or lie between their extremes
        print("max error %.3e, bound %.3e" % (err.max(), bound))
        assert err.max() <= bound
    else:
        # s = 0 bounds the L2 error over the whole (filled) array, normalised by n: sqrt(sum err^2 / n) <= tol * norm,
        # norm the header's; the valid positions are a part of that sum
        l2 = float(np.sqrt(np.sum(err ** 2) / n))
        print("L2 error over the valid positions %.3e, bound %.3e" % (l2, TOL * norm))
        assert l2 <= TOL * norm
    # (g) the container part in the other readers
    assert _np(hl.decompress(buf[:C], config=_cfg(), level=hl.infer_level(buf[:C], None, _cfg())[1])).shape == shape
    coarse = hl.decompress(buf[:C], config=_cfg(), level=0)
    assert tuple(coarse.shape) == tuple(hl.infer_level(buf[:C], 0, _cfg())[0]) and np.isfinite(_np(coarse)).all()
    v = hl.verify(buf[:C], filled if where == "host" else torch.from_numpy(filled).cuda(), config=_cfg())
    assert v.within == 1 and v.stats.nonfinite == 0 and v.stats.n == n


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dtype", CASES, ids=["34x33x32-f32", "17x130-f64"])
def test_nothing_masked_is_kind_2_and_the_plain_container(shape, dtype):
    import mgard_amd
    from mgard_amd import highlevel as hl
    data = inside_field(shape, dtype)
    buf = hl.compress_masked(data, TOL, INF, mgard_amd.REL, config=_cfg(), fill_value=1e20)
    info = hl.masked_info(buf)
    assert (info.kind, info.record_size, info.n_masked) == (mm.NONE, 0, 0)
    ref = hl.compress(data, TOL, INF, mgard_amd.REL, config=_cfg())
    C = int(info.container_size)
    assert C == len(ref) and len(buf) == C + mm.FOOTER_BYTES
    want = hl.decompress(ref, config=_cfg())
    assert np.array_equal(mm.int_view(hl.decompress(buf[:C], config=_cfg())), mm.int_view(want))
    assert np.array_equal(mm.int_view(hl.decompress_masked(buf, config=_cfg())), mm.int_view(want))
    assert not hl.decompress_mask(buf).any()


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host", "device"])
def test_full_readers_of_a_domain_decomposed_buffer(where):
    """The full array and the full mask ask nothing of the container's header but its shape, so a container in
    subdomains reads like any other; `level` is refused as mgh_decompress_level refuses it. The writer splits a host
    array whose footprint estimate (tests/util.py: reference_footprint, 639408 bytes here) reaches the budget: halves of
    33 along the first dimension. The mask is 10 % NaN, restored as -9999."""
    import torch
    import mgard_amd
    from mgard_amd import highlevel as hl
    from tests.util import reference_footprint
    shape, dtype = (33, 20, 17), np.float32
    data = inside_field(shape, dtype)
    data[np.random.default_rng(7).random(shape) < 0.10] = NAN
    mask = mm.classify(data, nonfinite=True, fill_value=None)
    assert 0.05 * data.size < mask.sum() < 0.15 * data.size
    budget = reference_footprint(shape, 4, dict_size=1024)
    assert data.nbytes < budget
    cfg = hl.Config(huff_dict_size=1024, max_memory_footprint=budget)
    hbuf = hl.compress_masked(data, TOL, INF, mgard_amd.REL, config=cfg, restore_value=-9999.0)
    C = int(hl.masked_info(hbuf).container_size)
    m = hl.metadata_parse(hbuf[:C].tobytes())
    assert m["domain_decomposed"] and (shape[m["dd_dim"]] - 1) // m["dd_size"] + 1 >= 2
    buf = hbuf if where == "host" else torch.from_numpy(hbuf).cuda()
    plain = _np(hl.decompress(buf[:C], config=cfg))
    out = hl.decompress_masked(buf, config=cfg)
    assert isinstance(out, np.ndarray) == (where == "host")
    out = _np(out)
    assert out.dtype == dtype and out.shape == shape
    assert np.all(mm.int_view(out)[mask] == mm.int_view(np.array([-9999.0], dtype=dtype))[0])
    assert np.array_equal(mm.int_view(out)[~mask], mm.int_view(plain)[~mask])
    got_mask = hl.decompress_mask(buf, config=cfg)
    assert got_mask.dtype in (np.bool_, torch.bool) and np.array_equal(_np(got_mask), mask)
    for reader in (hl.decompress_masked, hl.decompress_mask):
        with pytest.raises(mgard_amd.MgardHipError, match="domain-decomposed"):
            reader(buf, config=cfg, level=0)


@pytest.mark.gpu
def test_kind_selection():
    """The lossless record of dictionary 256 carries 3136 bytes before its first code unit (24 + 16 chunks' table + 8
    + the decodebook's 8 (128 + 256) + 16), so at 35904 elements (4488 packed bytes) kind 1 can win only below 2.4
    bits a byte: a ball of 0.3 of every extent leaves three rows in four empty and is far below that; a 50 % random
    mask has 8 bits a byte and cannot. At 2210 elements (280 packed bytes) nothing can."""
    import mgard_amd
    from mgard_amd import highlevel as hl
    for (shape, dtype), kind in itertools.product(CASES, ["ball", "random50"]):
        data, mask, kw = _marked(shape, dtype, kind)
        info = hl.masked_info(hl.compress_masked(data, TOL, INF, mgard_amd.REL, config=_cfg(), **kw))
        packed = 8 * ((data.size + 63) // 64)
        print(shape, kind, "kind", info.kind, "R", info.record_size, "packed", packed)
        assert info.record_size <= packed and info.kind in (mm.PACKED, mm.CODED)
        if info.kind == mm.PACKED:
            assert info.record_size == packed         # the words as they are: none of the record's overhead
        if kind == "ball" and shape == (34, 33, 32):
            assert info.kind == mm.CODED and info.record_size < packed
        if shape == (17, 130):
            assert info.kind == mm.PACKED


@pytest.mark.gpu
def test_refusals_leave_the_library_usable():
    import mgard_amd
    from mgard_amd import highlevel as hl
    shape, dtype = CASES[0]
    data, mask, kw = _marked(shape, dtype, "ball")

    def usable():
        out = hl.decompress_masked(hl.compress_masked(data, TOL, INF, mgard_amd.REL, config=_cfg(), **kw), config=_cfg())
        assert np.isnan(out[mask]).all() and np.isfinite(out[~mask]).all()

    buf = hl.compress_masked(data, TOL, INF, mgard_amd.REL, config=_cfg(), **kw)
    C = int(hl.masked_info(buf).container_size)
    # a plain container has no footer
    assert hl.masked_info(buf[:C]) is None
    with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
        hl.decompress_masked(buf[:C], config=_cfg())
    usable()
    # a corrupted footer (C off by one), a corrupted record (its CRC), a buffer cut short in front
    for at in (len(buf) - mm.FOOTER_BYTES, C + 5):
        bad = buf.copy()
        bad[at] ^= 1
        with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
            hl.masked_info(bad)
        with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
            hl.decompress_masked(bad, config=_cfg())
        with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
            hl.decompress_mask(bad, config=_cfg())
    with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
        hl.decompress_masked(buf[1:], config=_cfg())
    assert hl.masked_info(buf[:-1]) is None
    usable()
    # a pre-allocated output that holds the container but not the record and the footer, and one that holds nothing
    for cap in (C + 10, len(buf) - 1, 40):
        with pytest.raises(mgard_amd.MgardHipError, match="error -7"):
            hl.compress_masked(data, TOL, INF, mgard_amd.REL, config=_cfg(), out=np.empty(cap, dtype=np.uint8), **kw)
    exact = hl.compress_masked(data, TOL, INF, mgard_amd.REL, config=_cfg(), out=np.empty(len(buf), dtype=np.uint8), **kw)
    assert len(exact) == len(buf)
    usable()
    # flags = 0, a NaN fill value, and an array that does not fit the footprint with its filled copy
    with pytest.raises(mgard_amd.MgardHipError, match="error -1"):
        hl.compress_masked(data, TOL, INF, mgard_amd.REL, config=_cfg(), nonfinite=False, fill_value=None)
    with pytest.raises(mgard_amd.MgardHipError, match="error -1"):
        hl.compress_masked(data, TOL, INF, mgard_amd.REL, config=_cfg(), nonfinite=True, fill_value=NAN)
    small = hl.Config(huff_dict_size=1024, max_memory_footprint=data.nbytes - 1)
    with pytest.raises(mgard_amd.MgardHipError, match="max_memory_footprint"):
        hl.compress_masked(data, TOL, INF, mgard_amd.REL, config=small, **kw)
    usable()
