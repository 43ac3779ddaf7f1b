"""mgh_compress_pwrel and its readers: |x' - x| <= eps |x| at EVERY valid element, evaluated in float64 NumPy with no
position left out and no tolerance on the tolerance; signs, zeroed and non-finite positions to the bit; the parts of
the buffer ([masked buffer of y][flag record][56-byte footer]) against tests/pwrel_model.py and the existing readers.
Fields smooth and rough in the exponent, and eps down to the smallest the rule accepts (pwrel_plan.hpp: a delta of 64
ulps of the largest |y|, below which the container's own rounding is not covered)."""
import numpy as np
import pytest

from tests import mask_model as mm
from tests import pwrel_model as pm

pytestmark = pytest.mark.gpu

CASES = [((34, 33, 32), np.float32), ((17, 130), np.float64), ((1000,), np.float64), ((5, 6, 7, 9), np.float32)]
IDS = ["34x33x32-f32", "17x130-f64", "1000-f64", "5x6x7x9-f32"]
EPS = {np.float32: (1e-1, 1e-3), np.float64: (1e-2, 1e-6, 1e-10)}
RUNS = [(s, d, e) for s, d in CASES for e in EPS[d]]
RUN_IDS = ["%s-%g" % (i, e) for (s, d), i in zip(CASES, IDS) for e in EPS[d]]


def _floor(dtype):
    return float(dtype(1e-20))


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _cfg(**kw):
    from mgard_amd import highlevel as hl
    return hl.Config(huff_dict_size=1024, **kw)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_round_trip(x, out, eps, fl):
    """The contract at every element, in float64. Returns the largest relative error."""
    assert out.dtype == x.dtype and out.shape == x.shape
    cls = pm.classify(x, fl)
    valid, zeroed, nonfin = cls == pm.VALID, cls == pm.ZEROED, cls == pm.NONFINITE
    assert np.all(mm.int_view(out)[zeroed] == 0)                  # +0.0 to the bit
    assert np.isnan(out[nonfin]).all()
    assert np.isfinite(out[valid]).all() and np.all(out[valid] != 0)
    assert np.array_equal(np.signbit(out[valid]), np.signbit(x[valid]))
    if not valid.any():
        return 0.0
    xd, od = x[valid].astype(np.float64), out[valid].astype(np.float64)
    rel = np.abs(od - xd) / np.abs(xd)
    print("max relative error %.6e, eps %.1e" % (rel.max(), eps))
    assert np.all(np.abs(od - xd) <= eps * np.abs(xd))            # every valid position
    return float(rel.max())


FIELDS = {"smooth": pm.smooth_field, "decades": pm.decades_field}       # smooth, and rough, in the exponent


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("shape,dtype,eps", RUNS, ids=RUN_IDS)
def test_round_trip(shape, dtype, eps, where):
    _round_trip(shape, dtype, eps, where, "smooth")


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("shape,dtype,eps", RUNS, ids=RUN_IDS)
def test_round_trip_rough_in_the_exponent(shape, dtype, eps, where):
    """test_round_trip's cases on pwrel_model.decades_field (its own function, so that the ids of test_round_trip stay
    what they were): neighbours differ by up to 60 (float32) or 600 (float64) decades, so every level has large
    coefficients and y' carries the quantizer's error at full size."""
    _round_trip(shape, dtype, eps, where, "decades")


def _round_trip(shape, dtype, eps, where, field):
    import mgard_amd
    from mgard_amd import highlevel as hl
    fl = _floor(dtype)
    x = FIELDS[field](shape, dtype, abs_floor=fl)
    src = x if where == "host" else _dev(x)
    keep = x.copy()
    buf = hl.compress_pwrel(src, eps, fl, config=_cfg())
    assert isinstance(buf, np.ndarray) == (where == "host")
    assert np.array_equal(mm.int_view(_np(src)), mm.int_view(keep))          # the caller's array is not modified
    out = hl.decompress_pwrel(buf, config=_cfg())
    assert isinstance(out, np.ndarray) == (where == "host")
    worst = _check_round_trip(x, _np(out), eps, fl)
    # verify: the same maximum as NumPy, within
    cmp, within = hl.verify_pwrel(buf, src, config=_cfg())
    want = pm.compare(x, _np(out), fl)
    assert within == 1 and cmp.max_rel_err == worst == want["max_rel_err"]
    assert (cmp.n, cmp.n_valid, cmp.n_zeroed, cmp.n_nonfinite) == (x.size, want["n_valid"], want["n_zeroed"], want["n_nonfinite"])
    assert (cmp.n_class_mismatch, cmp.n_sign_mismatch) == (0, 0) and cmp.max_zeroed_abs == want["max_zeroed_abs"] < fl
    # info: the footer's fields, the counts, and the delta of the plan for the device's own ybound
    mask, flag = pm.bitmaps(x, fl)
    y, _, _, st = mgard_amd.pwrel_forward(_dev(x), fl)
    info = hl.pwrel_info(buf)
    foot = pm.parse_footer(_np(buf))
    delta = pm.abs_tolerance(dtype, eps, max(abs(st.ymin), abs(st.ymax)))
    assert (info.eps, info.abs_floor, info.delta) == (eps, fl, delta)
    assert (info.n_masked, info.n_flag) == (int(mask.sum()), int(flag.sum())) == (st.n_masked, st.n_flag)
    M, S, C = int(info.masked_size), int(info.flag_record_size), int(info.container_size)
    assert M + S + pm.FOOTER_BYTES == len(buf) and (foot["masked"], foot["record"], foot["kind"]) == (M, S, info.flag_kind)
    assert _np(buf)[-pm.FOOTER_BYTES:].tobytes() == pm.footer(M, _np(buf)[M:M + S].tobytes(), int(flag.sum()), eps, fl, info.flag_kind)
    # the first M bytes are a masked buffer of y (restore value 0), the whole buffer is not one
    minfo = hl.masked_info(buf[:M])
    assert minfo is not None and hl.masked_info(buf) is None
    assert (minfo.container_size, minfo.n_masked, minfo.kind, minfo.restore_value) == (C, int(mask.sum()), info.mask_kind, 0.0)
    assert np.array_equal(_np(hl.decompress_mask(buf[:M])), mask)
    # the container part holds the filled y within delta
    yd = _np(hl.decompress(buf[:C], config=_cfg())).astype(np.float64)
    filled = mm.fill(_np(y), mask, mm.fill_constant(_np(y), mask)).astype(np.float64)
    assert np.max(np.abs(yd - filled)) <= delta
    ym = _np(hl.decompress_masked(buf[:M], config=_cfg()))
    assert np.all(mm.int_view(ym)[mask] == 0) and np.array_equal(mm.int_view(ym)[~mask], mm.int_view(yd.astype(dtype))[~mask])


def test_rel_of_the_whole_array_does_not_keep_the_pointwise_bound():
    """What the feature is for: on a field of many decades a REL bound of 1e-3 (relative to the array's norm) leaves the
    small values with a pointwise relative error far above 1e-3."""
    import mgard_amd
    from mgard_amd import highlevel as hl
    shape, dtype = CASES[0]
    x = pm.smooth_field(shape, dtype, planted=False)
    out = hl.decompress(hl.compress(x, 1e-3, mgard_amd.INF, mgard_amd.REL, config=_cfg()), config=_cfg())
    rel = np.abs(out.astype(np.float64) - x.astype(np.float64)) / np.abs(x.astype(np.float64))
    print("REL 1e-3: max pointwise relative error %.3e" % rel.max())
    assert rel.max() > 1e-3
    _check_round_trip(x, hl.decompress_pwrel(hl.compress_pwrel(x, 1e-3, config=_cfg()), config=_cfg()), 1e-3, 0.0)


@pytest.mark.parametrize("shape,dtype", CASES[:2], ids=IDS[:2])
def test_all_zero_all_negative_and_nothing_to_record(shape, dtype):
    import mgard_amd
    from mgard_amd import highlevel as hl
    eps = 1e-3
    # all zero: everything is zeroed, delta = log2(1 + eps), both records say so
    z = np.zeros(shape, dtype=dtype)
    buf = hl.compress_pwrel(z, eps, config=_cfg())
    info = hl.pwrel_info(buf)
    assert (info.n_masked, info.n_flag, info.flag_kind, info.delta) == (z.size, 0, mm.NONE, pm.log2_1p(eps))
    out = hl.decompress_pwrel(buf, config=_cfg())
    assert np.all(mm.int_view(out) == 0)
    assert hl.verify_pwrel(buf, z, config=_cfg())[1] == 1
    # all negative: every flag bit is set
    neg = -np.abs(pm.smooth_field(shape, dtype, planted=False))
    buf = hl.compress_pwrel(neg, eps, config=_cfg())
    info = hl.pwrel_info(buf)
    assert (info.n_masked, info.n_flag, info.mask_kind) == (0, neg.size, mm.NONE) and info.flag_kind != mm.NONE
    _check_round_trip(neg, hl.decompress_pwrel(buf, config=_cfg()), eps, 0.0)
    # no negative, nothing masked: both kinds 2, and the container is mgh_compress(y, ABS, delta) byte for byte
    pos = np.abs(neg)
    buf = hl.compress_pwrel(pos, eps, config=_cfg())
    info = hl.pwrel_info(buf)
    assert (info.mask_kind, info.flag_kind, info.n_masked, info.n_flag) == (mm.NONE, mm.NONE, 0, 0)
    C = int(info.container_size)
    assert len(buf) == C + mm.FOOTER_BYTES + pm.FOOTER_BYTES
    y, _, _, st = mgard_amd.pwrel_forward(_dev(pos))
    delta = pm.abs_tolerance(dtype, eps, max(abs(st.ymin), abs(st.ymax)))
    ref = hl.compress(y, delta, mgard_amd.INF, mgard_amd.ABS, config=_cfg())
    assert info.delta == delta and np.array_equal(buf[:C], _np(ref))
    _check_round_trip(pos, hl.decompress_pwrel(buf, config=_cfg()), eps, 0.0)


def test_domain_decomposed():
    """Blocks of 33 on 70 x 45 x 37, forced like tests/test_gpu_masked_views.py forces its decomposed case."""
    from mgard_amd import highlevel as hl
    shape, dtype = (70, 45, 37), np.float32
    fl, eps = _floor(dtype), 1e-3
    x = pm.smooth_field(shape, dtype, abs_floor=fl)
    cfg = _cfg(domain_decomposition=hl.DD_BLOCK, block_size=33)
    buf = hl.compress_pwrel(x, eps, fl, config=cfg)
    C = int(hl.pwrel_info(buf).container_size)
    assert hl.metadata_parse(buf[:C].tobytes())["domain_decomposed"]
    _check_round_trip(x, hl.decompress_pwrel(buf, config=cfg), eps, fl)
    assert hl.verify_pwrel(buf, x, config=cfg)[1] == 1


def _device_y(x, fl):
    """(the filled y the container holds, the mask, ybound), from the device's own forward pass"""
    import mgard_amd
    y, _, _, st = mgard_amd.pwrel_forward(_dev(x), fl)
    mask, _ = pm.bitmaps(x, fl)
    return mm.fill(_np(y), mask, mm.fill_constant(_np(y), mask)), mask, max(abs(st.ymin), abs(st.ymax))


def _at_the_limit(x, fl, cfg, multiples=(1.0, 2.0), lossy=False):
    """Compress at the smallest eps the rule accepts for the device's own ybound (pm.smallest_accepted_eps: within 1 %
    of it) and at its multiples: the bound at every valid element, verify, and the model's delta. 0.9 of it is
    refused. lossy: the container must not have stored y as it is (y' differs from y somewhere)."""
    import mgard_amd
    from mgard_amd import highlevel as hl
    filled, mask, yb = _device_y(x, fl)
    e0 = pm.smallest_accepted_eps(x.dtype, yb)
    u = pm.ulp(x.dtype, yb)
    for k in multiples:
        eps = k * e0
        buf = hl.compress_pwrel(x, eps, fl, config=cfg)
        info = hl.pwrel_info(buf)
        delta = pm.abs_tolerance(x.dtype, eps, yb)
        assert info.delta == delta >= pm.K_MIN * u
        yd = _np(hl.decompress(buf[:int(info.container_size)], config=cfg)).astype(np.float64)
        err = float(np.max(np.abs(yd - filled.astype(np.float64))[~mask])) if (~mask).any() else 0.0
        print("ybound %.6f  eps %.6e  delta %.2f ulp  max|y' - y| %.2f ulp  container %d bytes of %d"
              % (yb, eps, delta / u, err / u, info.container_size, x.nbytes))
        assert err <= pm.budget(x.dtype, eps, yb) and (err > 0 or not lossy)
        rel = _check_round_trip(x, _np(hl.decompress_pwrel(buf, config=cfg)), eps, fl)
        cmp, within = hl.verify_pwrel(buf, x, config=cfg)
        assert within == 1 and cmp.max_rel_err == rel and (cmp.n_class_mismatch, cmp.n_sign_mismatch) == (0, 0)
    with pytest.raises(mgard_amd.MgardHipError, match="cannot carry"):
        hl.compress_pwrel(x, 0.9 * e0, fl, config=cfg)


LIMIT_CASES = [((5, 6, 7, 9), np.float32), ((34, 33, 32), np.float32), ((5, 6, 7, 9), np.float64), ((17, 130), np.float64)]
LIMIT_IDS = ["5x6x7x9-f32", "34x33x32-f32", "5x6x7x9-f64", "17x130-f64"]


@pytest.mark.parametrize("field", list(FIELDS))
@pytest.mark.parametrize("shape,dtype", LIMIT_CASES, ids=LIMIT_IDS)
def test_bound_holds_down_to_the_refusal_limit(shape, dtype, field):
    """The bound at the smallest eps the rule accepts (a delta of 64 ulps of the largest |y|), at twice that eps, and the
    refusal at 0.9 of it; eps comes from the model's rule and the device's own ybound, none is written down here.

    The container's guarantee |y' - y| <= delta holds in exact arithmetic; decomposing, quantizing and recomposing in T
    costs up to 19 ulps more at a delta of a few ulps (tests/test_pwrel_rounding_cpu.py has the measurement). The
    rule of the commit before this test accepted such deltas: 34x33x32 float32 smooth at eps = 1.3e-5 (651 of 35904
    elements over eps, the largest 2.7 eps) and 5x6x7x9 float32 smooth at eps = 3e-5 (11 of 1890, 2.6 eps) were
    accepted and break the bound. Those figures were PREDICTED with the CPU oracle, to which tests/test_gpu_parity.py
    pins the GPU transform; they were not observed on a GPU, and with this library's writer they cannot be: on the GPU
    the container of each of these shapes came out larger than the array at every eps tried (0.1 down to the limit) and
    was stored as it is, so y' = y and only the roundings of log2 and exp2 remain. What WAS observed on the GPU is the
    container exceeding its delta where it does quantize (test_container_exceeds_a_delta_of_one_and_two_ulps), and the
    cases that quantize at the limit are test_bound_holds_at_the_refusal_limit_where_the_container_is_lossy. Both eps
    are refused now."""
    fl = _floor(dtype)
    _at_the_limit(FIELDS[field](shape, dtype, abs_floor=fl), fl, _cfg())


def test_bound_holds_at_the_refusal_limit_with_a_third_of_the_elements_zeroed():
    """The fill at masked positions enters the transform of y, so its rounding is not what the all-valid CPU table
    measures: 30 % of a decades field below abs_floor, at the smallest accepted eps."""
    shape, dtype = (34, 33, 32), np.float32
    fl = float(dtype(1e-12))
    x = pm.decades_field(shape, dtype, abs_floor=fl)
    zeroed = float((pm.classify(x, fl) == pm.ZEROED).mean())
    assert 0.27 < zeroed < 0.33
    _at_the_limit(x, fl, _cfg(), multiples=(1.0,))


def test_domain_decomposed_at_the_refusal_limit():
    """test_domain_decomposed's blocks at the smallest accepted eps: every block has a hierarchy of its own and all
    share one delta."""
    from mgard_amd import highlevel as hl
    shape, dtype = (70, 45, 37), np.float32
    fl = _floor(dtype)
    cfg = _cfg(domain_decomposition=hl.DD_BLOCK, block_size=33)
    for field in FIELDS:
        x = FIELDS[field](shape, dtype, abs_floor=fl)
        _at_the_limit(x, fl, cfg, multiples=(1.0,))
    buf = hl.compress_pwrel(x, pm.smallest_accepted_eps(dtype, _device_y(x, fl)[2]), fl, config=cfg)
    assert hl.metadata_parse(buf[:int(hl.pwrel_info(buf).container_size)].tobytes())["domain_decomposed"]


LOSSY_CASES = [((100001,), 1024), ((513, 513), 8192)]


@pytest.mark.parametrize("shape,dict_size", LOSSY_CASES, ids=["100001-dict1024", "513x513-dict8192"])
def test_bound_holds_at_the_refusal_limit_where_the_container_is_lossy(shape, dict_size):
    """A container that would come out larger than the array stores it as it is, and y' = y: that is what happens to
    every case of test_bound_holds_down_to_the_refusal_limit (observed on the GPU: each container is the array plus its
    header), because at a delta of 64 ulps the quantized coefficients of a field that is not smooth to 12 bits all lie
    outside the dictionary. These fields are: float32, smooth, 100001 and 513 x 513 (float64 is always stored as it
    is at this delta). Here the container quantizes, and y' differs from y: at the limit, twice it, and 16 and 128
    times it (eps about 1e-2 and 9e-2), which no other test of this file reaches with a quantizing container."""
    from mgard_amd import highlevel as hl
    dtype = np.float32
    fl = _floor(dtype)
    _at_the_limit(pm.smooth_field(shape, dtype, abs_floor=fl), fl, hl.Config(huff_dict_size=dict_size),
                  multiples=(1.0, 2.0, 16.0, 128.0), lossy=True)


def test_container_exceeds_a_delta_of_one_and_two_ulps():
    """Why the rule refuses small deltas, observed on the GPU: mgh_compress of y = log2|x| (float32, smooth, 100001, all
    valid) under ABS, s = inf at delta = 1 and 2 ulps of the largest |y| comes back with max |y' - y| 2 and 1 ulps ABOVE
    delta -- the oracle's figures to the bit (tests/test_pwrel_rounding_cpu.py) -- and at 64 ulps far below it."""
    import mgard_amd
    from mgard_amd import highlevel as hl
    x = pm.smooth_field((100001,), np.float32, planted=False)
    y, mask, yb = _device_y(x, 0.0)
    assert not mask.any() and np.array_equal(y, pm.forward(x))
    u = pm.ulp(np.float32, yb)
    ms = [1, 2, 64]
    got = []
    for m in ms:
        yd = hl.decompress(hl.compress(y, m * u, mgard_amd.INF, mgard_amd.ABS, config=_cfg()), config=_cfg())
        got.append(float(np.max(np.abs(yd.astype(np.float64) - y.astype(np.float64)))))
    _, want = pm.oracle_y_errors(x, [m * u for m in ms])
    print("excess over delta, ulps:", [(g - m * u) / u for g, m in zip(got, ms)])
    assert got == want and got[0] > 1 * u and got[1] > 2 * u and 0 < got[2] < 64 * u


def test_refusals_leave_the_library_usable():
    import mgard_amd
    from mgard_amd import highlevel as hl
    shape, dtype = CASES[0]
    fl, eps = _floor(dtype), 1e-3
    x = pm.smooth_field(shape, dtype, abs_floor=fl)

    def usable():
        _check_round_trip(x, hl.decompress_pwrel(hl.compress_pwrel(x, eps, fl, config=_cfg()), config=_cfg()), eps, fl)

    for bad in (0.0, 1.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(mgard_amd.MgardHipError, match="error -1"):
            hl.compress_pwrel(x, bad, fl, config=_cfg())
    # float32 cannot carry 1e-7: refused, never a looser bound
    with pytest.raises(mgard_amd.MgardHipError, match="cannot carry"):
        hl.compress_pwrel(x, 1e-7, fl, config=_cfg())
    with pytest.raises(mgard_amd.MgardHipError, match="error -1"):
        hl.compress_pwrel(x, eps, -1.0, config=_cfg())
    usable()
    buf = hl.compress_pwrel(x, eps, fl, config=_cfg())
    info = hl.pwrel_info(buf)
    M, C = int(info.masked_size), int(info.container_size)
    assert info.flag_record_size > 0
    # a plain container and a masked buffer are not such buffers
    for other in (buf[:C], buf[:M]):
        assert hl.pwrel_info(other) is None
        with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
            hl.decompress_pwrel(other, config=_cfg())
        with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
            hl.verify_pwrel(other, x, config=_cfg())
    usable()
    # a flipped byte in the flag record: its CRC; a corrupted footer; a buffer cut short in front and behind
    bad = buf.copy()
    bad[M + 3] ^= 1
    with pytest.raises(mgard_amd.MgardHipError, match="CRC32"):
        hl.decompress_pwrel(bad, config=_cfg())
    with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
        hl.pwrel_info(bad)
    bad = buf.copy()
    bad[len(buf) - pm.FOOTER_BYTES] ^= 1
    with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
        hl.decompress_pwrel(bad, config=_cfg())
    with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
        hl.decompress_pwrel(buf[1:], config=_cfg())
    assert hl.pwrel_info(buf[:-1]) is None
    with pytest.raises(mgard_amd.MgardHipError, match="error -8"):
        hl.decompress_pwrel(buf[:-1], config=_cfg())
    usable()
    # a pre-allocated output one byte too small, and one that fits exactly
    for cap in (len(buf) - 1, M + 10, 60):
        with pytest.raises(mgard_amd.MgardHipError, match="error -7"):
            hl.compress_pwrel(x, eps, fl, config=_cfg(), out=np.empty(cap, dtype=np.uint8))
    exact = hl.compress_pwrel(x, eps, fl, config=_cfg(), out=np.empty(len(buf), dtype=np.uint8))
    assert np.array_equal(exact, buf)
    # the footprint, and an original of another type or size in verify
    with pytest.raises(mgard_amd.MgardHipError, match="max_memory_footprint"):
        hl.compress_pwrel(x, eps, fl, config=_cfg(max_memory_footprint=x.nbytes - 1))
    with pytest.raises(mgard_amd.MgardHipError, match="error -1"):
        hl.verify_pwrel(buf, x.astype(np.float64), config=_cfg())
    usable()
