"""GPU tests of compression to a measured error target: mgh_quantize_roundtrip against the
quantizer and dequantizer it fuses, mgh_achieved_errors against mgh_verify of the containers mgh_compress
writes, mgh_compress_target against the walk restated with compress + verify per candidate, and the edges.

Every comparison is an equality of bits or of integers, or an inequality the search guarantees by
construction. The containers compared are Huffman records: where the writer stores the array itself (a RAW
record: it is exact) the candidate's statistics are the quantizer's, an upper bound -- the documented limit of
mgh_achieved_errors --, which the small dictionaries and coarse tolerances here stay clear of and which
test_a_raw_container_is_exact_and_the_candidate_bounds_it pins on its own."""
import ctypes as C

import numpy as np
import pytest

from tests import payload as pl
from tests.test_gpu_budget import _tolerances
from tests.util import BLOCK, nonuniform_coords, smooth_field

pytestmark = pytest.mark.gpu

INF = float("inf")
F32, F64 = np.float32, np.float64
FUSED3 = (34, 33, 32)  # takes the fused level kernels in mgh_compress (tests/test_gpu_decompose_quantize_routes.py)
SMALL = (33, 17, 20)   # rows of 20 elements: 16-byte vectors straddle rows
MGH_ERR_INVALID_ARGUMENT, MGH_ERR_TARGET_NOT_MET = -1, -9
FIELDS = ("n", "nonfinite", "max_abs_err", "argmax", "sum_sq_err", "ref_min", "ref_max", "ref_abs_max", "ref_sum_sq")
EXACT = ("n", "nonfinite", "max_abs_err", "argmax")


def _gpu():
    import torch
    import mgard_amd
    from mgard_amd import highlevel
    return torch, mgard_amd, highlevel


def _bits(x):
    return int(x) if isinstance(x, (int, np.integer)) else float(x).hex()


def _same(got, want, fields=FIELDS):
    return [(k, getattr(got, k), getattr(want, k)) for k in fields if _bits(getattr(got, k)) != _bits(getattr(want, k))]


def _int_view(t):
    import torch
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64).cpu().numpy()


# ---- 1. the round trip is the quantizer's ------------------------------------------------------------------
# (shape, dtype, non-uniform grid, coefficient tensor starts one element into its allocation)
ROUND_CASES = [
    ((1001,), F32, False, False),
    ((1001,), F64, False, True),
    ((65, 40), F32, False, True),
    ((65, 40), F64, False, False),
    (SMALL, F32, False, False),
    (SMALL, F64, False, False),
    (SMALL, F32, True, False),
    (FUSED3, F32, False, False),
    (FUSED3, F64, True, False),
    ((5, 9, 9, 17), F32, False, False),
    ((5, 9, 9, 17), F64, False, True),
    ((3, 3, 5, 5, 9), F64, False, False),
    ((3, 3, 5, 5, 9), F32, False, True),
]


@pytest.mark.parametrize("shape,dt,nonuniform,offset", ROUND_CASES)
def test_roundtrip_is_dequantize_of_quantize(shape, dt, nonuniform, offset):
    torch, mg, _ = _gpu()
    h = mg.Hierarchy(shape, dt, coords=nonuniform_coords(shape, dt) if nonuniform else None)
    d = torch.from_numpy(smooth_field(shape, dt)).cuda()
    dense = h.decompose(d)
    n = int(np.prod(shape))
    c = dense
    if offset:  # the misaligned scalar route: a view that starts one element into an allocation
        store = torch.empty(n + 1, dtype=dense.dtype, device=dense.device)
        c = store[1:].view(shape)
        c.copy_(dense)
        assert c.data_ptr() % 16 != 0 and c.is_contiguous()
    tols = _tolerances(5)
    for rel in (False, True):
        eb = mg.REL if rel else mg.ABS
        for s in (INF, 0.0, 1.0):
            norm = h.norm(d, s) if rel else 1.0
            for k, tol in enumerate(tols):
                what = (shape, np.dtype(dt).name, "REL" if rel else "ABS", s, tol)
                got = _int_view(h.quantize_roundtrip(c, eb, tol, s, norm))
                for dict_size, prep in ((64, True), (8192, True), (8192, False)):
                    q, oi, ov, nout = h.quantize(dense, eb, tol, s, norm, dict_size=dict_size, prep_huffman=prep)
                    want = _int_view(h.dequantize(q, eb, tol, s, norm, dict_size=dict_size, prep_huffman=prep,
                                                  outlier_idx=oi, outlier_val=ov))
                    assert np.array_equal(got, want), (what, dict_size, prep, np.nonzero((got != want).ravel())[0][:8])
                    if dict_size == 64 and k == 0:
                        assert nout > 0.9 * n, what       # (nearly every value travels through the outlier list)
                if k == len(tols) - 1:
                    assert not got.any(), what            # (everything quantizes to zero)
                # in place
                work = c.clone() if not offset else c
                keep = c.clone()
                assert np.array_equal(_int_view(h.quantize_roundtrip(work, eb, tol, s, norm, out=work)), got), what
                if offset:
                    c.copy_(keep)
    # a pitched input (mgh_set_ld) gives the same array
    if len(shape) > 1:
        ld = list(shape)
        ld[-1] += 3
        if len(shape) > 2:
            ld[-2] += 1
        pitched = torch.zeros([shape[0]] + ld[1:], dtype=dense.dtype, device=dense.device)
        pitched[tuple(slice(0, m) for m in shape)] = dense
        norm = h.norm(d, 0.0)
        want = _int_view(h.quantize_roundtrip(dense, mg.REL, 1e-3, 0.0, norm))
        h.set_ld(mg.LD_IN, ld)
        got = _int_view(h.quantize_roundtrip(pitched, mg.REL, 1e-3, 0.0, norm))
        h.set_ld(mg.LD_IN, None)
        assert got.shape == want.shape and np.array_equal(got, want)
    h.close()


# ---- 2. candidates are containers ----------------------------------------------------------------------------
def _config(hl, dict_size, **kw):
    cfg = hl.Config(**kw)
    cfg.huff_dict_size = dict_size
    return cfg


def _is_raw(hl, buf, u):
    b = bytes(buf.cpu().numpy() if hasattr(buf, "cpu") else buf)
    recs = pl.split_container(b, hl.metadata_parse(b)["metadata_size"])
    assert len(recs) == 1
    return len(recs[0]) == u.nbytes


def _canonical(hl, buf):
    """A container of one Huffman record, byte for byte, with ONE freedom taken out: the order of the (index,
    value) pairs of the outlier lists, which is the order of the quantizer's atomics and differs between two
    runs of mgh_compress on the same input (tests/test_gpu_cpp_budget.py says the same of its containers).
    Everything else -- header, sizes, code tables, chunk table, code units, synchronisation points, the SET of
    outliers -- is compared as bytes."""
    b = bytes(buf.cpu().numpy() if hasattr(buf, "cpu") else buf)
    meta = hl.metadata_parse(b)["metadata_size"]
    (rec,) = pl.split_container(b, meta)
    r = pl.parse_huffman_record(rec)
    order = np.argsort(r["outlier_idx"], kind="stable")
    fields = [b[:meta + 8], len(b)]
    for k in sorted(r):
        v = r[k]
        if k in ("outlier_idx", "outliers"):
            v = v[order]
        fields.append((k, v.tobytes() if hasattr(v, "tobytes") else v))
    return fields


# (shape, dtype, REL?, s, dictionary, non-uniform grid, extra configuration, log10 of the first and the last of
# five log-spaced tolerances). Arrays this small are stored RAW at fine tolerances (the record's fixed part and
# its 16-byte outliers outweigh them): the dictionaries and the ranges are those at which the writer was seen to
# keep a Huffman record, which every case asserts of at least three of its tolerances.
ACH_CASES = [
    ((1001,), F64, False, INF, 64, False, {}, (-2.5, -0.5)),
    ((65, 40), F32, True, INF, 256, False, {}, (-1.0, 1.0)),
    (SMALL, F64, True, INF, 256, False, {}, (-1.0, 1.0)),
    (SMALL, F32, False, INF, 1024, True, {}, (-1.0, 1.0)),
    (SMALL, F32, True, 0.0, 256, False, {}, (-2.0, 0.0)),
    (FUSED3, F32, True, INF, 1024, False, {}, (-1.5, 0.5)),
    (FUSED3, F64, False, INF, 1024, False, {}, (-1.5, 0.5)),
    (FUSED3, F32, True, 0.0, 1024, False, {}, (-2.5, -0.5)),
    (FUSED3, F32, True, INF, 1024, False, {"lossless": 2}, (-2.5, -0.5)),
    (FUSED3, F64, True, INF, 1024, False, {"reorder": 1}, (-1.5, 0.5)),
    ((5, 9, 9, 17), F32, False, INF, 1024, False, {}, (-0.5, 1.0)),
    ((3, 3, 5, 5, 9), F64, True, INF, 1024, False, {}, (-0.5, 1.0)),
]
_lossy_seen = []


@pytest.mark.parametrize("shape,dt,rel,s,dict_size,nonuniform,extra,decades", ACH_CASES)
def test_achieved_errors_are_verify_of_the_containers(shape, dt, rel, s, dict_size, nonuniform, extra, decades):
    torch, mg, hl = _gpu()
    ACH_TOLS = [float(t) for t in np.logspace(decades[0], decades[1], 5)]
    u = smooth_field(shape, dt)
    coords = nonuniform_coords(shape, dt) if nonuniform else None
    cfg = _config(hl, dict_size, **extra)
    mode = mg.REL if rel else mg.ABS
    d = torch.from_numpy(u).cuda()
    on_dev = hl.achieved_errors(d, ACH_TOLS, s, mode, coords=coords, config=cfg)
    on_host = hl.achieved_errors(u, ACH_TOLS, s, mode, coords=coords, config=cfg)
    assert len(on_dev) == len(on_host) == len(ACH_TOLS)
    huffman = 0
    for tol, got_d, got_h in zip(ACH_TOLS, on_dev, on_host):
        buf = hl.compress(d, tol, s, mode, coords=coords, config=cfg)
        raw = _is_raw(hl, buf, u)
        want_d = hl.verify(buf, d, config=cfg)
        want_h = hl.verify(hl.compress(u, tol, s, mode, coords=coords, config=cfg), u, config=cfg)
        print(shape, np.dtype(dt).name, "REL" if rel else "ABS", s, tol, "raw" if raw else "huffman", got_d, want_d.stats)
        if raw:  # (exact; the candidate is the quantizer's error, within the bound: the documented limit)
            assert want_d.stats.max_abs_err == 0 and got_d.nonfinite == 0
            if s == INF:
                assert got_d.max_abs_err <= want_d.bound
            continue
        huffman += 1
        assert not _same(got_d, want_d.stats), (tol, _same(got_d, want_d.stats))
        assert not _same(got_h, want_h.stats, EXACT), (tol, _same(got_h, want_h.stats, EXACT))
        assert want_d.within == 1
        _lossy_seen.append(got_d.max_abs_err > 0)
    assert huffman >= 3, "the case must compare Huffman records"
    hl._hl().mgh_release_cache()


def test_achieved_errors_compared_lossy_containers():
    assert _lossy_seen and all(_lossy_seen)


def test_a_raw_container_is_exact_and_the_candidate_bounds_it():
    """The documented limit: at a tolerance whose record does not shrink, mgh_compress stores the array itself.
    mgh_verify then reports a zero error; the candidate reports the quantizer's, which keeps the bound."""
    torch, mg, hl = _gpu()
    u = smooth_field(SMALL, F32)
    d = torch.from_numpy(u).cuda()
    buf = hl.compress(d, 1e-3, INF, mg.REL)
    assert _is_raw(hl, buf, u)
    r = hl.verify(buf, d)
    (got,) = hl.achieved_errors(d, [1e-3], INF, mg.REL)
    assert r.stats.max_abs_err == 0 and 0 < got.max_abs_err <= r.bound
    assert not _same(got, r.stats, ("n", "nonfinite", "ref_min", "ref_max", "ref_abs_max", "ref_sum_sq"))
    hl._hl().mgh_release_cache()


# ---- 3. the search -----------------------------------------------------------------------------------------------
# (two decades each, inside the range in which these arrays are Huffman records at this dictionary)
SEARCH_SETUPS = {"fused-f32": (FUSED3, F32, True, 1024, 5e-2, 5e0), "small-f64": (SMALL, F64, False, 1024, 8e-2, 8e0)}
_verified = {}


def _verify_of(name, tol):
    """stats of verify(compress(tol)) for a device-resident original, once per tolerance: code that exists
    without the feature."""
    torch, mg, hl = _gpu()
    shape, dt, rel, dict_size, _, _ = SEARCH_SETUPS[name]
    key = (name, float(tol))
    if key not in _verified:
        d = torch.from_numpy(smooth_field(shape, dt)).cuda()
        cfg = _config(hl, dict_size)
        buf = hl.compress(d, float(tol), INF, mg.REL if rel else mg.ABS, config=cfg)
        assert not _is_raw(hl, buf, smooth_field(shape, dt)), (name, tol)
        _verified[key] = (hl.verify(buf, d, config=cfg).stats, _canonical(hl, buf))
    return _verified[key]


def _figure(st, metric):
    return (st.max_abs_err, st.rmse, st.psnr)[metric]


def _meets(st, metric, target):
    if st.nonfinite:
        return False
    return _figure(st, metric) >= target if metric == 2 else _figure(st, metric) <= target


@pytest.fixture(scope="module", autouse=True)
def _drop_verified():
    yield
    _verified.clear()


@pytest.mark.parametrize("rounds", [1, 8])
@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(SEARCH_SETUPS))
def test_compress_target_walks_the_restated_search(name, metric, rounds):
    torch, mg, hl = _gpu()
    shape, dt, rel, dict_size, tol_min, tol_max = SEARCH_SETUPS[name]
    mode = mg.REL if rel else mg.ABS
    cfg = _config(hl, dict_size)
    d = torch.from_numpy(smooth_field(shape, dt)).cuda()
    lo, hi = _figure(_verify_of(name, tol_min)[0], metric), _figure(_verify_of(name, tol_max)[0], metric)
    # between the ends, so that neither decides: geometric mean of the errors, arithmetic mean of the dB values
    target = 0.5 * (lo + hi) if metric == 2 else float(np.sqrt(lo) * np.sqrt(hi))
    assert (hi < target < lo) if metric == 2 else (lo < target < hi), (lo, target, hi)
    # the walk, with compress + verify per candidate
    assert not _meets(_verify_of(name, tol_max)[0], metric, target) and _meets(_verify_of(name, tol_min)[0], metric, target)
    a, b = np.float64(tol_min), np.float64(tol_max)
    for _ in range(rounds):
        m = np.sqrt(a) * np.sqrt(b)
        if _meets(_verify_of(name, m)[0], metric, target):
            a = m
        else:
            b = m
    buf, tol_used, stats, candidates = hl.compress_target(d, metric, target, tol_min, tol_max, rounds=rounds, s=INF,
                                                          mode=mode, config=cfg)
    print(name, metric, rounds, "target", target, "tol", tol_used, "b", float(b), stats)
    assert float(tol_used).hex() == float(a).hex(), (tol_used, float(a))
    assert candidates == 2 + rounds
    want_stats, want_bytes = _verify_of(name, a)
    assert _canonical(hl, buf) == want_bytes               # the writer's container, byte for byte (_canonical)
    assert not _same(stats, want_stats), _same(stats, want_stats)
    assert not _same(hl.verify(buf, d, config=cfg).stats, want_stats)
    assert _meets(stats, metric, target)
    assert not _meets(_verify_of(name, b)[0], metric, target)  # the bracket's other end does not meet the target
    hl._hl().mgh_release_cache()


# ---- 4. edges ------------------------------------------------------------------------------------------------------
def _target_rc(hl, u, metric, target, tol_min, tol_max, rounds, cfg, s=INF, mode=0):
    """The C call itself, output NOT pre-allocated: (status, output pointer, tol_used, candidates)."""
    L = hl._hl()
    out, size, used, cand = C.c_void_p(0xdead0), C.c_size_t(0), C.c_double(-1.0), C.c_int(-1)
    shp = (C.c_uint64 * u.ndim)(*u.shape)
    rc = L.mgh_compress_target(u.ndim, 0 if u.dtype == np.float32 else 1, shp, metric, target, tol_min, tol_max, rounds, s,
                               mode, C.c_void_p(u.ctypes.data), C.byref(out), C.byref(size), None, C.byref(cfg), 0,
                               C.byref(used), None, C.byref(cand))
    return rc, out.value, used.value, cand.value


def test_edges_and_refusals_leave_the_library_usable():
    torch, mg, hl = _gpu()
    u = smooth_field(SMALL, F32)
    ok = _config(hl, 1024)

    def round_trip(cfg=ok):
        v = hl.decompress(hl.compress(u, 1e-3, INF, mg.REL, config=cfg), config=cfg)
        assert float(np.max(np.abs(v - u))) <= 1e-3 * float(np.max(np.abs(u)))

    # so loose that tol_max meets it: one candidate
    for metric, target in ((0, 1e30), (1, 1e30), (2, -1e30)):
        buf, tol_used, stats, candidates = hl.compress_target(u, metric, target, 1e-3, 1.0, rounds=4, config=ok)
        assert tol_used == 1.0 and candidates == 1
        assert _canonical(hl, buf) == _canonical(hl, hl.compress(u, 1.0, INF, mg.REL, config=ok))
        assert not _same(stats, hl.verify(buf, u, config=ok).stats, EXACT)
    # so tight that tol_min fails: its own status, nothing allocated, the pointer untouched
    for metric, target in ((0, 0.0), (1, 1e-300), (2, 1e4)):
        rc, out, used, cand = _target_rc(hl, u, metric, target, 1e-1, 1.0, 4, ok)
        assert rc == MGH_ERR_TARGET_NOT_MET and out == 0xdead0 and used == -1.0, (metric, rc)
        assert b"tol_min" in hl._hl().mgh_last_error()
        round_trip()
    with pytest.raises(mg.MgardHipError, match="error %d: compress_target: " % MGH_ERR_TARGET_NOT_MET):
        hl.compress_target(u, 0, 0.0, 1e-1, 1.0, config=ok)
    # a configuration that decomposes the domain
    decomposing = _config(hl, 256, domain_decomposition=BLOCK, block_size=11)  # 3 x 2 x 2 subdomains
    rc, out, _, _ = _target_rc(hl, u, 0, 1e-2, 1e-3, 1e-1, 4, decomposing)
    assert rc == MGH_ERR_INVALID_ARGUMENT and out == 0xdead0
    with pytest.raises(mg.MgardHipError, match="error %d: achieved errors: " % MGH_ERR_INVALID_ARGUMENT):
        hl.achieved_errors(u, [1e-3], config=decomposing)
    round_trip(decomposing)
    # arguments
    nan = float("nan")
    for metric, target, tol_min, tol_max, rounds in ((-1, 1e-2, 1e-3, 1e-1, 4), (3, 1e-2, 1e-3, 1e-1, 4), (0, nan, 1e-3, 1e-1, 4),
                                                     (0, 1e-2, 0.0, 1e-1, 4), (0, 1e-2, -1e-3, 1e-1, 4), (0, 1e-2, 1e-1, 1e-3, 4),
                                                     (0, 1e-2, nan, 1e-1, 4), (0, 1e-2, 1e-3, INF, 4), (0, 1e-2, 1e-3, 1e-1, 0),
                                                     (0, 1e-2, 1e-3, 1e-1, 17)):
        rc, out, _, _ = _target_rc(hl, u, metric, target, tol_min, tol_max, rounds, ok)
        assert rc == MGH_ERR_INVALID_ARGUMENT and out == 0xdead0, (metric, target, tol_min, tol_max, rounds)
    round_trip()
    for tols in ([], [1e-3] * 65):
        with pytest.raises(mg.MgardHipError, match="error %d" % MGH_ERR_INVALID_ARGUMENT):
            hl.achieved_errors(u, tols, config=ok)
    assert len(hl.achieved_errors(u, [1e-2] * 64, config=ok)) == 64
    round_trip()
    # the size calls still refuse what they refused (their checks were split from the shared decomposition)
    with pytest.raises(mg.MgardHipError, match="error %d: size estimates: lossless" % MGH_ERR_INVALID_ARGUMENT):
        hl.estimate_sizes(u, [1e-3], config=_config(hl, 256, lossless=hl.HUFFMAN_ZSTD))
    hl._hl().mgh_release_cache()


def test_a_nan_in_the_input_meets_no_target():
    torch, mg, hl = _gpu()
    u = smooth_field(SMALL, F32)
    u[7, 5, 3] = np.nan
    ok = _config(hl, 256)
    for data in (u, torch.from_numpy(u).cuda()):
        (st,) = hl.achieved_errors(data, [1e-2], INF, mg.ABS, config=ok)
        assert st.nonfinite > 0 and st.n == u.size
    for metric, target in ((0, 1e30), (2, -1e30)):
        rc, out, _, cand = _target_rc(hl, u, metric, target, 1e-3, 1e-1, 4, ok, mode=mg.ABS)
        assert rc == MGH_ERR_TARGET_NOT_MET and out == 0xdead0
    v = smooth_field(SMALL, F32)
    assert float(np.max(np.abs(hl.decompress(hl.compress(v, 1e-3, INF, mg.REL, config=ok), config=ok) - v))) <= 1e-3 * 2
    hl._hl().mgh_release_cache()
