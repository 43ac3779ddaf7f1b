"""GPU tests of the second entry into the high-level writer: mgh_compress_ladder -- one
array, K tolerances, K containers from ONE decomposition -- against K mgh_compress calls, the counters of
mgh_last_compress_stats (the claim "one decomposition", also of mgh_compress_budget / _target, whose final
write takes the same entry), the outlier-overflow retry, pre-allocated outputs and the refusals.

Every comparison is an equality of bytes or integers. Huffman containers are compared byte for byte up to the
order of the outlier pairs (_canonical of tests/test_gpu_target.py: that order is the order of the quantizer's
atomics and differs between two mgh_compress calls as well); Huffman_Zstd containers are inflated and their
records compared the same way (_same_container says why their lengths cannot be)."""
import ctypes as C

import numpy as np
import pytest

from tests import payload as pl
from tests.test_gpu_target import ACH_CASES, FUSED3, SMALL, _canonical, _config, _is_raw
from tests.util import BLOCK, nonuniform_coords, smooth_field

pytestmark = pytest.mark.gpu

INF = float("inf")
F32, F64 = np.float32, np.float64
MGH_ERR_INVALID_ARGUMENT, MGH_ERR_OUTPUT_TOO_LARGE = -1, -7
HUFFMAN_ZSTD = 2


def _gpu():
    import torch
    import mgard_amd
    from mgard_amd import highlevel
    return torch, mgard_amd, highlevel


def _bytes(buf):
    return bytes(buf.cpu().numpy() if hasattr(buf, "cpu") else buf)


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _inflate(hl, buf):
    """The Huffman record inside the one Zstd record of a container: [u64 size][zstd frame] (Zstd.hpp:69-90)."""
    b = _bytes(buf)
    (rec,) = pl.split_container(b, hl.metadata_parse(b)["metadata_size"])
    z = C.CDLL("libzstd.so.1")
    z.ZSTD_decompress.restype = C.c_size_t
    z.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    n = int.from_bytes(rec[:8], "little")
    out = C.create_string_buffer(max(n, 1))
    assert z.ZSTD_decompress(out, n, rec[8:], len(rec) - 8) == n
    return out.raw[:n]


def _canonical_record(rec):
    r = pl.parse_huffman_record(rec)
    order = np.argsort(r["outlier_idx"], kind="stable")
    return [(k, (r[k][order] if k in ("outlier_idx", "outliers") else r[k])) for k in sorted(r)], len(order)


def _same_container(hl, got, want, u, cfg, zstd):
    """Returns whether the pair was a lossy (Huffman / Zstd) record.

    Zstd containers. The issue asked for equal length and an equal size prefix. Two mgh_compress calls on the
    same input do not have that themselves: the frame is the compressed Huffman record, the record holds the
    outlier pairs in the order of the quantizer's atomics, and a frame's LENGTH depends on that order (FUSED3
    f32, REL, dictionary 1024, measured on one MI355X: tol 3.162e-3, 28 560 outliers: 118 329 and 119 307 bytes
    from two mgh_compress calls, 105 756 from the ladder; tol 1e-2, 19 792 outliers: 97 149 / 96 688 / 85 177;
    tol 3.162e-1, 7 outliers: 26 620 / 26 620 / 26 620 -- the inflated records equal in length and, up to that
    order, in every byte each time). So the frames are inflated here and the records inside compared the way
    Huffman containers are -- byte for byte up to the order of the outlier pairs, which implies the equal
    record length in the frame's first 8 bytes --, the headers compared as bytes, the reconstructions as
    bits, and the container's length and size prefix held equal wherever the order has no freedom (at most
    one outlier)."""
    raw = _is_raw(hl, want, u)
    assert _is_raw(hl, got, u) == raw
    if raw:
        assert _bytes(got) == _bytes(want)
        return False
    if not zstd:
        assert _canonical(hl, got) == _canonical(hl, want)
        return True
    g, w = _bytes(got), _bytes(want)
    meta = hl.metadata_parse(w)["metadata_size"]
    assert g[:meta] == w[:meta]
    rg, rw = _inflate(hl, got), _inflate(hl, want)
    (cg, ng), (cw, nw) = _canonical_record(rg), _canonical_record(rw)
    assert len(rg) == len(rw) and ng == nw
    assert all(kg == kw and np.array_equal(vg, vw) for (kg, vg), (kw, vw) in zip(cg, cw))
    if nw <= 1:
        assert len(g) == len(w) and g[:meta + 8] == w[:meta + 8]
    assert np.array_equal(_bits(hl.decompress(got, config=cfg)), _bits(hl.decompress(want, config=cfg)))
    return True


@pytest.mark.parametrize("shape,dt,rel,s,dict_size,nonuniform,extra,decades", ACH_CASES)
def test_ladder_containers_are_compress_containers(shape, dt, rel, s, dict_size, nonuniform, extra, decades):
    torch, mg, hl = _gpu()
    tols = [float(t) for t in np.logspace(decades[0], decades[1], 5)]
    u = smooth_field(shape, dt)
    coords = nonuniform_coords(shape, dt) if nonuniform else None
    cfg = _config(hl, dict_size, **extra)
    mode = mg.REL if rel else mg.ABS
    zstd = extra.get("lossless") == HUFFMAN_ZSTD
    d = torch.from_numpy(u).cuda()
    for data in (d, u):
        got = hl.compress_ladder(data, tols, s, mode, coords=coords, config=cfg)
        st = hl.last_compress_stats()
        assert len(got) == len(tols)
        assert all(hasattr(g, "cpu") == hasattr(data, "cpu") for g in got)   # (the input's memory space)
        lossy = raws = 0
        for tol, g in zip(tols, got):
            want = hl.compress(data, tol, s, mode, coords=coords, config=cfg)
            one = hl.last_compress_stats()
            assert one["decompositions"] == 1 and one["records"] == 1 and one["quantize_passes"] == 1, one
            was_lossy = _same_container(hl, g, want, u, cfg, zstd)
            assert one["raw_records"] == (0 if was_lossy else 1)
            lossy += was_lossy
            raws += not was_lossy
        assert lossy >= 3, "the case must compare Huffman / Zstd records"
        assert st["decompositions"] == 1 and st["records"] == len(tols) and st["raw_records"] == raws, st
        assert st["quantize_passes"] == len(tols) + st["outlier_retries"], st
    hl._hl().mgh_release_cache()


def test_ladder_header_norm_is_compress_header_norm_over_several_ring_chunks():
    """Pageable host input of 17.2 MB: two pieces of the 16 MB ring, so the norm of a REL bound with s = 0 is a
    sum of squares over two partial sums in both entries into the writer. The ladder's header, norm included,
    must be mgh_compress's byte for byte -- it is only while both entries split the input the same way."""
    torch, mg, hl = _gpu()
    u = smooth_field((129, 130, 257), F32)
    assert u.nbytes > 16 << 20
    cfg = _config(hl, 1024)
    tols = [1e-2, 1e-3]
    got = hl.compress_ladder(u, tols, 0.0, mg.REL, config=cfg)
    for tol, g in zip(tols, got):
        want = hl.compress(u, tol, 0.0, mg.REL, config=cfg)
        gb, wb = _bytes(g), _bytes(want)
        meta = hl.metadata_parse(wb)["metadata_size"]
        assert gb[:meta] == wb[:meta]
        _same_container(hl, g, want, u, cfg, zstd=False)
    hl._hl().mgh_release_cache()


def test_budget_and_target_write_from_their_one_decomposition():
    torch, mg, hl = _gpu()
    cfg = _config(hl, 1024)
    u = smooth_field(FUSED3, F32)
    for data in (torch.from_numpy(u).cuda(), u):
        whole = hl.compress(data, 5e-2, INF, mg.REL, config=cfg)
        buf, tol_used, est = hl.compress_budget(data, len(_bytes(whole)), 5e-3, 5e0, rounds=2, config=cfg)
        st = hl.last_compress_stats()
        assert st["decompositions"] == 1 and st["records"] == 1 and st["quantize_passes"] == 1, st
        assert _canonical(hl, buf) == _canonical(hl, hl.compress(data, tol_used, INF, mg.REL, config=cfg))
        assert st["raw_records"] == 0
        buf, tol_used, stats, cand = hl.compress_target(data, 0, 1e30, 5e-2, 5e0, rounds=2, config=cfg)
        st = hl.last_compress_stats()
        assert st["decompositions"] == 1 and st["records"] == 1 and st["quantize_passes"] == 1, st
        assert _canonical(hl, buf) == _canonical(hl, hl.compress(data, tol_used, INF, mg.REL, config=cfg))
    hl._hl().mgh_release_cache()


def test_outlier_overflow_is_retried_once_and_gives_the_same_container():
    torch, mg, hl = _gpu()
    shape, dict_size, tol = FUSED3, 1024, 1e-1   # (a few hundred outliers, and still a Huffman record)
    u = smooth_field(shape, F32)
    d = torch.from_numpy(u).cuda()
    h = mg.Hierarchy(shape, F32)
    _, outl = h.quantize_histograms(h.decompose(d), [tol], mg.REL, INF, h.norm(d, INF), dict_size=dict_size)
    h.close()
    count = int(outl[0])
    assert count >= 2, count
    for extra in ({}, {"reorder": 1}):  # (the symbol route and the int64 route)
        hl._hl().mgh_release_cache()    # (the lanes' outlier lists only ever grow: start from none)
        tight = _config(hl, dict_size, estimate_outlier_ratio=0.5 * count / u.size, **extra)
        (got,) = hl.compress_ladder(d, [tol], INF, mg.REL, config=tight)
        st = hl.last_compress_stats()
        assert st["outlier_retries"] == 1 and st["quantize_passes"] == 2 and st["decompositions"] == 1, st
        want = hl.compress(d, tol, INF, mg.REL, config=_config(hl, dict_size, **extra))
        assert hl.last_compress_stats()["outlier_retries"] == 0
        assert not _is_raw(hl, want, u)
        assert _canonical(hl, got) == _canonical(hl, want)
    hl._hl().mgh_release_cache()


def test_preallocated_outputs_exact_and_one_byte_short():
    torch, mg, hl = _gpu()
    cfg = _config(hl, 1024)
    u = smooth_field(FUSED3, F32)
    tols = [5e-2, 2e-1, 1e0]
    want = [hl.compress(u, t, INF, mg.REL, config=cfg) for t in tols]
    assert not any(_is_raw(hl, w, u) for w in want)
    sizes = [len(w) for w in want]
    outs = [np.zeros(n, dtype=np.uint8) for n in sizes]
    got = hl.compress_ladder(u, tols, INF, mg.REL, config=cfg, outs=outs)
    assert [len(g) for g in got] == sizes
    assert all(_canonical(hl, g) == _canonical(hl, w) for g, w in zip(got, want))
    # one byte less for the second tolerance: its status, the container before it intact
    outs = [np.zeros(sizes[0], dtype=np.uint8), np.zeros(sizes[1] - 1, dtype=np.uint8), np.zeros(sizes[2], dtype=np.uint8)]
    with pytest.raises(mg.MgardHipError, match="error %d" % MGH_ERR_OUTPUT_TOO_LARGE):
        hl.compress_ladder(u, tols, INF, mg.REL, config=cfg, outs=outs)
    assert _canonical(hl, outs[0]) == _canonical(hl, want[0])
    assert not outs[2].any()
    # device outputs: the ladder takes a capacity exactly as mgh_compress takes it
    d = torch.from_numpy(u).cuda()
    for short in (0, 1):
        def attempt(call):
            try:
                return len(call())
            except mg.MgardHipError as e:
                return str(e).split(":")[0]
        cap = sizes[1] - short
        one = attempt(lambda: hl.compress(d, tols[1], INF, mg.REL, config=cfg,
                                          out=torch.zeros(cap, dtype=torch.uint8, device="cuda")))
        lad = attempt(lambda: hl.compress_ladder(d, tols[1:2], INF, mg.REL, config=cfg,
                                                 outs=[torch.zeros(cap, dtype=torch.uint8, device="cuda")])[0])
        assert one == lad, (short, one, lad)
    # allocated by the call (the C interface): a failure at tolerance 1 leaves container 0 the caller's
    L = hl._hl()
    free_device = L.mgh_free_device
    k = len(tols)
    ptrs, szs = (C.c_void_p * k)(*([0xdead0] * k)), (C.c_size_t * k)()
    rc = L.mgh_compress_ladder(u.ndim, 0, (C.c_uint64 * u.ndim)(*u.shape), k, (C.c_double * k)(*tols), INF, mg.REL,
                               C.c_void_p(d.data_ptr()), ptrs, szs, None, C.byref(cfg), 0)
    assert rc == 0 and [int(x) for x in szs] == sizes and all(ptrs[i] not in (None, 0xdead0) for i in range(k))
    back = torch.empty(sizes[2], dtype=torch.uint8, device="cuda")
    assert L.mgh_memcpy(C.c_void_p(back.data_ptr()), C.c_void_p(ptrs[2]), sizes[2]) == 0
    assert _canonical(hl, back) == _canonical(hl, want[2])
    for i in range(k):
        free_device(C.c_void_p(ptrs[i]))
    hl._hl().mgh_release_cache()


def test_refusals_leave_the_library_usable():
    torch, mg, hl = _gpu()
    u = smooth_field(SMALL, F32)
    ok = _config(hl, 1024)

    def round_trip(cfg=ok):
        v = hl.decompress(hl.compress(u, 1e-3, INF, mg.REL, config=cfg), config=cfg)
        assert float(np.max(np.abs(v - u))) <= 1e-3 * float(np.max(np.abs(u)))

    def rc_of(tols, cfg=ok):
        """The C call itself, outputs NOT pre-allocated: (status, output pointers)."""
        k = len(tols)
        ptrs, szs = (C.c_void_p * max(k, 1))(*([0xdead0] * max(k, 1))), (C.c_size_t * max(k, 1))()
        rc = hl._hl().mgh_compress_ladder(u.ndim, 0, (C.c_uint64 * u.ndim)(*u.shape), k, (C.c_double * max(k, 1))(*tols),
                                          INF, mg.REL, C.c_void_p(u.ctypes.data), ptrs, szs, None, C.byref(cfg), 0)
        return rc, [ptrs[i] for i in range(max(k, 1))]

    decomposing = _config(hl, 256, domain_decomposition=BLOCK, block_size=11)  # 3 x 2 x 2 subdomains
    rc, ptrs = rc_of([1e-2, 1e-1], decomposing)
    assert rc == MGH_ERR_INVALID_ARGUMENT and all(p is None for p in ptrs)
    assert b"compress_ladder: the configuration decomposes" in hl._hl().mgh_last_error()
    round_trip(decomposing)
    for tols in ([], [1e-2] * 65, [1e-2, 0.0], [-1e-2], [1e-2, float("nan")], [INF]):
        rc, ptrs = rc_of(tols)
        assert rc == MGH_ERR_INVALID_ARGUMENT and all(p == 0xdead0 for p in ptrs), tols
        round_trip()
    with pytest.raises(mg.MgardHipError, match="error %d: compress_ladder: " % MGH_ERR_INVALID_ARGUMENT):
        hl.compress_ladder(u, [], config=ok)
    assert len(hl.compress_ladder(u, [1e-1] * 64, config=ok)) == 64
    round_trip()
    hl._hl().mgh_release_cache()
