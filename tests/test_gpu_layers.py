"""GPU tests of the precision layers: mgh_compress_layers -- K containers that refine
one array tolerance by tolerance, each holding what the ones before it left of the coefficients -- and their
readers mgh_layers_* / mgh_decompress_layers.

The reference is the chain the header states, built once per case from the stand-alone stages and torch:
    r_0 = decompose(u);  q_k = quantize(r_k; tol_k);  r_{k+1} = r_k - dequantize(q_k; tol_k);
    acc_k = dequantize(q_0) + ... + dequantize(q_k);  u_k = recompose(acc_k).
Every comparison with it is an equality of integers or of bits. (E) and (S) are the two conditions with a margin:
the chain's own error is at most 0.09 of the bound on these shapes (CPU experiment with the oracle), and the
zeroth-order entropy of four layers is 0.38 of four ladder tiers'."""
import ctypes as C

import numpy as np
import pytest

from tests import payload as pl
from tests.test_gpu_ladder import _canonical_record, _inflate
from tests.test_gpu_target import ACH_CASES, FUSED3, SMALL, _canonical, _config, _is_raw
from tests.util import BLOCK, nonuniform_coords, smooth_field

pytestmark = pytest.mark.gpu

INF = float("inf")
F32, F64 = np.float32, np.float64
MGH_ERR_INVALID_ARGUMENT, MGH_ERR_OUTPUT_TOO_LARGE = -1, -7
HUFFMAN_ZSTD = 2
CASES = [c for c in ACH_CASES if not c[6].get("reorder")]


def _gpu():
    import torch
    import mgard_amd
    from mgard_amd import highlevel
    return torch, mgard_amd, highlevel


def _bytes(buf):
    return bytes(buf.cpu().numpy() if hasattr(buf, "cpu") else buf)


def _bits(a):
    a = a.contiguous().cpu().numpy() if hasattr(a, "cpu") else np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _tols(decades):
    """Four tolerances a decade apart, from where the case's decades start."""
    return [float(10.0 ** (decades[0] - k)) for k in range(4)]


def _sorted_pairs(idx, val):
    i, v = idx.cpu().numpy().astype(np.int64), val.cpu().numpy()
    order = np.argsort(i, kind="stable")
    return i[order], v[order]


class Chain:
    """The reference of one case: integers, lists and reconstructions of every layer."""

    def __init__(self, mg, torch, shape, dt, coords, mode, s, norm, dict_size, tols):
        self.h = h = mg.Hierarchy(shape, dt, coords=coords)
        self.d = torch.from_numpy(smooth_field(shape, dt)).cuda()
        r = h.decompose(self.d)
        self.q, self.lists, self.alone, self.u = [], [], [], []
        acc = None
        for tol in tols:
            q, oi, ov, n = h.quantize(r, mode, tol, s, norm, dict_size=dict_size, prep_huffman=True)
            assert n == oi.numel()
            back = h.dequantize(q.clone(), mode, tol, s, norm, dict_size=dict_size, outlier_idx=oi, outlier_val=ov)
            r = r - back
            acc = back if acc is None else acc + back
            self.q.append(q.cpu().numpy().ravel())
            self.lists.append(_sorted_pairs(oi, ov))
            self.alone.append(_bits(h.recompose(back)))   # the layer decoded on its own: a correction field
            self.u.append(_bits(h.recompose(acc)))        # the array after layers 0 .. k

    def close(self):
        self.h.close()


def _check_layers(hl, torch, chain, layers, cfg, zstd, n):
    """(W2), the layer as an ordinary container, (R1), (R2) for one set of layers."""
    ll = hl.Lossless()
    for k, buf in enumerate(layers):
        b = _bytes(buf)
        (rec,) = pl.split_container(b, hl.metadata_parse(b)["metadata_size"])
        assert len(rec) < n, (k, "a raw record")
        q, oi, ov = ll.decompress(rec, chain.q[k].size, lossless=HUFFMAN_ZSTD if zstd else 0)
        assert np.array_equal(q.cpu().numpy(), chain.q[k]), k                               # (W2)
        gi, gv = _sorted_pairs(oi, ov)
        assert np.array_equal(gi, chain.lists[k][0]) and np.array_equal(gv, chain.lists[k][1]), k
        assert np.array_equal(_bits(hl.decompress(buf, config=cfg)), chain.alone[k]), k     # an ordinary container
    ll.close()
    assert np.array_equal(_bits(hl.decompress_layers(layers[:1], config=cfg)),
                          _bits(hl.decompress(layers[0], config=cfg)))                      # (R1)
    with hl.Layers(layers[0], config=cfg) as r:
        for k in range(len(layers)):
            if k:
                assert r.add(layers[k]) is r
            assert r.count == k + 1 and r.tolerance == hl.metadata_parse(_bytes(layers[k]))["tol"]
            got = r.data()
            assert hasattr(got, "cpu") == hasattr(layers[0], "cpu")                         # (the containers' space)
            assert np.array_equal(_bits(got), chain.u[k]), k                                # (R2), stateful
            assert np.array_equal(_bits(hl.decompress_layers(layers[:k + 1], config=cfg)), chain.u[k]), k  # one-shot
            assert np.array_equal(_bits(r.data()), chain.u[k]), k                           # data() changes nothing


def _counters(hl, k):
    st = hl.last_compress_stats()
    assert st["decompositions"] == 1 and st["records"] == k and st["raw_records"] == 0, st
    assert st["quantize_passes"] == k + st["outlier_retries"], st
    return st


@pytest.mark.parametrize("shape,dt,rel,s,dict_size,nonuniform,extra,decades", CASES)
def test_layers_are_the_chain_and_read_back_as_the_chain(shape, dt, rel, s, dict_size, nonuniform, extra, decades):
    torch, mg, hl = _gpu()
    tols = _tols(decades)
    u = smooth_field(shape, dt)
    coords = nonuniform_coords(shape, dt) if nonuniform else None
    cfg = _config(hl, dict_size, **extra)
    mode = mg.REL if rel else mg.ABS
    zstd = extra.get("lossless") == HUFFMAN_ZSTD
    d = torch.from_numpy(u).cuda()
    chain = None
    for data in (d, u):
        layers = hl.compress_layers(data, tols, s, mode, coords=coords, config=cfg)
        _counters(hl, len(tols))
        assert len(layers) == len(tols) and all(hasattr(g, "cpu") == hasattr(data, "cpu") for g in layers)
        heads = [hl.metadata_parse(_bytes(g)) for g in layers]
        assert [h["tol"] for h in heads] == tols and all(h["norm"] == heads[0]["norm"] for h in heads)
        if chain is None:  # (the reference, once: the norm is the one every reader takes, the header's)
            norm = heads[0]["norm"] if rel else 1.0
            chain = Chain(mg, torch, shape, dt, coords, mode, s, norm, dict_size, tols)
            if rel and s == INF:
                assert norm == chain.h.norm(d, INF)
        # (W1) layer 0 is the container of mgh_compress(tols[0])
        want = hl.compress(data, tols[0], s, mode, coords=coords, config=cfg)
        assert not _is_raw(hl, want, u)
        if zstd:
            g, w = _bytes(layers[0]), _bytes(want)
            assert g[:heads[0]["metadata_size"]] == w[:heads[0]["metadata_size"]]
            (cg, ng), (cw, nw) = _canonical_record(_inflate(hl, layers[0])), _canonical_record(_inflate(hl, want))
            assert ng == nw and all(kg == kw and np.array_equal(vg, vw) for (kg, vg), (kw, vw) in zip(cg, cw))
        else:
            assert _canonical(hl, layers[0]) == _canonical(hl, want)
        _check_layers(hl, torch, chain, layers, cfg, zstd, u.nbytes)
        if s == INF:  # (E)
            for k, tol in enumerate(tols):
                bound = tol * norm if rel else tol
                err = mg.compare(u, hl.decompress_layers(layers[:k + 1], config=cfg)).max_abs_err
                print("layers %s %s k=%d max_abs_err %.3e bound %.3e" % (shape, np.dtype(dt).name, k, err, bound))
                assert err <= bound, (k, err, bound)
        if shape == FUSED3 and dt == F32 and rel and s == INF and not zstd:  # (S)
            ladder = hl.compress_ladder(data, tols, s, mode, coords=coords, config=cfg)
            ls, ts = sum(len(g) for g in layers), sum(len(g) for g in ladder)
            print("bytes: layers %d, ladder %d, finest tier alone %d" % (ls, ts, len(ladder[-1])))
            assert ls < ts, (ls, ts)
    chain.close()
    hl._hl().mgh_release_cache()


def test_outlier_overflow_retries_and_the_residual_is_of_the_unmodified_coefficients():
    torch, mg, hl = _gpu()
    """The ping-pong: layer 0 overflows its outlier lists, the quantizer runs again and must read the coefficients
    the first pass read. (FUSED3 with dictionary 1024 at 1e-1, the overflow case of tests/test_gpu_ladder.py: a few
    hundred outliers and still a Huffman record. SMALL with dictionary 64 sends so many values through the list
    that layer 0 would be stored raw, which the writer refuses.)"""
    shape, dict_size, tols = FUSED3, 1024, [1e-1, 1e-2, 1e-3, 1e-4]
    u = smooth_field(shape, F32)
    d = torch.from_numpy(u).cuda()
    h = mg.Hierarchy(shape, F32)
    norm = h.norm(d, INF)
    _, outl = h.quantize_histograms(h.decompose(d), tols[:1], mg.REL, INF, norm, dict_size=dict_size)
    h.close()
    count = int(outl[0])
    assert count >= 2, count
    chain = Chain(mg, torch, shape, F32, None, mg.REL, INF, norm, dict_size, tols)
    hl._hl().mgh_release_cache()    # (the lanes' outlier lists only ever grow: start from none)
    tight = _config(hl, dict_size, estimate_outlier_ratio=0.5 * count / u.size)
    layers = hl.compress_layers(d, tols, INF, mg.REL, config=tight)
    st = _counters(hl, len(tols))
    assert st["outlier_retries"] >= 1, st
    _check_layers(hl, torch, chain, layers, tight, False, u.nbytes)
    chain.close()
    hl._hl().mgh_release_cache()


def test_preallocated_outputs_a_short_one_keeps_the_layers_before_it():
    torch, mg, hl = _gpu()
    cfg = _config(hl, 1024)
    u = smooth_field(FUSED3, F32)
    tols = [1e-1, 1e-2, 1e-3]
    want = hl.compress_layers(u, tols, INF, mg.REL, config=cfg)
    sizes = [len(w) for w in want]
    outs = [np.zeros(n, dtype=np.uint8) for n in sizes]
    got = hl.compress_layers(u, tols, INF, mg.REL, config=cfg, outs=outs)
    assert [len(g) for g in got] == sizes and all(_canonical(hl, g) == _canonical(hl, w) for g, w in zip(got, want))
    outs = [np.zeros(sizes[0], dtype=np.uint8), np.zeros(sizes[1] - 1, dtype=np.uint8), np.zeros(sizes[2], dtype=np.uint8)]
    with pytest.raises(mg.MgardHipError, match="error %d" % MGH_ERR_OUTPUT_TOO_LARGE):
        hl.compress_layers(u, tols, INF, mg.REL, config=cfg, outs=outs)
    assert _canonical(hl, outs[0]) == _canonical(hl, want[0]) and not outs[2].any()
    again = hl.compress_layers(u, tols, INF, mg.REL, config=cfg)   # the library is usable, and says the same
    assert all(_canonical(hl, g) == _canonical(hl, w) for g, w in zip(again, want))
    full = hl.decompress_layers(again, config=cfg)
    assert float(np.abs(full - u).max()) <= tols[-1] * float(np.abs(u).max())
    # allocated by the call (the C interface), device input: device containers, the caller's to free
    L = hl._hl()
    d = torch.from_numpy(u).cuda()
    k = len(tols)
    ptrs, szs = (C.c_void_p * k)(*([0xdead0] * k)), (C.c_size_t * k)()
    rc = L.mgh_compress_layers(u.ndim, 0, (C.c_uint64 * u.ndim)(*u.shape), k, (C.c_double * k)(*tols), INF, mg.REL,
                               C.c_void_p(d.data_ptr()), ptrs, szs, None, C.byref(cfg), 0)
    assert rc == 0 and [int(x) for x in szs] == sizes and all(ptrs[i] not in (None, 0xdead0) for i in range(k))
    out = C.c_void_p()
    assert L.mgh_decompress_layers(k, ptrs, szs, C.byref(cfg), C.byref(out), 0) == 0 and out.value
    back = torch.empty(FUSED3, dtype=torch.float32, device="cuda")
    assert L.mgh_memcpy(C.c_void_p(back.data_ptr()), out, u.nbytes) == 0
    assert np.array_equal(_bits(back), _bits(full))
    for p in list(ptrs) + [out.value]:
        L.mgh_free_device(C.c_void_p(p))
    hl._hl().mgh_release_cache()


def test_writer_refusals_leave_the_library_usable():
    torch, mg, hl = _gpu()
    u = smooth_field(SMALL, F32)
    ok = _config(hl, 1024)

    def round_trip(cfg=ok):
        v = hl.decompress_layers(hl.compress_layers(u, [1e-1, 1e-2], INF, mg.REL, config=cfg), config=cfg)
        assert float(np.max(np.abs(v - u))) <= 1e-2 * float(np.max(np.abs(u)))

    def rc_of(tols, cfg=ok, data=u):
        """The C call itself, outputs NOT pre-allocated: (status, output pointers)."""
        k = len(tols)
        ptrs, szs = (C.c_void_p * max(k, 1))(*([0xdead0] * max(k, 1))), (C.c_size_t * max(k, 1))()
        rc = hl._hl().mgh_compress_layers(data.ndim, 0, (C.c_uint64 * data.ndim)(*data.shape), k,
                                          (C.c_double * max(k, 1))(*tols), INF, mg.ABS, C.c_void_p(data.ctypes.data), ptrs,
                                          szs, None, C.byref(cfg), 0)
        return rc, [ptrs[i] for i in range(max(k, 1))]

    err = lambda: hl._hl().mgh_last_error()
    for tols in ([], [10.0 ** -(k / 16) for k in range(65)], [1e-2, 1e-2], [1e-3, 1e-2], [1e-1, 1e-2, 1e-2],
                 [1e-2, 0.0], [-1e-2], [1e-2, float("nan")], [INF]):
        rc, ptrs = rc_of(tols)
        assert rc == MGH_ERR_INVALID_ARGUMENT and all(p == 0xdead0 for p in ptrs), tols
        assert b"compress_layers: " in err()
        round_trip()
    assert rc_of([1e-2, 1e-2])[0] == MGH_ERR_INVALID_ARGUMENT and b"strictly decreasing" in err()
    assert len(hl.compress_layers(u, [10.0 ** -(k / 16) for k in range(64)], config=ok)) == 64
    for cfg, msg in ((_config(hl, 256, domain_decomposition=BLOCK, block_size=11), b"decomposes the domain"),
                     (_config(hl, 1024, reorder=1), b"reorder = 1"), (_config(hl, 1023), b"dict_size"),
                     (_config(hl, 16384), b"dict_size")):
        rc, ptrs = rc_of([1e-1, 1e-2], cfg)
        assert rc == MGH_ERR_INVALID_ARGUMENT and all(p == 0xdead0 for p in ptrs) and msg in err(), (msg, err())
        round_trip()
    # a raw layer: noise, and a tolerance far below its float noise
    noise = np.random.default_rng(7).standard_normal(SMALL).astype(F32)
    assert _is_raw(hl, hl.compress(noise, 1e-12, INF, mg.ABS, config=ok), noise)
    rc, ptrs = rc_of([1e-12], data=noise)
    assert rc == MGH_ERR_INVALID_ARGUMENT and b"compress_layers: layer 0 would be stored raw" in err() and ptrs == [None]
    round_trip()
    outs = [np.zeros(noise.nbytes + 10 ** 6, dtype=np.uint8) for _ in range(2)]
    with pytest.raises(mg.MgardHipError, match="compress_layers: layer 1 would be stored raw"):
        hl.compress_layers(noise, [3.0, 1e-12], INF, mg.ABS, config=ok, outs=outs)
    first = hl.compress(noise, 3.0, INF, mg.ABS, config=ok)
    assert not _is_raw(hl, first, noise)
    assert _canonical(hl, outs[0][:len(first)]) == _canonical(hl, first)
    round_trip()
    hl._hl().mgh_release_cache()


def test_reader_refusals_leave_the_handle_as_it_was():
    torch, mg, hl = _gpu()
    cfg = _config(hl, 1024)
    u = smooth_field(SMALL, F32)
    tols = [1e-1, 1e-2, 1e-3]  # (SMALL is small: a finer FIRST layer would be stored raw)
    b = hl.compress_layers(u, tols, INF, mg.REL, config=cfg)
    other_norm = hl.compress_layers(2.0 * u, tols, INF, mg.REL, config=cfg)
    other_shape = hl.compress_layers(smooth_field(FUSED3, F32), tols, INF, mg.REL, config=cfg)
    other_type = hl.compress_layers(u.astype(F64), tols, INF, mg.REL, config=cfg)
    other_mode = hl.compress_layers(u, [1e-1 * float(np.abs(u).max())], INF, mg.ABS, config=cfg)
    dd = _config(hl, 1024, domain_decomposition=BLOCK, block_size=11)
    two = hl.compress(u, 1e-2, INF, mg.REL, config=dd)
    assert hl.metadata_parse(_bytes(two))["domain_decomposed"]
    reordered = hl.compress(u, 1e-2, INF, mg.REL, config=_config(hl, 1024, reorder=1))
    noise = np.random.default_rng(7).standard_normal(SMALL).astype(F32)
    raw = hl.compress(noise, 1e-12, INF, mg.ABS, config=cfg)
    assert _is_raw(hl, raw, noise)
    L = hl._hl()
    with hl.Layers(b[0], config=cfg) as r:
        r.add(b[1])
        before = _bits(r.data())
        for bad, msg in ((b[0], "tolerance"), (b[1], "tolerance"), (other_norm[2], "norm"), (other_shape[2], "shape"),
                         (other_type[2], "data type"), (other_mode[0], "error bound type"), (two, "domain-decomposed"),
                         (reordered, "reorder = 1"), (raw, "error bound type")):
            with pytest.raises(mg.MgardHipError, match="error %d: mgh_layers_add: .*%s" % (MGH_ERR_INVALID_ARGUMENT, msg)):
                r.add(bad)
            assert r.count == 2 and r.tolerance == tols[1] and np.array_equal(_bits(r.data()), before)
        want = _bits(hl.decompress_layers(b, config=cfg))
        assert np.array_equal(_bits(r.add(b[2]).data()), want)
    # layers swapped, a decomposed, a reordered and a raw container in front
    for bufs, msg in (([b[1], b[0]], "mgh_layers_add: the tolerance"), ([two], "mgh_layers_open: .*domain-decomposed"),
                      ([reordered], "mgh_layers_open: .*reorder = 1"), ([raw], "mgh_layers_open: .*raw")):
        with pytest.raises(mg.MgardHipError, match="error %d: %s" % (MGH_ERR_INVALID_ARGUMENT, msg)):
            hl.decompress_layers(bufs, config=cfg)
    for k in (0, 65):
        out = C.c_void_p()
        assert L.mgh_decompress_layers(k, (C.c_void_p * 1)(), (C.c_size_t * 1)(), C.byref(cfg), C.byref(out),
                                       0) == MGH_ERR_INVALID_ARGUMENT
    assert np.array_equal(_bits(hl.decompress_layers(b, config=cfg)), want)
    hl._hl().mgh_release_cache()
