"""GPU tests of the precision layers in level order: mgh_compress_level_layers -- the layers of
mgh_compress_layers as reorder = 1 records -- and their readers mgh_level_layers_* / mgh_decompress_level_layers,
which read layer k up to a level of its own from the head of that layer's record.

The reference is the chain of tests/test_gpu_layers.py (its Chain class), built once per case from the stand-alone
stages, plus mgh_level_linearize. Every comparison with it is an equality of integers or of bits; (E) is the one
condition with a margin."""
import numpy as np
import pytest

from tests import payload as pl
from tests.test_gpu_ladder import _canonical_record, _inflate
from tests.test_gpu_layers import Chain, _bits, _bytes, _sorted_pairs, _tols
from tests.test_gpu_level_layers_kernels import CASES, IDS
from tests.test_gpu_target import FUSED3, SMALL, _canonical, _config, _is_raw
from tests.util import BLOCK, nonuniform_coords, smooth_field

pytestmark = pytest.mark.gpu

INF = float("inf")
F32, F64 = np.float32, np.float64
MGH_ERR_INVALID_ARGUMENT = -1
HUFFMAN_ZSTD = 2


def _gpu():
    import torch
    import mgard_amd
    from mgard_amd import highlevel
    return torch, mgard_amd, highlevel


def _deq(chain, mg, k, mode, tol, s, norm, dict_size, torch):
    """dequantize(q_k) of the chain, in array order."""
    q = torch.from_numpy(chain.q[k]).cuda().reshape(chain.h.shape)
    oi, ov = (torch.from_numpy(a).cuda() for a in chain.lists[k])
    return chain.h.dequantize(q, mode, tol, s, norm, dict_size=dict_size, outlier_idx=oi, outlier_val=ov)


@pytest.mark.parametrize("shape,dt,rel,s,dict_size,nonuniform,extra,decades", CASES, ids=IDS)
def test_level_layers_are_the_chain_in_level_order_and_read_back_by_level(shape, dt, rel, s, dict_size, nonuniform, extra,
                                                                          decades):
    torch, mg, hl = _gpu()
    tols = _tols(decades)
    u = smooth_field(shape, dt)
    coords = nonuniform_coords(shape, dt) if nonuniform else None
    cfg = _config(hl, dict_size, **extra)          # (reorder = 0: the writer sets it)
    cfg1 = _config(hl, dict_size, reorder=1, **extra)
    mode = mg.REL if rel else mg.ABS
    zstd = extra.get("lossless") == HUFFMAN_ZSTD
    d = torch.from_numpy(u).cuda()
    chain = None
    for data in (d, u):
        layers = hl.compress_level_layers(data, tols, s, mode, coords=coords, config=cfg)
        st = hl.last_compress_stats()
        assert st["decompositions"] == 1 and st["records"] == len(tols) and st["raw_records"] == 0, st
        assert len(layers) == len(tols) and all(hasattr(g, "cpu") == hasattr(data, "cpu") for g in layers)
        heads = [hl.metadata_parse(_bytes(g)) for g in layers]
        assert [h["tol"] for h in heads] == tols and all(h["norm"] == heads[0]["norm"] for h in heads)
        assert all(h["reorder"] for h in heads)
        if chain is None:
            norm = heads[0]["norm"] if rel else 1.0
            chain = Chain(mg, torch, shape, dt, coords, mode, s, norm, dict_size, tols)
            h = chain.h
            L = h.l_target
            perm = h.level_linearize(torch.arange(u.size, dtype=torch.int64, device="cuda").reshape(shape)).reshape(-1)
            inv = torch.empty_like(perm)
            inv[perm] = torch.arange(u.size, dtype=torch.int64, device="cuda")
            backs = [_deq(chain, mg, k, mode, tols[k], s, norm, dict_size, torch) for k in range(len(tols))]
            N = [int(np.prod(h.level_shape(l))) for l in range(L + 1)]
        # (W1) layer 0 is the container of mgh_compress(tols[0], reorder = 1)
        want = hl.compress(data, tols[0], s, mode, coords=coords, config=cfg1)
        assert not _is_raw(hl, want, u)
        if zstd:
            g, w = _bytes(layers[0]), _bytes(want)
            assert g[:heads[0]["metadata_size"]] == w[:heads[0]["metadata_size"]]
            (cg, ng), (cw, nw) = _canonical_record(_inflate(hl, layers[0])), _canonical_record(_inflate(hl, want))
            assert ng == nw and all(kg == kw and np.array_equal(vg, vw) for (kg, vg), (kw, vw) in zip(cg, cw))
        else:
            assert _canonical(hl, layers[0]) == _canonical(hl, want)
        # every layer: the chain's integers and lists in level order, and an ordinary container
        ll = hl.Lossless()
        for k, buf in enumerate(layers):
            b = _bytes(buf)
            (rec,) = pl.split_container(b, hl.metadata_parse(b)["metadata_size"])
            assert len(rec) < u.nbytes, (k, "a raw record")
            q, oi, ov = ll.decompress(rec, chain.q[k].size, lossless=HUFFMAN_ZSTD if zstd else 0)
            assert np.array_equal(q.cpu().numpy(), chain.q[k][perm.cpu().numpy()]), k
            gi, gv = _sorted_pairs(oi, ov)
            wi = inv.cpu().numpy()[chain.lists[k][0]]
            order = np.argsort(wi, kind="stable")
            assert np.array_equal(gi, wi[order]) and np.array_equal(gv, chain.lists[k][1][order]), k
            assert np.array_equal(_bits(hl.decompress(buf, config=cfg)), chain.alone[k]), k
            if k == 0:  # ... that the reduced-resolution readers open
                got = hl.decompress(buf, config=cfg, level=max(L - 1, 0))
                assert np.array_equal(_bits(got), _bits(hl.decompress(want, config=cfg, level=max(L - 1, 0))))
        ll.close()
        # (R) every k, every level: stateful and one-shot, and data() changes nothing
        for lev in range(L + 1):
            acc = None
            with hl.LevelLayers(layers[0], lev, config=cfg) as r:
                for k in range(len(layers)):
                    if k:
                        assert r.add(layers[k], lev) is r
                    acc = backs[k] if acc is None else acc + backs[k]
                    wantl = _bits(h.recompose(acc, level=lev))
                    assert r.count == k + 1 and r.depth(k) == lev and r.tolerance(k) == tols[k]
                    got = r.data(lev)
                    assert hasattr(got, "cpu") == hasattr(layers[0], "cpu")
                    assert tuple(got.shape) == tuple(h.level_shape(lev))
                    assert np.array_equal(_bits(got), wantl), (k, lev)
                    if lev in (0, L - 1, L) or k == len(layers) - 1:
                        assert np.array_equal(_bits(hl.decompress_level_layers(layers[:k + 1], lev, config=cfg)), wantl), (k, lev)
                    assert np.array_equal(_bits(r.data(lev)), wantl), (k, lev)
                    if lev:
                        assert np.array_equal(_bits(r.data(lev - 1)), _bits(h.recompose(acc, level=lev - 1))), (k, lev)
        assert np.array_equal(_bits(hl.decompress_level_layers(layers, L, config=cfg)), chain.u[-1])
        # a mixed walk: the uncovered levels of each layer count as zero
        if L >= 2:
            with hl.LevelLayers(layers[0], L - 2, config=cfg) as r:
                r.add(layers[1], L - 2)
                r.extend(0, layers[0], L).extend(1, layers[1], L - 1)
                assert [r.depth(0), r.depth(1)] == [L, L - 1]
                b1 = backs[1].reshape(-1).clone()
                b1[perm[N[L - 1]:]] = 0
                wantl = _bits(h.recompose(backs[0] + b1.reshape(backs[0].shape)))
                assert np.array_equal(_bits(r.data(L)), wantl)
                assert np.array_equal(_bits(r.data(L - 1)), _bits(h.recompose(backs[0] + backs[1], level=L - 1)))
        if s == INF:  # (E)
            bound = tols[-1] * norm if rel else tols[-1]
            err = mg.compare(u, hl.decompress_level_layers(layers, L, config=cfg)).max_abs_err
            print("level layers %s %s max_abs_err %.3e bound %.3e" % (shape, np.dtype(dt).name, err, bound))
            assert err <= bound, (err, bound)
    chain.close()
    hl._hl().mgh_release_cache()


def test_a_level_reads_the_head_of_the_record_only():
    torch, mg, hl = _gpu()
    shape = FUSED3
    u = smooth_field(shape, F32)
    cfg = hl.Config(huff_dict_size=1024)
    block = int(cfg.huff_block_size)    # (the default, as tests/test_gpu_level_prefix.py: two chunks here, one for the head)
    tols = [1e-1, 1e-2, 1e-3]
    layers = hl.compress_level_layers(u, tols, INF, mg.REL, config=cfg)
    h = mg.Hierarchy(shape, F32)
    L = h.l_target
    N = [int(np.prod(h.level_shape(l))) for l in range(L + 1)]
    total = -(-u.size // block)
    need = -(-N[L - 1] // block)
    assert need < total
    recs = [len(pl.split_container(_bytes(b), hl.metadata_parse(_bytes(b))["metadata_size"])[0]) for b in layers]
    with hl.LevelLayers(layers[0], L - 1, config=cfg) as r:
        st = hl.last_decompress_stats()
        assert st["chunks_decoded"] == need and st["chunks_total"] == total and st["record_bytes"] == recs[0], st
        assert st["record_bytes_moved"] < recs[0], st
        r.add(layers[1], L - 1)
        st = hl.last_decompress_stats()
        assert st["chunks_decoded"] == need and st["chunks_total"] == total and st["record_bytes_moved"] < recs[1], st
        # going deeper decodes from the chunk that holds N_{L-1}: the boundary chunk again, nothing in front of it
        r.extend(0, layers[0], L)
        st = hl.last_decompress_stats()
        assert st["chunks_decoded"] == total - N[L - 1] // block, st
        assert need + st["chunks_decoded"] - total in (0, 1), st
        assert np.array_equal(_bits(r.data(L - 1)), _bits(hl.decompress_level_layers(layers[:2], L - 1, config=cfg)))
    h.close()
    hl._hl().mgh_release_cache()


def test_layers_data_level_is_recompose_to_level_of_the_reorder_0_chain():
    torch, mg, hl = _gpu()
    shape, dict_size, tols = SMALL, 1024, [1e-1, 1e-2, 1e-3]
    u = smooth_field(shape, F32)
    cfg = _config(hl, dict_size)
    layers = hl.compress_layers(u, tols, INF, mg.REL, config=cfg)
    norm = hl.metadata_parse(_bytes(layers[0]))["norm"]
    chain = Chain(mg, torch, shape, F32, None, mg.REL, INF, norm, dict_size, tols)
    h = chain.h
    acc = None
    with hl.Layers(layers[0], config=cfg) as r:
        for k in range(len(tols)):
            if k:
                r.add(layers[k])
            back = _deq(chain, mg, k, mg.REL, tols[k], INF, norm, dict_size, torch)
            acc = back if acc is None else acc + back
            for lev in range(h.l_target + 1):
                got = r.data(level=lev)
                assert tuple(got.shape) == tuple(h.level_shape(lev)) and not hasattr(got, "cpu")
                assert np.array_equal(_bits(got), _bits(h.recompose(acc, level=lev))), (k, lev)
            assert np.array_equal(_bits(r.data()), chain.u[k])
        with pytest.raises(mg.MgardHipError):
            r.data(level=h.l_target + 1)
    chain.close()
    hl._hl().mgh_release_cache()


def test_writer_refusals_leave_the_library_usable():
    torch, mg, hl = _gpu()
    u = smooth_field(SMALL, F32)
    ok = _config(hl, 1024)
    L = hl._hl()
    err = lambda: L.mgh_last_error()

    def refused(tols, cfg=ok, data=u, mode=mg.REL, msg=b""):
        with pytest.raises(mg.MgardHipError, match="error %d: compress_level_layers: " % MGH_ERR_INVALID_ARGUMENT):
            hl.compress_level_layers(data, tols, INF, mode, config=cfg)
        assert msg in err(), (msg, err())
        v = hl.decompress_level_layers(hl.compress_level_layers(u, [1e-1, 1e-2], INF, mg.REL, config=ok), 2, config=ok)
        assert v.shape == tuple(hl.infer_level(hl.compress(u, 1e-1, config=ok), 2)[0])

    for tols in ([10.0 ** -(k / 16) for k in range(65)], [1e-2, 1e-2], [1e-3, 1e-2], [1e-2, 0.0], [INF]):
        refused(tols)
    refused([1e-2, 1e-2], msg=b"strictly decreasing")
    refused([1e-1, 1e-2], cfg=_config(hl, 256, domain_decomposition=BLOCK, block_size=11), msg=b"decomposes the domain")
    refused([1e-1, 1e-2], cfg=_config(hl, 1023), msg=b"dict_size")
    noise = np.random.default_rng(7).standard_normal(SMALL).astype(F32)
    refused([1e-12], data=noise, mode=mg.ABS, msg=b"compress_level_layers: layer 0 would be stored raw")
    # reorder = 1 in the configuration is what the writer does anyway
    a = hl.compress_level_layers(u, [1e-1, 1e-2], INF, mg.REL, config=_config(hl, 1024, reorder=1))
    b = hl.compress_level_layers(u, [1e-1, 1e-2], INF, mg.REL, config=ok)
    assert all(_canonical(hl, x) == _canonical(hl, y) for x, y in zip(a, b))
    hl._hl().mgh_release_cache()


def test_reader_refusals_leave_the_handle_as_it_was():
    torch, mg, hl = _gpu()
    cfg = _config(hl, 1024)
    u = smooth_field(SMALL, F32)
    tols = [1e-1, 1e-2, 1e-3]
    b = hl.compress_level_layers(u, tols, INF, mg.REL, config=cfg)
    other_norm = hl.compress_level_layers(2.0 * u, tols, INF, mg.REL, config=cfg)
    other_shape = hl.compress_level_layers(smooth_field(FUSED3, F32), tols, INF, mg.REL, config=cfg)
    other_type = hl.compress_level_layers(u.astype(F64), tols, INF, mg.REL, config=cfg)
    other_mode = hl.compress_level_layers(u, [1e-1 * float(np.abs(u).max())], INF, mg.ABS, config=cfg)
    plain = hl.compress_layers(u, tols, INF, mg.REL, config=cfg)     # reorder = 0
    dd = _config(hl, 1024, domain_decomposition=BLOCK, block_size=11, reorder=1)
    two = hl.compress(u, 1e-2, INF, mg.REL, config=dd)
    assert hl.metadata_parse(_bytes(two))["domain_decomposed"]
    noise = np.random.default_rng(7).standard_normal(SMALL).astype(F32)
    raw = hl.compress(noise, 1e-12, INF, mg.ABS, config=_config(hl, 1024, reorder=1))
    assert _is_raw(hl, raw, noise)
    L = hl.infer_level(b[0], None, cfg)[1]
    assert L >= 3
    E = MGH_ERR_INVALID_ARGUMENT
    with hl.LevelLayers(b[0], L - 1, config=cfg) as r:
        r.add(b[1], L - 2)

        def state():
            return (r.count, [r.depth(k) for k in range(r.count)], [r.tolerance(k) for k in range(r.count)],
                    _bits(r.data(L - 1)).copy(), _bits(r.data(L - 2)).copy())

        def same(x, y):
            return x[:3] == y[:3] and np.array_equal(x[3], y[3]) and np.array_equal(x[4], y[4])

        before = state()
        for bad, lev, msg in ((b[0], 0, "tolerance"), (b[1], 0, "tolerance"), (other_norm[2], 0, "norm"),
                              (other_shape[2], 0, "shape"), (other_type[2], 0, "data type"),
                              (other_mode[0], 0, "error bound type"), (two, 0, "domain-decomposed"),
                              (plain[2], 0, "reorder = 0"), (raw, 0, "error bound type"),
                              (b[2], L - 1, "level"), (b[2], -1, "level")):
            with pytest.raises(mg.MgardHipError, match="error %d: mgh_level_layers_add: .*%s" % (E, msg)):
                r.add(bad, lev)
            assert same(state(), before), msg
        for k, bad, lev, msg in ((0, b[0], L - 1, "level"), (0, b[0], L + 1, "level"), (1, b[1], L, "level"),
                                 (1, b[1], L - 2, "level"), (1, b[2], L - 1, "not the one recorded"),
                                 (0, other_norm[0], L, "norm"), (0, plain[0], L, "reorder = 0"), (2, b[2], 0, "no layer 2")):
            with pytest.raises(mg.MgardHipError, match="error %d: mgh_level_layers_extend: .*%s" % (E, msg)):
                r.extend(k, bad, lev)
            assert same(state(), before), msg
        with pytest.raises(mg.MgardHipError, match="error %d: mgh_level_layers_data: " % E):
            r.data(L)
        assert same(state(), before)
        want = _bits(hl.decompress_level_layers(b, L - 2, config=cfg))
        assert np.array_equal(_bits(r.add(b[2], L - 2).data(L - 2)), want)
    for bufs, lev, msg in (([b[1], b[0]], 0, "mgh_level_layers_add: the tolerance"),
                           ([two], 0, "mgh_level_layers_open: .*domain-decomposed"),
                           ([plain[0]], 0, "mgh_level_layers_open: .*reorder = 0"), ([raw], 0, "mgh_level_layers_open: .*raw"),
                           ([b[0]], L + 1, "level"), ([b[0]], -1, "level")):
        with pytest.raises(mg.MgardHipError, match="error %d: .*%s" % (E, msg)):
            hl.decompress_level_layers(bufs, lev, config=cfg)
    hl._hl().mgh_release_cache()
