"""Reduced resolution from the head of a reorder = 1 record: k_box_from_linear (the box of a level straight from
the level-linearised head), mgh_dequantize_recompose_linear_to_level, the prefix decode of the lossless stage,
mgh_decompress_level on reorder = 1 containers and mgh_last_decompress_stats. Every comparison is bit-exact."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import oracle
from tests import payload
from tests.test_gpu_multires import CASES, HL_CASES, Setup, _cpu, _profile_of, assert_bit_equal
from tests.util import nonuniform_coords, smooth_field

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -0x0123456789ABCDEF
GUARD = 256


def _n(shape):
    return int(np.prod(shape))


BOX_SHAPES = [c[0] for c in HL_CASES] + [
    (130, 257),        # 2-D
    (64, 32, 128),     # 2^k
    (65, 33, 129),     # 2^k + 1
    (66, 34, 130),     # even, not a power of two
    (17, 17, 17),
    (8, 66, 70, 129),  # fused 4-D
    (300001,),         # 1-D: the row is longer than a row piece at several levels
]


@pytest.mark.parametrize("shape", BOX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_level_box_from_linear(shape):
    import torch
    import mgard_amd as mg
    h = mg.Hierarchy(shape, np.float32)
    o = oracle.Hierarchy(shape, np.float32)
    L = h.l_target
    rng = np.random.default_rng(_n(shape) % 65521)
    q = rng.integers(-2 ** 62, 2 ** 62, size=shape, dtype=np.int64)
    lin = o.level_linearize(q).reshape(-1)
    for level in range(L + 1):
        m = h.level_shape(level)
        n_l = _n(m)
        head = torch.from_numpy(lin[:n_l].copy()).cuda()  # exactly N_l long
        assert head.numel() == n_l
        out = torch.full((n_l + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
        h.level_box_from_linear(head, level, out=out)
        got = _cpu(out)
        assert np.all(got[n_l:] == SENTINEL), "level %d: the guard behind the box was written" % level
        want = np.ascontiguousarray(q[tuple(slice(0, e) for e in m)])
        assert_bit_equal(got[:n_l].reshape(m).view(np.uint64), want.view(np.uint64), "box of level %d" % level)
        assert np.array_equal(_cpu(head), lin[:n_l]), "the input was modified"
    full = torch.from_numpy(lin.copy()).cuda()
    back = h.level_linearize(full.reshape(shape), inverse=True)
    box = h.level_box_from_linear(full, L)
    assert np.array_equal(_cpu(box).reshape(-1), _cpu(back).reshape(-1)), "l_target against level_linearize(inverse)"


def _linear_case(S, ebtype, dict_size, levels=None, profile=False):
    """dequantize_recompose_linear(lin[:N_l]) against dequantize_recompose(q) on the full array, every level."""
    import torch
    import mgard_amd as mg
    h, L, s = S.h, S.L, S.s
    if ebtype == mg.REL:
        tol, norm = 1e-3, float(S.dt(oracle.norm(S.u, s, S.normalize)))
    else:
        tol, norm = 1e-3 * float(np.max(np.abs(S.u))), 1.0
    du = torch.from_numpy(S.u).cuda()
    q, oi, ov, n, _ = h.decompose_quantize(du, ebtype, tol, float(s), norm, dict_size=dict_size)
    oi_lin = oi.clone()
    lin = h.level_linearize(q, outlier_idx=oi_lin).reshape(-1)
    kw = dict(dict_size=dict_size, outlier_val=ov)
    inside_seen = behind_seen = False
    for level in (range(L + 1) if levels is None else levels):
        n_l = _n(h.level_shape(level))
        if n:
            inside_seen |= bool((oi_lin < n_l).any())
            behind_seen |= bool((oi_lin >= n_l).any())
        want = h.dequantize_recompose(q.clone(), ebtype, tol, float(s), norm, outlier_idx=oi, level=level, **kw)
        head = torch.cat([lin[:n_l].clone(), torch.full((GUARD,), SENTINEL, dtype=torch.int64, device="cuda")])
        got = h.dequantize_recompose_linear(head[:n_l], ebtype, tol, float(s), norm, outlier_idx=oi_lin, level=level,
                                            **kw)
        assert tuple(got.shape) == tuple(h.level_shape(level))
        assert_bit_equal(_cpu(got), _cpu(want), "dequantize_recompose_linear(level=%d)" % level)
        assert bool((head[n_l:] == SENTINEL).all()), "level %d: written behind the head" % level
    if profile and L >= 1:
        n_l = _n(h.level_shape(L - 1))
        prof = _profile_of(h, lambda: h.dequantize_recompose_linear(lin[:n_l].clone(), ebtype, tol, float(s), norm,
                                                                    outlier_idx=oi_lin, level=L - 1, **kw))
        print(prof)
        assert prof.get("box_from_linear", 0) == 1, prof
        assert prof.get("level_linearize", 0) == 0, prof
        return prof
    return inside_seen, behind_seen


# f32 and f64, uniform and non-uniform, s = inf and s = 0, every route of the level loops
LINEAR_CASES = [CASES[i] for i in (0, 1, 2, 6, 8, 10, 11, 12, 13)]


@pytest.mark.parametrize("dict_size", [64, 8192])
@pytest.mark.parametrize("ebtype", ["REL", "ABS"])
@pytest.mark.parametrize("case", LINEAR_CASES, ids=lambda c: "x".join(map(str, c[0])) + "-" + np.dtype(c[1]).name)
def test_dequantize_recompose_linear(case, ebtype, dict_size):
    import mgard_amd as mg
    S = Setup(case)
    seen = _linear_case(S, mg.REL if ebtype == "REL" else mg.ABS, dict_size)
    if dict_size == 64 and np.isinf(S.s) and S.L >= 2:
        assert seen == (True, True), "outliers were expected inside and behind the heads"


def test_dequantize_recompose_linear_profile():
    import mgard_amd as mg
    for case in (CASES[2], CASES[6], CASES[10]):
        _linear_case(Setup(case), mg.REL, 64, levels=[], profile=True)


@pytest.mark.parametrize("env, expect, absent", [
    ({"MGH_FORCE_V1": "1"}, ("box_dequantize", "gpk_rev"), ("recompose_head", "restore_q")),
    ({"MGH_NO_RECOMPOSE_HEAD": "1"}, ("head_in", "restore_q"), ("recompose_head", "box_dequantize")),
    ({"MGH_FORCE_ND": "1"}, ("box_dequantize", "nd_apply"), ("recompose_head", "restore_q")),
], ids=["force_v1", "no_head", "force_nd"])
def test_developer_switches_take_the_linear_head(monkeypatch, env, expect, absent):
    import mgard_amd as mg
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    S = Setup(((33, 40, 65), np.float32, dict(s=0.0), ""))
    _linear_case(S, mg.REL, 64)
    prof = _linear_case(S, mg.REL, 64, levels=[], profile=True)
    for k in expect:
        assert prof.get(k, 0) >= 1, (k, prof)
    for k in absent:
        assert prof.get(k, 0) == 0, (k, prof)


# ---- the lossless stage: decode a prefix -----------------------------------------------------------
def _symbols(n, dict_size, seed):
    """Skewed symbols in [1, dict) and a few out-of-dictionary entries (symbol 0 + the lists)."""
    rng = np.random.default_rng(seed)
    q = np.clip(np.rint(rng.normal(dict_size / 2, 6.0, size=n)), 1, dict_size - 1).astype(np.int64)
    idx = np.sort(rng.choice(n, size=min(n, 37), replace=False)).astype(np.int64)
    val = rng.integers(-10 ** 9, 10 ** 9, size=idx.size, dtype=np.int64)
    q[idx] = 0
    return q, idx, val


def _prefix_check(chunks=(20480, 512), kinds=("Huffman", "Huffman_Zstd")):
    import torch
    from mgard_amd import highlevel as hl
    ctx = hl.Lossless()
    for chunk in chunks:
        n = 3 * chunk + 77
        q, idx, val = _symbols(n, 8192, chunk)
        dq, di, dv = (torch.from_numpy(a).cuda() for a in (q, idx, val))
        for kind in kinds:
            lossless = hl.HUFFMAN if kind == "Huffman" else hl.HUFFMAN_ZSTD
            rec = ctx.compress(dq, 8192, chunk, lossless, outlier_idx=di, outlier_val=dv)
            full, fi, fv = ctx.decompress(rec, n, lossless)
            assert np.array_equal(_cpu(full), q), (chunk, kind)
            for device in (False, True):
                pay = torch.from_numpy(np.frombuffer(rec, dtype=np.uint8).copy()).cuda() if device else rec
                for p in (1, chunk - 1, chunk, chunk + 1, n - 1, n):
                    written = min(n, -(-p // chunk) * chunk)
                    out = torch.full((written + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
                    got, gi, gv = ctx.decompress(pay, n, lossless, prefix=p, out=out)
                    g = _cpu(got)
                    what = (chunk, kind, "device" if device else "host", p)
                    assert np.array_equal(g[:written], q[:written]), what
                    assert np.all(g[written:] == SENTINEL), ("the guard behind the prefix was written",) + what
                    order = np.argsort(_cpu(gi), kind="stable")
                    assert np.array_equal(_cpu(gi)[order], idx) and np.array_equal(_cpu(gv)[order], val), what
    ctx.close()


def test_lossless_decompress_prefix():
    _prefix_check()


@pytest.mark.parametrize("env", [{"MGH_HUFF_SYNC_DECODE": "0"}, {"MGH_HUFF_SERIAL_DECODE": "1"},
                                 {"MGH_HUFF_PAR_DECODE": "1"}], ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_lossless_decompress_prefix_under_decoder_switches(env):
    """The switches are read once per process: a child process each."""
    child_env = dict(os.environ, **env)
    child_env["PYTHONPATH"] = ROOT + os.pathsep + child_env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_level_prefix import _prefix_check; _prefix_check()"],
                       cwd=ROOT, env=child_env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the high-level call -----------------------------------------------------------------------------
def _record_offsets(rec):
    """(offset of the code units in the record, parsed record)"""
    r = payload.parse_huffman_record(rec)
    nchunk = len(r["bits"])
    off = 8 + 8 + 8 + 16 * nchunk + 8 + 8 * 128 + 8 * int(r["dict_size"]) + 8
    assert np.array_equal(np.frombuffer(rec, dtype="<u8", count=len(r["units"]), offset=off), r["units"])
    return off, r


def _moved_bound(rec, chunks):
    """Bytes of a host Huffman record the prefix decode may move: the head, the code units up to the end of the
    last needed chunk plus the one the decoders peek at, the outlier lists, the synchronisation entries of the
    needed chunks."""
    off, r = _record_offsets(rec)
    units = max(int(r["entry"][k]) + (int(r["bits"][k]) + 63) // 64 for k in range(chunks))
    return off + 8 * (units + 1) + 16 * len(r["outlier_idx"]) + (256 * chunks if r["sync"] is not None else 0)


@pytest.mark.parametrize("device_stream", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("lossless", ["Huffman", "Huffman_Zstd"])
@pytest.mark.parametrize("case", HL_CASES, ids=lambda c: "x".join(map(str, c[0])) + "-" + np.dtype(c[1]).name)
def test_decompress_level_decodes_the_head_only(case, lossless, device_stream):
    import torch
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    shape, dt, nonuniform = case
    tol = 1e-3
    coords = nonuniform_coords(shape, dt, seed=sum(shape)) if nonuniform else None
    u = smooth_field(shape, dt)
    du = torch.from_numpy(u).cuda()
    h = mg.Hierarchy(shape, dt, coords=coords)
    L = h.l_target
    n = _n(shape)
    for reorder in (1, 0):
        cfg = hl.Config(lossless=hl.HUFFMAN if lossless == "Huffman" else hl.HUFFMAN_ZSTD, reorder=reorder)
        block = int(cfg.huff_block_size)
        buf = hl.compress(du if device_stream else u, tol, np.inf, mg.REL, coords=coords, config=cfg)
        host = _cpu(buf) if device_stream else np.asarray(buf)
        meta = hl.metadata_parse(bytes(host[:65536]))
        norm = meta["norm"]
        rec, = payload.split_container(host, meta["metadata_size"])
        raw = len(rec) == u.nbytes  # (the lossless stage did not pay: the record is the data, nothing is decoded)
        q, oi, ov, _, _ = h.decompose_quantize(du, mg.REL, tol, np.inf, norm, dict_size=int(cfg.huff_dict_size))
        total = -(-n // block)
        for level in range(L + 1):
            got = hl.decompress(buf, config=cfg, level=level)
            st = hl.last_decompress_stats()
            got = _cpu(got) if device_stream else got
            if raw:
                assert st["subdomains"] == 1 and st["chunks_total"] == 0 and st["chunks_decoded"] == 0, st
                continue
            want = h.dequantize_recompose(q.clone(), mg.REL, tol, np.inf, norm, dict_size=int(cfg.huff_dict_size),
                                          outlier_idx=oi, outlier_val=ov, level=level)
            assert_bit_equal(got, _cpu(want), "decompress(level=%d, reorder=%d)" % (level, reorder))
            print(level, reorder, st)
            assert st["subdomains"] == 1 and st["chunks_total"] == total and st["record_bytes"] == len(rec), st
            if reorder == 1 and level < L:
                need = -(-_n(h.level_shape(level)) // block)
                assert st["chunks_decoded"] == need, (level, st)
                assert st["symbols_decoded"] == min(n, need * block), (level, st)
                if lossless == "Huffman" and not device_stream:
                    assert st["record_bytes_moved"] <= _moved_bound(rec, need), (level, st, _moved_bound(rec, need))
            else:
                assert st["chunks_decoded"] == total and st["symbols_decoded"] == n, (level, st)
        hl.decompress(buf, config=cfg)
        assert hl.last_decompress_stats()["chunks_decoded"] == (0 if raw else total)


def test_damaged_records():
    """Code units behind the last needed chunk do not matter; a chunk-table entry of a NEEDED chunk that points
    outside the stream is MGH_ERR_FORMAT, and the library stays usable."""
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    shape = (129, 130, 257)
    u = smooth_field(shape, np.float32)
    cfg = hl.Config(reorder=1)
    buf = np.asarray(hl.compress(u, 1e-3, np.inf, mg.REL, config=cfg)).copy()
    meta = hl.metadata_parse(bytes(buf[:65536]))
    rec, = payload.split_container(buf, meta["metadata_size"])
    off, r = _record_offsets(rec)
    base = meta["metadata_size"] + 8
    h = mg.Hierarchy(shape, np.float32)
    L = h.l_target
    level = L - 2
    need = -(-_n(h.level_shape(level)) // int(cfg.huff_block_size))
    assert need < len(r["bits"])
    want = hl.decompress(buf, config=cfg, level=level)
    units = max(int(r["entry"][k]) + (int(r["bits"][k]) + 63) // 64 for k in range(need))
    bad = buf.copy()
    bad[base + off + 8 * (units + 1): base + off + 8 * len(r["units"])] = 0xA5
    assert_bit_equal(hl.decompress(bad, config=cfg, level=level), want, "units behind the head overwritten")
    bad = buf.copy()
    entry0 = base + 24 + 8 * len(r["bits"])  # entry[0]
    bad[entry0:entry0 + 8] = np.frombuffer(struct.pack("<Q", len(r["units"]) + 5), dtype=np.uint8)
    with pytest.raises(mg.MgardHipError, match=r"error -8\b"):
        hl.decompress(bad, config=cfg, level=level)
    assert_bit_equal(hl.decompress(buf, config=cfg, level=level), want, "after the error")
