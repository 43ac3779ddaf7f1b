"""Level-by-level refinement on the device: mgh_refine_level against the linear path it is one step of, the
range decode of the lossless stage against a slice of the full decode, and the progressive reader against
mgh_decompress_level / mgh_decompress. Every comparison is bit-exact; the expected values come from calls the
suite pins to the oracle and the reference build elsewhere."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from tests import payload
from tests.test_gpu_level_prefix import GUARD, LINEAR_CASES, SENTINEL, _n, _symbols
from tests.test_gpu_multires import CASES, HL_CASES, Setup, _cpu, _profile_of, assert_bit_equal
from tests.util import nonuniform_coords, smooth_field

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one 4-D fused, one 5-D and one 1-D shape of BOX_SHAPES (tests/test_gpu_level_prefix.py)
EXTRA = [((8, 66, 70, 129), np.float32, dict(), "fused 4-D"),
         ((4, 3, 20, 5, 31), np.float64, dict(), "5-D: the generic N-D kernels"),
         ((300001,), np.float32, dict(), "1-D: rows longer than a row piece")]


def _refine_chain(S, ebtype, dict_size, profile=False):
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
    kw = dict(dict_size=dict_size, outlier_val=ov, outlier_idx=oi_lin)
    N = [_n(h.level_shape(l)) for l in range(L + 1)]
    cur = h.dequantize_recompose_linear(lin[:N[0]].clone(), ebtype, tol, float(s), norm, level=0, **kw)
    inside = outside = False
    tdt = cur.dtype
    prof = None
    for level in range(1, L + 1):
        want = h.dequantize_recompose_linear(lin[:N[level]].clone(), ebtype, tol, float(s), norm, level=level, **kw)
        cnt = N[level] - N[level - 1]
        seg = torch.cat([lin[N[level - 1]:N[level]].clone(),
                         torch.full((GUARD,), SENTINEL, dtype=torch.int64, device="cuda")])
        out = torch.empty(N[level] + GUARD, dtype=tdt, device="cuda")
        out[N[level]:] = -777.0
        coarse_before = cur.clone()
        if n:
            inside |= bool(((oi_lin >= N[level - 1]) & (oi_lin < N[level])).any())
            outside |= bool(((oi_lin < N[level - 1]) | (oi_lin >= N[level])).any())

        def step():
            return h.refine_level(cur, seg[:cnt], ebtype, tol, float(s), norm, level, dict_size=dict_size,
                                  outlier_idx=oi_lin, outlier_val=ov, out=out[:N[level]])
        if profile and level == L:
            prof = _profile_of(h, step)
        else:
            step()
        got = out[:N[level]].reshape(tuple(h.level_shape(level)))
        assert_bit_equal(_cpu(got), _cpu(want), "refine_level(level=%d)" % level)
        assert bool((out[N[level]:] == -777.0).all()), "level %d: written behind d_out" % level
        assert bool((seg[cnt:] == SENTINEL).all()), "level %d: written behind the segment" % level
        assert torch.equal(cur, coarse_before), "level %d: d_coarse was modified" % level
        cur = got.clone()  # the next step is fed this step's output
    return inside, outside, prof


@pytest.mark.parametrize("dict_size", [64, 8192])
@pytest.mark.parametrize("ebtype", ["REL", "ABS"])
@pytest.mark.parametrize("case", LINEAR_CASES + EXTRA, ids=lambda c: "x".join(map(str, c[0])) + "-" + np.dtype(c[1]).name)
def test_refine_level_chain(case, ebtype, dict_size):
    import mgard_amd as mg
    S = Setup(case)
    inside, outside, _ = _refine_chain(S, mg.REL if ebtype == "REL" else mg.ABS, dict_size)
    if dict_size == 64 and np.isinf(S.s) and S.L >= 2:
        assert (inside, outside) == (True, True), "outliers were expected inside and outside the segments"


def test_refine_level_profile():
    """A step at l_target of a fused 3-D case: the shell of the box, one level of launches, nothing below."""
    import mgard_amd as mg
    _, _, prof = _refine_chain(Setup(CASES[5]), mg.REL, 64, profile=True)
    print(prof)
    assert prof.get("shell_from_linear", 0) == 1, prof
    for k in ("box_from_linear", "recompose_head", "head_in", "level_linearize"):
        assert prof.get(k, 0) == 0, (k, prof)
    assert prof.get("restore_q", 0) == 1, prof


@pytest.mark.parametrize("env", [{"MGH_FORCE_V1": "1"}, {"MGH_FORCE_ND": "1"}, {"MGH_NO_RECOMPOSE_HEAD": "1"}],
                         ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_refine_level_under_developer_switches(monkeypatch, env):
    import mgard_amd as mg
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _refine_chain(Setup(((33, 40, 65), np.float32, dict(s=0.0), "")), mg.REL, 64)


@pytest.mark.parametrize("shape", [(65, 70, 129), (9, 8, 10, 17), (5000, 5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_entry_points_interleaved_on_one_handle(shape):
    """Every reconstruction entry shares the handle's compact boxes (qbox, level_box), nodal buffers and the
    helper that grows them: one call of each kind in turn on ONE handle -- the boxes asked for shrink, then
    grow; the second round starts with every buffer at its largest -- gives what the same call gives on a
    fresh handle, bit for bit. (65 x 70 x 129: fused 3-D, mixed symbol widths, a stop on the widened box
    alone; 9 x 8 x 10 x 17: the N-D kernels in place; 5000 x 5 x 7: the one-thread-per-element kernels on a
    compact box.)"""
    import torch
    import mgard_amd as mg
    dt, dict_size, tol, s = np.float32, 64, 1e-3, float("inf")
    u = smooth_field(shape, dt, seed=int(np.prod(shape)) % 100003, noise=1e-2)
    norm = float(dt(oracle.norm(u, s, True)))
    du = torch.from_numpy(u).cuda()
    prep = mg.Hierarchy(shape, dt)
    L = prep.l_target
    assert L >= 2
    q, oi, ov, n, _ = prep.decompose_quantize(du, mg.REL, tol, s, norm, dict_size=dict_size)
    assert n > 0
    coef = prep.decompose(du)
    oi_lin = oi.clone()
    lin = prep.level_linearize(q, outlier_idx=oi_lin).reshape(-1)
    N = [_n(prep.level_shape(l)) for l in range(L + 1)]
    kw = dict(dict_size=dict_size, outlier_idx=oi, outlier_val=ov)
    kwl = dict(dict_size=dict_size, outlier_idx=oi_lin, outlier_val=ov)
    a = (mg.REL, tol, s, norm)
    level1 = prep.dequantize_recompose_linear(lin[:N[1]].clone(), *a, level=1, **kwl)
    calls = [
        ("dequantize_recompose(level=L-1)", lambda h: h.dequantize_recompose(q.clone(), *a, level=L - 1, **kw)),
        ("linear(level=1)", lambda h: h.dequantize_recompose_linear(lin[:N[1]].clone(), *a, level=1, **kwl)),
        ("refine_level(2)", lambda h: h.refine_level(level1, lin[N[1]:N[2]].clone(), *a, 2, **kwl)),
    ]
    if prep.sym16_supported():
        sym, oi16, ov16, _, _ = prep.decompose_quantize_sym16(du, mg.REL, tol, s, norm, dict_size=dict_size)
        kw16 = dict(dict_size=dict_size, outlier_idx=oi16, outlier_val=ov16)
        calls += [("sym16(level=L-3)", lambda h: h.dequantize_recompose_sym16(sym, *a, level=max(L - 3, 0), **kw16)),
                  ("sym16()", lambda h: h.dequantize_recompose_sym16(sym, *a, **kw16))]
    else:
        assert shape != (65, 70, 129)
    calls += [
        ("recompose(level=0)", lambda h: h.recompose(coef, level=0)),
        ("dequantize_recompose()", lambda h: h.dequantize_recompose(q.clone(), *a, **kw)),
        ("linear(level=L)", lambda h: h.dequantize_recompose_linear(lin.clone(), *a, level=L, **kwl)),
    ]
    want = [_cpu(call(mg.Hierarchy(shape, dt))) for _, call in calls]
    shared = mg.Hierarchy(shape, dt)
    for round_ in (1, 2):
        for (name, call), w in zip(calls, want):
            assert_bit_equal(_cpu(call(shared)), w, "%s on the shared handle, round %d" % (name, round_))


# ---- the lossless stage: decode a chunk range ------------------------------------------------------
def test_lossless_decompress_range():
    import torch
    from mgard_amd import highlevel as hl
    ctx = hl.Lossless()
    for chunk in (20480, 512):
        n = 5 * chunk + 77
        q, idx, val = _symbols(n, 8192, chunk)
        dq, di, dv = (torch.from_numpy(a).cuda() for a in (q, idx, val))
        for lossless in (hl.HUFFMAN, hl.HUFFMAN_ZSTD):
            rec = ctx.compress(dq, 8192, chunk, lossless, outlier_idx=di, outlier_val=dv)
            full, _, _ = ctx.decompress(rec, n, lossless)
            assert np.array_equal(_cpu(full), q)
            for device in (False, True):
                pay = torch.from_numpy(np.frombuffer(rec, dtype=np.uint8).copy()).cuda() if device else rec
                ranges = [(0, chunk), (3, chunk + 5), (chunk + 7, 2 * chunk), (2 * chunk, 1), (4 * chunk - 1, 2),
                          (5 * chunk, 77), (5 * chunk + 76, 1), (chunk, n - chunk)]
                for first, count in ranges:
                    c0, c1 = first // chunk, (first + count - 1) // chunk
                    lo, hi = c0 * chunk, min(n, (c1 + 1) * chunk)
                    out = torch.full((hi - lo + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
                    before = hl.last_decompress_stats()
                    got, gi, gv = ctx.decompress(pay, n, lossless, first=first, count=count, out=out)
                    after = hl.last_decompress_stats()
                    what = (chunk, lossless, "device" if device else "host", first, count)
                    g = _cpu(got)
                    assert np.array_equal(g[:hi - lo], q[lo:hi]), what
                    assert np.all(g[hi - lo:] == SENTINEL), ("the guard behind the range was written",) + what
                    assert after["chunks_decoded"] - before["chunks_decoded"] == c1 - c0 + 1, what
                    assert after["symbols_decoded"] - before["symbols_decoded"] == hi - lo, what
                    order = np.argsort(_cpu(gi), kind="stable")
                    assert np.array_equal(_cpu(gi)[order], idx) and np.array_equal(_cpu(gv)[order], val), what
            with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
                ctx.decompress(rec, n, lossless, first=n, count=1)
            with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
                ctx.decompress(rec, n, lossless, first=0, count=0)
    ctx.close()


# ---- the progressive reader ------------------------------------------------------------------------
def _walk(buf, cfg, levels, device_stream, L):
    """Refines through `levels`; returns the per-refine stats. Each result against decompress(level)."""
    from mgard_amd import highlevel as hl
    stats = []
    with hl.Progressive(buf, cfg) as p:
        assert p.level == -1
        for level in levels:
            got = p.refine(level)
            st = hl.last_decompress_stats()
            assert p.level == level
            want = hl.decompress(buf, config=cfg, level=level)
            g, w = (_cpu(got), _cpu(want)) if device_stream else (got, want)
            assert_bit_equal(g, w, "Progressive.refine(%d)" % level)
            if level == L:
                full = hl.decompress(buf, config=cfg)
                assert_bit_equal(g, _cpu(full) if device_stream else full, "Progressive at l_target against decompress")
            stats.append(st)
        for bad in (levels[-1], 0):
            if bad <= p.level:
                with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
                    p.refine(bad)
        with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
            p.refine(L + 1)
    return stats


@pytest.mark.parametrize("device_stream", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("lossless", ["Huffman", "Huffman_Zstd"])
@pytest.mark.parametrize("case", HL_CASES, ids=lambda c: "x".join(map(str, c[0])) + "-" + np.dtype(c[1]).name)
def test_progressive_walk(case, lossless, device_stream):
    import torch
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    shape, dt, nonuniform = case
    coords = nonuniform_coords(shape, dt, seed=sum(shape)) if nonuniform else None
    u = smooth_field(shape, dt)
    cfg = hl.Config(lossless=hl.HUFFMAN if lossless == "Huffman" else hl.HUFFMAN_ZSTD, reorder=1)
    buf = hl.compress(torch.from_numpy(u).cuda() if device_stream else u, 1e-3, np.inf, mg.REL, coords=coords, config=cfg)
    L = hl.infer_level(buf, None, cfg)[1]
    host = _cpu(buf) if device_stream else np.asarray(buf)
    meta = hl.metadata_parse(bytes(host[:65536]))
    rec, = payload.split_container(host, meta["metadata_size"])
    raw = len(rec) == u.nbytes
    total = -(-_n(shape) // int(cfg.huff_block_size))
    need = [hl.infer_level_range(buf, l, cfg)[3] for l in range(L + 1)]
    walks = [list(range(L + 1))]
    if L >= 1:
        walks.append([L - 1, L])
    for levels in walks:
        stats = _walk(buf, cfg, levels, device_stream, L)
        if raw:
            continue
        print(levels, stats)
        assert all(st["chunks_total"] == total and st["subdomains"] == 1 for st in stats), stats
        assert sum(st["chunks_decoded"] for st in stats) == total, stats  # every chunk once
        prev = -1
        for level, st in zip(levels, stats):
            assert st["chunks_decoded"] <= sum(need[prev + 1:level + 1]) + 1, (level, st)
            prev = level


def test_progressive_refusals():
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    u = smooth_field((65, 70, 129), np.float32)
    plain = hl.compress(u, 1e-3, np.inf, mg.REL, config=hl.Config(reorder=0))
    with pytest.raises(hl.MgardHipError, match=r"error -1\b.*reorder = 1"):
        hl.Progressive(plain)
    dd = hl.compress(u, 1e-3, np.inf, mg.REL, config=hl.Config(reorder=1, domain_decomposition=hl.DD_BLOCK,
                                                                 block_size=40))
    assert hl.metadata_parse(bytes(np.asarray(dd)[:65536]))["domain_decomposed"]
    with pytest.raises(hl.MgardHipError, match=r"error -1\b.*domain-decomposed"):
        hl.Progressive(dd)
    cfg = hl.Config(reorder=1)
    good = hl.compress(u, 1e-3, np.inf, mg.REL, config=cfg)
    with hl.Progressive(good, cfg) as p:
        a = p.refine(2)
        with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
            p.refine(2)
        with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
            p.refine(1)
        b = p.refine(3)  # the reader works afterwards
    assert_bit_equal(a, hl.decompress(good, config=cfg, level=2), "after the refusals (2)")
    assert_bit_equal(b, hl.decompress(good, config=cfg, level=3), "after the refusals (3)")


def test_progressive_raw_record():
    """Random noise at a tight bound: the lossless stage does not pay, the record is the data itself."""
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    shape = (33, 40, 65)
    u = np.random.default_rng(5).standard_normal(shape).astype(np.float32)
    cfg = hl.Config(reorder=1)
    buf = hl.compress(u, 1e-7, np.inf, mg.REL, config=cfg)
    meta = hl.metadata_parse(bytes(np.asarray(buf)[:65536]))
    rec, = payload.split_container(np.asarray(buf), meta["metadata_size"])
    assert len(rec) == u.nbytes, "the record was expected to be stored raw"
    L = hl.infer_level(buf, None, cfg)[1]
    _walk(buf, cfg, list(range(L + 1)), False, L)
    with hl.Progressive(buf, cfg) as p:
        assert_bit_equal(p.refine(L), hl.decompress(buf, config=cfg), "raw record, straight to l_target")


def test_cpp_progressive_consumer(tmp_path):
    """open -> refine x 2 -> close through the C++ header mirror, against mgh_decompress_level."""
    import mgard_amd
    exe = str(tmp_path / "progressive_refine")
    lib = mgard_amd.lib_path()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "progressive_refine.cpp"),
                           "-L", os.path.dirname(lib), "-lmgard_hip", "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "progressive ok" in r.stdout, r.stdout
