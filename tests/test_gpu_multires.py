"""Reconstruction at a coarser level of the hierarchy (mgh_*_to_level, mgh_decompress_level) on the GPU.

Expected values: expected(L) = recompose(z_L)[nodes of level L], z_L = the coefficients zeroed outside
the corner box level_shape(L) -- by the CPU oracle and by the build of the reference (oracle/_ref),
floats through their bit patterns. tests/test_multires_cpu.py pins that yardstick itself.

The cases follow tests/test_gpu_reference_binary.py: one per kernel family of DESIGN.md's kernel
table, and EVERY level 0 .. l_target of each.
"""
import numpy as np
import pytest

import oracle
from oracle import ref
from tests.test_multires_cpu import expected_level, keep_rule
from tests.util import nonuniform_coords, smooth_field

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not ref.available(), reason="%s is not built (oracle.build_ref())" % ref.LIB_PATH)

REL, ABS = 0, 1

# (shape, dtype, options, the path the case targets); options as in test_gpu_reference_binary.py
CASES = [
    ((17, 17, 17), np.float32, dict(),
     "every level inside k_recompose_head: every stop below l_target is a stop INSIDE the head"),
    ((33, 40, 65), np.float64, dict(s=0.0),
     "head + one or two levels of their own launches; stops inside the head and above it"),
    ((65, 70, 129), np.float64, dict(coords="nonuniform", s=0.0),
     "fused 3-D level kernels, 8 x 32 tiles; mixed 16-bit symbols (total >= 2^18, L >= 4)"),
    ((40, 130, 9), np.float32, dict(normalize=False, s=1.0),
     "fused 3-D with 64 x 4 tiles (short fastest extent)"),
    ((70, 300, 5), np.float64, dict(max_level=1, s=-1.0),
     "64 x 4 tiles, hierarchy cut by max_level"),
    ((129, 130, 257), np.float32, dict(),
     "larger fused 3-D levels: streaming / LDS-DMA Thomas solves, 4 x 64 restore tiles"),
    ((5000, 5, 7), np.float32, dict(s=0.5),
     "thin array: the one-thread-per-element kernels (v1) on a compact box"),
    ((3000, 17, 17), np.float64, dict(coords="nonuniform", max_level="top-1"),
     "chunked strided solves, hierarchy cut by max_level"),
    ((8, 66, 70, 129), np.float32, dict(s=0.0),
     "fused 4-D slice path"),
    ((20, 40, 40, 40), np.float64, dict(normalize=False, max_level=1, s=1.0),
     "fused 4-D slice path, normalize_coordinates = False, max_level"),
    ((9, 8, 10, 17), np.float32, dict(coords="nonuniform"),
     "4-D outside the fused kernels: generic N-D kernels on a compact box"),
    ((4, 3, 70, 5, 131), np.float32, dict(s=1.0),
     "D = 5: generic N-D row kernels"),
    ((300001,), np.float32, dict(),
     "1-D long pencil"),
    ((257, 130), np.float64, dict(normalize=False, s=0.5, max_level="top-1"),
     "D = 2: the one-thread-per-element kernels"),
]
IDS = ["x".join(map(str, c[0])) + "-" + np.dtype(c[1]).name for c in CASES]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_bit_equal(got, want, what):
    gb, wb = _bits(got), _bits(want)
    assert gb.shape == wb.shape, (what, gb.shape, wb.shape)
    if not np.array_equal(gb, wb):
        bad = np.argwhere(gb != wb)
        i = tuple(bad[0])
        raise AssertionError("%s: %d/%d elements differ; first at %s: HIP %r expected %r" % (
            what, len(bad), gb.size, i, got[i], want[i]))


def _cpu(t):
    return t.cpu().numpy()


class Setup:
    def __init__(self, case, cls=oracle.Hierarchy):
        import mgard_amd as mg
        shape, dt, opt, _ = case
        self.shape, self.dt, self.opt = shape, dt, opt
        coords = nonuniform_coords(shape, dt, seed=sum(shape)) if opt.get("coords") else None
        self.normalize = opt.get("normalize", True)
        ml = opt.get("max_level")
        if ml == "top-1":
            ml = oracle.Hierarchy(shape, dt).l_target - 1
        kw = {} if ml is None else dict(max_level=ml)
        self.o = cls(shape, dt, coords=coords, normalize_coordinates=self.normalize, **kw)
        self.h = mg.Hierarchy(shape, dt, coords=coords, normalize_coordinates=self.normalize, max_level=ml)
        assert self.h.l_target == self.o.l_target
        self.L = self.h.l_target
        self.u = smooth_field(shape, dt, seed=int(np.prod(shape)) % 100003, noise=1e-2)
        self.s = opt.get("s", np.inf)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_recompose_to_level_equals_oracle(case):
    import torch
    S = Setup(case)
    c = S.o.decompose(S.u)
    dc = torch.from_numpy(c).cuda()
    for level in range(S.L + 1):
        assert S.h.level_shape(level) == S.o.level_shape(level)
        for d, n in enumerate(S.shape):
            assert np.array_equal(S.h.level_nodes(level, d), keep_rule(n, S.L - level))
        got = S.h.recompose(dc, level=level)
        assert tuple(got.shape) == S.o.level_shape(level)
        assert_bit_equal(_cpu(got), expected_level(S.o, c, level), "recompose(level=%d)" % level)
    assert_bit_equal(_cpu(S.h.recompose(dc, level=S.L)), _cpu(S.h.recompose(dc)), "level = l_target")
    assert np.array_equal(_cpu(dc), c), "the coefficients were modified"


@needs_ref
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_recompose_to_level_equals_reference_build(case):
    import torch
    S = Setup(case, ref.Hierarchy)
    c = S.o.decompose(S.u)
    dc = torch.from_numpy(c).cuda()
    for level in range(S.L + 1):
        assert_bit_equal(_cpu(S.h.recompose(dc, level=level)), expected_level(S.o, c, level),
                         "recompose(level=%d)" % level)


@pytest.mark.parametrize("dict_size", [64, 8192])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dequantize_recompose_to_level(case, dict_size):
    """From integers the GPU quantized: dict_size 64 leaves outliers inside and outside every box."""
    import torch
    import mgard_amd as mg
    S = Setup(case)
    h, o, L, s = S.h, S.o, S.L, S.s
    tol = 1e-3
    norm = float(S.dt(oracle.norm(S.u, s, S.normalize)))
    du = torch.from_numpy(S.u).cuda()
    q, oi, ov, n, _ = h.decompose_quantize(du, mg.REL, tol, float(s), norm, dict_size=dict_size)
    q0 = _cpu(q).copy()
    if dict_size == 64 and np.isinf(s):
        # s = inf: one bin is tol * norm / ((l_target + 1) * (1 + 3^D)) on every level, so values of the size
        # of the norm lie thousands of bins out and +-32 bins cannot hold the level-0 nodes
        assert n > 0
    v = o.dequantize(q0, oracle.REL, S.dt(tol), S.dt(s), S.dt(norm), dict_size, True,
                     outlier_idx=_cpu(oi).astype(np.uint64), outlier_val=_cpu(ov))
    kw = dict(dict_size=dict_size, outlier_idx=oi, outlier_val=ov)
    exp = [expected_level(o, v, level) for level in range(L + 1)]
    # every level from a fresh copy; the integers outside the box stay as they were
    for level in range(L + 1):
        qq = q.clone()
        got = h.dequantize_recompose(qq, mg.REL, tol, float(s), norm, level=level, **kw)
        assert_bit_equal(_cpu(got), exp[level], "dequantize_recompose(level=%d)" % level)
        if level < L:
            after = _cpu(qq)
            box = tuple(slice(0, m) for m in h.level_shape(level))
            outside = np.ones(S.shape, dtype=bool)
            outside[box] = False
            assert np.array_equal(after[outside], q0[outside]), "integers outside the box of level %d changed" % level
    # ... and levels 0, 1, ..., l_target in turn on ONE buffer
    qq = q.clone()
    for level in range(L + 1):
        got = h.dequantize_recompose(qq, mg.REL, tol, float(s), norm, level=level, **kw)
        assert_bit_equal(_cpu(got), exp[level], "in turn, level %d" % level)
    full = h.dequantize_recompose(q.clone(), mg.REL, tol, float(s), norm, **kw)
    assert_bit_equal(_cpu(got), _cpu(full), "level = l_target against the call without a level")
    # 16-bit symbols: the same values as from the integers
    if h.sym16_supported():
        sym, oi16, ov16, n16, _ = h.decompose_quantize_sym16(du, mg.REL, tol, float(s), norm, dict_size=dict_size)
        assert n16 == n
        sym0 = _cpu(sym.view(torch.int16)).copy()
        for level in range(L + 1):
            got16 = h.dequantize_recompose_sym16(sym, mg.REL, tol, float(s), norm, dict_size=dict_size,
                                                 outlier_idx=oi16, outlier_val=ov16, level=level)
            assert_bit_equal(_cpu(got16), exp[level], "sym16, level %d" % level)
        assert np.array_equal(_cpu(sym.view(torch.int16)), sym0), "the symbols were modified"


def test_sym16_runs_on_both_sides_of_the_mixed_threshold():
    """The sym16 leg above is not vacuous: the 3-D fused cases run it below (17^3) and above (65 x 70 x 129,
    129 x 130 x 257: total >= 2^18, L >= 4) the threshold of the mixed mode, and the fused 4-D case too."""
    import mgard_amd as mg
    for shape, mixed in (((17, 17, 17), False), ((65, 70, 129), True), ((129, 130, 257), True)):
        h = mg.Hierarchy(shape, np.float32)
        assert h.sym16_supported()
        assert (h.total >= 2 ** 18 and h.l_target >= 4) == mixed


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_level_out_of_range(case):
    import torch
    import mgard_amd as mg
    S = Setup(case)
    h = S.h
    c = S.o.decompose(S.u)
    dc = torch.from_numpy(c).cuda()
    q = torch.zeros(S.shape, dtype=torch.int64, device="cuda")
    out = torch.empty(S.shape, dtype=h.torch_dtype, device="cuda")
    for bad in (-1, S.L + 1):
        with pytest.raises(mg.MgardHipError, match=r"error -1\b"):
            h.recompose(dc, out=out, level=bad)
        with pytest.raises(mg.MgardHipError, match=r"error -1\b"):
            h.dequantize_recompose(q, mg.REL, 1e-3, np.inf, 1.0, out=out, level=bad)
        with pytest.raises(mg.MgardHipError, match=r"error -1\b"):
            h.level_nodes(bad, 0)
        if h.sym16_supported():
            sym = torch.zeros(S.shape, dtype=torch.int16, device="cuda").view(torch.uint16)
            with pytest.raises(mg.MgardHipError, match=r"error -1\b"):
                h.dequantize_recompose_sym16(sym, mg.REL, 1e-3, np.inf, 1.0, out=out, level=bad)
    assert_bit_equal(_cpu(h.recompose(dc, level=0)), expected_level(S.o, c, 0), "the handle after the errors")
    assert_bit_equal(_cpu(h.recompose(dc)), S.o.recompose(c), "the handle after the errors")


def test_no_full_size_work_below_the_finest_level():
    """257^3 f32 at l_target - 2: the level loop ends two levels early and nothing full-sized runs.
    Launch counts of the per-level kernels against the full call's."""
    import torch
    import mgard_amd as mg
    shape = (257, 257, 257)
    h = mg.Hierarchy(shape, np.float32)
    L = h.l_target
    u = smooth_field(shape, np.float32)
    du = torch.from_numpy(u).cuda()
    q, oi, ov, n, nrm = h.decompose_quantize(du, mg.REL, 1e-3, np.inf)
    sym, oi16, ov16, n16, _ = h.decompose_quantize_sym16(du, mg.REL, 1e-3, np.inf, nrm)
    per_level = ("restore_q", "restore_q_odd", "loadvec_q", "loadvec_q_small")

    def count(prof, names):
        return sum(prof.get(k, (0.0, 0))[1] for k in names)

    h.profile(True)
    h.dequantize_recompose(q.clone(), mg.REL, 1e-3, np.inf, nrm, outlier_idx=oi, outlier_val=ov)
    full = h.profile_read()
    h.dequantize_recompose(q.clone(), mg.REL, 1e-3, np.inf, nrm, outlier_idx=oi, outlier_val=ov, level=L - 2)
    part = h.profile_read()
    h.dequantize_recompose_sym16(sym, mg.REL, 1e-3, np.inf, nrm, outlier_idx=oi16, outlier_val=ov16)
    full16 = h.profile_read()
    h.dequantize_recompose_sym16(sym, mg.REL, 1e-3, np.inf, nrm, outlier_idx=oi16, outlier_val=ov16, level=L - 2)
    part16 = h.profile_read()
    h.profile(False)
    print("full", full, "\nlevel", part, "\nfull16", full16, "\nlevel16", part16)
    head = full["recompose_head"][1]
    assert head == 1 and part["recompose_head"][1] == 1
    own_levels_full = count(full, ("restore_q",))
    assert own_levels_full >= 3  # (the head kernel cannot hold 129^3: levels L-1 and L have their own launches)
    for prof, fullp in ((part, full), (part16, full16)):
        assert count(prof, ("restore_q",)) == own_levels_full - 2
        assert count(prof, ("restore_q_odd",)) == 0
        assert count(prof, ("loadvec_q", "loadvec_q_small")) == count(fullp, ("loadvec_q", "loadvec_q_small")) - 2
        assert count(prof, per_level) <= 2 * (L - 2)  # one loadvec + one restore per level actually run, at most
        assert count(prof, ("dequantize", "box_dequantize", "box_gather")) == 0  # (fused path: the box is read in place)
    # the mixed 16-bit path at or below L - ntop: ONE widened box (the stop level's), no table of the finest levels
    # (a name stays in the profile after a reset, with a count of zero)
    assert count(part16, ("widen_box",)) == 1 and count(part16, ("outlier_table",)) == 0
    assert count(full16, ("widen_box",)) == 1
    # the stop at l_target - 1 on symbols (above L - ntop): the full call's path minus the top level
    h.profile(True)
    h.dequantize_recompose_sym16(sym, mg.REL, 1e-3, np.inf, nrm, outlier_idx=oi16, outlier_val=ov16, level=L - 1)
    p1 = h.profile_read()
    h.profile(False)
    assert count(p1, ("restore_q",)) == own_levels_full - 1
    assert count(p1, ("loadvec_q", "loadvec_q_small")) == count(full16, ("loadvec_q", "loadvec_q_small")) - 1
    assert count(p1, ("widen_box",)) == 1 and count(p1, ("outlier_table",)) == (1 if n16 else 0)
    for k in ("ipk_f", "ipk_c", "ipk_r", "ipk_fc"):
        assert count(p1, (k,)) <= count(full16, (k,))


def test_widened_box_is_the_stop_levels():
    """Launch counts cannot see the SIZE of the widened box. mgh_device_bytes can: the compact int64 box is the
    only thing the mixed 16-bit path allocates on a fresh handle, and it is counted. 129 x 130 x 257 f32: the full
    call widens the box of level L - 2, a stop at L - 4 must widen level L - 4's and nothing larger."""
    import torch
    import mgard_amd as mg
    shape = (129, 130, 257)
    u = torch.from_numpy(smooth_field(shape, np.float32)).cuda()
    h0 = mg.Hierarchy(shape, np.float32)
    L = h0.l_target
    assert h0.total >= 2 ** 18 and L >= 6
    sym, oi, ov, n, nrm = h0.decompose_quantize_sym16(u, mg.REL, 1e-3, np.inf)
    grown = {}
    for level in (L - 4, L - 3, L - 2, None):
        h = mg.Hierarchy(shape, np.float32)
        before = h.device_bytes()
        h.dequantize_recompose_sym16(sym, mg.REL, 1e-3, np.inf, nrm, outlier_idx=oi, outlier_val=ov, level=level)
        torch.cuda.synchronize()
        grown[level] = h.device_bytes() - before
        h.close()
    print(grown)
    for level in (L - 4, L - 3, L - 2):
        assert grown[level] == 8 * int(np.prod(h0.level_shape(level))), (level, grown)
    assert grown[None] == grown[L - 2]  # (L >= 4: the two finest levels stay on symbols)


def _profile_of(h, call):
    h.profile(True)
    call()
    prof = h.profile_read()
    h.profile(False)
    return {k: v[1] for k, v in prof.items() if v[1]}


@pytest.mark.parametrize("env, expect, absent", [
    ({"MGH_FORCE_V1": "1"}, ("box_dequantize", "gpk_rev"), ("recompose_head", "restore_q", "dequantize")),
    ({"MGH_NO_RECOMPOSE_HEAD": "1"}, ("head_in", "restore_q"), ("recompose_head", "box_dequantize")),
    ({"MGH_FORCE_ND": "1"}, ("box_dequantize", "nd_apply"), ("recompose_head", "restore_q", "dequantize")),
], ids=["force_v1", "no_head", "force_nd"])
def test_developer_switches_take_a_level(monkeypatch, env, expect, absent):
    """A fused-shaped 3-D array on the routes the switches select (read when the hierarchy is created): the
    one-thread-per-element kernels and the generic N-D kernels on a compact box, the fused loop without the head
    kernel. Every level against the oracle; the profile says which route ran."""
    import torch
    import mgard_amd as mg
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    S = Setup(((33, 40, 65), np.float32, dict(s=0.0), ""))
    h, o, L = S.h, S.o, S.L
    c = o.decompose(S.u)
    dc = torch.from_numpy(c).cuda()
    norm = float(np.float32(oracle.norm(S.u, 0.0, True)))
    q, oi, ov, n, _ = h.decompose_quantize(torch.from_numpy(S.u).cuda(), mg.REL, 1e-3, 0.0, norm, dict_size=64)
    v = o.dequantize(_cpu(q), oracle.REL, np.float32(1e-3), np.float32(0.0), np.float32(norm), 64, True,
                     outlier_idx=_cpu(oi).astype(np.uint64), outlier_val=_cpu(ov))
    for level in range(L + 1):
        assert_bit_equal(_cpu(h.recompose(dc, level=level)), expected_level(o, c, level), "recompose(level=%d)" % level)
        got = h.dequantize_recompose(q.clone(), mg.REL, 1e-3, 0.0, norm, dict_size=64, outlier_idx=oi,
                                     outlier_val=ov, level=level)
        assert_bit_equal(_cpu(got), expected_level(o, v, level), "dequantize_recompose(level=%d)" % level)
    prof = _profile_of(h, lambda: h.dequantize_recompose(q.clone(), mg.REL, 1e-3, 0.0, norm, dict_size=64,
                                                         outlier_idx=oi, outlier_val=ov, level=L - 1))
    print(prof)
    for k in expect:
        assert prof.get(k, 0) >= 1, (k, prof)
    for k in absent:
        assert prof.get(k, 0) == 0, (k, prof)


def test_box_paths_launch_one_box_kernel():
    """Thin 3-D (one-thread-per-element kernels) and 5-D (generic N-D): ONE box_dequantize / box_gather over the
    stop level's box, no full-size dequantize, and as many level passes as levels run."""
    import torch
    import mgard_amd as mg
    for shape, per_level in (((5000, 5, 7), "gpk_rev"), ((5, 6, 70, 9, 131), "nd_apply")):
        h = mg.Hierarchy(shape, np.float32)
        L = h.l_target
        u = torch.from_numpy(smooth_field(shape, np.float32)).cuda()
        q, oi, ov, n, nrm = h.decompose_quantize(u, mg.REL, 1e-3, np.inf)
        c = h.decompose(u)
        level = L - 1
        pq = _profile_of(h, lambda: h.dequantize_recompose(q.clone(), mg.REL, 1e-3, np.inf, nrm, outlier_idx=oi,
                                                           outlier_val=ov, level=level))
        pc = _profile_of(h, lambda: h.recompose(c, level=level))
        print(shape, pq, pc)
        assert pq.get("box_dequantize") == 1 and pq.get("dequantize", 0) == 0 and pq.get(per_level, 0) == level and level >= 1
        assert pc.get("box_gather") == 1 and pc.get("ld_pack", 0) == 0 and pc.get(per_level, 0) == level


LD_SHAPES = [
    ((33, 40, 65), "fused 3-D: stops inside the head and above it"),
    ((129, 66, 130), "fused 3-D, several levels of their own launches"),
    ((40, 130, 9), "fused 3-D, 64 x 4 tiles"),
    ((300, 5, 7), "thin 3-D: one-thread-per-element kernels on a gathered box"),
    ((100, 129), "2-D"),
    ((8, 34, 36, 65), "fused 4-D"),
    ((9, 8, 10, 17), "4-D generic N-D kernels on a gathered box"),
    ((3, 4, 5, 6, 7), "5-D generic"),
]


@pytest.mark.parametrize("pad_mid", [False, True])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [s for s, _ in LD_SHAPES], ids=["x".join(map(str, s)) for s, _ in LD_SHAPES])
def test_pitched_coefficients_with_a_level(shape, dt, pad_mid):
    """mgh_set_ld with a level, in the style of tests/test_gpu_ld.py: MGH_LD_IN is honoured for the coefficients
    (read in place with the pitched strides by the fused kernels, gathered by k_box_gather elsewhere), MGH_LD_OUT
    does not apply -- the output is dense at every level, l_target included. Bit-equal to the dense call; the
    pitched array (padding = NaN) is left as it was."""
    import torch
    import mgard_amd as mg
    from tests.test_gpu_ld import _ld, _pitched
    u = torch.from_numpy(smooth_field(shape, dt, noise=1e-3)).cuda()
    ld = _ld(shape, np.dtype(dt).itemsize, pad_mid)
    h = mg.Hierarchy(shape, dt)
    L = h.l_target
    coef = h.decompose(u)
    q, oi, ov, n, nrm = h.decompose_quantize(u, mg.REL, 1e-3, np.inf, dict_size=64)
    dense = [h.recompose(coef, level=level) for level in range(L + 1)]
    dense_q = [h.dequantize_recompose(q.clone(), mg.REL, 1e-3, np.inf, nrm, dict_size=64, outlier_idx=oi,
                                      outlier_val=ov, level=level) for level in range(L + 1)]
    assert_bit_equal(_cpu(dense[L]), _cpu(h.recompose(coef)), "dense, level = l_target")
    cp = _pitched(torch, coef, ld)
    cp0 = cp.clone()
    for ld_out in (None, ld):
        h.set_ld(mg.LD_IN, ld)
        h.set_ld(mg.LD_OUT, ld_out)
        for level in range(L + 1):
            got = h.recompose(cp, level=level)
            assert tuple(got.shape) == h.level_shape(level)
            assert_bit_equal(_cpu(got), _cpu(dense[level]), "pitched coefficients, level %d, LD_OUT %r" % (level, ld_out))
            # the integers are always dense; a pitched OUTPUT setting must not reach these calls
            gq = h.dequantize_recompose(q.clone(), mg.REL, 1e-3, np.inf, nrm, dict_size=64, outlier_idx=oi,
                                        outlier_val=ov, level=level)
            assert_bit_equal(_cpu(gq), _cpu(dense_q[level]), "integers, level %d, LD_OUT %r" % (level, ld_out))
        assert torch.equal(cp.isnan(), cp0.isnan())
        assert_bit_equal(_cpu(torch.nan_to_num(cp)), _cpu(torch.nan_to_num(cp0)), "the pitched coefficients")
    h.set_ld(mg.LD_IN, None)
    h.set_ld(mg.LD_OUT, None)
    assert_bit_equal(_cpu(h.recompose(coef)), _cpu(dense[L]), "the handle afterwards")


def test_raw_record_below_l_target():
    """A record that is stored RAW for certain: white noise at a tolerance far below it does not compress. At
    l_target the data comes back as it is; below, the level of the integers of the header's bound."""
    import torch
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    shape = (33, 34, 65)
    u = np.random.default_rng(5).standard_normal(shape).astype(np.float32)
    tol = 1e-7
    buf = hl.compress(u, tol, np.inf, mg.REL)
    meta = hl.metadata_parse(bytes(buf[:4096]))
    assert buf.size - meta["metadata_size"] - 8 == u.nbytes, "the record is not raw"
    h = mg.Hierarchy(shape, np.float32)
    L = h.l_target
    assert np.array_equal(hl.decompress(buf, level=L), u) and np.array_equal(hl.decompress(buf), u)
    q, oi, ov, n, _ = h.decompose_quantize(torch.from_numpy(u).cuda(), mg.REL, tol, np.inf, meta["norm"],
                                           prep_huffman=False)
    for level in range(L):
        want = h.dequantize_recompose(q.clone(), mg.REL, tol, np.inf, meta["norm"], prep_huffman=False, level=level)
        assert_bit_equal(hl.decompress(buf, level=level), _cpu(want), "raw record, level %d" % level)


HL_CASES = [
    ((129, 130, 257), np.float32, False),
    ((65, 70, 129), np.float64, True),
    ((3001,), np.float32, False),
    ((9, 8, 10, 17), np.float32, False),
    ((4, 3, 20, 5, 31), np.float64, False),
]


@pytest.mark.parametrize("device_stream", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("reorder", [0, 1])
@pytest.mark.parametrize("lossless", ["Huffman", "Huffman_Zstd"])
@pytest.mark.parametrize("case", HL_CASES, ids=lambda c: "x".join(map(str, c[0])) + "-" + np.dtype(c[1]).name)
def test_decompress_level(case, lossless, reorder, device_stream):
    import torch
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    shape, dt, nonuniform = case
    tol = 1e-3
    coords = nonuniform_coords(shape, dt, seed=sum(shape)) if nonuniform else None
    u = smooth_field(shape, dt)
    cfg = hl.Config(lossless=hl.HUFFMAN if lossless == "Huffman" else hl.HUFFMAN_ZSTD, reorder=reorder)
    du = torch.from_numpy(u).cuda()
    buf = hl.compress(du if device_stream else u, tol, np.inf, mg.REL, coords=coords, config=cfg)
    head = _cpu(buf[:65536]) if device_stream else buf[:65536]
    meta = hl.metadata_parse(bytes(head))
    norm = meta["norm"]
    h = mg.Hierarchy(shape, dt, coords=coords)
    o = oracle.Hierarchy(shape, dt, coords=coords)
    L = h.l_target
    assert hl.infer_level(buf, None, cfg) == (None, L)
    q, oi, ov, n, _ = h.decompose_quantize(du, mg.REL, tol, np.inf, norm, dict_size=int(cfg.huff_dict_size))
    c = o.decompose(u)
    bound = tol * norm
    # A record the lossless stage could not shrink holds the DATA (GPUPipelines.hpp:414-417). mgh_decompress
    # returns it as it is, so at level = l_target -- whose contract is "the bytes of mgh_decompress" -- there are
    # no integers to compare with; below l_target such a record goes through the integers of the header's bound.
    raw = buf.numel() if device_stream else buf.size
    raw = raw - meta["metadata_size"] - 8 == u.nbytes
    full = hl.decompress(buf, config=cfg)
    full = _cpu(full) if device_stream else full
    for level in range(L + 1):
        assert hl.infer_level(buf, level, cfg) == (h.level_shape(level), L)
        got = hl.decompress(buf, config=cfg, level=level)
        assert isinstance(got, torch.Tensor) == device_stream
        got = _cpu(got) if device_stream else got
        want = h.dequantize_recompose(q.clone(), mg.REL, tol, np.inf, norm, dict_size=int(cfg.huff_dict_size),
                                      outlier_idx=oi, outlier_val=ov, level=level)
        assert_bit_equal(got, full if (raw and level == L) else _cpu(want), "decompress(level=%d)" % level)
        err = float(np.max(np.abs(got.astype(np.float64) - expected_level(o, c, level).astype(np.float64))))
        print("level %d: error %.3e, bound %.3e" % (level, err, bound))
        assert err <= bound, (level, err, bound)
    top = hl.decompress(buf, config=cfg, level=L)
    assert_bit_equal(_cpu(top) if device_stream else top, full, "level = l_target")


def test_decompress_level_refuses_a_decomposed_container():
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    u = smooth_field((129, 64, 65), np.float32)
    cfg = hl.Config(domain_decomposition=hl.DD_MAXDIM, max_memory_footprint=30 * u.size)
    buf = hl.compress(u, 1e-3, np.inf, mg.REL, config=cfg)
    meta = hl.metadata_parse(bytes(buf[:4096]))
    assert meta["domain_decomposed"] is True
    with pytest.raises(mg.MgardHipError, match=r"error -1\b.*domain-decomposed"):
        hl.decompress(buf, config=cfg, level=1)
    v = hl.decompress(buf, config=cfg)  # the library is usable afterwards
    assert float(np.max(np.abs(v - u))) <= 1e-3 * float(np.max(np.abs(u)))
    plain = hl.compress(u, 1e-3, np.inf, mg.REL)
    assert hl.decompress(plain, level=0).shape == hl.infer_level(plain, 0)[0]
