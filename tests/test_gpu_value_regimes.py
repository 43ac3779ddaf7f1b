"""Value regimes the other GPU tests never reach (they feed fields of magnitude 1 with uniform noise).

A. Quantizer decision points -- rounding ties of both signs, the dictionary edges, -0.0, the
   neighbours of 2^31 where a 32-bit conversion saturates -- planted as finest-level coefficients
   (tests/test_value_regimes_cpu.py proves the construction) and sent through every kernel that
   quantizes: integers, outlier set and outlier count are the oracle's, and at the targets that are hit
   exactly also what the rule gives by hand.
B. The way back from integers built by hand: the first and last symbol of the dictionary, outlier
   values that an int64 -> float conversion has to round.
C. Exponent range: power-of-two scalings of the input give the scaled result bit for bit (no absolute
   constant anywhere), and subnormal inputs and intermediates give what IEEE arithmetic gives.

The shapes are the smallest that select the kernel named (tests/test_gpu_reference_binary.py's CASES,
DESIGN.md's kernel table); none had to be replaced.
"""
import itertools

import numpy as np
import pytest

import oracle
from oracle import ref
from tests.test_gpu_reference_binary import CASES as REF_CASES
from tests.test_multires_cpu import expected_level
from tests.util import (level_volume, nonuniform_coords, planted_field, quantizer_targets, reordered_position,
                        rule_integer, smooth_field, solve_targets)

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not ref.available(), reason="%s is not built (oracle.build_ref())" % ref.LIB_PATH)

ABS = oracle.ABS
TOL = 1e-3
DICTS = (64, 8192, 65536)
DTS = [np.float32, np.float64]
INF = float("inf")


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


def _outliers(idx, val):
    idx, val = np.asarray(idx).astype(np.int64), np.asarray(val).astype(np.int64)
    order = np.argsort(idx, kind="stable")
    return list(zip(idx[order].tolist(), val[order].tolist()))


def _sid(shape):
    return "x".join(map(str, shape))


def _all_targets(dt):
    """The targets of the three dictionaries in one list (the small ones of 64 are among k = 0 .. 39)."""
    t = np.concatenate([quantizer_targets(dt, d) for d in DICTS])
    _, first = np.unique(_bits(t), return_index=True)
    return t[np.sort(first)]


def _level_map(o):
    """Level of every element of the reordered layout (the maximum of the per-dimension marks)."""
    D = len(o.shape)
    lev = np.zeros(o.shape, dtype=np.int8)
    for d in range(D):
        m = o.marks(d).astype(np.int8).reshape([-1 if k == d else 1 for k in range(D)])
        lev = np.maximum(lev, m)
    return lev


def _check_quantized(what, q, oi, ov, n, want, hand, dict_size):
    """Against the oracle's (integers, sorted outliers, count) and the hand-computed integers."""
    rq, rout, rn = want
    assert n == rn, (what, "outlier count", n, rn)
    q = (q if isinstance(q, np.ndarray) else _cpu(q)).astype(np.int64)
    assert np.array_equal(q, rq), "%s: %d integers differ from the oracle's" % (what, int(np.sum(q != rq)))
    got = _outliers(_cpu(oi), _cpu(ov))
    assert got == rout, "%s: outlier sets differ" % what
    outl = dict(got)
    flat = q.reshape(-1)
    for lin, target in hand:
        w, out = rule_integer(target, target.dtype, dict_size)
        if out:
            assert flat[lin] == 0 and outl.get(lin) == w, (what, target, w, flat[lin], outl.get(lin))
        else:
            assert flat[lin] == w and lin not in outl, (what, target, w, flat[lin])


# ---------------------------------------------------------------------------------------------------
# A. planted decision points
# ---------------------------------------------------------------------------------------------------
class Planted:
    """Input and expected output of one (shape, dtype, s): 1e-6 * smooth_field at the nodes with an odd
    index (the nodes with even indices only -- and the last node of an even extent, which is a coarse
    node too -- stay 0), one run of values that leave every dictionary (more than 64 in a row of the
    fastest dimension: a wave full of outliers), and every target at a seeded place of its own (lone
    outliers among small values)."""

    def __init__(self, shape, dt, s):
        self.shape, self.dt, self.s = shape, dt, s
        D = len(shape)
        o = self.o = oracle.Hierarchy(shape, dt)
        L = o.l_target
        self.qargs = (ABS, dt(TOL), dt(s), dt(1))
        qz = o.quantizers(*self.qargs, reciprocal=True)[L]
        vol = dt(1) if np.isinf(s) else level_volume(shape, dt)
        targets = _all_targets(dt)
        vals, hit = solve_targets(dt, targets, qz, vol)
        # (consecutive c move the product by 0.5 to 2 ulp of the target, so between every and every second
        # target has a c that hits it; a third of them keeps the hand-computed check from being empty)
        assert 3 * hit.sum() >= len(targets), (hit.sum(), len(targets))
        fine = [(np.arange(n) % 2 == 1) & (np.arange(n) < n - 1) for n in shape]
        mask = np.zeros(shape, dtype=bool)
        for d in range(D):
            mask |= fine[d].reshape([-1 if k == d else 1 for k in range(D)])
        u = np.where(mask, dt(1e-6) * smooth_field(shape, dt), dt(0)).astype(dt)
        big = solve_targets(dt, [40000.0], qz, vol)[0][0]  # outside the largest dictionary
        if D == 1:
            u[1001:1001 + 2 * 200:2] = big
        else:
            # (whole rows of the planes 1, 3, ...: next to each other in the reordered layout as well)
            rest = [range(1, shape[0] - 2, 2)] + [range(n - 2 if n % 2 == 0 else n) for n in shape[1:]]
            run = list(itertools.islice(itertools.product(*rest), max(300, 3 * shape[-1])))
            assert len(run) > 64
            u[tuple(np.array(run).T)] = big
        planted, pos = planted_field(shape, dt, vals, seed=sum(shape) + D)
        u[tuple(pos.T)] = vals
        self.u = np.ascontiguousarray(u)
        c = o.decompose(self.u)
        at = reordered_position(pos, shape, o.level_shape(L - 1))
        assert np.array_equal(_bits(c[tuple(at.T)]), _bits(vals)), "the construction does not hold here"
        lin = np.ravel_multi_index(tuple(at.T), shape)
        self.hand = [(int(lin[k]), targets[k]) for k in np.flatnonzero(hit)]
        self._other = {None: (o, c)}
        self._want = {}

    def want(self, dict_size, prep=True, cls=None):
        key = (dict_size, prep, cls)
        if key not in self._want:
            if cls not in self._other:
                other = cls(self.shape, self.dt)
                self._other[cls] = (other, other.decompose(self.u))
            o, c = self._other[cls]
            q, oi, ov, n = o.quantize(c, *self.qargs, dict_size=dict_size, prep_huffman=prep)
            self._want[key] = (q, _outliers(oi, ov), n)
        return self._want[key]


_planted = {}


def _planted_case(shape, dt, s):
    """One entry at a time (the parameters below keep the cases of one entry together)."""
    key = (shape, np.dtype(dt).name, s)
    if key not in _planted:
        _planted.clear()
        _planted[key] = Planted(shape, dt, s)
    return _planted[key]


F3, F4 = (65, 70, 129), (8, 66, 70, 129)
# (shape, switches, the kernels the case is there for)
PATHS = [
    (F3, {}, "fused 3-D level kernel, 8 x 32 tiles"),
    (F3, {"MGH_BOX": "0"}, "no box kernel: every level marches"),
    (F3, {"MGH_BOX": "2"}, "box kernel up to the long-march class"),
    (F3, {"MGH_BOX": "3", "MGH_TAIL_SOLVES": "0"}, "box kernel on every level, tail without the solves above it"),
    (F3, {"MGH_OUTLIER_AGG": "0"}, "outlier slots per wave and plane"),
    (F3, {"MGH_OUTLIER_AGG": "1"}, "outlier slots per workgroup from the LDS stash"),
    (F3, {"MGH_FORCE_V1": "1"}, "one-thread-per-element kernels"),
    ((40, 130, 9), {}, "fused 3-D, 64 x 4 tiles"),
    ((17, 17, 17), {}, "all levels in LDS: k_tail and k_head_out"),
    (F4, {}, "fused 4-D slice path"),
    (F4, {"MGH_FUSED4": "0", "MGH_ND_ROWS": "1"}, "generic N-D row kernels"),
    (F4, {"MGH_FUSED4": "0", "MGH_ND_ROWS": "0"}, "generic N-D kernels, one thread per element"),
    ((4, 3, 70, 5, 131), {}, "D = 5"),
    ((257, 130), {}, "D = 2"),
    ((300001,), {}, "D = 1"),
    ((5000, 5, 7), {}, "thin array: the simple kernels chosen by the hierarchy"),
]


def _path_params():
    shapes = []
    for shape, _, _ in PATHS:
        if shape not in shapes:
            shapes.append(shape)
    out = []
    for shape in shapes:
        for dt in DTS:
            for s in (INF, 0.0):
                for sh, env, _ in PATHS:
                    if sh == shape:
                        sw = ",".join("%s=%s" % (k[4:], v) for k, v in env.items()) or "default"
                        out.append(pytest.param(shape, dt, s, env,
                                                id="%s-%s-s%s-%s" % (_sid(shape), np.dtype(dt).name, s, sw)))
    return out


@pytest.mark.parametrize("shape,dt,s,env", _path_params())
def test_planted_decision_points_through_decompose_quantize(shape, dt, s, env, monkeypatch):
    """Every dictionary size with the dictionary shift, and prep_huffman = False: there the level kernel
    converts in 32 bits and redoes a whole wave in 64 bits when one value saturates -- the targets at and
    beyond 2^31 sit among small values."""
    import torch
    import mgard_amd as mg
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    P = _planted_case(shape, dt, s)
    h = mg.Hierarchy(shape, dt)
    du = torch.from_numpy(P.u).cuda()
    for d in DICTS:
        q, oi, ov, n, _ = h.decompose_quantize(du, mg.ABS, TOL, s, 1.0, dict_size=d)
        _check_quantized("dict_size %d" % d, q, oi, ov, n, P.want(d), P.hand, d)
    q, oi, ov, n, _ = h.decompose_quantize(du, mg.ABS, TOL, s, 1.0, prep_huffman=False)
    rq = P.want(8192, False)[0]
    assert n == 0 and np.array_equal(_cpu(q), rq), "prep_huffman = False: %d integers differ" % int(
        np.sum(_cpu(q) != rq))
    flat = _cpu(q).reshape(-1)
    for lin, target in P.hand:
        assert flat[lin] == rule_integer(target, dt, 0)[0], ("prep_huffman = False", target, flat[lin])
    h.close()


@pytest.mark.parametrize("mixed", ["1", "0"])
@pytest.mark.parametrize("s", [INF, 0.0])
@pytest.mark.parametrize("dt", DTS, ids=["float32", "float64"])
@pytest.mark.parametrize("shape", [F3, F4], ids=_sid)
def test_planted_decision_points_through_sym16(shape, dt, s, mixed, monkeypatch):
    """The (uint16_t) narrowing: symbol dict - 1 = 65535 and symbol 0 come out as they are."""
    import torch
    import mgard_amd as mg
    monkeypatch.setenv("MGH_SYM16_MIXED", mixed)
    P = _planted_case(shape, dt, s)
    h = mg.Hierarchy(shape, dt)
    assert h.sym16_supported()
    du = torch.from_numpy(P.u).cuda()
    for d in (65536, 64):
        sym, oi, ov, n, _ = h.decompose_quantize_sym16(du, mg.ABS, TOL, s, 1.0, dict_size=d)
        assert sym.dtype == torch.uint16
        _check_quantized("sym16, dict_size %d" % d, sym.view(torch.int16).cpu().numpy().view(np.uint16), oi, ov, n,
                         P.want(d), P.hand, d)
    h.close()


@needs_ref
@pytest.mark.parametrize("s", [INF, 0.0])
@pytest.mark.parametrize("dt", DTS, ids=["float32", "float64"])
@pytest.mark.parametrize("shape", [F3, F4, (4, 3, 70, 5, 131)], ids=_sid)
def test_planted_decision_points_against_the_reference_build(shape, dt, s):
    import torch
    import mgard_amd as mg
    P = _planted_case(shape, dt, s)
    h = mg.Hierarchy(shape, dt)
    du = torch.from_numpy(P.u).cuda()
    for d in DICTS:
        q, oi, ov, n, _ = h.decompose_quantize(du, mg.ABS, TOL, s, 1.0, dict_size=d)
        _check_quantized("reference, dict_size %d" % d, q, oi, ov, n, P.want(d, cls=ref.Hierarchy), P.hand, d)
    h.close()


@pytest.mark.parametrize("s", [INF, 0.0])
@pytest.mark.parametrize("dt", DTS, ids=["float32", "float64"])
@pytest.mark.parametrize("shape", [(17, 17, 17), (33, 40, 36), (9, 10, 17, 12), (3, 4, 5, 6, 7), (300,), (33, 20)],
                         ids=_sid)
def test_planted_decision_points_on_every_level_through_staged_quantize(shape, dt, s):
    """mgh_quantize on a coefficient array of the test's own: the quantizer (and with s = 0 the volume)
    differs per level, so the targets are solved per level -- level 0 and the coarse levels included,
    which the fused construction cannot control."""
    import torch
    import mgard_amd as mg
    o = oracle.Hierarchy(shape, dt)
    L = o.l_target
    qargs = (ABS, dt(TOL), dt(s), dt(1))
    qzs = o.quantizers(*qargs, reciprocal=True)
    lev = _level_map(o).reshape(-1)
    rng = np.random.default_rng(sum(shape))
    c = (1e-5 * rng.standard_normal(lev.size)).astype(dt)
    targets = _all_targets(dt)
    hand = []
    for l in range(L + 1):
        sites = np.flatnonzero(lev == l)
        k = min(len(sites), len(targets))
        t = targets[rng.permutation(len(targets))[:k]]
        at = rng.choice(sites, size=k, replace=False)
        vol = dt(1) if np.isinf(s) else level_volume(o.level_shape(l), dt)
        vals, hit = solve_targets(dt, t, qzs[l], vol)
        c[at] = vals
        hand += [(int(at[j]), t[j]) for j in np.flatnonzero(hit)]
    assert 3 * len(hand) >= min(lev.size, (L + 1) * len(targets)) // 2, len(hand)
    c = c.reshape(shape)
    h = mg.Hierarchy(shape, dt)
    dc = torch.from_numpy(c).cuda()
    for d in DICTS:
        rq, roi, rov, rn = o.quantize(c, *qargs, dict_size=d)
        q, oi, ov, n = h.quantize(dc, mg.ABS, TOL, s, 1.0, dict_size=d)
        _check_quantized("quantize, dict_size %d" % d, q, oi, ov, n, (rq, _outliers(roi, rov), rn), hand, d)
    rq = o.quantize(c, *qargs, prep_huffman=False)[0]
    q, oi, ov, n = h.quantize(dc, mg.ABS, TOL, s, 1.0, prep_huffman=False)
    assert n == 0 and np.array_equal(_cpu(q), rq)
    h.close()


# ---------------------------------------------------------------------------------------------------
# B. dequantize edges
# ---------------------------------------------------------------------------------------------------
OUTLIER_EDGES = [2 ** 24 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 53 + 1]


def _hand_made_integers(o, dict_size, seed):
    """(q, outlier_idx, outlier_val): symbols near the middle of the dictionary; on every level the symbols
    0, 1, half - 1, half, half + 1, dict - 1; on levels 0, l_target / 2 and l_target the outlier values
    +-x and +-x + half (the integer that is converted is the value less half) for x in OUTLIER_EDGES,
    with 0 in their place as the quantizer leaves it."""
    rng = np.random.default_rng(seed)
    half, L = dict_size // 2, o.l_target
    lev = _level_map(o).reshape(-1)
    q = rng.integers(max(0, half - 20), min(dict_size, half + 20), size=lev.size).astype(np.int64)
    edges = [0, 1, half - 1, half, half + 1, dict_size - 1]
    vals = [sgn * x + add for x in OUTLIER_EDGES for sgn in (1, -1) for add in (0, half)]
    oi, ov = [], []
    for l in range(L + 1):
        sites = rng.permutation(np.flatnonzero(lev == l))
        reps = max(1, min(4, len(sites) // (2 * len(edges))))
        k = min(len(sites), reps * len(edges))
        q[sites[:k]] = (edges * reps)[:k]
        if l in (0, L // 2, L):
            free = sites[k:k + len(vals)]
            q[free] = 0
            oi += free.tolist()
            ov += vals[:len(free)]
    assert len(oi) >= len(vals)
    return q.reshape(o.shape), np.array(oi, dtype=np.uint64), np.array(ov, dtype=np.int64)


@pytest.mark.parametrize("s", [INF, 0.0])
@pytest.mark.parametrize("dt", DTS, ids=["float32", "float64"])
@pytest.mark.parametrize("shape", [(17, 17, 17), F3, F4, (3, 4, 5, 6, 7)], ids=_sid)
def test_dequantize_edges(shape, dt, s):
    import torch
    import mgard_amd as mg
    o = oracle.Hierarchy(shape, dt)
    h = mg.Hierarchy(shape, dt)
    L = o.l_target
    Lc = L // 2
    qargs = (ABS, dt(TOL), dt(s), dt(1))
    gargs = (mg.ABS, TOL, s, 1.0)
    for d in DICTS:
        q, oi, ov = _hand_made_integers(o, d, seed=d + len(shape))
        v = o.dequantize(q, *qargs, dict_size=d, outlier_idx=oi, outlier_val=ov)
        full = o.recompose(v)
        dq = torch.from_numpy(q).cuda()
        kw = dict(dict_size=d, outlier_idx=torch.from_numpy(oi.astype(np.int64)).cuda(),
                  outlier_val=torch.from_numpy(ov).cuda())
        assert_bit_equal(_cpu(h.dequantize(dq.clone(), *gargs, **kw)), v, "dequantize, dict_size %d" % d)
        assert_bit_equal(_cpu(h.dequantize_recompose(dq.clone(), *gargs, **kw)), full,
                         "dequantize_recompose, dict_size %d" % d)
        coarse = expected_level(o, v, Lc)
        assert_bit_equal(_cpu(h.dequantize_recompose(dq.clone(), *gargs, level=Lc, **kw)), coarse,
                         "dequantize_recompose(level=%d), dict_size %d" % (Lc, d))
        if h.sym16_supported():
            assert q.min() == 0 and q.max() == d - 1
            sym = torch.from_numpy(q.astype(np.uint16).view(np.int16)).cuda().view(torch.uint16)
            assert_bit_equal(_cpu(h.dequantize_recompose_sym16(sym, *gargs, **kw)), full,
                             "dequantize_recompose_sym16, dict_size %d" % d)
            assert_bit_equal(_cpu(h.dequantize_recompose_sym16(sym, *gargs, level=Lc, **kw)), coarse,
                             "dequantize_recompose_sym16(level=%d), dict_size %d" % (Lc, d))
    h.close()


def test_dequantize_edges_run_the_sym16_way_back():
    import mgard_amd as mg
    for shape in ((17, 17, 17), F3, F4):
        assert mg.Hierarchy(shape, np.float32).sym16_supported()


# ---------------------------------------------------------------------------------------------------
# C. exponent range
# ---------------------------------------------------------------------------------------------------
NORMAL_E = {np.float32: (-100, -60, 100), np.float64: (-900, 900)}
# The exponents at which the scaled run must ALSO be the unscaled run scaled. Not float32 at e = -100:
# there the sweeps' products (values of 2^-107 times mesh widths squared) fall below 2^-126 and round
# on the subnormal grid, so plain IEEE arithmetic itself does not scale -- the CPU oracle differs from
# its own unscaled result in thousands of elements on (5000, 5, 7), (8, 66, 70, 129),
# (4, 3, 70, 5, 131), (300001,) and (129, 129, 257), and in none at e = -80 or -60. float64 at
# e = -900 keeps 122 binades above its smallest normal number, float32 at e = -100 only 26.
SCALING_E = {np.float32: (-60, 100), np.float64: (-900, 900)}
SUBNORMAL_E = {np.float32: -140, np.float64: -1060}
RANGE_CASES = [(c[0], c[1], c[2], {}) for c in REF_CASES if c[0] != (1025, 130, 257)] + [
    ((300001,), np.float32, dict(), {"MGH_IPK_SPEC_K": "2"}),
    ((129, 129, 257), np.float32, dict(), {"MGH_IPK_CHUNK_K": "3"}),
]
RANGE_IDS = ["%s-%s%s" % (_sid(c[0]), np.dtype(c[1]).name, "".join("-%s=%s" % (k[4:], v) for k, v in c[3].items()))
             for c in RANGE_CASES]


class Grid:
    def __init__(self, case, monkeypatch):
        import mgard_amd as mg
        shape, dt, opt, env = case
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        coords = nonuniform_coords(shape, dt, seed=sum(shape)) if opt.get("coords") else None
        normalize = opt.get("normalize", True)
        ml = opt.get("max_level")
        if ml == "top-1":
            ml = oracle.Hierarchy(shape, dt).l_target - 1
        self.o = oracle.Hierarchy(shape, dt, coords=coords, normalize_coordinates=normalize,
                                  **({} if ml is None else dict(max_level=ml)))
        self.h = mg.Hierarchy(shape, dt, coords=coords, normalize_coordinates=normalize, max_level=ml)
        assert self.h.l_target == self.o.l_target
        self.shape, self.dt, self.opt = shape, dt, opt
        self.u = smooth_field(shape, dt, seed=int(np.prod(shape)) % 100003, noise=1e-2)


@pytest.mark.parametrize("case", RANGE_CASES, ids=RANGE_IDS)
def test_power_of_two_scaling_in_the_normal_range(case, monkeypatch):
    """decompose(u 2^e) = the oracle's on the same input, e = -100, -60, +100 (float32), +-900 (float64), and
    = decompose(u) 2^e at the exponents of SCALING_E; the same for recompose. With an ABS bound of
    1e-3 2^e the integers are the oracle's and (SCALING_E) those of the unscaled run."""
    import torch
    import mgard_amd as mg
    G = Grid(case, monkeypatch)
    h, o, dt, u = G.h, G.o, G.dt, G.u
    dict_size, prep = G.opt.get("dict_size", 8192), G.opt.get("prep_huffman", True)
    c0 = _cpu(h.decompose(torch.from_numpy(u).cuda()))
    assert_bit_equal(c0, o.decompose(u), "decompose")
    r0 = _cpu(h.recompose(torch.from_numpy(c0).cuda()))
    q0, oi0, ov0, n0, _ = h.decompose_quantize(torch.from_numpy(u).cuda(), mg.ABS, TOL, INF, 1.0,
                                               dict_size=dict_size, prep_huffman=prep)
    q0, out0 = _cpu(q0), _outliers(_cpu(oi0), _cpu(ov0))
    for e in NORMAL_E[dt]:
        scales = e in SCALING_E[dt]
        ue = np.ldexp(u, e)
        ce = o.decompose(ue)
        assert np.all(np.isfinite(ce))
        got = _cpu(h.decompose(torch.from_numpy(ue).cuda()))
        assert_bit_equal(got, ce, "decompose, e = %d, against the oracle" % e)
        if scales:
            assert_bit_equal(got, np.ldexp(c0, e), "decompose, e = %d, against the unscaled run" % e)
        back = _cpu(h.recompose(torch.from_numpy(ce).cuda()))
        assert_bit_equal(back, o.recompose(ce), "recompose, e = %d, against the oracle" % e)
        if scales:
            assert_bit_equal(back, np.ldexp(r0, e), "recompose, e = %d, against the unscaled run" % e)
        tol = float(np.ldexp(TOL, e))
        qz = o.quantizers(ABS, dt(tol), dt(INF), dt(1), reciprocal=True)
        assert np.all(np.isfinite(qz)) and np.all(qz != 0), (e, qz)
        rq, roi, rov, rn = o.quantize(ce, ABS, dt(tol), dt(INF), dt(1), dict_size=dict_size, prep_huffman=prep)
        q, oi, ov, n, _ = h.decompose_quantize(torch.from_numpy(ue).cuda(), mg.ABS, tol, INF, 1.0,
                                               dict_size=dict_size, prep_huffman=prep)
        assert n == rn, (e, n, rn)
        assert np.array_equal(_cpu(q), rq), "e = %d: integers differ from the oracle's" % e
        assert _outliers(_cpu(oi), _cpu(ov)) == _outliers(roi, rov), "e = %d: outliers" % e
        if scales:
            assert n == n0 and np.array_equal(_cpu(q), q0), "e = %d: integers differ from the unscaled run's" % e
            assert _outliers(_cpu(oi), _cpu(ov)) == out0, "e = %d: outliers of the unscaled run" % e
    h.close()


@pytest.mark.parametrize("case", RANGE_CASES, ids=RANGE_IDS)
def test_subnormal_inputs_and_intermediates(case, monkeypatch):
    """u 2^-140 (float32) / u 2^-1060 (float64): IEEE gradual underflow in every sweep, compared with the
    oracle on the same input, which (checked first) holds subnormals, no NaN and few exact zeros."""
    import torch
    G = Grid(case, monkeypatch)
    h, o, dt = G.h, G.o, G.dt
    ue = np.ldexp(G.u, SUBNORMAL_E[dt])
    ce = o.decompose(ue)
    re = o.recompose(ce)
    tiny = np.finfo(dt).tiny
    for a in (ue, ce, re):
        assert not np.any(np.isnan(a))
        assert np.any((a != 0) & (np.abs(a) < tiny)), "no subnormal values"
        assert np.mean(a == 0) < 0.10, "%.1f %% exact zeros" % (100 * np.mean(a == 0))
    assert_bit_equal(_cpu(h.decompose(torch.from_numpy(ue).cuda())), ce, "decompose of subnormal input")
    assert_bit_equal(_cpu(h.recompose(torch.from_numpy(ce).cuda())), re, "recompose of subnormal coefficients")
    h.close()
