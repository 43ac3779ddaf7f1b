"""Every entry point with a `void *stream` on a busy NON-DEFAULT stream (tests/stream_order.py): the inputs are
still being produced on the stream when the call is made and are overwritten on it right behind the call, with
no host synchronisation in between. Expected values are the CPU oracle's (oracle.Hierarchy), tests/payload.py's
and tests/mask_model.py's, bit for bit; nothing is compared with a second run of the library.

CASE_TABLE is module-level data (importable without torch): tests/test_stream_cases_cpu.py holds it against the
two public headers, so an entry point with a stream parameter cannot be added without a row here.

The fused 4-D route runs (8, 66, 70, 129) float32, 4.8 M elements."""
import ctypes as C

import numpy as np
import pytest

import oracle
from tests import mask_model as mm
from tests import payload as pl
from tests import stream_order as so
from tests.compare_ref import assert_stats, ref_stats
from tests.ipk_stream_cases import CASES as IPK_CASES
from tests.test_gpu_parity import _outlier_set, assert_bit_equal
from tests.test_multires_cpu import expected_level
from tests.test_prolong_cpu import zeroed
from tests.util import huffman_symbols, nonuniform_coords, smooth_field

pytestmark = pytest.mark.gpu

INF = float("inf")
TOL, DICT = 1e-3, 8192
_IPK = {c["id"]: c for c in IPK_CASES}["f64-lds0"]

# route: (shape, dtype, non-uniform coordinates, environment)
ROUTES = {
    "1d": ((1025,), np.float32, False, {}),
    "2d": ((129, 33), np.float64, False, {}),
    "fused3": ((65, 70, 129), np.float32, False, {}),
    "fused3-nonuniform": ((34, 33, 32), np.float64, True, {}),
    "box": ((5, 5, 5), np.float32, False, {}),
    "thin": ((5000, 5, 7), np.float32, False, {}),
    "ipk-stream": (_IPK["shape"], np.float64, _IPK["nonuniform"], _IPK["env"]),
    # (the r-solve of the top level, 201 x 16 x 26, is a k_ipk_dma launch: test_the_ipk_dma_route_launches_k_ipk_dma)
    "ipk-dma": ((400, 30, 50), np.float32, False, {"MGH_IPK_DMA_MIN": "0"}),
    "fused4": ((8, 66, 70, 129), np.float32, False, {}),
    "nd5": ((3, 4, 5, 6, 7), np.float64, False, {}),
}
# (shapes of test_two_hierarchies_on_two_streams)
TWO = {"two-a": ((65, 70, 129), np.float32, False, {}), "two-b": ((66, 131, 260), np.float64, False, {})}
ALL = tuple(ROUTES)
F3 = ("fused3",)
SYM16 = ("1d", "fused3", "fused4")
NOH = ("fused3",)  # (calls without a hierarchy: the fused 3-D route's arrays)

# (case function, entry points it drives, routes)
CASE_TABLE = [
    ("norm", ("mgh_norm",), ALL),
    ("decompose", ("mgh_decompose",), ALL),
    ("recompose", ("mgh_recompose",), ALL),
    ("quantize", ("mgh_quantize",), ALL),
    ("dequantize", ("mgh_dequantize",), ALL),
    ("decompose_quantize", ("mgh_decompose_quantize",), ALL),
    ("dequantize_recompose", ("mgh_dequantize_recompose",), ALL),
    ("decompose_quantize_sym16", ("mgh_decompose_quantize_sym16",), SYM16),
    ("dequantize_recompose_sym16", ("mgh_dequantize_recompose_sym16",), SYM16),
    ("norm_device", ("mgh_norm_device",), F3),
    ("decompose_quantize_dn", ("mgh_decompose_quantize_dn",), F3),
    ("norm_stream", ("mgh_norm_stream_begin", "mgh_norm_stream_add", "mgh_norm_stream_end"), F3),
    ("quantize_histograms", ("mgh_quantize_histograms",), F3),
    ("quantize_roundtrip", ("mgh_quantize_roundtrip",), F3),
    ("quantize_symbols", ("mgh_quantize_symbols",), F3),
    ("quantize_symbols_residual", ("mgh_quantize_symbols_residual",), F3),
    ("dequantize_add", ("mgh_dequantize_add",), F3),
    ("recompose_to_level", ("mgh_recompose_to_level",), F3),
    ("dequantize_recompose_to_level", ("mgh_dequantize_recompose_to_level",), F3),
    ("dequantize_recompose_sym16_to_level", ("mgh_dequantize_recompose_sym16_to_level",), F3),
    ("level_linearize", ("mgh_level_linearize",), F3),
    ("level_box_from_linear", ("mgh_level_box_from_linear",), F3),
    ("dequantize_recompose_linear_to_level", ("mgh_dequantize_recompose_linear_to_level",), F3),
    ("refine_level", ("mgh_refine_level",), F3),
    # (mgard_hip.h: "Every other shape ..." runs the level loops of mgh_recompose instead of the kernel)
    ("prolong", ("mgh_prolong",), ("fused3", "2d")),
    ("prolong_window", ("mgh_prolong_window",), ("fused3", "2d")),
    ("prolong_window_strided", ("mgh_prolong_window_strided",), ("fused3", "thin")),
    ("outlier_restore", ("mgh_outlier_restore",), NOH),
    ("mask_scan", ("mgh_mask_scan",), NOH),
    ("mask_fill", ("mgh_mask_fill",), NOH),
    ("mask_restore", ("mgh_mask_restore",), NOH),
    ("compare", ("mgh_compare",), NOH),
    ("histogram_sym16", ("mgh_histogram_sym16",), NOH),
    ("lossless_compress", ("mgh_lossless_compress", "mgh_lossless_compress_sym16"), NOH),
    ("lossless_compress_device", ("mgh_lossless_compress_device", "mgh_lossless_compress_device_sym16"), NOH),
    ("lossless_decompress", ("mgh_lossless_decompress", "mgh_lossless_decompress_prefix",
                             "mgh_lossless_decompress_range", "mgh_lossless_decompress_sym16"), NOH),
]
PAIRS = [(name, route) for name, _, routes in CASE_TABLE for route in routes]


def _gpu():
    import torch
    import mgard_amd
    return torch, mgard_amd


# ---- the oracle's side: computed once per route, shared, never written to -----------------------------------
class Ref:
    def __init__(self, route):
        shape, dt, nonuniform, env = ROUTES[route] if route in ROUTES else TWO[route]
        self.shape, self.dt, self.env = shape, dt, env
        self.coords = nonuniform_coords(shape, dt, seed=sum(shape)) if nonuniform else None
        self.o = oracle.Hierarchy(shape, dt, coords=self.coords)
        self.N = int(np.prod(shape))
        self._memo = {}

    def get(self, key, make):
        if key not in self._memo:
            v = make()
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._memo[key] = v
        return self._memo[key]

    # which = "u" (the real array) or "p" (poison: another seeded smooth field)
    def field(self, which):
        seed, noise = (20260101, 3e-3) if which == "u" else (777, 2e-2)
        return self.get(("field", which), lambda: smooth_field(self.shape, self.dt, seed=seed, noise=noise))

    def norm(self, which):
        return self.get(("norm", which), lambda: float(oracle.norm(self.field(which), self.dt(INF))))

    def coef(self, which):
        return self.get(("coef", which), lambda: self.o.decompose(self.field(which)))

    def back(self, which):
        return self.get(("back", which), lambda: self.o.recompose(self.coef(which)))

    def quant(self, which, eb=oracle.REL, tol=TOL, s=INF, norm=None, dict_size=DICT):
        """(q, outlier idx as int64, outlier val, count) of the oracle's quantizer."""
        dt = self.dt
        nrm = self.norm(which) if norm is None else norm

        def make():
            q, oi, ov, n = self.o.quantize(self.coef(which), eb, dt(tol), dt(s), dt(nrm), dict_size=dict_size,
                                           outlier_cap=self.N)
            return q, oi.astype(np.int64), ov, n
        return self.get(("quant", which, eb, tol, s, nrm, dict_size), make)

    def deq(self, which, eb=oracle.REL, tol=TOL, s=INF, norm=None, dict_size=DICT):
        dt = self.dt
        nrm = self.norm(which) if norm is None else norm

        def make():
            q, oi, ov, _ = self.quant(which, eb, tol, s, nrm, dict_size)
            return self.o.dequantize(q, eb, dt(tol), dt(s), dt(nrm), dict_size=dict_size, outlier_idx=oi.astype(np.uint64),
                                     outlier_val=ov)
        return self.get(("deq", which, eb, tol, s, nrm, dict_size), make)

    def rback(self, which, **kw):
        return self.get(("rback", which, tuple(sorted(kw.items()))), lambda: self.o.recompose(self.deq(which, **kw)))

    def other_list(self, k):
        """A valid outlier list of exactly k entries that is not the real one: distinct positions, small values."""
        def make():
            rng = np.random.default_rng(5)
            return rng.permutation(self.N)[:k].astype(np.int64), rng.integers(-3000, 3000, k).astype(np.int64)
        return self.get(("other", k), make)

    def qinputs(self, **kw):
        """(real, poison) of (q, outlier idx, outlier val): the poison integers are the other array's, its list
        cut or replaced to the real list's length."""
        q, oi, ov, _ = self.quant("u", **kw)
        pq = self.quant("p", **kw)[0]
        poi, pov = self.other_list(len(oi))
        return [q, oi, ov], [pq, poi, pov]

    # ---- level-linearised side
    def linear(self, which):
        return self.get(("lin", which), lambda: self.o.level_linearize(self.quant(which)[0]))

    def linear_pos(self):
        """Position in the level-linearised array of every position of the reordered one."""
        def make():
            src = self.o.level_linearize(np.arange(self.N, dtype=np.int64))
            pos = np.empty(self.N, dtype=np.int64)
            pos[src] = np.arange(self.N, dtype=np.int64)
            return pos
        return self.get("linpos", make)

    def level_count(self, level):
        return int(np.prod(self.o.level_shape(level)))

    def level_values(self, which, level, of="deq"):
        src = self.deq(which) if of == "deq" else self.coef(which)
        return self.get(("level", which, level, of), lambda: expected_level(self.o, src, level))


_REFS = {}


def ref_of(route):
    if route not in _REFS:
        _REFS[route] = Ref(route)
    return _REFS[route]


class Ctx:
    """One case on one route: the oracle's side, a hierarchy and the stream."""

    def __init__(self, route, stream, monkeypatch, hierarchy=True):
        self.torch, self.mg = _gpu()
        self.route, self.R, self.stream = route, ref_of(route), stream
        for k, v in self.R.env.items():
            monkeypatch.setenv(k, v)
        self.h = self.mg.Hierarchy(self.R.shape, self.R.dt, coords=self.R.coords) if hierarchy else None

    def dev(self, a):
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        return self.torch.from_numpy(a.copy()).cuda()

    def run(self, real, poison, call, ms=20):
        return so.run_ordered(self.stream, [self.dev(a) for a in real], [self.dev(a) for a in poison], call, ms)

    def close(self):
        if self.h is not None:
            self.h.close()


def _np(t):
    return t.cpu().numpy()


def _assert_list(oi, ov, roi, rov, what=""):
    gi, gv = _outlier_set(_np(oi), _np(ov))
    ri, rv = _outlier_set(roi, rov)
    assert np.array_equal(gi, ri) and np.array_equal(gv, rv), what + ": outlier set"


def _lists(oi, ov):
    """The binding's outlier arguments: None for an empty list."""
    return dict(outlier_idx=oi if oi.numel() else None, outlier_val=ov if ov.numel() else None)


# ---- the stages and the fused calls, every route ---------------------------------------------------------------
def _case_norm(c):
    R = c.R
    got = c.run([R.field("u")], [R.field("p")], lambda x: c.h.norm(x, INF))
    assert got == R.norm("u"), (got, R.norm("u"))  # (max|x| is exact in any order)


def _case_decompose(c):
    R = c.R
    got = c.run([R.field("u")], [R.field("p")], lambda x: c.h.decompose(x))
    assert_bit_equal(_np(got), R.coef("u"), "decompose")


def _case_recompose(c):
    R = c.R
    got = c.run([R.coef("u")], [R.coef("p")], lambda x: c.h.recompose(x))
    assert_bit_equal(_np(got), R.back("u"), "recompose")


def _case_quantize(c):
    R, mg = c.R, c.mg
    q, oi, ov, n = c.run([R.coef("u")], [R.coef("p")],
                         lambda x: c.h.quantize(x, mg.REL, TOL, INF, R.norm("u"), dict_size=DICT))
    rq, roi, rov, rn = R.quant("u")
    assert n == rn
    assert np.array_equal(_np(q), rq), "quantized integers"
    _assert_list(oi, ov, roi, rov, "quantize")


def _case_dequantize(c):
    R, mg = c.R, c.mg
    real, poison = R.qinputs()
    got = c.run(real, poison, lambda q, oi, ov: c.h.dequantize(q, mg.REL, TOL, INF, R.norm("u"), dict_size=DICT,
                                                               **_lists(oi, ov)))
    assert_bit_equal(_np(got), R.deq("u"), "dequantize")


def _case_decompose_quantize(c):
    R, mg = c.R, c.mg
    # norm = 0: the call reduces the norm itself, on the stream, before it builds the quantizer table
    q, oi, ov, n, nrm = c.run([R.field("u")], [R.field("p")],
                              lambda x: c.h.decompose_quantize(x, mg.REL, TOL, INF, dict_size=DICT))
    rq, roi, rov, rn = R.quant("u")
    assert nrm == R.norm("u") and n == rn
    assert np.array_equal(_np(q), rq), "quantized integers"
    _assert_list(oi, ov, roi, rov, "decompose_quantize")


def _case_dequantize_recompose(c):
    R, mg = c.R, c.mg
    real, poison = R.qinputs()
    got = c.run(real, poison, lambda q, oi, ov: c.h.dequantize_recompose(q, mg.REL, TOL, INF, R.norm("u"), dict_size=DICT,
                                                                         **_lists(oi, ov)))
    assert_bit_equal(_np(got), R.rback("u"), "dequantize_recompose")


def _case_decompose_quantize_sym16(c):
    R, mg, torch = c.R, c.mg, c.torch
    if c.route not in ("fused3", "fused4"):  # (mgard_hip.h: only where the fused kernels run)
        with pytest.raises(mg.MgardHipError):
            c.run([R.field("u")], [R.field("p")], lambda x: c.h.decompose_quantize_sym16(x, mg.REL, TOL, INF, dict_size=DICT))
        return
    sym, oi, ov, n, nrm = c.run([R.field("u")], [R.field("p")],
                                lambda x: c.h.decompose_quantize_sym16(x, mg.REL, TOL, INF, dict_size=DICT))
    rq, roi, rov, rn = R.quant("u")
    assert nrm == R.norm("u") and n == rn
    assert np.array_equal(_np(sym.view(torch.int16)).view(np.uint16).astype(np.int64), rq), "symbols"
    _assert_list(oi, ov, roi, rov, "decompose_quantize_sym16")


def _case_dequantize_recompose_sym16(c):
    R, mg = c.R, c.mg
    real, poison = R.qinputs()
    real[0], poison[0] = real[0].astype(np.uint16), poison[0].astype(np.uint16)
    call = lambda q, oi, ov: c.h.dequantize_recompose_sym16(q, mg.REL, TOL, INF, R.norm("u"), dict_size=DICT, **_lists(oi, ov))
    if not c.h.sym16_supported():  # (the library's documented predicate for this call)
        assert c.route != "fused3"
        with pytest.raises(mg.MgardHipError):
            c.run(real, poison, call)
        return
    assert_bit_equal(_np(c.run(real, poison, call)), R.rback("u"), "dequantize_recompose_sym16")


# ---- the fused 3-D route: every other entry point ---------------------------------------------------------------
def _case_norm_device(c):
    R = c.R
    got = c.run([R.field("u")], [R.field("p")], lambda x: c.h.norm_device(x, INF))
    assert R.dt(got.item()) == R.dt(R.norm("u"))


def _case_decompose_quantize_dn(c):
    """The bound of one of 8 subdomains under a GLOBAL norm that is itself produced on the stream."""
    R, mg, torch, dt = c.R, c.mg, c.torch, c.R.dt
    g = dt(R.norm("u"))
    atol = dt(TOL) * g  # (calc_local_abs_tol, REL, s = inf)

    def call(x, dn):
        bufs = (torch.empty(R.shape, dtype=torch.int64, device="cuda"),) + c.h._outlier_bufs(R.N)
        return c.h.decompose_quantize_dn(x, mg.REL, TOL, INF, dn, 8, bufs, dict_size=DICT)
    q, oi, ov, cnt = c.run([R.field("u"), np.array([g], dtype=dt)], [R.field("p"), np.array([dt(R.norm("p"))], dtype=dt)], call)
    rq, roi, rov, rn = R.quant("u", eb=oracle.ABS, tol=float(atol), norm=1.0)
    n = int(cnt.item())
    assert n == rn
    assert np.array_equal(_np(q), rq)
    _assert_list(oi[:n], ov[:n], roi, rov, "decompose_quantize_dn")


def _case_norm_stream(c):
    R, mg = c.R, c.mg
    parts = [R.N // 3, R.N - R.N // 3]

    def fused(x):
        c.h.norm_stream(x, INF, parts)
        return c.h.decompose_quantize(x, mg.REL, TOL, INF, dict_size=DICT)
    q, oi, ov, n, nrm = c.run([R.field("u")], [R.field("p")], fused)
    rq, roi, rov, rn = R.quant("u")
    assert nrm == R.norm("u") and n == rn
    assert np.array_equal(_np(q), rq)
    _assert_list(oi, ov, roi, rov, "streamed norm")

    def ended(x):
        c.h.norm_stream(x, INF, parts)
        return c.h.norm_stream_end(INF)
    assert c.run([R.field("u")], [R.field("p")], ended) == R.norm("u")


def _case_quantize_histograms(c):
    R, mg = c.R, c.mg
    tols = [1e-3, 2e-4]
    freq, outl = c.run([R.coef("u")], [R.coef("p")],
                       lambda x: c.h.quantize_histograms(x, tols, mg.REL, INF, R.norm("u"), dict_size=DICT))
    for k, tol in enumerate(tols):
        rq, _, _, rn = R.quant("u", tol=tol)
        assert np.array_equal(_np(freq[k]).astype(np.int64), np.bincount(rq.reshape(-1), minlength=DICT)), tol
        assert int(outl[k].item()) == rn


def _case_quantize_roundtrip(c):
    R, mg = c.R, c.mg
    got = c.run([R.coef("u")], [R.coef("p")], lambda x: c.h.quantize_roundtrip(x, mg.REL, TOL, INF, R.norm("u")))
    assert_bit_equal(_np(got), R.deq("u"), "quantize_roundtrip")


def _check_symbols(c, sym, freq, oi, ov):
    rq, roi, rov, rn = c.R.quant("u")
    assert np.array_equal(_np(sym.view(c.torch.int16)).view(np.uint16).astype(np.int64), rq), "symbols"
    assert np.array_equal(_np(freq).astype(np.int64), np.bincount(rq.reshape(-1), minlength=DICT)), "histogram"
    assert oi.numel() == rn
    _assert_list(oi, ov, roi, rov, "quantize_symbols")


def _case_quantize_symbols(c):
    R, mg = c.R, c.mg
    # (the binding zeroes the bins and the counter with torch.zeros on the current stream: behind the chain)
    sym, freq, oi, ov = c.run([R.coef("u")], [R.coef("p")],
                              lambda x: c.h.quantize_symbols(x, mg.REL, TOL, INF, R.norm("u"), dict_size=DICT))
    _check_symbols(c, sym, freq, oi, ov)


def _case_quantize_symbols_residual(c):
    R, mg = c.R, c.mg
    sym, freq, oi, ov, res = c.run([R.coef("u")], [R.coef("p")],
                                   lambda x: c.h.quantize_symbols_residual(x, mg.REL, TOL, INF, R.norm("u"), dict_size=DICT))
    _check_symbols(c, sym, freq, oi, ov)
    assert_bit_equal(_np(res), R.coef("u") - R.deq("u"), "residual")


def _case_dequantize_add(c):
    R, mg = c.R, c.mg
    real, poison = R.qinputs()

    def call(q, oi, ov, acc):
        first = c.h.dequantize_add(q, mg.REL, TOL, INF, R.norm("u"), dict_size=DICT, **_lists(oi, ov))
        c.h.dequantize_add(q, mg.REL, TOL, INF, R.norm("u"), dict_size=DICT, acc=acc, **_lists(oi, ov))
        return first, acc.clone()
    first, added = c.run(real + [R.field("u")], poison + [R.field("p")], call)
    assert_bit_equal(_np(first), R.deq("u"), "dequantize_add(first)")
    assert_bit_equal(_np(added), R.field("u") + R.deq("u"), "dequantize_add")


def _level(c):
    return c.R.o.l_target - 1


def _case_recompose_to_level(c):
    R, L = c.R, _level(c)
    got = c.run([R.coef("u")], [R.coef("p")], lambda x: c.h.recompose(x, level=L))
    assert_bit_equal(_np(got), R.level_values("u", L, of="coef"), "recompose_to_level")


def _case_dequantize_recompose_to_level(c):
    R, mg, L = c.R, c.mg, _level(c)
    real, poison = R.qinputs()
    got = c.run(real, poison, lambda q, oi, ov: c.h.dequantize_recompose(q, mg.REL, TOL, INF, R.norm("u"), dict_size=DICT,
                                                                         level=L, **_lists(oi, ov)))
    assert_bit_equal(_np(got), R.level_values("u", L), "dequantize_recompose_to_level")


def _case_dequantize_recompose_sym16_to_level(c):
    R, mg, L = c.R, c.mg, _level(c)
    real, poison = R.qinputs()
    real[0], poison[0] = real[0].astype(np.uint16), poison[0].astype(np.uint16)
    got = c.run(real, poison, lambda q, oi, ov: c.h.dequantize_recompose_sym16(q, mg.REL, TOL, INF, R.norm("u"), dict_size=DICT,
                                                                               level=L, **_lists(oi, ov)))
    assert_bit_equal(_np(got), R.level_values("u", L), "dequantize_recompose_sym16_to_level")


def _case_level_linearize(c):
    R = c.R
    roi = R.quant("u")[1]

    def call(q, oi):
        return c.h.level_linearize(q, outlier_idx=oi if oi.numel() else None), oi.clone()
    lin, oi = c.run([R.quant("u")[0], roi], [R.quant("p")[0], R.other_list(len(roi))[0]], call)
    assert np.array_equal(_np(lin).reshape(-1), R.linear("u")), "level_linearize"
    assert np.array_equal(_np(oi), R.linear_pos()[roi]), "linearised outlier positions"


def _linear_inputs(c, lo, hi):
    """(real, poison) of (integers [lo, hi) of the level-linearised array, linearised outlier positions, values)."""
    R = c.R
    _, roi, rov, _ = R.quant("u")
    poi, pov = R.other_list(len(roi))
    return [R.linear("u")[lo:hi], R.linear_pos()[roi], rov], [R.linear("p")[lo:hi], poi, pov]


def _case_level_box_from_linear(c):
    R, L = c.R, _level(c)
    n = R.level_count(L)
    got = c.run([R.linear("u")[:n]], [R.linear("p")[:n]], lambda lin: c.h.level_box_from_linear(lin, L))
    box = tuple(slice(0, m) for m in R.o.level_shape(L))
    assert np.array_equal(_np(got), R.quant("u")[0][box]), "level_box_from_linear"


def _case_dequantize_recompose_linear_to_level(c):
    R, mg, L = c.R, c.mg, _level(c)
    real, poison = _linear_inputs(c, 0, R.level_count(L))
    got = c.run(real, poison, lambda lin, oi, ov: c.h.dequantize_recompose_linear(
        lin, mg.REL, TOL, INF, R.norm("u"), dict_size=DICT, level=L, **_lists(oi, ov)))
    assert_bit_equal(_np(got), R.level_values("u", L), "dequantize_recompose_linear_to_level")


def _case_refine_level(c):
    R, mg, L = c.R, c.mg, _level(c)
    real, poison = _linear_inputs(c, R.level_count(L - 1), R.level_count(L))
    got = c.run([R.level_values("u", L - 1)] + real, [R.level_values("p", L - 1)] + poison,
                lambda coarse, seg, oi, ov: c.h.refine_level(coarse, seg, mg.REL, TOL, INF, R.norm("u"), L, dict_size=DICT,
                                                             **_lists(oi, ov)))
    assert_bit_equal(_np(got), R.level_values("u", L), "refine_level")


def _prolonged(R, which, L):
    return R.get(("prolonged", which, L), lambda: R.o.recompose(zeroed(R.o, R.coef(which), L)))


def _window(R):
    lo = tuple(min(3 + 2 * d, n - 2) for d, n in enumerate(R.shape))
    ext = tuple(max(1, (n - l) // 2) for l, n in zip(lo, R.shape))
    return lo, ext


def _case_prolong(c):
    R, L = c.R, _level(c)
    got = c.run([R.level_values("u", L, of="coef")], [R.level_values("p", L, of="coef")], lambda x: c.h.prolong(x, L))
    assert_bit_equal(_np(got), _prolonged(R, "u", L), "prolong")


def _case_prolong_window(c):
    R, L = c.R, _level(c)
    lo, ext = _window(R)
    got = c.run([R.level_values("u", L, of="coef")], [R.level_values("p", L, of="coef")],
                lambda x: c.h.prolong(x, L, window=(lo, ext)))
    crop = tuple(slice(l, l + e) for l, e in zip(lo, ext))
    assert_bit_equal(_np(got), np.ascontiguousarray(_prolonged(R, "u", L)[crop]), "prolong_window")


def _case_prolong_window_strided(c):
    """The window written into its own place of an array of the hierarchy's shape that holds a marker."""
    R, L, torch, mg = c.R, _level(c), c.torch, c.mg
    lo, ext = _window(R)
    D = len(R.shape)
    u64 = lambda v: (C.c_uint64 * D)(*[int(x) for x in v])
    MARK = -777.0

    def call(x):
        out = torch.full(R.shape, MARK, dtype=c.h.torch_dtype, device="cuda")
        first = out[tuple(slice(l, None) for l in lo)]
        mg._check(mg.load_library().mgh_prolong_window_strided(
            c.h._h, L, C.c_void_p(x.data_ptr()), u64(lo), u64(ext), C.c_void_p(first.data_ptr()), u64(out.stride()),
            mg._stream()))
        return out
    got = c.run([R.level_values("u", L, of="coef")], [R.level_values("p", L, of="coef")], call)
    want = np.full(R.shape, MARK, dtype=R.dt)
    crop = tuple(slice(l, l + e) for l, e in zip(lo, ext))
    want[crop] = _prolonged(R, "u", L)[crop]
    assert_bit_equal(_np(got), want, "prolong_window_strided")


# ---- calls without a hierarchy -----------------------------------------------------------------------------------
def _case_outlier_restore(c):
    R, mg = c.R, c.mg
    real, poison = R.qinputs()

    def call(q, oi, ov):
        p = lambda t: C.c_void_p(t.data_ptr())
        mg._check(mg.load_library().mgh_outlier_restore(p(q), q.numel(), p(oi), p(ov), oi.numel(), mg._stream()))
        return q.clone()
    got = c.run(real, poison, call)
    want = np.array(real[0], copy=True).reshape(-1)
    want[real[1]] = real[2]
    assert len(real[1]) > 0
    assert np.array_equal(_np(got).reshape(-1), want), "outlier_restore"


FILL = -9999.0


def _masked_field(R, which):
    """The route's field with NaN and fill values planted (rows with none, with some, a whole segment of them)."""
    def make():
        a = np.array(R.field(which), copy=True)
        rng = np.random.default_rng(3 if which == "u" else 4)
        flat = a.reshape(-1)
        flat[rng.choice(a.size, a.size // 50, replace=False)] = FILL
        if which == "u":
            flat[rng.choice(a.size, a.size // 200, replace=False)] = np.nan
        a[1, 2, :] = FILL
        return a
    return R.get(("masked", which), make)


def _mask_of(R, which):
    return R.get(("mask", which), lambda: mm.classify(_masked_field(R, which), True, FILL))


def _case_mask_scan(c):
    R, mg = c.R, c.mg
    words, st = c.run([_masked_field(R, "u")], [_masked_field(R, "p")], lambda x: mg.mask_scan(x, True, FILL))
    mask = _mask_of(R, "u")
    assert np.array_equal(_np(words).view(np.uint64), mm.packed_words(mask)), "mask words"
    n, nm, vmin, vmax = mm.stats(_masked_field(R, "u"), mask)
    assert (st.n, st.n_masked) == (n, nm)
    assert np.float64(st.vmin).view(np.uint64) == np.float64(vmin).view(np.uint64)
    assert np.float64(st.vmax).view(np.uint64) == np.float64(vmax).view(np.uint64)


def _case_mask_fill(c):
    R, mg = c.R, c.mg
    a, mask = _masked_field(R, "u"), _mask_of(R, "u")
    cst = mm.fill_constant(a, mask)
    got = c.run([a, mm.packed_words(mask)], [_masked_field(R, "p"), mm.packed_words(_mask_of(R, "p"))],
                lambda x, w: mg.mask_fill(x, w, float(cst)))
    assert np.array_equal(mm.int_view(_np(got)), mm.int_view(mm.fill(a, mask, cst))), "mask_fill"


def _case_mask_restore(c):
    R, mg = c.R, c.mg
    mask = _mask_of(R, "u")
    got = c.run([R.field("u"), mm.packed_words(mask)], [R.field("p"), mm.packed_words(_mask_of(R, "p"))],
                lambda x, w: mg.mask_restore(x, w, 1e20).clone())
    assert np.array_equal(mm.int_view(_np(got)), mm.int_view(mm.restore(R.field("u"), mask, 1e20))), "mask_restore"


def _case_compare(c):
    R, mg = c.R, c.mg
    got = c.run([R.field("u"), R.rback("u")], [R.field("p"), R.rback("p")], lambda a, b: mg.compare(a, b))
    assert_stats(got, ref_stats(R.field("u"), R.rback("u")), what="compare")


# ---- the lossless stage ------------------------------------------------------------------------------------------
HCHUNK, HDICT = 4096, 8192
HN = 3 * HCHUNK + 7


def _symbols(which):
    """Real: quantizer-like symbols. Poison: the same symbols in another order inside every chunk -- the same
    histogram, code and bits per chunk, so its record has the real record's length to the byte."""
    q = huffman_symbols(HN, seed=3, width=20.0, dict_size=HDICT)
    if which == "p":
        rng = np.random.default_rng(9)
        q = np.concatenate([rng.permutation(q[a:a + HCHUNK]) for a in range(0, HN, HCHUNK)])
    return q


def _hlists(which):
    return ((np.array([1, HN // 3], dtype=np.int64), np.array([-5, 99999], dtype=np.int64)) if which == "u" else
            (np.array([7, HN // 2], dtype=np.int64), np.array([123, -99999], dtype=np.int64)))


def _lossless(c):
    from mgard_amd import highlevel as hl
    return hl, hl.Lossless()


def _check_record(rec, sym, oi, ov, what):
    r = pl.parse_huffman_record(bytes(rec))
    assert (r["primary_count"], r["dict_size"], r["chunk_size"]) == (HN, HDICT, HCHUNK), what
    assert np.array_equal(pl.decode_huffman_record(r), sym), what + ": symbols of the record"
    assert np.array_equal(r["outlier_idx"].astype(np.int64), oi) and np.array_equal(r["outliers"], ov), what


def _case_histogram_sym16(c):
    torch, mg = c.torch, c.mg
    from mgard_amd import highlevel as hl

    def call(sym):
        freq = torch.zeros(HDICT, dtype=torch.int32, device="cuda")  # (the caller's zeroing, on the stream)
        mg._check(hl._hl().mgh_histogram_sym16(C.c_void_p(sym.data_ptr()), HN, HDICT, C.c_void_p(freq.data_ptr()), mg._stream()))
        return freq
    got = c.run([_symbols("u").astype(np.uint16)], [_symbols("p")[::-1].astype(np.uint16) // 2], call)
    assert np.array_equal(_np(got).astype(np.int64), np.bincount(_symbols("u"), minlength=HDICT)), "histogram_sym16"


def _sym_inputs(narrow):
    cast = (lambda a: a.astype(np.uint16)) if narrow else (lambda a: a)
    # (poison for the ENCODER: other symbols altogether, so that a record of them differs in every section)
    other = huffman_symbols(HN, seed=8, width=7.0, dict_size=HDICT)
    return [cast(_symbols("u"))] + list(_hlists("u")), [cast(other)] + list(_hlists("p"))


def _case_lossless_compress(c):
    hl, ctx = _lossless(c)
    for narrow in (False, True):
        real, poison = _sym_inputs(narrow)
        rec = c.run(real, poison, lambda q, oi, ov: ctx.compress(q, HDICT, HCHUNK, hl.HUFFMAN, 3, oi, ov))
        _check_record(rec, _symbols("u"), *_hlists("u"), what="lossless_compress%s" % ("_sym16" if narrow else ""))
    ctx.close()


def _case_lossless_compress_device(c):
    hl, ctx = _lossless(c)
    torch = c.torch
    for narrow in (False, True):
        real, poison = _sym_inputs(narrow)

        def call(q, oi, ov):
            out = torch.zeros(8 * HN + (1 << 20), dtype=torch.uint8, device="cuda")
            return ctx.compress_device(q, out, HDICT, HCHUNK, outlier_idx=oi, outlier_val=ov)
        rec = c.run(real, poison, call)
        _check_record(_np(rec), _symbols("u"), *_hlists("u"), what="lossless_compress_device%s" % ("_sym16" if narrow else ""))
    ctx.close()


_RECORDS = {}


def _record(which):
    """A device-resident record of the symbols, written beforehand (synchronised) and read back by the independent
    reader of tests/payload.py before it serves as an input."""
    if which not in _RECORDS:
        torch, mg = _gpu()
        from mgard_amd import highlevel as hl
        ctx = hl.Lossless()
        oi, ov = _hlists(which)
        rec = ctx.compress(torch.from_numpy(_symbols(which)).cuda(), HDICT, HCHUNK, hl.HUFFMAN, 3,
                           torch.from_numpy(oi).cuda(), torch.from_numpy(ov).cuda())
        torch.cuda.synchronize()
        ctx.close()
        _check_record(rec, _symbols(which), oi, ov, "record " + which)
        _RECORDS[which] = np.frombuffer(rec, dtype=np.uint8).copy()
    return _RECORDS[which]


def _case_lossless_decompress(c):
    hl, ctx = _lossless(c)
    torch = c.torch
    real, poison = [_record("u")], [_record("p")]
    assert real[0].shape == poison[0].shape and not np.array_equal(real[0], poison[0])
    sym, (roi, rov) = _symbols("u"), _hlists("u")

    def check(q, oi, ov, want, what):
        got = _np(q.view(torch.int16)).view(np.uint16).astype(np.int64) if q.dtype == torch.uint16 else _np(q)
        assert np.array_equal(got, want), what
        assert np.array_equal(_np(oi), roi) and np.array_equal(_np(ov), rov), what + ": outlier lists"

    q, oi, ov = c.run(real, poison, lambda rec: ctx.decompress(rec, HN))
    check(q, oi, ov, sym, "lossless_decompress")
    q, oi, ov = c.run(real, poison, lambda rec: ctx.decompress(rec, HN, prefix=HCHUNK + 5, out=torch.zeros(2 * HCHUNK, dtype=torch.int64, device="cuda")))
    check(q, oi, ov, sym[:2 * HCHUNK], "lossless_decompress_prefix")
    q, oi, ov = c.run(real, poison, lambda rec: ctx.decompress(rec, HN, first=HCHUNK + 1, count=HCHUNK, out=torch.zeros(2 * HCHUNK, dtype=torch.int64, device="cuda")))
    check(q, oi, ov, sym[HCHUNK:3 * HCHUNK], "lossless_decompress_range")
    q, oi, ov = c.run(real, poison, lambda rec: ctx.decompress(rec, HN, sym16=True))
    check(q, oi, ov, sym, "lossless_decompress_sym16")
    ctx.close()


_NO_HIERARCHY = {"outlier_restore", "mask_scan", "mask_fill", "mask_restore", "compare", "histogram_sym16",
                 "lossless_compress", "lossless_compress_device", "lossless_decompress"}
_streams = {}


def _side_stream(k=0):
    """At most two side streams in the process (and the default stream): three alive at once."""
    torch, _ = _gpu()
    if k not in _streams:
        _streams[k] = torch.cuda.Stream()
    return _streams[k]


def _run_case(name, route, stream, monkeypatch):
    c = Ctx(route, stream, monkeypatch, hierarchy=name not in _NO_HIERARCHY)
    try:
        globals()["_case_" + name](c)
    finally:
        c.close()


@pytest.mark.parametrize("name,route", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_entry_point_in_stream_order(name, route, monkeypatch):
    _run_case(name, route, _side_stream(), monkeypatch)


def test_the_ipk_dma_route_launches_k_ipk_dma(monkeypatch):
    """What the "ipk-dma" route is there for: the plan log of its hierarchy shows the r-solve of the top level as
    a Dma solve, adding in decompose and subtracting in recompose. (On the fused route the f- and c-solve of a
    box whose planes fit LDS never reach k_ipk_dma, whatever MGH_IPK_DMA_MIN says.)"""
    c = Ctx("ipk-dma", _side_stream(), monkeypatch)
    try:
        c.h.profile(True)
        _case_decompose(c)
        _case_recompose(c)
        dma = {(r["axis"], r["m"], r["add"]) for r in c.h.ipk_plans() if r["family"] == "Dma"}
        assert dma == {(0, (201, 16, 26), +1), (0, (201, 16, 26), -1)}, dma
    finally:
        c.close()


@pytest.mark.parametrize("name", [n for n, _, routes in CASE_TABLE if "fused3" in routes])
def test_default_stream_results_unchanged(name, monkeypatch):
    """The same harness and cases with the default stream: a failure above that does not show here is the
    stream's, one that shows here too is the harness's or the case's."""
    torch, _ = _gpu()
    _run_case(name, "fused3", torch.cuda.default_stream(), monkeypatch)


# ---- host-side bookkeeping between calls ---------------------------------------------------------------------------
A_KW = dict(eb=oracle.REL, tol=1e-3, s=INF, dict_size=8192)
B_KW = dict(eb=oracle.ABS, tol=1e-5, s=0.0, norm=1.0, dict_size=64)


def _bufs(torch, h):
    return (torch.empty(h.shape, dtype=torch.int64, device="cuda"),) + h._outlier_bufs(h.total)


def _check_bufs(bufs, want, what):
    q, cnt, idx, val = bufs
    rq, roi, rov, rn = want
    n = int(cnt.item())
    assert n == rn, what
    assert np.array_equal(_np(q), rq), what + ": quantized integers"
    _assert_list(idx[:n], val[:n], roi, rov, what)


@pytest.mark.parametrize("route", ["fused3", "fused4"])
def test_back_to_back_calls_on_one_hierarchy(route, monkeypatch):
    """A, B, A on one stream and one hierarchy with nothing in between: another tolerance, dictionary, bound type
    and s per call (the quantizer table and the norm of a call must not reach the kernels of its neighbours)."""
    c = Ctx(route, _side_stream(), monkeypatch)
    R, mg, torch, h = c.R, c.mg, c.torch, c.h

    def encode(a, b):
        out = [_bufs(torch, h) for _ in range(3)]
        # A: REL without a norm and without a host read-back: the norm stays on the device
        h.decompose_quantize(a, mg.REL, 1e-3, INF, dict_size=8192, bufs=out[0], want_norm=False)
        h.decompose_quantize(b, mg.ABS, 1e-5, 0.0, norm=1.0, dict_size=64, bufs=out[1], want_norm=False)
        h.decompose_quantize(a, mg.REL, 1e-3, INF, dict_size=8192, bufs=out[2], want_norm=False)
        return out
    # (the poison of A is B and the other way round)
    out = c.run([R.field("u"), R.field("p")], [R.field("p"), R.field("u")], encode)
    _check_bufs(out[0], R.quant("u", **A_KW), "A")
    _check_bufs(out[1], R.quant("p", **B_KW), "B")
    _check_bufs(out[2], R.quant("u", **A_KW), "A again")

    qa, oia, ova, _ = R.quant("u", **A_KW)
    qb, oib, ovb, _ = R.quant("p", **B_KW)
    pa, pb = R.other_list(len(oia)), R.other_list(len(oib))

    def decode(qa, oia, ova, qb, oib, ovb):
        ra = h.dequantize_recompose(qa, mg.REL, 1e-3, INF, R.norm("u"), dict_size=8192, **_lists(oia, ova))
        rb = h.dequantize_recompose(qb, mg.ABS, 1e-5, 0.0, 1.0, dict_size=64, **_lists(oib, ovb))
        ra2 = h.dequantize_recompose(qa, mg.REL, 1e-3, INF, R.norm("u"), dict_size=8192, **_lists(oia, ova))
        return ra, rb, ra2
    ra, rb, ra2 = c.run([qa, oia, ova, qb, oib, ovb], [qb, pa[0], pa[1], qa, pb[0], pb[1]], decode)
    kw_a = {k: v for k, v in A_KW.items()}
    assert_bit_equal(_np(ra), R.rback("u", **kw_a), "A back")
    assert_bit_equal(_np(rb), R.rback("p", **B_KW), "B back")
    assert_bit_equal(_np(ra2), R.rback("u", **kw_a), "A back again")
    c.close()


@pytest.mark.parametrize("routes", [("two-a", "two-b"), ("fused3", "fused3")], ids=["different-shapes", "equal-shapes"])
def test_two_hierarchies_on_two_streams(routes, monkeypatch):
    """Two hierarchies, each on its own side stream behind its own delay (20 ms, 35 ms), their calls enqueued
    A, B, A, B and synchronised at the end only. Equal shapes: where a scratch buffer of the process or the device
    shared by mistake would collide. The second hierarchy works on the other field."""
    torch, mg = _gpu()
    R = [ref_of(r) for r in routes]
    which = ["u", "p"]
    other = ["p", "u"]
    streams = [_side_stream(0), _side_stream(1)]
    hs = [mg.Hierarchy(r.shape, r.dt) for r in R]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    real, poison = [], []
    for k in range(2):
        q, oi, ov, _ = R[k].quant(which[k])
        poi, pov = R[k].other_list(len(oi))
        real.append([dev(a) for a in (R[k].field(which[k]), q, oi, ov)])
        poison.append([dev(a) for a in (R[k].field(other[k]), R[k].quant(other[k])[0], poi, pov)])
    so.warm_up(*streams)
    work = [so.prepare(real[k], poison[k]) for k in range(2)]
    events = [so.produce(streams[k], work[k], real[k], ms=(20, 35)[k]) for k in range(2)]
    so.guard(*events)
    enc, dec = [None, None], [None, None]
    for k in range(2):
        with torch.cuda.stream(streams[k]):
            x = work[k][0]
            enc[k] = _bufs(torch, hs[k])
            hs[k].decompose_quantize(x, mg.REL, TOL, INF, norm=R[k].norm(which[k]), dict_size=DICT, bufs=enc[k], want_norm=False)
    for k in range(2):
        with torch.cuda.stream(streams[k]):
            _, q, oi, ov = work[k]
            dec[k] = hs[k].dequantize_recompose(q, mg.REL, TOL, INF, R[k].norm(which[k]), dict_size=DICT, **_lists(oi, ov))
    for k in range(2):
        with torch.cuda.stream(streams[k]):
            for w, p in zip(work[k], poison[k]):
                w.copy_(p)
    for s in streams:
        s.synchronize()
    for k in range(2):
        _check_bufs(enc[k], R[k].quant(which[k]), "hierarchy %d" % k)
        assert_bit_equal(_np(dec[k]), R[k].rback(which[k]), "hierarchy %d: dequantize_recompose" % k)
        hs[k].close()
