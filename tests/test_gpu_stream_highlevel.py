"""The stream contract of the container calls (include/mgard_hip_compress.h, above mgh_pin_memory; the docstring
of mgard_amd/highlevel.py), with the harness of tests/stream_order.py.

The C ABI promises that an input the NULL stream is still producing is complete before the first stage reads
it; work in flight on non-blocking streams is NOT waited for. The Python binding adds the wait for the current
torch stream. Both are pinned here: the array a call is given is still being produced when the call is entered
(guarded), and is overwritten right behind the call.

Expected values: a fully synchronised run of the same call on the same input. The decompressed arrays are
compared bit for bit (container bytes are not: the order of the outlier lists is not deterministic), and the
error bound is held against the input as tests/test_gpu_highlevel.py::test_compress_decompress_roundtrip holds it.

Poison containers are cut or zero-padded to the real container's length; the poison field is the smoother one,
so its containers are the shorter ones."""
import numpy as np
import pytest

from tests import stream_order as so
from tests.compare_ref import EXACT
from tests.util import smooth_field

pytestmark = pytest.mark.gpu

SHAPE, TOL, INF = (65, 70, 129), 1e-3, float("inf")
TOLS = [1e-2, 1e-3]
FILL = -9999.0
DTYPES = [np.float32, np.float64]


def _mods():
    import torch
    import mgard_amd
    from mgard_amd import highlevel
    return torch, mgard_amd, highlevel


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and np.array_equal(g, w), "%s: %d of %d values differ from the synchronised run" % (
        what, int((g != w).sum()) if g.shape == w.shape else -1, w.size)


def _within(u, v, tol, what):
    """The L-infinity bound of a REL, s = inf container, as test_compress_decompress_roundtrip computes it."""
    v = v.cpu().numpy() if hasattr(v, "cpu") else v
    ok = np.isfinite(u)
    err = float(np.max(np.abs(u[ok].astype(np.float64) - v[ok].astype(np.float64))))
    bound = tol * float(np.max(np.abs(u[ok])))
    assert err <= bound * (1 + 1e-6), (what, err, bound)


def _fit(poison, n):
    """A poison container cut or zero-padded to n bytes."""
    out = np.zeros(n, dtype=np.uint8)
    k = min(n, poison.size)
    out[:k] = poison[:k]
    return out


_SYNC = {}


def _sync(dt):
    """Everything of a data type from fully synchronised runs on the default stream, made once: the fields (real
    and poison), and per call the real run's result and the poison inputs."""
    key = np.dtype(dt).name
    if key in _SYNC:
        return _SYNC[key]
    torch, mg, hl = _mods()
    E = {}
    E["u"] = smooth_field(SHAPE, dt)
    E["p"] = smooth_field(SHAPE, dt, seed=777, noise=1e-4)
    E["um"], E["pm"] = np.array(E["u"], copy=True), np.array(E["p"], copy=True)
    rng = np.random.default_rng(2)
    E["um"].reshape(-1)[rng.choice(E["u"].size, E["u"].size // 100, replace=False)] = FILL
    E["pm"].reshape(-1)[rng.choice(E["u"].size, E["u"].size // 100, replace=False)] = FILL
    E["cfg1"] = hl.Config(reorder=1)
    for w, m in (("u", "um"), ("p", "pm")):
        d = torch.from_numpy(E[w]).cuda()
        E["buf_" + w] = hl.compress(d, TOL, INF, mg.REL).cpu().numpy()
        E["lin_" + w] = hl.compress(d, TOL, INF, mg.REL, config=E["cfg1"]).cpu().numpy()
        E["ladder_" + w] = [b.cpu().numpy() for b in hl.compress_ladder(d, TOLS, INF, mg.REL)]
        E["layers_" + w] = [b.cpu().numpy() for b in hl.compress_layers(d, TOLS, INF, mg.REL)]
        E["masked_" + w] = hl.compress_masked(torch.from_numpy(E[m]).cuda(), TOL, INF, mg.REL, nonfinite=False,
                                              fill_value=FILL, restore_value=FILL).cpu().numpy()
    dev = lambda a: torch.from_numpy(a).cuda()
    du = dev(E["u"])
    E["v"] = hl.decompress(dev(E["buf_u"])).cpu().numpy()
    E["v_ladder"] = [hl.decompress(dev(b)).cpu().numpy() for b in E["ladder_u"]]
    E["v_layers"] = hl.decompress_layers([dev(b) for b in E["layers_u"]]).cpu().numpy()
    E["v_masked"] = hl.decompress_masked(dev(E["masked_u"])).cpu().numpy()
    E["verify"] = hl.verify(dev(E["buf_u"]), du)
    E["sizes"] = hl.estimate_sizes(du, TOLS, INF, mg.REL)
    E["errors"] = hl.achieved_errors(du, TOLS, INF, mg.REL)
    lt = hl.infer_level(E["lin_u"], None, E["cfg1"])[1]
    E["levels"] = (lt - 2, lt)
    with hl.Progressive(dev(E["lin_u"]), E["cfg1"]) as pr:
        E["v_levels"] = [pr.refine(l).cpu().numpy() for l in E["levels"]]
    torch.cuda.synchronize()
    # the synchronised runs themselves hold the bound
    _within(E["u"], E["v"], TOL, "synchronised run")
    assert E["buf_p"].size <= E["buf_u"].size
    _SYNC[key] = E
    return E


def _dev(torch, arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _check_all(E, mg, hl, run, cases=None):
    """Every container call of the issue through run(real, poison, call) -> call's result."""
    torch = _mods()[0]
    u = E["u"]
    sync_dec = lambda b: hl.decompress(b)  # (after run(): the stream is idle, the buffer complete)

    def case(name):
        return cases is None or name in cases

    if case("compress"):
        buf = run([u], [E["p"]], lambda x: hl.compress(x, TOL, INF, mg.REL))
        v = sync_dec(buf)
        _same(v, E["v"], "compress")
        _within(u, v, TOL, "compress")
    if case("decompress"):
        v = run([E["buf_u"]], [_fit(E["buf_p"], E["buf_u"].size)], lambda b: hl.decompress(b))
        _same(v, E["v"], "decompress")
        _within(u, v, TOL, "decompress")
    if case("compress_ladder"):
        bufs = run([u], [E["p"]], lambda x: hl.compress_ladder(x, TOLS, INF, mg.REL))
        for k, b in enumerate(bufs):
            v = sync_dec(b)
            _same(v, E["v_ladder"][k], "compress_ladder[%d]" % k)
            _within(u, v, TOLS[k], "compress_ladder[%d]" % k)
    if case("compress_layers"):
        bufs = run([u], [E["p"]], lambda x: hl.compress_layers(x, TOLS, INF, mg.REL))
        v = hl.decompress_layers(bufs)
        _same(v, E["v_layers"], "compress_layers")
        _within(u, v, TOLS[-1], "compress_layers")
    if case("decompress_layers"):
        real = E["layers_u"]
        v = run(real, [_fit(p, r.size) for p, r in zip(E["layers_p"], real)], lambda *bufs: hl.decompress_layers(list(bufs)))
        _same(v, E["v_layers"], "decompress_layers")
        _within(u, v, TOLS[-1], "decompress_layers")
    if case("compress_masked"):
        buf = run([E["um"]], [E["pm"]], lambda x: hl.compress_masked(x, TOL, INF, mg.REL, nonfinite=False, fill_value=FILL,
                                                                    restore_value=FILL))
        v = hl.decompress_masked(buf)
        _same(v, E["v_masked"], "compress_masked")
    if case("decompress_masked"):
        v = run([E["masked_u"]], [_fit(E["masked_p"], E["masked_u"].size)], lambda b: hl.decompress_masked(b))
        _same(v, E["v_masked"], "decompress_masked")
        valid = E["um"] != E["um"].dtype.type(FILL)
        w = v.cpu().numpy()
        assert np.all(w[~valid] == w.dtype.type(FILL))
        _within(np.where(valid, E["um"], np.nan), w, TOL, "decompress_masked")
    if case("verify"):
        r = run([E["buf_u"], u], [_fit(E["buf_p"], E["buf_u"].size), E["p"]], lambda b, x: hl.verify(b, x))
        for k in EXACT:
            assert getattr(r.stats, k) == getattr(E["verify"].stats, k), ("verify", k)
        assert (r.within, r.bound_kind, r.bound) == (1, 0, E["verify"].bound)
    if case("estimate_sizes"):
        r = run([u], [E["p"]], lambda x: hl.estimate_sizes(x, TOLS, INF, mg.REL))
        assert [bytes(e) for e in r] == [bytes(e) for e in E["sizes"]], (r, E["sizes"])
    if case("achieved_errors"):
        r = run([u], [E["p"]], lambda x: hl.achieved_errors(x, TOLS, INF, mg.REL))
        for got, want, tol in zip(r, E["errors"], TOLS):
            for k in EXACT:
                assert getattr(got, k) == getattr(want, k), ("achieved_errors", tol, k)
            assert got.max_abs_err <= tol * float(np.max(np.abs(u))) * (1 + 1e-6)
    if case("progressive"):
        def walk(b):
            with hl.Progressive(b, E["cfg1"]) as pr:
                return [pr.refine(l) for l in E["levels"]]
        got = run([E["lin_u"]], [_fit(E["lin_p"], E["lin_u"].size)], walk)
        for l, g, w in zip(E["levels"], got, E["v_levels"]):
            _same(g, w, "Progressive.refine(%d)" % l)
        _within(u, got[-1], TOL, "Progressive.refine(l_target)")


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_null_stream_producer_is_waited_for(dt):
    """What the C ABI promises: producer and call both on the default (NULL) stream, the producer still running
    when the call is entered."""
    torch, mg, hl = _mods()
    E = _sync(dt)
    S = torch.cuda.default_stream()
    run = lambda real, poison, call: so.run_ordered(S, _dev(torch, real), _dev(torch, poison), call)
    _check_all(E, mg, hl, run, cases=("compress", "decompress"))


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_side_stream_producer_through_the_python_binding(dt):
    """What the Python binding adds: the same producer on a torch side stream (non-blocking), the call made inside
    `with torch.cuda.stream(S)`. Without the binding's wait for the current stream the library reads its input
    while S is still busy ahead of the copy that produces it."""
    torch, mg, hl = _mods()
    E = _sync(dt)
    from tests.test_gpu_stream_order import _side_stream
    S = _side_stream()
    run = lambda real, poison, call: so.run_ordered(S, _dev(torch, real), _dev(torch, poison), call)
    _check_all(E, mg, hl, run)
