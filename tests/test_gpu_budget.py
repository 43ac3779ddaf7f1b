"""GPU tests of the sizes-before-compressing calls: mgh_quantize_histograms against the
quantizer it shadows, mgh_estimate_sizes against the containers mgh_compress writes, mgh_compress_budget
against the search restated in NumPy (tests/size_model.py) on histograms from the CPU oracle, and the
refusals.

Every comparison is an equality or an inequality of integers: a histogram is a count, a container's size a
function of counts, and the search walks doubles made by sqrt and one multiply."""
import numpy as np
import pytest

from tests import payload as pl
from tests import size_model as sm
from tests.util import BLOCK, nonuniform_coords, smooth_field

pytestmark = pytest.mark.gpu

INF = float("inf")
F32, F64 = np.float32, np.float64
FUSED3 = (34, 33, 32)  # takes the fused level kernels in mgh_compress (tests/test_gpu_decompose_quantize_routes.py)
SMALL = (33, 17, 20)
MGH_ERR_INVALID_ARGUMENT, MGH_ERR_OUTPUT_TOO_LARGE = -1, -7


def _gpu():
    import torch
    import mgard_amd
    from mgard_amd import highlevel
    return torch, mgard_amd, highlevel


# ---- 1. the histograms are the quantizer's -----------------------------------------------------------------
# (shape, dtype, REL?, s, dict, ntol, non-uniform grid). dict 8192: 1 / 5 / 9 tolerances are one / two / three
# launches; 16384: 1 / 3, 4 / 5; 64: 9 are two.
HIST_CASES = [
    ((1000,), F32, False, INF, 8192, 1, False),
    ((1000,), F64, True, 0.0, 64, 9, False),
    ((65, 40), F32, True, 0.0, 16384, 5, False),
    ((65, 40), F64, False, INF, 8192, 4, False),
    (SMALL, F32, True, INF, 8192, 9, False),
    (SMALL, F64, False, 0.0, 16384, 3, False),
    (SMALL, F32, False, 0.0, 64, 5, True),
    ((5, 9, 9, 17), F32, True, 0.0, 8192, 3, False),
    ((5, 9, 9, 17), F64, True, INF, 64, 4, False),
    ((3, 3, 5, 5, 9), F64, False, 0.0, 8192, 5, False),
    ((3, 3, 5, 5, 9), F32, True, INF, 16384, 1, False),
    (FUSED3, F32, True, 0.0, 8192, 9, False),
    (FUSED3, F64, False, INF, 16384, 4, False),
]


def _tolerances(ntol):
    """One so small that nearly every value leaves the dictionary, one so large that every value lands in
    dict / 2, the rest between (ntol >= 3); a single one: in the middle."""
    if ntol < 3:
        return [1e-3, 1e-2][:ntol]
    return [1e-13] + [float(t) for t in np.logspace(-5, -1, ntol - 2)] + [1e6]


@pytest.mark.parametrize("shape,dt,rel,s,dict_size,ntol,nonuniform", HIST_CASES)
def test_histograms_are_the_quantizers(shape, dt, rel, s, dict_size, ntol, nonuniform):
    torch, mg, _ = _gpu()
    h = mg.Hierarchy(shape, dt, coords=nonuniform_coords(shape, dt) if nonuniform else None)
    d = torch.from_numpy(smooth_field(shape, dt)).cuda()
    c = h.decompose(d)
    eb = mg.REL if rel else mg.ABS
    norm = h.norm(d, s) if rel else 1.0
    tols = _tolerances(ntol)
    freq, outl = h.quantize_histograms(c, tols, eb, s, norm, dict_size=dict_size)
    freq, outl = freq.cpu().numpy(), outl.cpu().numpy()
    n = int(np.prod(shape))
    assert freq.shape == (ntol, dict_size) and (freq.sum(axis=1) == n).all()
    for k, tol in enumerate(tols):
        q, _, _, nout = h.quantize(c, eb, tol, s, norm, dict_size=dict_size)
        want = np.bincount(q.cpu().numpy().ravel(), minlength=dict_size)
        assert int(outl[k]) == nout, (k, tol)
        assert np.array_equal(freq[k], want), (k, tol, np.nonzero(freq[k] != want)[0][:8])
    if ntol >= 3:
        assert outl[0] > 0.9 * n                                       # nearly every value an outlier ...
        assert freq[-1, dict_size // 2] == n and outl[-1] == 0         # ... and every value in the middle bin
    if shape in ((65, 40), SMALL):
        # the misaligned scalar route: a view that starts one element into an allocation
        store = torch.empty(n + 1, dtype=c.dtype, device=c.device)
        off = store[1:].view(shape)
        off.copy_(c)
        assert off.data_ptr() % 16 != 0 and off.is_contiguous()
        freq1, outl1 = h.quantize_histograms(off, tols, eb, s, norm, dict_size=dict_size)
        assert np.array_equal(freq1.cpu().numpy(), freq) and np.array_equal(outl1.cpu().numpy(), outl)
    # a second call on the same handle zeroes its outputs itself
    freq2, outl2 = h.quantize_histograms(c, tols[:1], eb, s, norm, dict_size=dict_size)
    assert np.array_equal(freq2.cpu().numpy()[0], freq[0]) and int(outl2[0]) == int(outl[0])
    h.close()


def test_histogram_call_checks_its_arguments():
    torch, mg, _ = _gpu()
    h = mg.Hierarchy((17, 20), F32)
    c = h.decompose(torch.from_numpy(smooth_field((17, 20), F32)).cuda())
    for tols, dict_size in (([], 8192), ([1e-3] * 65, 8192), ([1e-3], 1), ([1e-3], 16385)):
        with pytest.raises(mg.MgardHipError, match="error %d" % MGH_ERR_INVALID_ARGUMENT):
            h.quantize_histograms(c, tols, mg.ABS, INF, 1.0, dict_size=dict_size)
    freq, _ = h.quantize_histograms(c, [1e-3] * 64, mg.ABS, INF, 1.0, dict_size=64)
    assert (freq.cpu().numpy() == freq.cpu().numpy()[0]).all()
    h.close()


# ---- 2. the estimates bracket what is written ----------------------------------------------------------------
# (shape, dtype, REL?, s, huff_block_size or None, huff_dict_size or None, reorder, device input)
# REL with s = 0 is the norm-bits case: the quantizers of the candidates are scaled by the norm mgh_compress
# reduces -- piece by piece while a host array arrives (FUSED3, host), in one pass otherwise. float32 there: a
# float64 sum of squares does not reproduce its last bit from run to run (atomicAdd order), in mgh_compress
# itself as little as here.
EST_CASES = [
    (SMALL, F32, True, 0.0, 1024, 256, 0, False),
    (SMALL, F32, False, INF, None, 256, 1, True),
    (FUSED3, F64, False, 0.0, 1024, None, 0, True),
    (FUSED3, F32, True, INF, None, None, 1, False),
    (FUSED3, F32, True, 0.0, None, 256, 0, False),
    (FUSED3, F32, True, 0.0, 1024, None, 0, True),
    ((65, 40), F64, False, 0.0, 1024, 256, 0, False),
]
EST_TOLS = [1e-10, 1e-5, 1e-4, 1e-3, 1e-2, 1e3]


def _config(hl, block, dict_size, reorder=0, **kw):
    cfg = hl.Config(reorder=reorder, **kw)
    if block:
        cfg.huff_block_size = block
    if dict_size:
        cfg.huff_dict_size = dict_size
    return cfg


def _record_of(hl, buf):
    b = bytes(buf.cpu().numpy() if hasattr(buf, "cpu") else buf)
    recs = pl.split_container(b, hl.metadata_parse(b)["metadata_size"])
    assert len(recs) == 1
    return recs[0]


_raw_seen = set()


@pytest.mark.parametrize("shape,dt,rel,s,block,dict_size,reorder,on_device", EST_CASES)
def test_estimates_bracket_the_containers(shape, dt, rel, s, block, dict_size, reorder, on_device):
    torch, mg, hl = _gpu()
    u = smooth_field(shape, dt)
    data = torch.from_numpy(u).cuda() if on_device else u
    mode = mg.REL if rel else mg.ABS
    cfg = _config(hl, block, dict_size, reorder)
    n, elem = u.size, u.itemsize
    nchunk = sm.nchunks(n, int(cfg.huff_block_size))
    est = hl.estimate_sizes(data, EST_TOLS, s, mode, config=cfg)
    assert [e.tol for e in est] == EST_TOLS
    for e in est:
        buf = hl.compress(data, e.tol, s, mode, config=cfg)
        size = int(buf.numel() if on_device else buf.size)
        print(shape, np.dtype(dt).name, e, size)
        assert e.bytes_min <= size <= e.bytes_max, (e, size)
        assert e.bytes_max - e.bytes_min <= 8 * nchunk
        rec = _record_of(hl, buf)
        raw = len(rec) == n * elem
        _raw_seen.add(raw)
        if e.raw != -1:
            assert e.raw == int(raw), (e, len(rec))
        if not raw:
            r = pl.parse_huffman_record(rec)
            assert len(r["outlier_idx"]) == e.outliers
            assert int(r["bits"].sum()) == e.code_bits
    assert est[0].raw == 1 and est[-1].raw == 0  # (the list runs from incompressible to nearly empty)
    hl._hl().mgh_release_cache()


def test_estimates_saw_raw_and_huffman_records():
    assert _raw_seen == {True, False}


# ---- 3. the budget ---------------------------------------------------------------------------------------
class OracleSizes:
    """bytes_max of a tolerance WITHOUT the code under test: decomposition and quantizer of oracle/,
    numpy.bincount, code lengths from the host-only mgh_huffman_codebook, the NumPy PayloadLayout."""

    def __init__(self, shape, dt, rel, s, dict_size, block):
        import oracle
        _, mg, hl = _gpu()
        self.hl, self.oracle = hl, oracle
        self.u = smooth_field(shape, dt)
        self.shape, self.dt, self.rel, self.s, self.dict_size, self.block = shape, np.dtype(dt).type, rel, s, dict_size, block
        self.o = oracle.Hierarchy(shape, dt)
        self.coeff = self.o.decompose(self.u)
        self.norm = oracle.norm(self.u, s) if rel else 1.0
        self.memo = {}

    def bytes_max(self, tol):
        tol = float(tol)
        if tol not in self.memo:
            o, dt = self.oracle, self.dt
            q, _, _, nout = self.o.quantize(self.coeff, o.REL if self.rel else o.ABS, dt(tol), dt(self.s), dt(self.norm),
                                            dict_size=self.dict_size)
            freq = np.bincount(np.asarray(q).ravel(), minlength=self.dict_size).astype(np.uint32)
            code = self.hl.huffman_codebook(freq)[0]
            bits = int((freq.astype(np.uint64) * (code >> np.uint64(56))).sum())
            n = self.u.size
            rec = sm.record_bracket(n, self.dict_size, self.block, bits, int(nout),
                                    sm.has_sync(sm.HUFFMAN, self.dict_size, self.block, bits, n))
            meta = len(self.hl.metadata_serialize(0 if dt == np.float32 else 1, self.shape, 0 if self.rel else 1, tol,
                                                  self.s, norm=self.norm if self.rel else 0.0,
                                                  dict_size=self.dict_size, block_size=self.block))
            self.memo[tol] = sm.container_bracket(meta, n, self.u.itemsize, rec)[1]
        return self.memo[tol]


BUDGET_SETUPS = {"small-f32": (SMALL, F32, True, INF, 64, 20480), "fused-f64": (FUSED3, F64, False, INF, 256, 20480)}
_oracles = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_oracles():
    yield
    _oracles.clear()


def _oracle_sizes(name):
    if name not in _oracles:
        _oracles[name] = OracleSizes(*BUDGET_SETUPS[name])
    return _oracles[name]


TOL_MIN, TOL_MAX = 1e-4, 1e2  # six decades (smooth_field is rough on grids this small: a dictionary of 64 needs quanta of its size)


@pytest.mark.parametrize("rounds", [1, 4])
@pytest.mark.parametrize("fraction", [0.10, 0.25, 0.50])
@pytest.mark.parametrize("name", sorted(BUDGET_SETUPS))
def test_budget(name, fraction, rounds):
    torch, mg, hl = _gpu()
    O = _oracle_sizes(name)
    shape, dt, rel, s, dict_size, block = BUDGET_SETUPS[name]
    mode = mg.REL if rel else mg.ABS
    cfg = _config(hl, block, dict_size)
    u = O.u
    data = torch.from_numpy(u).cuda() if name == "fused-f64" else u
    budget = int(fraction * u.nbytes)
    want, finer = sm.search(lambda t: O.bytes_max(t) <= budget, TOL_MIN, TOL_MAX, rounds)
    assert want is not None and finer is not None, "the case must search"
    buf, tol_used, est = hl.compress_budget(data, budget, TOL_MIN, TOL_MAX, rounds=rounds, s=s, mode=mode, config=cfg)
    size = int(buf.numel() if hasattr(buf, "numel") else buf.size)
    print(name, fraction, rounds, "budget", budget, "size", size, "tol", tol_used, est)
    assert size <= budget
    assert float(tol_used).hex() == float(want).hex(), (tol_used, want)
    assert est.tol == tol_used and est.bytes_min <= size <= est.bytes_max <= budget
    assert est.bytes_max == O.bytes_max(tol_used)
    # the container is mgh_compress(tol_used)'s
    ref = hl.compress(data, tol_used, s, mode, config=cfg)
    assert int(ref.numel() if hasattr(ref, "numel") else ref.size) == size
    a, b = hl.decompress(buf, config=cfg), hl.decompress(ref, config=cfg)
    a, b = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in (a, b))
    assert np.array_equal(a, b)
    assert hl.metadata_parse(bytes(buf.cpu().numpy() if hasattr(buf, "cpu") else buf))["tol"] == tol_used
    assert hl.verify(buf, data, config=cfg).within == 1
    # the next finer candidate of the last round does not fit
    nxt, = hl.estimate_sizes(data, [float(finer)], s, mode, config=cfg)
    assert nxt.bytes_max > budget, (nxt, budget)
    hl._hl().mgh_release_cache()


@pytest.mark.parametrize("name", sorted(BUDGET_SETUPS))
def test_budget_returns_tol_min_when_it_fits(name):
    torch, mg, hl = _gpu()
    shape, dt, rel, s, dict_size, block = BUDGET_SETUPS[name]
    u = smooth_field(shape, dt)
    cfg = _config(hl, block, dict_size)
    buf, tol_used, est = hl.compress_budget(u, u.nbytes + 4096, TOL_MIN, TOL_MAX, rounds=4, s=s,
                                            mode=mg.REL if rel else mg.ABS, config=cfg)
    assert tol_used == TOL_MIN and est.tol == TOL_MIN and est.bytes_min <= buf.size <= est.bytes_max <= u.nbytes + 4096
    hl._hl().mgh_release_cache()


# ---- 4. refusals ---------------------------------------------------------------------------------------------
def _budget_rc(hl, u, max_bytes, tol_min, tol_max, rounds, cfg, s=INF, mode=0):
    """The C call itself, output NOT pre-allocated: (status, output pointer, tol_used)."""
    import ctypes as C
    L = hl._hl()
    out, size, used = C.c_void_p(0xdead0), C.c_size_t(0), C.c_double(-1.0)
    shp = (C.c_uint64 * u.ndim)(*u.shape)
    rc = L.mgh_compress_budget(u.ndim, 0 if u.dtype == np.float32 else 1, shp, max_bytes, tol_min, tol_max, rounds, s,
                               mode, C.c_void_p(u.ctypes.data), C.byref(out), C.byref(size), None, C.byref(cfg), 0,
                               C.byref(used), None)
    return rc, out.value, used.value


def test_refusals_leave_the_library_usable():
    torch, mg, hl = _gpu()
    u = smooth_field(SMALL, F32)
    ok = _config(hl, None, 256)

    def round_trip():
        v = hl.decompress(hl.compress(u, 1e-3, INF, mg.REL, config=ok), config=ok)
        assert float(np.max(np.abs(v - u))) <= 1e-3 * float(np.max(np.abs(u)))

    # below the record's fixed part (decodebook of 256 entries alone: 3 KB): nothing allocated, pointer untouched
    rc, out, used = _budget_rc(hl, u, 1000, 1e-7, 1e-1, 4, ok)
    assert rc == MGH_ERR_OUTPUT_TOO_LARGE and out == 0xdead0 and used == -1.0
    round_trip()
    zstd = _config(hl, None, 256, lossless=hl.HUFFMAN_ZSTD)
    decomposing = _config(hl, None, 256, domain_decomposition=BLOCK, block_size=11)  # 3 x 2 x 2 subdomains
    for cfg in (zstd, decomposing):
        rc, out, _ = _budget_rc(hl, u, u.nbytes, 1e-7, 1e-1, 4, cfg)
        assert rc == MGH_ERR_INVALID_ARGUMENT and out == 0xdead0
        with pytest.raises(mg.MgardHipError, match="error %d: size estimates: " % MGH_ERR_INVALID_ARGUMENT):
            hl.estimate_sizes(u, [1e-3], config=cfg)
        round_trip()
    for tol_min, tol_max, rounds in ((0.0, 1e-1, 4), (-1e-3, 1e-1, 4), (1e-1, 1e-3, 4), (1e-7, 1e-1, 0), (1e-7, 1e-1, 9),
                                     (float("nan"), 1e-1, 4), (1e-7, INF, 4)):
        rc, out, _ = _budget_rc(hl, u, u.nbytes, tol_min, tol_max, rounds, ok)
        assert rc == MGH_ERR_INVALID_ARGUMENT and out == 0xdead0, (tol_min, tol_max, rounds)
    round_trip()
    for tols in ([], [1e-3] * 65):
        with pytest.raises(mg.MgardHipError, match="error %d" % MGH_ERR_INVALID_ARGUMENT):
            hl.estimate_sizes(u, tols, config=ok)
    round_trip()
    # a decomposing configuration still compresses the ordinary way
    v = hl.decompress(hl.compress(u, 1e-3, INF, mg.REL, config=decomposing), config=decomposing)
    assert float(np.max(np.abs(v - u))) <= 1e-3 * float(np.max(np.abs(u)))
    hl._hl().mgh_release_cache()
