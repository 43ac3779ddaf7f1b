"""Reduced resolution of domain-decomposed containers on the GPU (mgh_decompress_coarsened).

The expectation is stitched in the test from calls that are pinned elsewhere (tests/test_gpu_multires.py,
tests/test_gpu_reference_binary.py): per subdomain a Hierarchy of the block's shape (and the block's slice of the
coordinates), decompose_quantize of the block with the ABS bound mgh_decompress uses for a subdomain, and
dequantize_recompose(level = l_target_i - k). The blocks are placed by the geometry tests/test_coarsened_cpu.py
restates. The result must equal that bit for bit, from a host and from a device stream, for every k in 0 .. K.
Every block is also held against the CPU oracle's level values within its local bound.
"""
import itertools

import numpy as np
import pytest

import oracle
from tests.test_coarsened_cpu import BLOCK, MAXDIM, VARIABLE, blocks, keep, steps_to_two
from tests.test_gpu_multires import assert_bit_equal
from tests.test_multires_cpu import expected_level
from tests.util import nonuniform_coords, smooth_field

pytestmark = pytest.mark.gpu

TOL = 1e-3

# name: (shape, dtype, non-uniform, decomposition, config keywords, expected dd_size, K, REL?, s)
CASES = {
    "maxdim0": ((129, 64, 65), np.float32, False, MAXDIM, dict(max_memory_footprint=40 * 129 * 64 * 65), 65, 6, True, np.inf),
    "maxdim1": ((40, 130, 33), np.float32, False, MAXDIM, dict(max_memory_footprint=40 * 40 * 130 * 33), 65, 5, True, np.inf),
    "block": ((70, 45, 37), np.float32, False, BLOCK, dict(block_size=33), 33, 2, True, np.inf),
    "variable-f64-nonuniform": ((65, 70, 129), np.float64, True, VARIABLE,
                                dict(domain_decomposition_dim=2, domain_decomposition_sizes=[65, 64]), 65, 6, True, np.inf),
    "variable-4d": ((9, 8, 10, 34), np.float32, False, VARIABLE,
                    dict(domain_decomposition_dim=3, domain_decomposition_sizes=[17, 17]), 17, 3, True, np.inf),
    "maxdim0-rel-s0": ((129, 64, 65), np.float32, False, MAXDIM, dict(max_memory_footprint=40 * 129 * 64 * 65), 65, 6, True, 0.0),
}


def _cfg(name, lossless="Huffman", reorder=0):
    from mgard_amd import highlevel as hl
    method, kw = CASES[name][3], CASES[name][4]
    return hl.Config(domain_decomposition=method, reorder=reorder,
                     lossless=hl.HUFFMAN if lossless == "Huffman" else hl.HUFFMAN_ZSTD, **kw)


def local_tol(dt, rel, tol, s, norm, nsub):
    """calc_local_abs_tol in the data type's precision."""
    t, nrm = dt(tol), dt(norm)
    if rel:
        if np.isinf(s):
            return t * nrm
        return np.sqrt((t * nrm) * (t * nrm) / dt(nsub))
    if np.isinf(s):
        return t
    return np.sqrt((t * t) / dt(nsub))


class Expectation:
    """Everything of a case that does not depend on reorder / lossless / where the stream lives: computed once."""

    def __init__(self, name):
        import torch
        import mgard_amd as mg
        from mgard_amd import highlevel as hl
        shape, dt, nonuniform, method, kw, dd_size, K, rel, s = CASES[name]
        self.shape, self.dt, self.K, self.rel, self.s = shape, dt, K, rel, s
        self.coords = nonuniform_coords(shape, dt, seed=sum(shape)) if nonuniform else None
        self.u = smooth_field(shape, dt)
        sizes = kw.get("domain_decomposition_sizes")
        dim = kw.get("domain_decomposition_dim", int(np.argmax(shape)))
        self.grid = blocks(shape, (method, dim, dd_size), sizes)
        assert min(steps_to_two(e) for g in self.grid for _, e in g) == K
        self.subdomains = list(itertools.product(*self.grid))  # row-major over the decomposition grid
        # the norm of the header: what the compressor computed
        cfg = _cfg(name)
        buf = hl.compress(self.u, TOL, s, mg.REL if rel else mg.ABS, coords=self.coords, config=cfg)
        meta = hl.metadata_parse(bytes(buf[:65536]))
        self.norm = meta["norm"]
        self.ltol = local_tol(dt, rel, TOL, s, self.norm, len(self.subdomains))
        self.per_k = [[None] * len(self.subdomains) for _ in range(K + 1)]
        self.oracle_k = [[None] * len(self.subdomains) for _ in range(K + 1)]
        for i, box in enumerate(self.subdomains):
            sl = tuple(slice(o, o + e) for o, e in box)
            bshape = tuple(e for _, e in box)
            bcoords = None if self.coords is None else [c[o:o + e] for c, (o, e) in zip(self.coords, box)]
            blk = np.ascontiguousarray(self.u[sl])
            h = mg.Hierarchy(bshape, dt, coords=bcoords)
            o = oracle.Hierarchy(bshape, dt, coords=bcoords)
            assert h.l_target == o.l_target >= K
            q, oi, ov, n, _ = h.decompose_quantize(torch.from_numpy(blk).cuda(), mg.ABS, float(self.ltol), float(s),
                                                   self.norm)
            c = o.decompose(blk)
            for k in range(K + 1):
                lvl = h.l_target - k
                want = h.dequantize_recompose(q.clone(), mg.ABS, float(self.ltol), float(s), self.norm,
                                              outlier_idx=oi, outlier_val=ov, level=lvl)
                assert tuple(want.shape) == tuple(len(keep(e, k)) for e in bshape)
                self.per_k[k][i] = want.cpu().numpy()
                self.oracle_k[k][i] = expected_level(o, c, lvl)
            h.close()

    def stitch(self, parts):
        return np.block(_nest([p for p in parts], [len(g) for g in self.grid]))


def _nest(flat, counts):
    if len(counts) == 1:
        return list(flat)
    step = len(flat) // counts[0]
    return [_nest(flat[j * step:(j + 1) * step], counts[1:]) for j in range(counts[0])]


_EXPECT = {}


def expectation(name):
    if name not in _EXPECT:
        _EXPECT[name] = Expectation(name)
    return _EXPECT[name]


def _compress(name, E, lossless, reorder, device_stream):
    import torch
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    cfg = _cfg(name, lossless, reorder)
    data = torch.from_numpy(E.u).cuda() if device_stream else E.u
    buf = hl.compress(data, TOL, E.s, mg.REL if E.rel else mg.ABS, coords=E.coords, config=cfg)
    head = buf[:65536].cpu().numpy() if device_stream else buf[:65536]
    meta = hl.metadata_parse(bytes(head))
    assert meta["domain_decomposed"] is True and meta["dd_size"] == CASES[name][5], meta
    assert meta["dd_method"] == CASES[name][3] and meta["norm"] == E.norm
    return buf, cfg


def raw_records(buf, E):
    """Per subdomain: is its record the data itself? (GPUPipelines.hpp:414-417: a record that is not smaller than
    the subdomain is replaced by it, so a raw record has exactly the subdomain's bytes.) mgh_decompress returns
    such a subdomain as it is; below full resolution it goes through the integers of the subdomain's bound."""
    from mgard_amd import highlevel as hl
    host = buf.cpu().numpy() if hasattr(buf, "cpu") else buf
    at = hl.metadata_parse(bytes(host[:65536]))["metadata_size"]
    flags = []
    for box in E.subdomains:
        size = int(np.frombuffer(bytes(host[at:at + 8]), dtype=np.uint64)[0])
        flags.append(size == int(np.prod([e for _, e in box])) * np.dtype(E.dt).itemsize)
        at += 8 + size
    assert at == host.size
    return flags


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


@pytest.mark.parametrize("lossless", ["Huffman", "Huffman_Zstd"])
@pytest.mark.parametrize("reorder", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_decompress_coarsened(name, reorder, lossless):
    import torch
    from mgard_amd import highlevel as hl
    E = expectation(name)
    K = E.K
    for device_stream in (False, True):
        buf, cfg = _compress(name, E, lossless, reorder, device_stream)
        assert hl.infer_coarsened(buf, None, cfg) == (None, K)
        full = _host(hl.decompress(buf, config=cfg))
        raw = raw_records(buf, E)
        print("%s: raw records %r" % (name, raw))
        if name.startswith("maxdim0"):
            assert not any(raw)  # (at least these slabs are Huffman records for certain: large and smooth)
        data = [np.ascontiguousarray(E.u[tuple(slice(o, o + e) for o, e in box)]) for box in E.subdomains]
        for k in range(K + 1):
            # full resolution of a raw record is the data; everything else comes from the integers
            want = E.stitch([data[i] if (k == 0 and raw[i]) else E.per_k[k][i] for i in range(len(raw))])
            shape, _ = hl.infer_coarsened(buf, k, cfg)
            assert shape == want.shape
            got = hl.decompress(buf, config=cfg, coarsen=k)
            assert isinstance(got, torch.Tensor) == device_stream
            got = _host(got)
            what = "%s, coarsen=%d, %s stream" % (name, k, "device" if device_stream else "host")
            if k == 0:
                assert_bit_equal(got, full, what + " against decompress")
            assert_bit_equal(got, want, what)
            # every block against the oracle's level values, within the bound of the subdomain
            ix = [hl.infer_coarsened_nodes(buf, k, d, cfg) for d in range(len(E.shape))]
            assert tuple(len(x) for x in ix) == shape
            ref = E.stitch(E.oracle_k[k])
            err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
            if np.isinf(E.s):
                print("%s: max error %.3e, local bound %.3e" % (what, err.max(), E.ltol))
                assert err.max() <= E.ltol, (what, err.max(), E.ltol)
            else:
                # s = 0: the bound is on the L2 norm of the error of a subdomain (oracle.norm, unit cube)
                off = [np.cumsum([0] + [len(keep(e, k)) for _, e in g]) for g in E.grid]
                for sid in itertools.product(*[range(len(g)) for g in E.grid]):
                    sl = tuple(slice(o[j], o[j + 1]) for o, j in zip(off, sid))
                    e2 = oracle.norm(np.ascontiguousarray(err[sl]), 0.0, True)
                    print("%s block %r: L2 error %.3e, local bound %.3e" % (what, sid, e2, E.ltol))
                    assert e2 <= E.ltol, (what, sid, e2, E.ltol)
        with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
            hl.decompress(buf, config=cfg, coarsen=K + 1)
        assert_bit_equal(_host(hl.decompress(buf, config=cfg)), full, "the library after the refusal")


def test_block_has_twelve_subdomains_and_refuses_three_halvings():
    from mgard_amd import highlevel as hl
    E = expectation("block")
    assert len(E.subdomains) == 12 and E.K == 2
    buf, cfg = _compress("block", E, "Huffman", 0, False)
    with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
        hl.decompress(buf, config=cfg, coarsen=3)
    hl.decompress(buf, config=cfg, coarsen=2)
    assert hl.last_decompress_stats()["subdomains"] == 12


@pytest.mark.parametrize("device_stream", [False, True], ids=["host", "device"])
def test_only_the_heads_are_decoded(device_stream):
    """reorder = 1, two halvings of two slabs of 65 and 64 planes: a head of 17 x 17 x 17 integers per block is
    one 20480-symbol chunk."""
    from mgard_amd import highlevel as hl
    E = expectation("maxdim0")
    buf, cfg = _compress("maxdim0", E, "Huffman", 1, device_stream)
    assert 17 ** 3 <= int(cfg.huff_block_size)
    got = _host(hl.decompress(buf, config=cfg, coarsen=2))
    st = hl.last_decompress_stats()
    print(st)
    assert_bit_equal(got, E.stitch(E.per_k[2]), "coarsen=2")
    assert st["subdomains"] == 2
    assert st["chunks_decoded"] == 2 and st["chunks_total"] > 2
    if not device_stream:
        assert st["record_bytes_moved"] < st["record_bytes"]
    hl.decompress(buf, config=cfg)
    full = hl.last_decompress_stats()
    assert full["subdomains"] == 2 and full["chunks_decoded"] == full["chunks_total"] == st["chunks_total"]


def test_raw_records():
    """Noise at a bound below it does not compress: both slabs are stored raw."""
    import torch
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    shape = (66, 34, 33)
    u = np.random.default_rng(5).standard_normal(shape).astype(np.float32)
    tol = 1e-7
    cfg = hl.Config(domain_decomposition=hl.DD_VARIABLE, domain_decomposition_dim=0, domain_decomposition_sizes=[33, 33])
    buf = hl.compress(u, tol, np.inf, mg.REL, config=cfg)
    meta = hl.metadata_parse(bytes(buf[:4096]))
    assert meta["domain_decomposed"] is True and meta["dd_size"] == 33
    assert buf.size - meta["metadata_size"] - 2 * 8 == u.nbytes, "the records are not raw"
    assert_bit_equal(hl.decompress(buf, config=cfg, coarsen=0), hl.decompress(buf, config=cfg), "coarsen=0")
    assert np.array_equal(hl.decompress(buf, config=cfg, coarsen=0), u)
    ltol = local_tol(np.float32, True, tol, np.inf, meta["norm"], 2)
    parts = []
    for j in range(2):
        h = mg.Hierarchy((33, 34, 33), np.float32)
        blk = torch.from_numpy(np.ascontiguousarray(u[33 * j:33 * j + 33])).cuda()
        q, oi, ov, n, _ = h.decompose_quantize(blk, mg.ABS, float(ltol), np.inf, meta["norm"], prep_huffman=False)
        parts.append(h.dequantize_recompose(q, mg.ABS, float(ltol), np.inf, meta["norm"], prep_huffman=False,
                                            level=h.l_target - 1).cpu().numpy())
    assert_bit_equal(hl.decompress(buf, config=cfg, coarsen=1), np.concatenate(parts, axis=0), "raw records, coarsen=1")


def test_wrong_output_size_writes_nothing():
    import torch
    from mgard_amd import highlevel as hl
    E = expectation("maxdim1")
    buf, cfg = _compress("maxdim1", E, "Huffman", 0, False)
    shape, _ = hl.infer_coarsened(buf, 1, cfg)
    out = np.full(int(np.prod(shape)) + 1, 7.0, dtype=np.float32)
    with pytest.raises(ValueError):
        hl.decompress(buf, config=cfg, coarsen=1, out=out)
    assert np.all(out == 7.0)
    dbuf = torch.from_numpy(buf).cuda()
    dout = torch.full((int(np.prod(shape)) - 1,), 7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        hl.decompress(dbuf, config=cfg, coarsen=1, out=dout)
    assert bool(torch.all(dout == 7.0))
    good = np.empty(shape, dtype=np.float32)
    assert hl.decompress(buf, config=cfg, coarsen=1, out=good) is good
    assert_bit_equal(good, E.stitch(E.per_k[1]), "pre-allocated output")


@pytest.mark.parametrize("reorder", [0, 1])
def test_one_subdomain_is_decompress_level(reorder):
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    u = smooth_field((33, 40, 65), np.float32)
    cfg = hl.Config(reorder=reorder)
    buf = hl.compress(u, TOL, np.inf, mg.REL, config=cfg)
    assert hl.metadata_parse(bytes(buf[:4096]))["domain_decomposed"] is False
    _, L = hl.infer_level(buf, None, cfg)
    assert hl.infer_coarsened(buf, None, cfg) == (None, L)
    for k in range(L + 1):
        assert_bit_equal(hl.decompress(buf, config=cfg, coarsen=k), hl.decompress(buf, config=cfg, level=L - k),
                         "coarsen=%d against level=%d" % (k, L - k))
