"""Full-grid preview of containers on the GPU (mgh_decompress_preview, mgh_progressive_preview).

The expectation is derived per subdomain as in tests/test_gpu_coarsened.py -- a Hierarchy of the block's shape,
decompose_quantize of the block with the ABS bound mgh_decompress uses for a subdomain -- and then, in place of the
level nodes, the WHOLE recomposition by the CPU oracle of the dequantized coefficients with everything outside the
corner box of level l_target_i - k zeroed, placed in the subdomain's box of the full array. Bit patterns, no tolerance.
"""
import itertools

import numpy as np
import pytest

import oracle
from tests.test_coarsened_cpu import BLOCK, MAXDIM, VARIABLE, blocks, steps_to_two
from tests.test_gpu_coarsened import local_tol, raw_records
from tests.test_prolong_cpu import assert_same_bits, zeroed
from tests.util import smooth_field

pytestmark = pytest.mark.gpu

TOL = 1e-3
HUFF_BLOCK = 2048  # (small enough that the head of every block below is fewer chunks than its record)

# name: (shape, decomposition, config keywords, expected dd_size or None for one subdomain)
CASES = {
    "one": ((33, 40, 34), None, {}, None),
    "maxdim": ((66, 40, 34), MAXDIM, dict(max_memory_footprint=40 * 66 * 40 * 34), 33),
    "block": ((66, 40, 34), BLOCK, dict(block_size=17), 17),
    "variable": ((66, 40, 34), VARIABLE, dict(domain_decomposition_dim=0, domain_decomposition_sizes=[33, 33]), 33),
}


def _cfg(name, lossless="Huffman", reorder=0):
    from mgard_amd import highlevel as hl
    _, method, kw, _ = CASES[name]
    extra = {} if method is None else dict(domain_decomposition=method)
    return hl.Config(reorder=reorder, huff_block_size=HUFF_BLOCK,
                     lossless=hl.HUFFMAN if lossless == "Huffman" else hl.HUFFMAN_ZSTD, **extra, **kw)


class Expectation:
    def __init__(self, name):
        import torch
        import mgard_amd as mg
        from mgard_amd import highlevel as hl
        shape, method, kw, dd_size = CASES[name]
        self.shape, self.dt = shape, np.float32
        self.u = smooth_field(shape, np.float32)
        if method is None:
            self.subdomains = [tuple((0, n) for n in shape)]
        else:
            dim = kw.get("domain_decomposition_dim", int(np.argmax(shape)))
            grid = blocks(shape, (method, dim, dd_size), kw.get("domain_decomposition_sizes"))
            self.subdomains = list(itertools.product(*grid))
        self.K = min(steps_to_two(e) for box in self.subdomains for _, e in box)
        buf = hl.compress(self.u, TOL, np.inf, mg.REL, config=_cfg(name))
        meta = hl.metadata_parse(bytes(buf[:65536]))
        assert meta["domain_decomposed"] is (method is not None)
        self.norm = meta["norm"]
        nsub = len(self.subdomains)
        self.ltol = local_tol(np.float32, True, TOL, np.inf, self.norm, nsub) if method is not None else None
        # per subdomain: its box, its data, and the dequantized coefficients of a Huffman record (dictionary) and of
        # a RAW record (stored as the data: below full resolution it goes through integers without a dictionary)
        self.sub = []
        for box in self.subdomains:
            sl = tuple(slice(o, o + e) for o, e in box)
            bshape = tuple(e for _, e in box)
            blk = np.ascontiguousarray(self.u[sl])
            h = mg.Hierarchy(bshape, np.float32)
            O = oracle.Hierarchy(bshape, np.float32)
            eb, tol = (mg.ABS, float(self.ltol)) if method is not None else (mg.REL, TOL)
            q, oi, ov, n, _ = h.decompose_quantize(torch.from_numpy(blk).cuda(), eb, tol, np.inf, self.norm)
            c = O.dequantize(q.cpu().numpy(), eb, np.float32(tol), np.float32(np.inf), np.float32(self.norm),
                             outlier_idx=oi.cpu().numpy(), outlier_val=ov.cpu().numpy())
            q0 = h.decompose_quantize(torch.from_numpy(blk).cuda(), eb, tol, np.inf, self.norm, prep_huffman=False)[0]
            c0 = O.dequantize(q0.cpu().numpy(), eb, np.float32(tol), np.float32(np.inf), np.float32(self.norm),
                              prep_huffman=False)
            self.sub.append((sl, O, blk, c, c0))
            h.close()
        self._made = {}

    def preview(self, k, raw):
        """The expected array for `k` halvings of a container whose records are raw where `raw` says so."""
        key = (k, tuple(raw))
        if key not in self._made:
            full = np.empty(self.shape, np.float32)
            for (sl, O, blk, c, c0), is_raw in zip(self.sub, raw):
                if is_raw and k == 0:
                    full[sl] = blk
                else:
                    full[sl] = O.recompose(zeroed(O, c0 if is_raw else c, O.l_target - k))
            self._made[key] = full
        return self._made[key]


_EXPECT = {}


def expectation(name):
    if name not in _EXPECT:
        _EXPECT[name] = Expectation(name)
    return _EXPECT[name]


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


@pytest.mark.parametrize("lossless", ["Huffman", "Huffman_Zstd"])
@pytest.mark.parametrize("reorder", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_decompress_preview(name, reorder, lossless):
    import torch
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    E = expectation(name)
    cfg = _cfg(name, lossless, reorder)
    for device_stream in (False, True):
        data = torch.from_numpy(E.u).cuda() if device_stream else E.u
        buf = hl.compress(data, TOL, np.inf, mg.REL, config=cfg)
        raw = raw_records(buf, E)
        print("%s reorder=%d %s: raw records %r" % (name, reorder, lossless, raw))
        full = _host(hl.decompress(buf, config=cfg))
        total = None
        for k in range(E.K + 1):
            got = hl.decompress_preview(buf, k, config=cfg)
            st = hl.last_decompress_stats()
            assert isinstance(got, torch.Tensor) == device_stream
            got = _host(got)
            what = "%s reorder=%d %s coarsen=%d, %s stream" % (name, reorder, lossless, k,
                                                              "device" if device_stream else "host")
            assert got.shape == E.shape
            if k == 0:
                assert_same_bits(got, full, what + " against decompress")
                total = st["chunks_total"]
                assert st["chunks_decoded"] == total
            assert_same_bits(got, E.preview(k, raw), what)
            assert st["subdomains"] == len(E.subdomains)
            if reorder == 1 and k >= 1 and not any(raw):
                print(what, st)
                assert st["chunks_decoded"] < st["chunks_total"] == total, (what, st)
        with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
            hl.decompress_preview(buf, E.K + 1, config=cfg)
    with pytest.raises(ValueError):
        hl.decompress_preview(buf, None, config=cfg)


def test_raw_record():
    """Noise at a bound below it does not compress: both slabs are stored raw; a preview goes through the integers
    of the subdomain's bound (no dictionary)."""
    import torch
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    shape = (66, 34, 33)
    u = np.random.default_rng(5).standard_normal(shape).astype(np.float32)
    tol = 1e-7
    cfg = hl.Config(domain_decomposition=hl.DD_VARIABLE, domain_decomposition_dim=0, domain_decomposition_sizes=[33, 33])
    buf = hl.compress(u, tol, np.inf, mg.REL, config=cfg)
    meta = hl.metadata_parse(bytes(buf[:4096]))
    assert buf.size - meta["metadata_size"] - 2 * 8 == u.nbytes, "the records are not raw"
    assert np.array_equal(hl.decompress_preview(buf, 0, config=cfg), u)
    ltol = local_tol(np.float32, True, tol, np.inf, meta["norm"], 2)
    for k in (1, 2):
        parts = []
        for j in range(2):
            h = mg.Hierarchy((33, 34, 33), np.float32)
            O = oracle.Hierarchy((33, 34, 33), np.float32)
            blk = torch.from_numpy(np.ascontiguousarray(u[33 * j:33 * j + 33])).cuda()
            q, oi, ov, n, _ = h.decompose_quantize(blk, mg.ABS, float(ltol), np.inf, meta["norm"], prep_huffman=False)
            c = O.dequantize(q.cpu().numpy(), mg.ABS, np.float32(ltol), np.float32(np.inf), np.float32(meta["norm"]),
                             prep_huffman=False)
            parts.append(O.recompose(zeroed(O, c, O.l_target - k)))
            h.close()
        for dev in (False, True):
            b = torch.from_numpy(buf).cuda() if dev else buf
            got = _host(hl.decompress_preview(b, k, config=cfg))
            assert_same_bits(got, np.concatenate(parts, axis=0), "raw records, coarsen=%d, device=%r" % (k, dev))


@pytest.mark.parametrize("device_stream", [False, True], ids=["host", "device"])
def test_progressive_preview(device_stream):
    import torch
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    E = expectation("one")
    cfg = _cfg("one", "Huffman", 1)
    data = torch.from_numpy(E.u).cuda() if device_stream else E.u
    buf = hl.compress(data, TOL, np.inf, mg.REL, config=cfg)
    _, L = hl.infer_level(buf, None, cfg)
    assert L == E.K
    with hl.Progressive(buf, cfg) as p, hl.Progressive(buf, cfg) as plain:
        with pytest.raises(hl.MgardHipError):
            p.preview()
        for level in range(L + 1):
            a = _host(p.refine(level))
            b = _host(plain.refine(level))
            assert_same_bits(a, b, "refine(%d) after a preview against a reader that never previewed" % level)
            got = p.preview()
            assert isinstance(got, torch.Tensor) == device_stream
            got = _host(got)
            assert_same_bits(got, _host(hl.decompress_preview(buf, L - level, config=cfg)),
                             "preview at level %d against the one-shot preview" % level)
            assert_same_bits(got, E.preview(L - level, raw_records(buf, E)), "preview at level %d" % level)
            assert p.level == level
