"""Windowed full-grid preview of containers on the GPU (mgh_decompress_preview_window, mgh_progressive_preview_window).

Every window result must equal the crop of the expectation of tests/test_gpu_preview.py (the CPU oracle's recomposition
per subdomain, placed in the full array) and the crop of hl.decompress_preview of the same container. Bit patterns, no
tolerance. The containers are 66 x 40 x 34 cut at row 33 of dimension 0 (maxdim, variable), in 17-blocks (block), and
33 x 40 x 34 in one piece.
"""
import numpy as np
import pytest

from tests.test_gpu_coarsened import raw_records
from tests.test_gpu_preview import CASES, TOL, _cfg, _host, expectation
from tests.test_prolong_cpu import assert_same_bits
from tests.test_prolong_window_cpu import crop

pytestmark = pytest.mark.gpu


def windows(shape):
    """(name, lo, ext): the full array, a box inside one subdomain, a box across the border of dimension 0 (rows
    30 .. 36; the one-piece array has no border there, the rows are the last three), a plane on each side of the
    border (rows 32 and 33), a single node."""
    n0 = shape[0]
    rows = (30, 7) if n0 > 36 else (30, n0 - 30)
    return [("full", (0, 0, 0), tuple(shape)),
            ("inside", (3, 5, 7), (9, 11, 6)),
            ("across", (rows[0], 2, 1), (rows[1], 30, 33)),
            ("plane32", (32, 0, 0), (1, shape[1], shape[2])),
            ("plane33", (min(33, n0 - 1), 0, 0), (1, shape[1], shape[2])),
            ("node", (min(35, n0 - 1), 39, 33), (1, 1, 1))]


def _check_container(name, reorder, lossless):
    import torch
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    E = expectation(name)
    cfg = _cfg(name, lossless, reorder)
    for device_stream in (False, True):
        data = torch.from_numpy(E.u).cuda() if device_stream else E.u
        buf = hl.compress(data, TOL, np.inf, mg.REL, config=cfg)
        raw = raw_records(buf, E)
        for k in range(E.K + 1):
            full = _host(hl.decompress_preview(buf, k, config=cfg))
            for wname, lo, ext in windows(E.shape):
                got = hl.decompress_preview(buf, k, config=cfg, window=(lo, ext))
                assert isinstance(got, torch.Tensor) == device_stream
                got = _host(got)
                what = "%s reorder=%d %s coarsen=%d window %s, %s stream" % (
                    name, reorder, lossless, k, wname, "device" if device_stream else "host")
                assert got.shape == tuple(ext), what
                assert_same_bits(got, crop(E.preview(k, raw), lo, ext), what)
                assert_same_bits(got, crop(full, lo, ext), what + " against the crop of decompress_preview")


@pytest.mark.parametrize("reorder", [0, 1])
@pytest.mark.parametrize("name", ["one", "maxdim", "block", "variable"])
def test_container_windows(name, reorder):
    assert name in CASES
    _check_container(name, reorder, "Huffman")


def test_container_windows_huffman_zstd():
    _check_container("maxdim", 1, "Huffman_Zstd")


@pytest.mark.parametrize("reorder", [0, 1])
def test_statistics(reorder):
    """Only the subdomains under the window are opened: the counters are those of their records alone."""
    import torch
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    E = expectation("maxdim")
    cfg = _cfg("maxdim", "Huffman", reorder)
    assert len(E.subdomains) == 2
    for device_stream in (False, True):
        data = torch.from_numpy(E.u).cuda() if device_stream else E.u
        buf = hl.compress(data, TOL, np.inf, mg.REL, config=cfg)
        raw = raw_records(buf, E)
        for k in range(E.K + 1):
            hl.decompress_preview(buf, k, config=cfg)
            whole = hl.last_decompress_stats()
            assert whole["subdomains"] == 2
            per = []
            for j, (lo, ext) in enumerate((((3, 5, 7), (9, 11, 6)), ((40, 0, 0), (1, 40, 34)))):
                hl.decompress_preview(buf, k, config=cfg, window=(lo, ext))
                st = hl.last_decompress_stats()
                what = "reorder=%d coarsen=%d slab %d, device=%r: %r" % (reorder, k, j, device_stream, st)
                assert st["subdomains"] == 1, what
                assert 0 < st["record_bytes"] < whole["record_bytes"], what
                if reorder == 1 and k >= 1 and not any(raw):
                    assert st["chunks_decoded"] < st["chunks_total"], what
                per.append(st)
            # (the two slabs hold one record each: what the windows report one by one is what the full call reports)
            assert per[0]["record_bytes"] + per[1]["record_bytes"] == whole["record_bytes"], (per, whole)
            assert per[0]["chunks_total"] + per[1]["chunks_total"] == whole["chunks_total"], (per, whole)
            assert per[0]["chunks_decoded"] + per[1]["chunks_decoded"] == whole["chunks_decoded"], (per, whole)
            hl.decompress_preview(buf, k, config=cfg, window=((30, 2, 1), (7, 30, 33)))
            st = hl.last_decompress_stats()
            assert st["subdomains"] == 2 and st["record_bytes"] == whole["record_bytes"], st
            assert st["chunks_total"] == whole["chunks_total"] and st["chunks_decoded"] == whole["chunks_decoded"], st


@pytest.mark.parametrize("device_stream", [False, True], ids=["host", "device"])
def test_progressive_window(device_stream):
    import torch
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    E = expectation("one")
    cfg = _cfg("one", "Huffman", 1)
    data = torch.from_numpy(E.u).cuda() if device_stream else E.u
    buf = hl.compress(data, TOL, np.inf, mg.REL, config=cfg)
    _, L = hl.infer_level(buf, None, cfg)
    with hl.Progressive(buf, cfg) as p:
        with pytest.raises(hl.MgardHipError):
            p.preview(window=((0, 0, 0), (1, 1, 1)))
        for level in range(L + 1):
            a = _host(p.refine(level))
            assert_same_bits(a, _host(hl.decompress(buf, config=cfg, level=level)),
                             "refine(%d) after window previews against decompress(level)" % level)
            full = _host(p.preview())
            for wname, lo, ext in windows(E.shape):
                got = p.preview(window=(lo, ext))
                assert isinstance(got, torch.Tensor) == device_stream
                assert_same_bits(_host(got), crop(full, lo, ext), "level %d window %s" % (level, wname))
            assert p.level == level
        with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
            p.preview(window=((0, 0, 0), (34, 1, 1)))


def test_errors():
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    E = expectation("maxdim")
    cfg = _cfg("maxdim", "Huffman", 1)
    buf = hl.compress(E.u, TOL, np.inf, mg.REL, config=cfg)
    good = ((3, 5, 7), (9, 11, 6))
    with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
        hl.decompress_preview(buf, E.K + 1, config=cfg, window=good)
    for lo, ext in (((0, 0, 0), (67, 1, 1)), ((66, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, 0, 1)), ((0, 39, 0), (1, 2, 1))):
        out = np.full(ext, 7, np.float32) if min(ext) else None
        with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
            hl.decompress_preview(buf, 1, config=cfg, window=(lo, ext), out=out)
        assert out is None or (out == 7).all()
    with pytest.raises(ValueError):
        hl.decompress_preview(buf, 1, config=cfg, window=((0, 0), (1, 1)))
    got = hl.decompress_preview(buf, 1, config=cfg, window=good)
    assert_same_bits(got, crop(hl.decompress_preview(buf, 1, config=cfg), *good), "the library works afterwards")
