"""mgh_lossless_decompress on damaged records that the host-side parser (mgard_amd/csrc/huffman_record.hpp)
refuses before anything is launched: MGH_ERR_FORMAT for a record in host memory and for the same bytes in
device memory, and the context decodes a sound record afterwards. (What the parser makes of every kind of
damage is pinned on the CPU: tests/test_huffman_record_cpu.py.)"""
import struct

import numpy as np
import pytest

from tests import payload as pl

pytestmark = pytest.mark.gpu


def test_records_refused_by_the_host_parse_on_both_placements():
    import torch
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    n, chunk, dict_size = 3 * 1024 + 77, 1024, 8192
    rng = np.random.default_rng(5)
    q = np.clip(np.rint(4096 + 40 * rng.standard_normal(n)), 0, dict_size - 1).astype(np.int64)
    oi = np.array([0, n // 2, n - 1], dtype=np.int64)
    ov = np.array([-70000, 123456, 8192], dtype=np.int64)
    q[oi] = 0
    ctx = hl.Lossless()
    rec = ctx.compress(torch.from_numpy(q).cuda(), dict_size, chunk, hl.HUFFMAN, 3, torch.from_numpy(oi).cuda(),
                       torch.from_numpy(ov).cuda())
    r = pl.parse_huffman_record(rec)
    nchunk, units = len(r["bits"]), len(r["units"])
    assert nchunk == 4 and r["sync"] is not None and len(r["outlier_idx"]) == 3
    ddata = 24 + 16 * nchunk + 8 + 8 * 128 + 8 * dict_size + 8
    lists_end = ddata + 8 * units + 8 + 16 * 3

    def put(off, value):
        b = bytearray(rec)
        struct.pack_into("<Q", b, off, value)
        return bytes(b)

    def check_clean():
        for placed in (rec, torch.from_numpy(np.frombuffer(rec, np.uint8).copy()).cuda()):
            back, bi, bv = ctx.decompress(placed, n)
            assert np.array_equal(back.cpu().numpy(), q)
            assert np.array_equal(bi.cpu().numpy(), oi) and np.array_equal(bv.cpu().numpy(), ov)

    check_clean()
    damaged = {
        "cut inside the fixed header": rec[:20],
        "cut inside the decodebook": rec[:ddata - 4000],
        "primary_count is not n": put(0, n + 1),
        "entry[0] past the stream": put(24 + 8 * nchunk, units + 1),
        # 8 bytes short of the end of the outlier lists: 8 (mod 16) behind the count, too few for the section
        "a remainder that fits neither the lists nor the section": rec[:lists_end - 8],
    }
    for what, bad in damaged.items():
        for placed in (bad, torch.from_numpy(np.frombuffer(bad, np.uint8).copy()).cuda()):
            with pytest.raises(mg.MgardHipError, match=r"error -8\b"):
                ctx.decompress(placed, n)
    check_clean()
    ctx.close()
