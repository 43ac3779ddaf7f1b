"""The 16-bit-symbol instantiations of the Huffman stage -- k_histogram<uint16_t>, k_encode_chain<uint16_t, uint32_t>
(and <uint16_t, uint64_t>), k_decode_ring<uint16_t>, k_decode_sync<uint16_t> -- driven directly through
mgh_lossless_compress[_device]_sym16 / mgh_lossless_decompress_sym16 on the streams the int64 tests were written
for: codes past the root table, past root + 11 bits and past 27 bits, sorted streams, one symbol, the whole
dictionary, tail chunks of one symbol, odd chunk lengths (2-byte aligned chunk starts in the output).

Everything is bit for bit, against two things that do not go through the code under test: the independent reader of
tests/payload.py (parse, decode, recomputed synchronisation points) and the record the int64 entry writes from the
same values, which the int64 tests pin. Output buffers carry 64 guard elements holding a marker.

CASES is the table; the 65535 / 65536 / 70000 rows are written WITHOUT a synchronisation section (the encoder
writes one for chunks of at most 20480 symbols, size_plan.hpp: record_has_sync), so the `chunk <= 65535` edge of
decode_plan is met with a section appended here: the recomputed points at 65535, where the decoder uses them, and
entries of all ones at 65536 and 70000, where it must not look at them."""
import contextlib
import ctypes
import functools
import os
import struct

import numpy as np
import pytest

from tests import payload as pl
from tests.util import huffman_symbols

pytestmark = pytest.mark.gpu

MARK = 0xA5A5  # what guard elements hold
GUARD = 64
PY_MAX = 40000  # symbols the independent (bit-serial) decoder is given


def _mods():
    import torch
    import mgard_amd
    from mgard_amd import highlevel as hl
    return torch, mgard_amd, hl


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f


def _fib_stream(k):
    """Symbol 100 + j occurs fib(j) times, rarest first: the deepest Huffman tree a histogram of this size gives."""
    return np.concatenate([np.full(f, 100 + j, np.int64) for j, f in enumerate(_fib(k))])


# id -> (stream, dict, chunk, n)
CASES = {
    "normal60": ("normal60", 8192, 20480, 3 * 20480 + 777),
    "normal8-tail1": ("normal8", 8192, 20480, 2 * 20480 + 1),
    "narrow": ("narrow", 8192, 20480, 3 * 20480),
    "sorted": ("sorted", 8192, 20480, 2 * 20480 + 5),
    "uniform4096": ("uniform4096", 8192, 4096, 50001),
    "fib24-chunk1025": ("fib24", 8192, 1025, 121392),
    "fib31-rarest-first": ("fib31o", 8192, 2048, 3524577),
    "fib31-permuted": ("fib31p", 8192, 2048, 3524577),
    "single": ("single", 8192, 1024, 5000),
    "full-8192-1024": ("full", 8192, 1024, 3 * 8192),
    "full-8192-3333": ("full", 8192, 3333, 3 * 8192),
    "full-16384-1024": ("full", 16384, 1024, 3 * 16384),
    "full-16384-3333": ("full", 16384, 3333, 3 * 16384),
    "dict64-chunk65535": ("normal10", 64, 65535, 2 * 65535 + 9),
    "dict64-chunk65536": ("normal10", 64, 65536, 2 * 65536 + 9),
    "dict64-chunk70000": ("normal10", 64, 70000, 2 * 70000 + 9),
    "n1": ("edges", 1024, 1024, 1),
    "n1024": ("edges", 1024, 1024, 1024),
    "n1025": ("edges", 1024, 1024, 1025),
}
RANGE_CASES = ["fib24-chunk1025", "full-8192-3333"]  # several chunks, odd chunk length
SWITCHES = [("1", "2"), ("1", "0"), ("1", "1"), ("0", "1")]  # (MGH_HUFF_SYNC_DECODE, MGH_HUFF_PAIR)
TABLE_BITS = ["8", None, "14"]  # MGH_HUFF_TB


@functools.lru_cache(maxsize=None)
def _case(name):
    """(q int64 read-only, q16, dict, chunk, outlier_idx, outlier_val) of a row of CASES."""
    stream, dict_size, chunk, n = CASES[name]
    rng = np.random.default_rng(11)
    if stream == "normal60":
        q = huffman_symbols(n, width=60.0)
        # symbol 0 and symbol dict - 1 at the first and last position of chunks
        q[0], q[chunk - 1], q[chunk], q[2 * chunk - 1], q[3 * chunk], q[n - 1] = 0, dict_size - 1, dict_size - 1, 0, 0, dict_size - 1
    elif stream == "normal8":
        q = huffman_symbols(n, width=8.0)
    elif stream == "narrow":
        q = huffman_symbols(n, width=0.4)
    elif stream == "sorted":
        q = np.sort(huffman_symbols(n, width=300.0))
    elif stream == "uniform4096":
        q = rng.integers(2048, 2048 + 4096, n).astype(np.int64)
    elif stream == "fib24":
        q = rng.permutation(_fib_stream(24))
    elif stream == "fib31o":
        q = _fib_stream(31)
    elif stream == "fib31p":
        q = np.random.default_rng(5).permutation(_fib_stream(31))
    elif stream == "single":
        q = np.full(n, 4096, np.int64)
    elif stream == "full":
        q = np.arange(dict_size, dtype=np.int64).repeat(3)
    elif stream == "normal10":
        q = huffman_symbols(n, width=10.0, dict_size=dict_size)
        q[0], q[chunk - 1], q[chunk], q[n - 1] = dict_size - 1, 0, 0, dict_size - 1
    else:  # n = 1, n = chunk, n = chunk + 1 (the tail chunk is symbol 0 alone)
        q = huffman_symbols(n, width=30.0, dict_size=dict_size)
        q[0], q[min(n, chunk) - 1], q[n - 1] = dict_size - 1, dict_size - 1, 0 if n > chunk else dict_size - 1
    assert q.shape == (n,) and q.dtype == np.int64 and 0 <= q.min() and q.max() < dict_size
    q16 = q.astype(np.uint16)
    oi = np.unique(np.array([1, n // 3], dtype=np.int64).clip(0, n - 1))
    ov = np.array([-5, 99999][:len(oi)], dtype=np.int64)
    for a in (q, q16, oi, ov):
        a.flags.writeable = False
    return q, q16, dict_size, chunk, oi, ov


@contextlib.contextmanager
def _env(**kw):
    """MGH_* switches for the block (None: unset), put back afterwards."""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_ctx = None


def _context():
    """One lossless context for the module (the refusal test wants a context that has seen other work)."""
    global _ctx
    if _ctx is None:
        _ctx = _mods()[2].Lossless()
    return _ctx


def _dev16(torch, a16):
    """uint16 values as a cuda int16 tensor (the same two bytes; torch compares int16 on the device)."""
    return torch.from_numpy(np.ascontiguousarray(a16).view(np.int16).copy()).cuda()


def _marked(torch, n):
    return _dev16(torch, np.full(n, MARK, np.uint16))


@functools.lru_cache(maxsize=None)
def _records(name):
    """(record from q16, the same written with MGH_HUFF_SYNC=0, record from q by the int64 entry, that with
    MGH_HUFF_SYNC=0): bytes. Written once per case and shared."""
    torch, mg, hl = _mods()
    q, q16, dict_size, chunk, oi, ov = _case(name)
    ctx = _context()
    d64, d16 = torch.from_numpy(q.copy()).cuda(), _dev16(torch, q16)
    args = (dict_size, chunk, hl.HUFFMAN, 3, torch.from_numpy(oi.copy()).cuda(), torch.from_numpy(ov.copy()).cuda())
    with _env(MGH_HUFF_SYNC="1"):
        rec16, rec64 = ctx.compress(d16, *args), ctx.compress(d64, *args)
    with _env(MGH_HUFF_SYNC="0"):
        plain16, plain64 = ctx.compress(d16, *args), ctx.compress(d64, *args)
    return rec16, plain16, rec64, plain64


def _with_section(rec, entries):
    """A record without a synchronisation section, with one appended."""
    assert pl.parse_huffman_record(rec)["sync"] is None
    return rec + struct.pack("<Q", pl.SYNC_TAG) + np.ascontiguousarray(entries, dtype="<u4").tobytes()


# ---- (a) the record is the one the int64 entry writes ------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_record_from_16_bit_symbols_is_the_int64_entrys_record(name):
    torch, mg, hl = _mods()
    q, q16, dict_size, chunk, oi, ov = _case(name)
    rec16, plain16, rec64, plain64 = _records(name)
    assert rec16 == rec64 and plain16 == plain64
    r = pl.parse_huffman_record(rec16)
    assert (r["primary_count"], r["dict_size"], r["chunk_size"]) == (q.size, dict_size, chunk)
    assert pl.parse_huffman_record(plain16)["sync"] is None and rec16[:len(plain16)] == plain16
    # the section: 4 bits per symbol or more, chunks the encoder keeps in registers (size_plan.hpp: record_has_sync)
    bits = int(r["bits"].astype(np.int64).sum())
    assert (r["sync"] is not None) == (1024 <= chunk <= 20480 and bits >= 4 * q.size), (bits, q.size)
    if name == "narrow" or name.startswith("dict64"):
        assert r["sync"] is None
    if name in ("normal60", "sorted", "uniform4096", "normal8-tail1", "full-8192-3333", "n1024", "n1025"):
        assert r["sync"] is not None
    ctx = _context()
    d16 = _dev16(torch, q16)
    d_oi, d_ov = torch.from_numpy(oi.copy()).cuda(), torch.from_numpy(ov.copy()).cuda()
    # symbols at an address that is only 2-byte aligned: the kernels' element-wise reads instead of 16-byte ones
    shifted = _dev16(torch, np.concatenate([[MARK], q16]).astype(np.uint16))[1:]
    assert shifted.data_ptr() % 4 == 2
    assert ctx.compress(shifted, dict_size, chunk, hl.HUFFMAN, 3, d_oi, d_ov) == rec64
    # uint16 and int16 tensors are the same symbols
    assert ctx.compress(d16.view(torch.uint16), dict_size, chunk, hl.HUFFMAN, 3, d_oi, d_ov) == rec64
    # in place into a record of the caller at 256-aligned + {0, 3, 4}: the pool outside the record untouched
    for shift in (0, 3, 4):
        pool = torch.full((len(rec64) + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
        base = (-pool.data_ptr()) % 256 + shift
        rec = ctx.compress_device(d16, pool[base:], dict_size, chunk, outlier_idx=d_oi, outlier_val=d_ov)
        assert rec.data_ptr() % 256 == shift and rec.numel() == len(rec64)
        assert bytes(rec.cpu().numpy()) == rec64, shift
        assert bool((pool[:base] == 0x5A).all()) and bool((pool[base + rec.numel():] == 0x5A).all()), shift


def _inflate(rec):
    """The Huffman record inside a Huffman_Zstd record: [u64 size][zstd frame]."""
    z = ctypes.CDLL("libzstd.so.1")
    z.ZSTD_decompress.restype = ctypes.c_size_t
    z.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    raw, = struct.unpack_from("<Q", rec, 0)
    buf = ctypes.create_string_buffer(raw)
    assert z.ZSTD_decompress(buf, raw, rec[8:], len(rec) - 8) == raw
    return buf.raw


@pytest.mark.parametrize("name", ["normal60", "fib24-chunk1025", "full-16384-3333", "n1025"])
def test_huffman_zstd_from_16_bit_symbols(name):
    torch, mg, hl = _mods()
    q, q16, dict_size, chunk, oi, ov = _case(name)
    ctx = _context()
    d_oi, d_ov = torch.from_numpy(oi.copy()).cuda(), torch.from_numpy(ov.copy()).cuda()
    z16 = ctx.compress(_dev16(torch, q16), dict_size, chunk, hl.HUFFMAN_ZSTD, 3, d_oi, d_ov)
    z64 = ctx.compress(torch.from_numpy(q.copy()).cuda(), dict_size, chunk, hl.HUFFMAN_ZSTD, 3, d_oi, d_ov)
    inner = _inflate(z16)
    assert inner == _inflate(z64)
    assert inner == _records(name)[3]  # (a frame holds the record without the section)
    want = torch.cat([_dev16(torch, q16), _marked(torch, GUARD)])
    for payload in (z16, torch.frombuffer(bytearray(b"xyz" + z16), dtype=torch.uint8).cuda()[3:]):
        out = _marked(torch, q.size + GUARD)
        back, bi, bv = ctx.decompress(payload, q.size, hl.HUFFMAN_ZSTD, out=out, sym16=True)
        assert torch.equal(out, want)
        assert torch.equal(bi, d_oi) and torch.equal(bv, d_ov)


# ---- (b) the independent reader ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_independent_reader_decodes_the_record(name):
    """tests/payload.py reads the record written from 16-bit symbols and recomputes its synchronisation points.
    Streams of more than 40000 symbols: their first 40000, compressed on their own (the reader is bit-serial)."""
    torch, mg, hl = _mods()
    q, q16, dict_size, chunk, oi, ov = _case(name)
    if q.size <= PY_MAX:
        rec, sym = _records(name)[0], q
    else:
        sym = q[:PY_MAX]
        with _env(MGH_HUFF_SYNC="1"):
            rec = _context().compress(_dev16(torch, q16[:PY_MAX]), dict_size, chunk)
            assert rec == _context().compress(torch.from_numpy(sym.copy()).cuda(), dict_size, chunk)
    r = pl.parse_huffman_record(rec)
    assert np.array_equal(pl.decode_huffman_record(r), sym)
    if r["sync"] is not None:
        np.testing.assert_array_equal(r["sync"], pl.expected_sync_points(r, sym))
    if q.size <= PY_MAX:
        assert np.array_equal(r["outlier_idx"].astype(np.int64), oi) and np.array_equal(r["outliers"], ov)


def test_fib31_codebook_has_codes_past_27_bits():
    """The lengths the two fib31 rows rely on: past the 12-bit root table, past root + 11 bits (comparison path)
    and past 27 bits (escape entries of the 32-bit code table); none past 32 (the ring decoder's limit)."""
    torch, mg, hl = _mods()
    for name, lo, hi in (("fib31-permuted", 28, 32), ("fib31-rarest-first", 28, 32), ("fib24-chunk1025", 20, 23)):
        q, _, dict_size, _, _, _ = _case(name)
        code, _, _, _ = hl.huffman_codebook(np.bincount(q, minlength=dict_size).astype(np.uint32))
        longest = int((code >> np.uint64(56)).max())
        assert lo <= longest <= hi, (name, longest)


# ---- (c) decoding to 16-bit symbols ---------------------------------------------------------------------------
def _placements(torch, rec):
    """The record in host memory, in device memory, and in device memory three bytes into a buffer."""
    return [("host", rec), ("device", torch.frombuffer(bytearray(rec), dtype=torch.uint8).cuda()),
            ("device+3", torch.frombuffer(bytearray(b"xyz" + rec), dtype=torch.uint8).cuda()[3:])]


@pytest.mark.parametrize("name", list(CASES))
def test_decode_to_16_bit_symbols(name):
    torch, mg, hl = _mods()
    q, q16, dict_size, chunk, oi, ov = _case(name)
    n = q.size
    rec, plain = _records(name)[:2]
    ctx = _context()
    d_oi, d_ov = torch.from_numpy(oi.copy()).cuda(), torch.from_numpy(ov.copy()).cuda()
    want = torch.cat([_dev16(torch, q16), _marked(torch, GUARD)])
    d64 = torch.from_numpy(q.copy()).cuda()
    payloads = [("written", rec)] + ([("MGH_HUFF_SYNC=0", plain)] if plain != rec else [])
    if name.startswith("dict64"):  # the chunk <= 65535 edge of decode_plan's D.sync, with a section appended here
        r = pl.parse_huffman_record(rec)
        if chunk <= 65535:
            payloads.append(("recomputed section", _with_section(rec, pl.expected_sync_points(r, q))))
        else:
            payloads.append(("section that must not be used", _with_section(rec, np.full(64 * len(r["bits"]), 0xFFFFFFFF))))
    placed = [(what, where, p) for what, b in payloads for where, p in _placements(torch, b)]
    out = _marked(torch, n + GUARD)
    for sync_decode, pair in SWITCHES:
        for tb in TABLE_BITS:
            with _env(MGH_HUFF_SYNC_DECODE=sync_decode, MGH_HUFF_PAIR=pair, MGH_HUFF_TB=tb):
                for what, where, payload in placed:
                    out.fill_(MARK - 65536)
                    back, bi, bv = ctx.decompress(payload, n, hl.HUFFMAN, out=out, sym16=True)
                    if not torch.equal(out, want):  # (where, for the message)
                        got = out.cpu().numpy().view(np.uint16)
                        bad = np.nonzero(got != want.cpu().numpy().view(np.uint16))[0]
                        raise AssertionError("%s, %s, SYNC_DECODE=%s PAIR=%s TB=%s: %d elements differ, first at %d of %d "
                                             "(chunk %d)" % (what, where, sync_decode, pair, tb, bad.size, bad[0], n, chunk))
                    assert torch.equal(bi, d_oi) and torch.equal(bv, d_ov), (what, where)
                # (the int64 instantiations under the same switches: MGH_HUFF_TB is in no other test)
                back64, _, _ = ctx.decompress(rec, n)
                assert torch.equal(back64, d64), (sync_decode, pair, tb)
    # without `out`: a uint16 tensor of n elements
    back, _, _ = ctx.decompress(rec, n, sym16=True)
    assert back.dtype == torch.uint16 and back.shape == (n,) and np.array_equal(back.cpu().numpy(), q16)
    # and the int64 decoder reads the record written from 16-bit symbols
    back64, _, _ = ctx.decompress(rec, n)
    assert np.array_equal(back64.cpu().numpy(), q)


# ---- (d) ranges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RANGE_CASES)
def test_ranges_decode_to_16_bit_symbols(name):
    """A range moves the output pointer by (c0 - cf) * chunk elements of the narrower type, on an odd chunk length:
    d_symbols[0 ...) receives the integers from the start of the first decoded chunk to the end of the last, and
    nothing behind them."""
    torch, mg, hl = _mods()
    q, q16, dict_size, chunk, oi, ov = _case(name)
    n = q.size
    assert chunk % 2 == 1 and n > 4 * chunk and n % chunk
    nchunk = (n - 1) // chunk + 1
    rec, plain = _records(name)[:2]
    ctx = _context()
    d_oi, d_ov = torch.from_numpy(oi.copy()).cuda(), torch.from_numpy(ov.copy()).cuda()
    ranges = [(0, chunk), (5, 10),                         # the first chunk only
              (3 * chunk + 7, 100), (chunk, chunk),        # one middle chunk
              (2 * chunk - 3, 10),                         # a range that straddles two chunks
              (chunk - 1, chunk + 2),                      # ... and one that touches three
              (n - 1, 1), ((nchunk - 1) * chunk, 1),       # the tail chunk only
              ((nchunk - 2) * chunk + 1, chunk),           # the last whole chunk and the tail
              (1, n - 1)]                                  # every chunk, as a range
    placed = [(what, where, p) for what, b in (("written", rec), ("MGH_HUFF_SYNC=0", plain)) if what == "written" or b != rec
              for where, p in _placements(torch, b)]
    for first, count in ranges:
        c0, c1 = first // chunk, (first + count - 1) // chunk
        piece = q16[c0 * chunk:min(n, (c1 + 1) * chunk)]
        want = torch.cat([_dev16(torch, piece), _marked(torch, GUARD)])
        out = _marked(torch, piece.size + GUARD)
        for sync_decode, pair, tb in (("1", "1", None), ("1", "2", "8"), ("0", "1", "14")):
            with _env(MGH_HUFF_SYNC_DECODE=sync_decode, MGH_HUFF_PAIR=pair, MGH_HUFF_TB=tb):
                for what, where, payload in placed:
                    out.fill_(MARK - 65536)
                    _, bi, bv = ctx.decompress(payload, n, hl.HUFFMAN, out=out, first=first, count=count, sym16=True)
                    assert torch.equal(out, want), (first, count, what, where, sync_decode, pair, tb)
                    assert torch.equal(bi, d_oi) and torch.equal(bv, d_ov)
    # a range outside the record is refused
    out = _marked(torch, n + GUARD)
    for first, count in ((0, 0), (n, 1), (1, n), (n - 1, 2)):
        with pytest.raises(mg.MgardHipError, match="error -1"):
            ctx.decompress(rec, n, out=out, first=first, count=count, sym16=True)
    assert torch.equal(out, _marked(torch, n + GUARD))


# ---- (e) refusals -----------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_and_the_context_alone():
    torch, mg, hl = _mods()
    ctx = _context()
    # the single-pass encoder stages dict * 8 + chunk * 2 bytes: more than 140 KiB is refused for 16-bit symbols
    q = huffman_symbols(3 * 8192 + 5, width=50.0, dict_size=16384)
    d16 = _dev16(torch, q.astype(np.uint16))
    assert 16384 * 8 + 8192 * 2 > 140 * 1024
    for lossless in (hl.HUFFMAN, hl.HUFFMAN_ZSTD):
        with pytest.raises(mg.MgardHipError, match="error -1"):
            ctx.compress(d16, 16384, 8192, lossless)
    pool = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda")
    with pytest.raises(mg.MgardHipError, match="error -1"):
        ctx.compress_device(d16, pool, 16384, 8192)
    assert bool((pool == 0x5A).all())
    assert 16384 * 8 + 6144 * 2 == 140 * 1024  # ... and the largest chunk that dictionary takes is not
    rec = ctx.compress(d16, 16384, 6144)
    assert rec == ctx.compress(torch.from_numpy(q).cuda(), 16384, 6144)
    # a record of chunks shorter than 1024 is not the ring decoder's: refused, nothing written
    q = huffman_symbols(5 * 1000 + 3, width=20.0)
    q16 = q.astype(np.uint16)
    short = ctx.compress(_dev16(torch, q16), 8192, 1000)
    assert short == ctx.compress(torch.from_numpy(q).cuda(), 8192, 1000)
    out = _marked(torch, q.size + GUARD)
    for payload in (short, torch.frombuffer(bytearray(short), dtype=torch.uint8).cuda()):
        with pytest.raises(mg.MgardHipError, match="error -1"):
            ctx.decompress(payload, q.size, out=out, sym16=True)
        with pytest.raises(mg.MgardHipError, match="error -1"):
            ctx.decompress(payload, q.size, out=out, first=1000, count=5, sym16=True)
    assert torch.equal(out, _marked(torch, q.size + GUARD))
    back, _, _ = ctx.decompress(short, q.size)  # (the int64 entry takes it)
    assert np.array_equal(back.cpu().numpy(), q)
    # the same context goes on working
    rec = ctx.compress(_dev16(torch, q16), 8192, 1024)
    out = _marked(torch, q.size + GUARD)
    ctx.decompress(rec, q.size, out=out, sym16=True)
    assert torch.equal(out, torch.cat([_dev16(torch, q16), _marked(torch, GUARD)]))
