"""CPU tests of mgard_amd/csrc/huffman_record.hpp -- the layout of the serialized Huffman record, the parser of
an untrusted one (record_fixed + record_plan), the choice of the decoder (decode_plan) and the rule of the
decode-while-it-arrives path (chunks_landed) -- through tests/cpp/huffman_record_dump.cpp (g++ against the
header alone, no HIP).

Valid records come from oracle/huffman_ref.get_codebook + tests/payload.write_huffman_record, as in
test_huffman_reference_rules.py; what the parser finds in them is compared with tests/payload.parse_huffman_record
(the independent reader), and the range arithmetic with its definitions restated here.
Damaged records are one mutation of a valid one each. The verdict expected of every one -- accepted, or
MGH_ERR_FORMAT with which message -- is _model(): the checks of lossless_decompress() as they stood before
the parser moved into the header, restated in the same order, so that a record with two defects names the
same one. The one deliberate difference: a chunk's bit count within 63 of 2^64 used to wrap in
(bits + 63) / 64 and pass as a chunk of no units; it is refused ("chunk outside the code stream").
The same program is also built with -fsanitize=address,undefined and run once, as a stand-alone binary, over
the whole damaged set: every span the parser gets is a heap block of exactly its size."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import huffman_ref as ref
from tests import payload as pl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgard_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "huffman_record_dump.cpp")
ALL = 2 ** 64 - 1
TRUNCATED = "Huffman record truncated"
HEADER = "Huffman record: header does not match the subdomain"
CHUNK_LEN = "Huffman record: chunk length does not match the header"
BOOK = "Huffman record: decodebook size"
LISTS = "Huffman record: outlier lists"
OUTSIDE = "Huffman record: chunk outside the code stream"


def _build(tmp_path_factory, name, extra=()):
    exe = str(tmp_path_factory.mktemp(name) / "huffman_record_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", CSRC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return _build(tmp_path_factory, "huffman_record")


def _run(exe, text):
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=300).stdout
    res = []
    for line in out.splitlines():
        kind, _, rest = line.partition(" ")
        if kind == "err" or "=" not in rest:
            res.append((kind, rest))
        else:
            res.append((kind, {k: int(v) if v.lstrip("-").isdigit() else v for k, v in (f.split("=") for f in rest.split())}))
    return res


# ---- valid records ---------------------------------------------------------------------------------------
def _lengths(freq):
    """Huffman code lengths, non-increasing along the stable ascending order of the counts (what get_codebook
    expects): the lengths of a Huffman tree, dealt out longest first."""
    import heapq
    used = [int(s) for s in np.nonzero(freq)[0]]
    lens = np.zeros(len(freq), np.int64)
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    heap = [(int(freq[s]), i, (s,)) for i, s in enumerate(used)]
    heapq.heapify(heap)
    depth = dict.fromkeys(used, 0)
    tick = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
        tick += 1
    order = sorted(used, key=lambda s: (int(freq[s]), s))
    for s, l in zip(order, sorted(depth.values(), reverse=True)):
        lens[s] = l
    return lens


def _codebook(dict_size):
    rng = np.random.default_rng(dict_size)
    f = np.zeros(dict_size, np.uint32)
    k = 12 if dict_size == 16 else 300
    f[rng.choice(dict_size, k, replace=False)] = (1e5 * 0.8 ** np.arange(k)).astype(np.uint32) + 1
    return f, ref.get_codebook(f, _lengths(f))


CODEBOOKS = {d: _codebook(d) for d in (16, 8192)}


def _record(n, chunk, dict_size, outliers, sync, seed=0):
    f, (code, first, entry, keys) = CODEBOOKS[dict_size]
    rng = np.random.default_rng(1000 * n + chunk + seed)
    used = np.nonzero(f)[0]
    sym = rng.choice(used, n, p=f[used] / f[used].sum())
    oidx = sorted(rng.choice(n, min(n, 3), replace=False).tolist()) if outliers else []
    rec = bytes(pl.write_huffman_record(sym, dict_size, chunk, code, first, entry, keys, oidx, [7 - 5 * k for k in range(len(oidx))]))
    if sync:
        nchunk = (n - 1) // chunk + 1
        rec += struct.pack("<Q", pl.SYNC_TAG) + bytes(256 * nchunk)
    return rec


def _valid_cases():
    out = []
    for chunk, dict_size, outliers, sync in itertools.product((7, 512, 1024), (16, 8192), (False, True), (False, True)):
        for n in (1, chunk - 1, chunk, chunk + 1, 3 * chunk + 77):
            out.append((n, chunk, dict_size, outliers, sync))
    return out


class Files:
    """Records as files for the dump program (one file per distinct content)."""

    def __init__(self, root):
        self.root, self.seen = root, {}

    def __call__(self, rec):
        rec = bytes(rec)
        if rec not in self.seen:
            path = os.path.join(self.root, "r%d.bin" % len(self.seen))
            with open(path, "wb") as f:
                f.write(rec)
            self.seen[rec] = path
        return self.seen[rec]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return Files(str(tmp_path_factory.mktemp("records")))


@pytest.fixture(scope="module")
def valid(files):
    return [(case, _record(*case)) for case in _valid_cases()]


def _parse_cmd(files, rec, n, n_prefix=ALL, first=0, q_cap=ALL, keep=0, on_dev=0, sync_decode=1):
    return "parse %s %d %d %d %d %d %d %d\n" % (files(rec), n, n_prefix, first, q_cap, keep, on_dev, sync_decode)


def _ceil64(bits):
    return -(-int(bits) // 64)


def test_header_compiles_alone_without_hip(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "huffman_record.hpp"\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", CSRC, str(src)])


def test_valid_records_parse_to_what_the_independent_reader_finds(dump, files, valid):
    text = ""
    for (n, chunk, dict_size, outliers, sync), rec in valid:
        r = pl.parse_huffman_record(rec)
        text += "layout %d %d %d %d %d\n" % (len(r["bits"]), dict_size, len(r["units"]), len(r["outlier_idx"]), sync)
        text += _parse_cmd(files, rec, n) + _parse_cmd(files, rec, n, on_dev=1) + _parse_cmd(files, rec, n, sync_decode=0)
    res = _run(dump, text)
    assert len(res) == 4 * len(valid)
    for k, ((n, chunk, dict_size, outliers, sync), rec) in enumerate(valid):
        r = pl.parse_huffman_record(rec)
        nchunk, units, oc = len(r["bits"]), len(r["units"]), len(r["outlier_idx"])
        assert nchunk == (n - 1) // chunk + 1 and oc == (min(n, 3) if outliers else 0) and (r["sync"] is not None) == sync
        (kind, lay), host, dev, nosync = res[4 * k:4 * k + 4]
        assert kind == "layout" and lay["total"] == len(rec) and lay["sync_bytes"] == 8 + 256 * nchunk
        # the offsets of the writer's layout are where the independent reader found the members
        off = {"huffmeta": 24, "decodebook_size": 24 + 16 * nchunk}
        off["decodebook"] = off["decodebook_size"] + 8
        off["ddata_size"] = off["decodebook"] + 8 * 128 + 8 * dict_size
        off["ddata"] = off["ddata_size"] + 8
        off["outlier_count"] = off["ddata"] + 8 * units
        off["outlier_idx"] = off["outlier_count"] + 8
        off["outliers"] = off["outlier_idx"] + 8 * oc
        off["sync_tag"] = off["outliers"] + 8 * oc if sync else 0
        off["sync"] = off["sync_tag"] + 8 if sync else 0
        for name, at in off.items():
            assert lay[name] == at, (name, n, chunk, dict_size)
        for name, arr in (("huffmeta", r["bits"]), ("decodebook", r["first"]), ("ddata", r["units"]),
                          ("outlier_idx", r["outlier_idx"]), ("outliers", r["outliers"].view(np.uint64))):
            assert np.array_equal(np.frombuffer(rec, "<u8", len(arr), off[name]), arr), name
        assert struct.unpack_from("<QQ", rec + bytes(8), off["outlier_count"])[0] == oc
        assert struct.unpack_from("<Q", rec, off["ddata_size"])[0] == units
        assert not sync or struct.unpack_from("<Q", rec, off["sync_tag"])[0] == pl.SYNC_TAG
        first = [int(x) for x in r["first"]]
        want = dict(dict=dict_size, chunk=chunk, nchunk=nchunk, huffmeta=off["huffmeta"], decodebook=off["decodebook"],
                    ddata=off["ddata"], ndec=nchunk, cf=0, n_dec=n, tb0=0, tb_cnt=nchunk, dbsize=8 * 128 + 8 * dict_size,
                    units=units, ocount=oc, o_oc=off["outlier_count"], o_oidx=off["outlier_idx"], o_oval=off["outliers"],
                    o_sync=off["outliers"] + 8 * oc + 8, has_sync=int(sync), units_lo=0, units_need=units,
                    book_max_len=max(l for l in range(1, 64) if first[l] != ALL))
        assert host == ("ok", want), (n, chunk, dict_size, outliers, sync)
        assert dev == ("ok", want), "the device path (no count word, no tag) finds the same"
        assert nosync == ("ok", dict(want, has_sync=0))


def _range_points(n, chunk):
    return sorted({x for x in (1, chunk - 1, chunk, chunk + 1, n - 1, n) if 1 <= x <= n})


def test_range_arithmetic_against_its_definitions(dump, files, valid):
    text, jobs = "", []
    for (n, chunk, dict_size, outliers, sync), rec in valid:
        if dict_size == 8192 and not (outliers and sync):
            continue  # (the range arithmetic does not look at the decodebook: one variant of the large one)
        for n_prefix in _range_points(n, chunk):
            for first in [0] + [x for x in _range_points(n, chunk) if x < n_prefix]:
                for keep, on_dev in ((0, 0), (1, 1)):
                    text += _parse_cmd(files, rec, n, n_prefix, first, keep=keep, on_dev=on_dev)
                    jobs.append((rec, n, chunk, n_prefix, first, keep))
    res = _run(dump, text)
    assert len(res) == len(jobs) > 1000
    parsed = {}
    for (rec, n, chunk, n_prefix, first, keep), (kind, got) in zip(jobs, res):
        assert kind == "ok", got
        r = parsed.setdefault(rec, pl.parse_huffman_record(rec))
        bits, entry, units = [int(x) for x in r["bits"]], [int(x) for x in r["entry"]], len(r["units"])
        nchunk = (n - 1) // chunk + 1
        ndec = min(nchunk, (min(n_prefix, n) - 1) // chunk + 1)  # chunks that hold the first n_prefix integers
        cf = first // chunk                                       # the chunk that holds integer `first`
        assert (got["ndec"], got["cf"], got["n_dec"]) == (ndec, cf, min(n, ndec * chunk))
        assert (got["tb0"], got["tb_cnt"]) == ((0, nchunk) if keep else (cf, ndec - cf))
        need = units if ndec == nchunk else max(entry[k] + _ceil64(bits[k]) for k in range(ndec))
        lo = min(need, min(entry[k] for k in range(cf, ndec))) if cf else 0
        assert (got["units_lo"], got["units_need"]) == (lo, need), (n, chunk, n_prefix, first)
        assert got["ocount"] == len(r["outlier_idx"]) and got["has_sync"] == int(r["sync"] is not None)


# ---- damaged records -------------------------------------------------------------------------------------
def _model(rec, n, n_prefix=ALL, first=0, q_cap=ALL, on_dev=0):
    """The verdict on a record: None (accepted; then also whether its synchronisation section is used) or the
    message of MGH_ERR_FORMAT -- the checks in the order lossless_decompress() made them."""
    psize = len(rec)

    def u64(off):
        return struct.unpack_from("<Q", rec, off)[0]

    if psize < 24:
        return TRUNCATED, None
    primary, hm = u64(0), u64(16)
    dict_size, chunk = struct.unpack_from("<ii", rec, 8)
    if primary != n or dict_size <= 0 or dict_size > 16384 or chunk <= 0 or hm != 2 * ((n - 1) // chunk + 1):
        return HEADER, None
    nchunk = hm // 2
    ndec = 0 if n_prefix == 0 else min(nchunk, (min(n_prefix, n) - 1) // chunk + 1)
    cf = first // chunk
    if ndec and min(n, ndec * chunk) - cf * chunk > q_cap:
        return CHUNK_LEN, None
    ddata = 24 + 16 * nchunk + 8 + 8 * 128 + 8 * dict_size + 8
    if ddata > psize:
        return TRUNCATED, None
    if u64(24 + 16 * nchunk) != 8 * 128 + 8 * dict_size:
        return BOOK, None
    units = u64(ddata - 8)
    if units > (psize - ddata) // 8:
        return TRUNCATED, None
    o_oc = ddata + 8 * units
    if psize - o_oc < 8:
        return TRUNCATED, None
    sync_bytes = 8 + 256 * nchunk
    rem = psize - o_oc - 8
    has_sync = rem % 16 == 8 and rem >= sync_bytes
    if on_dev:
        if rem % 16 != 0 and not has_sync:
            return LISTS, None
        ocount = (rem - (sync_bytes if has_sync else 0)) // 16
    else:
        ocount = u64(o_oc)
        if has_sync and (ocount > (rem - sync_bytes) // 16 or rem - 16 * ocount != sync_bytes):
            has_sync = False
    if ocount > rem // 16:
        return TRUNCATED, None
    if has_sync and not on_dev and u64(o_oc + 8 + 16 * ocount) != pl.SYNC_TAG:
        has_sync = False
    for k in range(nchunk):
        bits, ent = u64(24 + 8 * k), u64(24 + 8 * (nchunk + k))
        if ent > units or _ceil64(bits) > units - ent:
            return OUTSIDE, None
    return None, has_sync


def _put(rec, off, fmt, value):
    b = bytearray(rec)
    struct.pack_into(fmt, b, off, value)
    return bytes(b)


def _damaged():
    """[(name, record, n, n_prefix)]; every record one mutation away from a valid one."""
    out = []
    for tag, (n, chunk, dict_size) in (("small", (30, 7, 16)), ("large", (3 * 1024 + 77, 1024, 8192))):
        plain, full = _record(n, chunk, dict_size, True, False), _record(n, chunk, dict_size, True, True)
        r = pl.parse_huffman_record(full)
        nchunk, units, oc = len(r["bits"]), len(r["units"]), len(r["outlier_idx"])
        ddata = 24 + 16 * nchunk + 8 + 8 * 128 + 8 * dict_size + 8
        o_oc = ddata + 8 * units
        ent = lambda k: 24 + 8 * (nchunk + k)
        last = nchunk - 1
        cases = [("primary", _put(full, 0, "<Q", n + 1))]
        cases += [("dict=%d" % d, _put(full, 8, "<i", d)) for d in (0, -1, 16385)]
        cases += [("chunk=%d" % c, _put(full, 12, "<i", c)) for c in (0, -1)]
        cases += [("huffmeta%+d" % d, _put(full, 16, "<Q", 2 * nchunk + d)) for d in (-2, 2)]
        cases += [("decodebook size", _put(full, 24 + 16 * nchunk, "<Q", 8 * 128 + 8 * dict_size + 8))]
        cases += [("units one more than fits", _put(rec, ddata - 8, "<Q", (len(rec) - ddata) // 8 + 1)) for rec in (plain, full)]
        cases += [("entry[0] past the stream", _put(full, ent(0), "<Q", units + 1)),
                  ("entry[last] past the stream", _put(full, ent(last), "<Q", units + 1)),
                  ("bits[last] past the stream", _put(full, 24 + 8 * last, "<Q", 64 * (units - int(r["entry"][last])) + 1)),
                  ("bits[0] = 2^64 - 1", _put(full, 24, "<Q", ALL)),
                  ("bits[last] = 2^64 - 63", _put(full, 24 + 8 * last, "<Q", ALL - 62)),
                  ("ocount larger than the bytes left", _put(plain, o_oc, "<Q", oc + 1)),
                  ("ocount huge", _put(full, o_oc, "<Q", 2 ** 61)),
                  ("wrong tag", _put(full, o_oc + 8 + 16 * oc, "<Q", pl.SYNC_TAG ^ 1)),
                  ("remainder 8 mod 16, shorter than the section", plain + bytes(8)),
                  ("remainder 8 mod 16, the lists cut", plain[:-8]),
                  ("section one entry short", full[:-4]), ("section cut by 16", full[:-16])]
        for name, rec in cases:
            out.append(("%s: %s" % (tag, name), rec, n, ALL))
            out.append(("%s: %s, first chunk only" % (tag, name), rec, n, 1))
    n, chunk, dict_size = 30, 7, 16
    for sync in (False, True):
        rec = _record(n, chunk, dict_size, True, sync)
        out += [("truncated to %d of %d%s" % (k, len(rec), " (sync)" if sync else ""), rec[:k], n, ALL) for k in range(len(rec))]
    return out


DAMAGED = _damaged()


def _damaged_text(files):
    return "".join(_parse_cmd(files, rec, n, n_prefix, on_dev=on_dev) for _, rec, n, n_prefix in DAMAGED for on_dev in (0, 1))


def _check_damaged(res):
    assert len(res) == 2 * len(DAMAGED)
    verdicts = {}
    for k, (name, rec, n, n_prefix) in enumerate(DAMAGED):
        for on_dev in (0, 1):
            kind, got = res[2 * k + on_dev]
            bad, has_sync = _model(rec, n, n_prefix, on_dev=on_dev)
            if bad is None:
                assert kind == "ok" and got["has_sync"] == int(has_sync), (name, on_dev, got)
            else:
                assert (kind, got) == ("err", bad), (name, on_dev)
            verdicts[name, on_dev] = bad
    return verdicts


def test_damaged_records_are_refused_with_the_same_message(dump, files):
    v = _check_damaged(_run(dump, _damaged_text(files)))
    # the verdicts themselves, so that the model cannot drift along with the parser
    for tag in ("small", "large"):
        for suffix in ("", ", first chunk only"):  # (the loop over the chunk table covers chunks that are not needed)
            def at(name, on_dev):
                return v["%s: %s%s" % (tag, name, suffix), on_dev]
            for on_dev in (0, 1):
                for name in ("primary", "dict=0", "dict=-1", "dict=16385", "chunk=0", "chunk=-1", "huffmeta-2", "huffmeta+2"):
                    assert at(name, on_dev) == HEADER
                assert at("decodebook size", on_dev) == BOOK and at("units one more than fits", on_dev) == TRUNCATED
                for name in ("entry[0] past the stream", "entry[last] past the stream", "bits[last] past the stream",
                             "bits[0] = 2^64 - 1", "bits[last] = 2^64 - 63"):
                    assert at(name, on_dev) == OUTSIDE
                # a section that is too short: a host record decodes without it; a device record's size must fit --
                # 16 bytes less fit one outlier less and the section, and then the tag is not where the kernel looks
                assert at("section one entry short", on_dev) == (LISTS if on_dev else None)
                assert at("section cut by 16", on_dev) is None
                # accepted, and decoded without the points (a device record's tag is the kernel's to check)
                assert at("wrong tag", on_dev) is None
            # a host record says how many outliers it has; a device record's size does
            assert at("ocount larger than the bytes left", 0) == TRUNCATED and at("ocount huge", 0) == TRUNCATED
            assert at("ocount larger than the bytes left", 1) is None and at("ocount huge", 1) is None
            assert at("remainder 8 mod 16, the lists cut", 0) == TRUNCATED and at("remainder 8 mod 16, the lists cut", 1) == LISTS
            assert at("remainder 8 mod 16, shorter than the section", 0) is None
            assert at("remainder 8 mod 16, shorter than the section", 1) == LISTS
    # a host record cut anywhere in front of the end of its outlier lists is refused
    rec = _record(30, 7, 16, True, False)
    for k in range(len(rec)):
        assert v["truncated to %d of %d" % (k, len(rec)), 0] is not None, k
    assert sum(v["truncated to %d of %d" % (k, len(rec)), 1] is None for k in range(len(rec))) <= 3  # (whole outliers cut off)


def test_chunk_length_against_the_output_capacity(dump, files):
    n, chunk = 3 * 7 + 5, 7
    rec = _record(n, chunk, 16, False, False)
    cases = [(ALL, 0, n, None), (ALL, 0, n - 1, CHUNK_LEN), (8, 0, 14, None), (8, 0, 13, CHUNK_LEN), (n, 22, 5, None),
             (n, 22, 4, CHUNK_LEN), (15, 7, 14, None), (15, 7, 13, CHUNK_LEN)]
    res = _run(dump, "".join(_parse_cmd(files, rec, n, p, f, q_cap=q) for p, f, q, _ in cases))
    for (kind, got), (_, _, _, want) in zip(res, cases):
        assert (kind == "ok") if want is None else ((kind, got) == ("err", want))
    # two defects: the capacity is looked at before the length of the record
    (kind, got), = _run(dump, _parse_cmd(files, rec[:30], n, q_cap=n - 1))
    assert (kind, got) == ("err", CHUNK_LEN)


def test_program_is_clean_under_address_and_undefined_sanitizers(tmp_path_factory, files, valid):
    exe = _build(tmp_path_factory, "huffman_record_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    text = _damaged_text(files)
    (case, rec) = valid[-1]
    text += _parse_cmd(files, rec, case[0], 1025, 1024) + "landed %s %d %d 0 0 9 0\n" % (files(rec), case[0], ALL)
    text += "layout 4 16 9 3 1\ndecode 8192 1024 3149 300 1 12 4 0 0 0 1 unset\n"
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-4000:]
    out = p.stdout.splitlines()
    assert len(out) == 2 * len(DAMAGED) + 4
    res = [(l.partition(" ")[0], l.partition(" ")[2]) for l in out[:2 * len(DAMAGED)]]
    for k, (name, r, n, n_prefix) in enumerate(DAMAGED):
        for on_dev in (0, 1):
            bad, _ = _model(r, n, n_prefix, on_dev=on_dev)
            assert res[2 * k + on_dev][0] == ("ok" if bad is None else "err") and (bad is None or res[2 * k + on_dev][1] == bad), name


# ---- the decoder ---------------------------------------------------------------------------------------
def _decode_model(dict_size, chunk, n, units, has_sync, book_max, ndec, cf, serial, par, pair, tb):
    """decode_plan's conditions as lossless_decompress() stated them."""
    keys = (dict_size * 2 + 7) // 8 * 8 + 16 * 64 * 8
    if not serial and not par and 1024 <= chunk <= 2 ** 24 and dict_size <= 65536 and book_max <= 32:
        sync = has_sync and chunk <= 65535
        rtb = max(8, min(14, 12 if tb is None else tb))
        # (the pair table's root, 8 << rtb bytes, beside the rings of 8 waves in the launch's 150 KiB: 13 bits at most)
        fits = (8 << rtb) + 8 * (8 * 64 * 8 + 64 * 17 * 2) <= 150 * 1024
        return dict(kind="ring", sync=int(sync), tb=0, lds=0, rtb=rtb,
                    pair=int(sync and fits and (pair == 2 or (pair == 1 and units * 64.0 <= 6.5 * n))))
    if ndec <= cf:
        return dict(kind="none", sync=0, pair=0, tb=0, rtb=0, lds=0)
    t = 15
    while t > 8 and (4 << t) + keys > 154 * 1024:
        t -= 1
    t = max(8, min(t, t if tb is None else tb))
    if not serial and chunk >= 1024:
        stage = (dict_size + 3) // 4 * 8 + 16 * 64 * 32 * 2
        while t > 8 and (4 << t) + stage > 150 * 1024:
            t -= 1
        return dict(kind="par", sync=0, pair=0, tb=t, rtb=0, lds=(4 << t) + stage)
    return dict(kind="serial", sync=0, pair=0, tb=t, rtb=0, lds=(4 << t) + keys)


def test_decoder_choice(dump):
    base = dict(dict_size=8192, chunk=20480, n=10 ** 6, units=10 ** 5, has_sync=1, book_max=20, ndec=49, cf=0, serial=0, par=0,
                pair=1, tb=None)
    cases = [base]
    cases += [dict(base, chunk=c, book_max=b) for c in (1023, 1024) for b in (32, 33)]
    cases += [dict(base, chunk=c) for c in (65535, 65536, 2 ** 24, 2 ** 24 + 1)]
    cases += [dict(base, n=64000, units=u) for u in (6499, 6500, 6501)]  # units * 64 against 6.5 * n = 416000
    cases += [dict(base, n=64000, units=u, pair=p) for u in (6500, 6501) for p in (0, 1, 2)]
    cases += [dict(base, n=64000, units=6000, has_sync=0, pair=p) for p in (1, 2)]
    cases += [dict(base, serial=s, par=p, chunk=c) for s in (0, 1) for p in (0, 1) for c in (512, 1024)]
    cases += [dict(base, tb=t, book_max=b, chunk=c) for t in (-3, 0, 7, *range(8, 17)) for b, c in ((20, 20480), (40, 20480), (20, 512))]
    cases += [dict(base, dict_size=d, book_max=b, chunk=c) for d in (16, 16384) for b in (20, 40) for c in (512, 4096)]
    cases += [dict(base, ndec=n_, cf=c, book_max=b) for n_, c in ((0, 0), (3, 3)) for b in (20, 40)]  # nothing to decode
    names = ("dict_size", "chunk", "n", "units", "has_sync", "book_max", "ndec", "cf", "serial", "par", "pair", "tb")
    res = _run(dump, "".join("decode " + " ".join("unset" if c[k] is None else str(c[k]) for k in names) + "\n" for c in cases))
    assert len(res) == len(cases)
    for c, (kind, got) in zip(cases, res):
        assert kind == "decode" and got == _decode_model(**c), c
    by = {tuple(sorted(c.items())): got for c, (_, got) in zip(cases, res)}
    pick = lambda **kw: by[tuple(sorted(dict(base, **kw).items()))]
    # ... and the landmarks by name
    assert pick()["kind"] == "ring" and pick()["rtb"] == 12
    assert [pick(chunk=c, book_max=b)["kind"] for c in (1023, 1024) for b in (32, 33)] == ["serial", "serial", "ring", "par"]
    assert [pick(n=64000, units=u)["pair"] for u in (6499, 6500, 6501)] == [1, 1, 0]
    assert [pick(chunk=c)["pair"] for c in (65535, 65536)] == [1, 0] and pick(chunk=2 ** 24 + 1)["kind"] == "par"
    assert pick(serial=1, par=0, chunk=1024)["kind"] == "serial" and pick(serial=0, par=1, chunk=1024)["kind"] == "par"
    assert pick(tb=15, book_max=40, chunk=20480)["tb"] == 14 and pick(tb=15, book_max=20, chunk=512)["tb"] == 15
    assert pick(tb=15, book_max=20, chunk=20480)["rtb"] == 14 and pick(tb=8, book_max=20, chunk=20480)["rtb"] == 8
    # (a root table of 14 bits leaves no room for pairs: that launch asked for more LDS than a workgroup has)
    assert [pick(tb=t, book_max=20, chunk=20480)["pair"] for t in (12, 13, 14, 15)] == [1, 1, 0, 0]
    # (a value outside the switch's range is clamped, never taken for "not set")
    assert pick(tb=0, book_max=20, chunk=20480)["rtb"] == 8 and pick(tb=0, book_max=20, chunk=512)["tb"] == 8


def test_sym16_output_takes_the_ring_decoder_or_nothing(dump):
    """sym16_refusal: a caller whose output holds 16-bit symbols (mgh_lossless_decompress_sym16) is refused for
    every plan that is not the ring decoder's -- the other decoders write int64 values -- and for none that is.
    The plans: each condition of decode_plan's first branch on both sides of its edge."""
    base = dict(dict_size=8192, chunk=20480, n=10 ** 6, units=10 ** 5, has_sync=1, book_max=20, ndec=49, cf=0, serial=0, par=0,
                pair=1, tb=None)
    cases = [base]
    cases += [dict(base, chunk=c) for c in (1000, 1023, 1024, 1025, 65535, 65536, 2 ** 24, 2 ** 24 + 1)]
    cases += [dict(base, book_max=b) for b in (1, 32, 33, 56)]
    cases += [dict(base, serial=s, par=p, chunk=c) for s in (0, 1) for p in (0, 1) for c in (512, 1024)]
    cases += [dict(base, has_sync=h, pair=p, tb=t) for h in (0, 1) for p in (0, 1, 2) for t in (None, 8, 14)]
    cases += [dict(base, dict_size=d) for d in (2, 64, 16384)]
    cases += [dict(base, ndec=n_, cf=c, book_max=b) for n_, c in ((0, 0), (3, 3)) for b in (20, 40)]  # nothing to decode
    names = ("dict_size", "chunk", "n", "units", "has_sync", "book_max", "ndec", "cf", "serial", "par", "pair", "tb")
    res = _run(dump, "".join("decode16 " + " ".join("unset" if c[k] is None else str(c[k]) for k in names) + "\n" for c in cases))
    assert len(res) == len(cases)
    seen = set()
    for c, (kind, got) in zip(cases, res):
        want = _decode_model(**c)["kind"]
        assert kind == "decode16" and got == dict(kind=want, refused=int(want != "ring")), c
        seen.add(want)
    assert seen == {"ring", "par", "serial", "none"}
    by = {tuple(sorted(c.items())): got["refused"] for c, (_, got) in zip(cases, res)}
    pick = lambda **kw: by[tuple(sorted(dict(base, **kw).items()))]
    # ... and the landmarks by name: the refusals the C ABI documents
    assert pick() == 0 and [pick(chunk=c) for c in (1000, 1023, 1024, 65536)] == [1, 1, 0, 0]
    assert [pick(book_max=b) for b in (32, 33)] == [0, 1]
    assert pick(serial=1, par=0, chunk=1024) == 1 and pick(serial=0, par=1, chunk=1024) == 1
    assert pick(has_sync=0, pair=1, tb=8) == 0 and pick(has_sync=1, pair=2, tb=14) == 0
    assert pick(ndec=3, cf=3, book_max=40) == 1 and pick(ndec=3, cf=3, book_max=20) == 0


def test_chunks_landed(dump, files):
    n, chunk = 40 * 7 + 3, 7
    rec = _record(n, chunk, 16, False, False)
    r = pl.parse_huffman_record(rec)
    bits, entry, units = [int(x) for x in r["bits"]], [int(x) for x in r["entry"]], len(r["units"])
    for n_prefix in (ALL, 100):
        ndec = min(len(bits), (min(n_prefix, n) - 1) // chunk + 1)
        haves = list(range(0, units + 3))
        cmd = "landed %s %d %d 0 %%d %%d %%d\n" % (files(rec), n, n_prefix)
        hi = [int(got) for _, got in _run(dump, "".join(cmd % (0, h, 0) for h in haves))]
        assert hi == sorted(hi) and max(hi) <= ndec  # monotone, never past ndec
        for h, c_hi in zip(haves, hi):
            # chunk k counts only when its units and the one behind them are there; the chunks counted are the
            # longest run of such chunks from the start
            want = 0
            while want < ndec and entry[want] + _ceil64(bits[want]) + 1 <= h:
                want += 1
            assert c_hi == want, (h, c_hi, want)
        # the last piece: everything, whatever has landed by the count; and a start from chunks already done
        assert [int(got) for _, got in _run(dump, cmd % (5, 0, 1) + cmd % (2, units + 2, 0))] == [ndec, ndec]
