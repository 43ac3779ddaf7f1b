"""CPU test of mgard_amd/csrc/mask_plan.hpp: the footer behind the container of a masked array (serialise, parse,
every refusal), the choice of the record's kind, the fill constant and the segment geometry of the fill.

tests/cpp/mask_plan_dump.cpp is compiled with g++ against the header alone (no HIP) and once more with
-fsanitize=address,undefined as a stand-alone binary. The expectations are tests/mask_model.py."""
import os
import subprocess

import numpy as np
import pytest

from tests import mask_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgard_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "mask_plan_dump.cpp")
NF = (1, 63, 64, 65, 1023, 1024, 1025, 2049)


def _build(tmp_path_factory, name, extra=()):
    exe = str(tmp_path_factory.mktemp(name) / "mask_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", CSRC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return _build(tmp_path_factory, "mask_plan")


def _run(exe, text):
    return subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=300).stdout.splitlines()


def _hex(b):
    return bytes(b).hex() or "-"


def test_header_compiles_alone_without_hip(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "mask_plan.hpp"\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", CSRC, str(src)])


# ---- footer ------------------------------------------------------------------------------------------------------
N = 1000                                                  # elements of the array the made-up container holds
CONTAINER = bytes(range(200, 256)) + b"MGARD" * 9          # 101 bytes standing in for a container
PACKED = bytes(np.random.default_rng(5).integers(0, 256, 8 * ((N + 63) // 64), dtype=np.uint8))
CODED = b"\x01\x02\x03" * 11                                # 33 bytes < 128


def _buffer(record, kind, n_masked=17, bits=0x7fc00000, container=CONTAINER):
    return container + record + mm.footer(len(container), record, n_masked, bits, kind)


def _open(dump, buf, n=N, is_double=0):
    return _run(dump, "open %d %d %s\n" % (n, is_double, _hex(buf)))[0]


def test_footer_serialises_as_the_restatement_and_round_trips(dump):
    cases = [(101, 17, 0x7fc00000, mm.PACKED, PACKED), (101, 3, 0x7ff8000000000000, mm.CODED, CODED),
             (2 ** 40 + 5, 0, 0, mm.NONE, b""), (1, 2 ** 32 - 1, 2 ** 64 - 1, mm.PACKED, b"\xff" * 8)]
    out = _run(dump, "".join("ser %d %d %d %d %s\n" % (c, nm, bits, kind, _hex(rec)) for c, nm, bits, kind, rec in cases))
    for line, (c, nm, bits, kind, rec) in zip(out, cases):
        want = mm.footer(c, rec, nm, bits, kind)
        assert len(want) == mm.FOOTER_BYTES and bytes.fromhex(line) == want
        assert mm.parse_footer(want) == dict(container=c, record=len(rec), n_masked=nm, restore_bits=bits, kind=kind,
                                             crc=mm.parse_footer(want)["crc"])
    for rec, kind, nm in ((PACKED, mm.PACKED, 17), (CODED, mm.CODED, 17), (b"", mm.NONE, 0)):
        assert _open(dump, _buffer(rec, kind, nm)) == "ok %d %d %d %d %d" % (len(CONTAINER), len(rec), nm, 0x7fc00000, kind)
    # a float64 array may carry 64 restore bits, a float32 array may not
    nan64 = 0x7ff8000000000000
    assert _open(dump, _buffer(PACKED, mm.PACKED, bits=nan64), is_double=1).startswith("ok ")
    assert _open(dump, _buffer(PACKED, mm.PACKED, bits=nan64), is_double=0).startswith("bad ")


def test_every_refusal(dump):
    good = _buffer(PACKED, mm.PACKED)
    assert _open(dump, good).startswith("ok ")
    # truncated by one byte: the magic is no longer where a footer ends -- not a masked buffer
    assert _open(dump, good[:-1]) == "none"
    assert _open(dump, good[1:]).startswith("bad ")       # ... and one byte short in front: C + R + 48 != size
    assert _open(dump, b"") == "none" and _open(dump, good[-47:]) == "none"
    # wrong magic
    assert _open(dump, good[:-1] + b"2") == "none"
    assert _open(dump, CONTAINER) == "none"
    # C + R + 48 != size
    assert "not the buffer" in _open(dump, good[:50] + b"\x00" + good[50:])
    f = mm.footer(len(CONTAINER) + 1, PACKED, 17, 0, mm.PACKED)
    assert "not the buffer" in _open(dump, CONTAINER + PACKED + f)
    f = mm.footer(2 ** 64 - 40, PACKED, 17, 0, mm.PACKED)   # (C + R wraps around)
    assert _open(dump, CONTAINER + PACKED + f).startswith("bad ")
    # R inconsistent with kind, and with the n of the container's header
    assert "kind 2" in _open(dump, _buffer(PACKED, mm.NONE, 0))
    assert "kind 2" in _open(dump, _buffer(b"", mm.NONE, 5))
    assert _open(dump, _buffer(b"", mm.PACKED)).startswith("bad ")
    assert "kind 0" in _open(dump, _buffer(PACKED[:-8], mm.PACKED))
    assert "kind 0" in _open(dump, _buffer(PACKED, mm.PACKED), n=N + 64)
    assert "kind 1" in _open(dump, _buffer(PACKED, mm.CODED))
    assert "unknown kind" in _open(dump, _buffer(PACKED, 3))
    assert "more masked" in _open(dump, _buffer(PACKED, mm.PACKED, N + 1))
    assert _open(dump, _buffer(PACKED, mm.PACKED, N)).startswith("ok ")
    # a flipped record byte fails the crc, wherever it is
    for at in (0, len(PACKED) // 2, len(PACKED) - 1):
        bad = bytearray(good)
        bad[len(CONTAINER) + at] ^= 0x10
        assert "CRC32" in _open(dump, bad)
    bad = bytearray(good)
    bad[3] ^= 0xff                                          # (the container is not the footer's business)
    assert _open(dump, bad).startswith("ok ")


def test_kind_constant_and_restore_bits(dump):
    nb = 8 * ((N + 63) // 64)
    rows = [(N, 0, 0, mm.NONE), (N, 0, 5, mm.NONE), (N, 7, 0, mm.PACKED), (N, 7, nb, mm.PACKED), (N, 7, nb + 1, mm.PACKED),
            (N, 7, nb - 1, mm.CODED), (N, N, 1, mm.CODED)]
    out = _run(dump, "".join("kind %d %d %d\n" % r[:3] for r in rows))
    assert [int(x) for x in out] == [r[3] for r in rows]
    # dictionary 256 under the single-pass encoder: 256 * 8 + chunk * 2 <= 140 KiB
    chunks = [0, 1, 1024, 20480, 70656, 70657, 2 ** 24, 2 ** 30]
    assert [int(x) for x in _run(dump, "".join("codable %d\n" % c for c in chunks))] == [0, 1, 1, 1, 1, 0, 0, 0]
    pairs = [(0.0, 0.0), (-1.0, 3.0), (1e308, 1.7e308), (-1.7e308, 1.7e308), (-0.0, -0.0), (5e-324, 5e-324), (-3.5, -3.5)]
    out = _run(dump, "".join("c %s %s\n" % (float(a).hex(), float(b).hex()) for a, b in pairs))
    for line, (a, b) in zip(out, pairs):
        want = 0.5 * np.float64(a) + 0.5 * np.float64(b)
        assert np.float64(float.fromhex(line)).view(np.int64) == np.float64(want).view(np.int64)
    vals = [(0, float("nan")), (1, float("nan")), (0, -9999.0), (1, 1e20), (0, 1e20), (0, float("inf")), (1, -0.0)]
    out = _run(dump, "".join("bits %d %s\n" % (d, float(v).hex()) for d, v in vals))
    for line, (d, v) in zip(out, vals):
        bits, back = line.split()
        dt = np.float64 if d else np.float32
        assert int(bits) == mm.value_bits(dt, v)
        assert mm.value_bits(dt, float.fromhex(back)) == int(bits)


# ---- segment geometry --------------------------------------------------------------------------------------------
def _shapes():
    return [(nf,) for nf in NF] + [(3, nf) for nf in NF] + [(7, 1025), (130, 65), (5, 9, 67), (2, 3, 2049), (3, 5, 9, 66)]


def _parse_seg(line):
    f = line.split()
    return int(f[0]), [tuple(int(x) for x in s.split(":")) for s in f[1:]]


def test_segment_geometry(dump):
    shapes = _shapes()
    out = _run(dump, "".join("seg %d %s\n" % (len(s), " ".join(map(str, s))) for s in shapes))
    for line, shape in zip(out, shapes):
        total, segs = _parse_seg(line)
        want = mm.segments(shape)
        assert total == len(want) == len(segs)
        assert [(s[0], s[1]) for s in segs] == want
        assert [s[2:] for s in segs] == [mm.segment_words(a, n) for a, n in want]
        n = int(np.prod(shape))
        # the segments tile the array in order, none crosses a row, none is longer than 1024, none touches more than
        # 17 words or a word the array does not have
        assert segs[0][0] == 0 and sum(s[1] for s in segs) == n
        for (a, ln, first, shift, nw), nxt in zip(segs, segs[1:] + [(n,)]):
            assert a + ln == nxt[0] and 1 <= ln <= mm.SEGMENT and a // shape[-1] == (a + ln - 1) // shape[-1]
            assert nw <= 17 and first + nw <= (n + 63) // 64 and (nw == 17 or not (ln == mm.SEGMENT and shift))
    # the misaligned case is there: a full segment that starts inside a word
    assert any(s[1] == mm.SEGMENT and s[3] != 0 for line in out for s in _parse_seg(line)[1])


def test_program_is_clean_under_address_and_undefined_sanitizers(tmp_path_factory):
    exe = _build(tmp_path_factory, "mask_plan_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    good = _buffer(PACKED, mm.PACKED)
    text = "".join("seg %d %s\n" % (len(s), " ".join(map(str, s))) for s in _shapes())
    for buf in (good, good[:-1], good[1:], b"", good[-48:], good[-47:], _buffer(b"", mm.NONE, 0), _buffer(CODED, mm.CODED),
                CONTAINER + PACKED + mm.footer(2 ** 64 - 40, PACKED, 17, 0, mm.PACKED)):
        text += "open %d 0 %s\n" % (N, _hex(buf))
    text += "ser 101 17 2143289344 0 %s\nser 5 0 0 2 -\nkind 1000 7 3\ncodable 20480\n" % _hex(PACKED)
    text += "c %s %s\nbits 0 nan\nbits 1 nan\n" % ((-1.5).hex(), (2.5).hex())
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-4000:]
    assert len(p.stdout.splitlines()) == text.count("\n")
