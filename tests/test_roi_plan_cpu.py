"""CPU test of mgard_amd/csrc/roi_plan.hpp: the rules of the boxes (one case per refusal), the tolerance of a box's
residual against the same formula in Python to the bit (both refusal edges and R = 0 included), the box table and
footer (serialise, parse, every truncation and every flipped size field), and the three footers' magics, each of
which the other two reject.

tests/cpp/roi_plan_dump.cpp is compiled with g++ against the header alone (no HIP) and once more with
-fsanitize=address,undefined as a stand-alone binary. The expectations are tests/roi_model.py."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import mask_model as mm
from tests import pwrel_model as pm
from tests import roi_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgard_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "roi_plan_dump.cpp")
INF = float("inf")


def _build(tmp_path_factory, name, extra=()):
    exe = str(tmp_path_factory.mktemp(name) / "roi_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", CSRC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return _build(tmp_path_factory, "roi_plan")


def _run(exe, text):
    return subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=300).stdout.splitlines()


def _hex(b):
    return bytes(b).hex() or "-"


def test_header_compiles_alone_without_hip(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "roi_plan.hpp"\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", CSRC, str(src)])


# ---- the boxes ---------------------------------------------------------------------------------------------------
SHAPE = (33, 40, 65)
GOOD = ((4, 5, 3), (17, 25, 57), 1e-4)


def _chk_line(shape, tol, s, boxes, nbox=None):
    words = ["chk", len(shape), *shape, float(tol).hex(), float(s).hex(), len(boxes) if nbox is None else nbox]
    for lo, ext, t in boxes:
        words += [*lo, *ext, float(t).hex()]
    return " ".join(str(w) for w in words) + "\n"


BOX_CASES = [
    # (id, shape, tol, s, boxes, word of the refusal or None)
    ("good", SHAPE, 1e-2, INF, [GOOD], None),
    ("sixteen-boxes", (100, 9), 1e-2, INF, [((6 * i, 0), (3, 9), 1e-3) for i in range(16)], None),
    ("touching-boxes", SHAPE, 1e-2, INF, [((0, 0, 0), (9, 40, 65), 1e-3), ((9, 0, 0), (9, 40, 65), 1e-4)], None),
    ("whole-array", SHAPE, 1e-2, INF, [((0, 0, 0), SHAPE, 1e-3)], None),
    ("no-box", SHAPE, 1e-2, INF, [], "nbox must be in 1 .. 16"),
    ("seventeen-boxes", (200, 9), 1e-2, INF, [((6 * i, 0), (3, 9), 1e-3) for i in range(17)], "nbox must be in 1 .. 16"),
    ("leaves-the-array", SHAPE, 1e-2, INF, [((4, 5, 9), (17, 25, 57), 1e-4)], "leaves the array"),
    ("starts-outside", SHAPE, 1e-2, INF, [((33, 5, 3), (3, 3, 3), 1e-4)], "leaves the array"),
    ("huge-extent", SHAPE, 1e-2, INF, [((4, 5, 3), (2 ** 64 - 2, 25, 57), 1e-4)], "leaves the array"),
    ("extent-two", SHAPE, 1e-2, INF, [((4, 5, 3), (17, 2, 57), 1e-4)], "at least 3"),
    ("extent-zero", SHAPE, 1e-2, INF, [((4, 5, 3), (17, 25, 0), 1e-4)], "at least 3"),
    ("overlap", SHAPE, 1e-2, INF, [GOOD, ((20, 29, 59), (3, 3, 3), 1e-3)], "pairwise disjoint"),
    ("same-box-twice", SHAPE, 1e-2, INF, [GOOD, GOOD], "pairwise disjoint"),
    ("tol-not-tighter", SHAPE, 1e-2, INF, [((4, 5, 3), (17, 25, 57), 1e-2)], "0 < tol_i < tol"),
    ("tol-zero", SHAPE, 1e-2, INF, [((4, 5, 3), (17, 25, 57), 0.0)], "0 < tol_i < tol"),
    ("tol-negative", SHAPE, 1e-2, INF, [((4, 5, 3), (17, 25, 57), -1e-4)], "0 < tol_i < tol"),
    ("tol-nan", SHAPE, 1e-2, INF, [((4, 5, 3), (17, 25, 57), float("nan"))], "0 < tol_i < tol"),
    ("s-zero", SHAPE, 1e-2, 0.0, [GOOD], "s must be infinite"),
    ("s-one", SHAPE, 1e-2, 1.0, [GOOD], "s must be infinite"),
    ("s-minus-inf", SHAPE, 1e-2, -INF, [GOOD], "s must be infinite"),
    ("s-nan", SHAPE, 1e-2, float("nan"), [GOOD], "s must be infinite"),
    ("2^32-elements", (65536, 65536), 1e-2, INF, [((0, 0), (3, 3), 1e-3)], "2^32 - 1 elements"),
    ("2^32-1-elements", (65537, 65535), 1e-2, INF, [((0, 0), (3, 3), 1e-3)], None),
]


@pytest.mark.parametrize("name,shape,tol,s,boxes,refusal", BOX_CASES, ids=[c[0] for c in BOX_CASES])
def test_box_rules(dump, name, shape, tol, s, boxes, refusal):
    out = _run(dump, _chk_line(shape, tol, s, boxes))[0]
    want = rm.check_boxes(shape, tol, s, boxes)
    assert want == refusal                                       # (the model agrees with the table)
    assert out == "ok" if refusal is None else (out.startswith("bad compress_roi: ") and refusal in out), out


def test_footprint(dump):
    out = _run(dump, "fit 1000 2000\nfit 1000 1999\nfit 0 0\nfit 9223372036854775808 18446744073709551615\n"
                     "fit 9223372036854775807 18446744073709551615\n")
    assert out[0] == "ok" and "not streamed in parts" in out[1] and out[2] == "ok"
    assert out[3].startswith("bad ") and out[4] == "ok"


# ---- tolerance ---------------------------------------------------------------------------------------------------
def _tol(dump, rows):
    out = _run(dump, "".join("tol %d %s %s %s\n" % (d, float(a).hex(), float(r).hex(), float(m).hex()) for d, a, r, m in rows))
    return [float.fromhex(o.split()[1]) if o.startswith("ok ") else None for o in out], out


def _dt(d):
    return np.float64 if d else np.float32


def test_tolres_is_the_formula_to_the_bit(dump):
    rng = np.random.default_rng(5)
    rows = [(d, a, r, m) for d in (0, 1) for a in (1e-4, 2.5e-4, 1e-2, 3.0) for r in (0.0, 1e-6, 1e-3, 2e-2, 1.0)
            for m in (0.0, 1.0, 2.5, 1000.0, 1e6)]
    rows += [(int(d), 10.0 ** a, 10.0 ** r, 10.0 ** m) for d, a, r, m in
             zip(rng.integers(0, 2, 400), rng.uniform(-12, 2, 400), rng.uniform(-14, 3, 400), rng.uniform(-3, 8, 400))]
    got, out = _tol(dump, rows)
    want = [rm.tolres(_dt(d), a, r, m) for d, a, r, m in rows]
    assert got == want
    assert sum(w is None for w in want) > 50 and sum(w is not None for w in want) > 200
    assert all("cannot carry" in o for o, w in zip(out, want) if w is None)
    for (d, a, r, m), t in zip(rows, want):
        if t is not None and r > 0:
            assert 0.5 * a <= t < a and t >= 64 * rm.ulp(_dt(d), r)
            # the inequality it exists for: tolres + u(R) / 2 + u(M + A) / 2 <= A, in exact rational arithmetic
            from fractions import Fraction as F
            assert F(t) + F(rm.ulp(_dt(d), r)) / 2 + F(rm.ulp(_dt(d), m + a)) / 2 <= F(a)


def test_tolres_refusal_edges_and_zero_residual(dump):
    # R = 0: nothing is stored, tolres = A, whatever M is (the base is exact there)
    got, _ = _tol(dump, [(0, 1e-4, 0.0, 1.0), (0, 1e-9, 0.0, 1e6), (1, 1e-300, 0.0, 1e300)])
    assert got == [1e-4, 1e-9, 1e-300]
    for d in (0, 1):
        dt = _dt(d)
        # edge 1: tolres < A / 2 -- with R tiny, u(M + A) / 2 takes half of A where A = u(M + A), just beyond it
        m = 1.0
        u = rm.ulp(dt, m)
        for a, ok in ((1.01 * u, True), (0.99 * u, False)):
            got, out = _tol(dump, [(d, a, a * 2.0 ** -30, m)])
            assert (got[0] is not None) == ok == (rm.tolres(dt, a, a * 2.0 ** -30, m) is not None), (d, a, out)
            assert ok or "cannot carry" in out[0]
        # edge 2: tolres < 64 u(R) -- M = 0 and R = A, so tolres is about A (1 - eps) and 64 u(R) about 64 eps A: held;
        # with the residual 2^k times the bound, 64 ulps of R (64 * 2^-23 R or less for float, 2^-52 for double) outgrow
        # the bound at k = 17 or 18 (float), 46 or 47 (double), by where a 2^k lies in its binade
        a = 1e-3
        ks = [k for k in range(60) if rm.tolres(dt, a, a * 2.0 ** k, 0.0) is not None]
        last = max(k for k in range(60) if 64 * rm.ulp(dt, a * 2.0 ** k) <= 0.999 * a)
        assert ks == list(range(last + 1)) and last in ((16, 17) if d == 0 else (45, 46))
        got, out = _tol(dump, [(d, a, a * 2.0 ** max(ks), 0.0), (d, a, a * 2.0 ** (max(ks) + 1), 0.0)])
        assert got[0] == rm.tolres(dt, a, a * 2.0 ** max(ks), 0.0) and got[1] is None and "64 ulps" in out[1]
    # bad statistics and bounds
    _, out = _tol(dump, [(0, 0.0, 1.0, 1.0), (0, INF, 1.0, 1.0), (0, 1e-3, float("nan"), 1.0), (0, 1e-3, 1.0, INF), (1, 1e-3, -1.0, 1.0)])
    assert all(o.startswith("bad roi: ") for o in out)
    # the float refusal of the documents: 1e-9 of a norm of 2.5 with values up to 2.5
    assert rm.tolres(np.float32, 2.5e-9, 1e-2, 2.5) is None and rm.tolres(np.float64, 2.5e-9, 1e-2, 2.5) is not None


# ---- table and footer --------------------------------------------------------------------------------------------
CONT = bytes(range(7, 207))                                   # 200 bytes standing in for a container
REC0, REC1 = bytes(np.random.default_rng(3).integers(0, 256, 77, dtype=np.uint8)), b"\x01\x02\x03" * 11
BOXES = [((4, 5, 3), (17, 25, 57), 1e-4, 9.5e-5, REC0), ((30, 0, 0), (3, 40, 65), 1e-3, 9.9e-4, b""),
         ((0, 0, 60), (3, 3, 5), 2e-3, 1.5e-3, REC1)]


def _ser_line(container, boxes):
    words = ["ser", container, len(boxes)]
    for lo, ext, tol, tr, rec in boxes:
        words += [*rm._aligned(lo, 0), *rm._aligned(ext, 1), float(tol).hex(), float(tr).hex(), _hex(rec)]
    return " ".join(str(w) for w in words) + "\n"


def _open(dump, buf, shape=SHAPE):
    return _run(dump, "open %d %s %s\n" % (len(shape), " ".join(str(e) for e in shape), _hex(buf)))[0]


def test_trailer_serialises_as_the_model_and_round_trips(dump):
    for container, boxes in ((len(CONT), BOXES), (2 ** 40 + 5, BOXES[:1]), (1, [((7,), (9,), 0.5, 0.25, b"")] * 16)):
        got = bytes.fromhex(_run(dump, _ser_line(container, boxes))[0])
        assert got == rm.trailer(container, boxes) and len(got) == 120 * len(boxes) + 40
    buf = rm.buffer(CONT, BOXES)
    f = _open(dump, buf).split()
    assert f[:3] == ["ok", str(len(CONT)), "3"]
    model = rm.parse(buf)
    assert model["container"] == len(CONT)
    at = len(CONT)
    for i, (lo, ext, tol, tr, rec) in enumerate(BOXES):
        w = f[3 + 14 * i:3 + 14 * (i + 1)]
        assert [int(v) for v in w[:10]] == rm._aligned(lo, 0) + rm._aligned(ext, 1) == list(model["boxes"][i]["lo"] + model["boxes"][i]["ext"])
        assert [float.fromhex(v) for v in w[10:12]] == [tol, tr] and [int(v) for v in w[12:]] == [at, len(rec)]
        at += len(rec)


def test_every_truncation_is_refused(dump):
    buf = rm.buffer(CONT, BOXES)
    lines = _run(dump, "".join("open 3 33 40 65 %s\n" % _hex(buf[:n]) for n in range(len(buf))))
    assert all(l == "none" or l.startswith("bad ") for l in lines), [l for l in lines if l.startswith("ok")]
    # ... and from the front, where the magic stays in place: the sizes no longer add up
    lines = _run(dump, "".join("open 3 33 40 65 %s\n" % _hex(buf[n:]) for n in range(1, len(buf) - 40, 7)))
    assert all(l.startswith("bad ") for l in lines)


def test_every_flipped_size_field_is_refused(dump):
    buf = rm.buffer(CONT, BOXES)
    table_at = len(buf) - 40 - 120 * len(BOXES)
    foot = len(buf) - 40

    def patched(at, fmt, value, fix_crc):
        b = bytearray(buf)
        b[at:at + struct.calcsize(fmt)] = struct.pack(fmt, value)
        if fix_crc:  # (a forger who recomputes the table's CRC: the sizes themselves must be caught)
            import zlib
            b[foot + 24:foot + 28] = struct.pack("<I", zlib.crc32(bytes(b[table_at:foot])) & 0xffffffff)
        return bytes(b)

    texts = []
    # the footer: container, nbox, table_bytes, the padding
    for at, values in ((foot, (0, len(CONT) - 1, len(CONT) + 1, len(buf), 2 ** 63, 2 ** 64 - 1)),
                       (foot + 8, (0, 2, 4, 17, 2 ** 32 + 3, 2 ** 64 - 1)),
                       (foot + 16, (0, 120, 359, 361, 480, 2 ** 64 - 120, 2 ** 64 - 1))):
        texts += [patched(at, "<Q", v, False) for v in values]
    texts.append(patched(foot + 28, "<I", 1, False))
    # the table, with its CRC made right again: every offset and size, an extent of 0, a box that leaves the array,
    # a leading dimension that is not (0, 1), a tolerance that is no tolerance, the padding
    for i in range(len(BOXES)):
        e = table_at + 120 * i
        off, size = struct.unpack("<QQ", buf[e + 96:e + 112])
        for v in (off + 1, off - 1, 0, 2 ** 64 - 1):
            texts.append(patched(e + 96, "<Q", v, True))
        for v in (size + 1, size + 10 ** 6, 2 ** 64 - 1, 2 ** 64 - off) + ((size - 1,) if size else ()):
            texts.append(patched(e + 104, "<Q", v, True))
        texts.append(patched(e + 40 + 8 * 4, "<Q", 0, True))
        texts.append(patched(e + 40 + 8 * 4, "<Q", 2 ** 40, True))
        texts.append(patched(e + 8 * 2, "<Q", 33, True))
        texts.append(patched(e + 40 + 8 * 3, "<Q", 41, True))
        texts.append(patched(e, "<Q", 1, True))
        texts.append(patched(e + 40, "<Q", 2, True))
        texts.append(patched(e + 80, "<d", float("nan"), True))
        texts.append(patched(e + 88, "<d", -1.0, True))
        texts.append(patched(e + 116, "<I", 7, True))
    # ... and without the fix, any flipped table byte fails the CRC; a flipped record byte its record's
    texts += [patched(table_at + k, "<B", buf[table_at + k] ^ 0x20, False) for k in range(0, 360, 13)]
    lines = _run(dump, "".join("open 3 33 40 65 %s\n" % _hex(t) for t in texts))
    assert len(lines) == len(texts) and all(l.startswith("bad ") for l in lines), [l for l in lines if not l.startswith("bad ")]
    for at in (len(CONT), len(CONT) + 76, len(CONT) + 77, len(CONT) + 77 + 32):
        assert "roi record: CRC32" in _open(dump, patched(at, "<B", buf[at] ^ 1, False))
    assert _open(dump, patched(3, "<B", 0, False)).startswith("ok ")   # (the container is not this footer's business)
    # the array of the container's header decides whether a box fits
    assert "leaves the array" in _open(dump, buf, (33, 40, 64)) and "more dimensions" in _open(dump, buf, (40, 65))


def test_the_three_magics_reject_each_other(dump):
    masked = CONT + mm.footer(len(CONT), b"", 0, 0, mm.NONE)
    pwrel = masked + pm.footer(len(masked), b"", 0, 1e-3, 0.0, mm.NONE)
    roi = rm.buffer(CONT, BOXES)
    out = _run(dump, "".join("magic %s\n" % _hex(b) for b in (masked, pwrel, roi, CONT, b"", rm.MAGIC, pm.MAGIC, mm.MAGIC)))
    assert out == ["100", "010", "001", "000", "000", "000", "000", "000"]
    assert len({rm.MAGIC, pm.MAGIC, mm.MAGIC}) == 3
    # a buffer with boxes whose container part is a masked or pointwise-relative buffer still ends in the box magic only
    assert _run(dump, "magic %s\n" % _hex(rm.buffer(pwrel, BOXES[:1])))[0] == "001"
    assert _open(dump, masked) == "none" and _open(dump, pwrel) == "none"


def test_program_is_clean_under_address_and_undefined_sanitizers(tmp_path_factory):
    exe = _build(tmp_path_factory, "roi_plan_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    buf = rm.buffer(CONT, BOXES)
    foot = len(buf) - 40
    text = "".join(_chk_line(shape, tol, s, boxes) for _, shape, tol, s, boxes, _ in BOX_CASES)
    text += "fit 1000 1999\nfit 5 10\n"
    text += "".join("tol %d %s %s %s\n" % (d, float(a).hex(), float(r).hex(), float(m).hex())
                    for d in (0, 1) for a in (1e-9, 1e-4) for r in (0.0, 1e-3, 1e30) for m in (0.0, 2.5))
    text += "tol 0 nan 0x1p0 0x1p0\n"
    text += _ser_line(len(CONT), BOXES) + _ser_line(5, [])
    for n in list(range(0, 60)) + list(range(len(buf) - 45, len(buf) + 1)):
        text += "open 3 33 40 65 %s\n" % _hex(buf[:n])
    for at, v in ((foot, 2 ** 64 - 1), (foot + 8, 2 ** 64 - 1), (foot + 16, 2 ** 64 - 120), (foot + 8, 16), (foot + 16, 1920)):
        b = bytearray(buf)
        b[at:at + 8] = struct.pack("<Q", v)
        text += "open 3 33 40 65 %s\n" % _hex(b)
    text += "magic %s\nmagic -\nmagic %s\n" % (_hex(buf), _hex(buf[-20:]))
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-4000:]
    assert len(p.stdout.splitlines()) == text.count("\n")
