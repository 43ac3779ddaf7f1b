"""Python restatement of the region of interest (mgard_amd/csrc/roi_plan.hpp), written from the text of the interface:
the rules of the boxes, the tolerance of a box's residual, and the box table and footer behind the records. Nothing
here looks at the library."""
import math
import struct
import zlib

import numpy as np

FOOTER_BYTES = 40
ENTRY_BYTES = 120
MAGIC = b"MGHROI01"
MAX_BOXES = 16
MAX_DIM = 5
MIN_ULPS = 64.0          # the measured limit of the container path (pwrel_plan.hpp: kPwrelMinUlps)


def ulp(dtype, v):
    """the distance from |v| to the next larger number of `dtype`, |v| rounded UP to it first"""
    v = abs(float(v))
    if dtype == np.float64:
        return math.nextafter(v, math.inf) - v
    f = np.float32(v)
    if float(f) < v:
        f = np.nextafter(f, np.float32(np.inf))
    return float(np.nextafter(f, np.float32(np.inf))) - float(f)


def tolres(dtype, A, R, M):
    """tolres of a box with absolute bound A, R = max |r|, M = max |x|; None where the call is refused"""
    if R == 0:
        return float(A)
    uR, uX = ulp(dtype, R), ulp(dtype, M + A)
    t = math.nextafter(A - 0.5 * uR - 0.5 * uX, -math.inf)
    if not t >= 0.5 * A or not t >= MIN_ULPS * uR:
        return None
    return t


def check_boxes(shape, tol, s, boxes):
    """None, or a word of the refusal: boxes = [(lo, ext, tol_i), ...]"""
    if not (math.isinf(s) and s > 0):
        return "s must be infinite"
    if not (math.isfinite(tol) and tol > 0):
        return "tol must be positive"
    if int(np.prod([int(e) for e in shape], dtype=object)) >= 2 ** 32 or min(shape) == 0:
        return "2^32 - 1 elements"
    if not 1 <= len(boxes) <= MAX_BOXES:
        return "nbox must be in 1 .. 16"
    for lo, ext, t in boxes:
        for a, e, n in zip(lo, ext, shape):
            if a >= n or e > n - a:
                return "leaves the array"
            if e < 3:
                return "at least 3"
        if not (t > 0 and t < tol):
            return "0 < tol_i < tol"
    for i, (lo, ext, _) in enumerate(boxes):
        for lo2, ext2, _ in boxes[i + 1:]:
            if all(a < b + f and b < a + e for a, e, b, f in zip(lo, ext, lo2, ext2)):
                return "pairwise disjoint"
    return None


def _aligned(values, lead):
    return [lead] * (MAX_DIM - len(values)) + [int(v) for v in values]


def entry(lo, ext, tol, tolres_, offset, record):
    return struct.pack("<5Q5QddQQII", *_aligned(lo, 0), *_aligned(ext, 1), tol, tolres_, offset, len(record),
                       zlib.crc32(bytes(record)) & 0xffffffff, 0)


def trailer(container, boxes):
    """table and footer: boxes = [(lo, ext, tol, tolres, record bytes), ...], the records back to back behind the container"""
    table, at = b"", container
    for lo, ext, tol, tr, rec in boxes:
        table += entry(lo, ext, tol, tr, at, rec)
        at += len(rec)
    return table + struct.pack("<QQQII", container, len(boxes), len(table), zlib.crc32(table) & 0xffffffff, 0) + MAGIC


def buffer(container_bytes, boxes):
    return bytes(container_bytes) + b"".join(bytes(b[4]) for b in boxes) + trailer(len(container_bytes), boxes)


def parse(buf):
    """dict(container, boxes=[dict(lo, ext, tol, tolres, offset, size, crc)]) of a well-formed buffer"""
    buf = bytes(buf)
    assert buf[-8:] == MAGIC
    container, nbox, tb, crc, pad = struct.unpack("<QQQII", buf[-FOOTER_BYTES:-8])
    table = buf[len(buf) - FOOTER_BYTES - tb:len(buf) - FOOTER_BYTES]
    assert tb == nbox * ENTRY_BYTES and zlib.crc32(table) & 0xffffffff == crc and pad == 0
    boxes = []
    for i in range(nbox):
        f = struct.unpack("<5Q5QddQQII", table[i * ENTRY_BYTES:(i + 1) * ENTRY_BYTES])
        boxes.append(dict(lo=f[0:5], ext=f[5:10], tol=f[10], tolres=f[11], offset=f[12], size=f[13], crc=f[14]))
    return dict(container=container, boxes=boxes)
