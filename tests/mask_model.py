"""NumPy restatement of the missing-value masks (include/mgard_hip.h: mgh_mask_scan / _fill / _restore, and the
trailer of mgard_amd/csrc/mask_plan.hpp), written from the text of the interface with a plain per-segment loop.
Nothing here looks at the library."""
import struct
import zlib

import numpy as np

NONFINITE, VALUE = 1, 2
SEGMENT = 1024
FOOTER_BYTES = 48
MAGIC = b"MGHMASK1"
PACKED, CODED, NONE = 0, 1, 2


def classify(data, nonfinite=True, fill_value=None):
    """Boolean mask of the data's shape: NaN / +-Inf and / or x == (T)fill_value."""
    m = np.zeros(data.shape, dtype=bool)
    if nonfinite:
        m |= ~np.isfinite(data)
    if fill_value is not None:
        m |= data == data.dtype.type(fill_value)
    return m


def packed_words(mask):
    """ceil(n / 64) uint64: bit i % 64 of word i / 64 for flat element i; the unused high bits zero."""
    flat = np.ascontiguousarray(mask).reshape(-1)
    nw = (flat.size + 63) // 64
    bits = np.zeros(nw * 64, dtype=np.uint8)
    bits[:flat.size] = flat
    return np.packbits(bits.reshape(nw, 64), axis=1, bitorder="little").view("<u8").reshape(nw)


def stats(data, mask):
    """(n, n_masked, vmin, vmax) over the valid elements, as doubles; -0.0 orders below +0.0; 0, 0 with none."""
    valid = data[~mask].astype(np.float64)
    if valid.size == 0:
        return data.size, int(mask.sum()), 0.0, 0.0
    vmin, vmax = float(valid.min()), float(valid.max())
    if vmin == 0.0:
        vmin = -0.0 if np.any((valid == 0) & np.signbit(valid)) else 0.0
    if vmax == 0.0:
        vmax = 0.0 if np.any((valid == 0) & ~np.signbit(valid)) else -0.0
    return data.size, int(mask.sum()), vmin, vmax


def fill_constant(data, mask):
    """(T)(0.5 vmin + 0.5 vmax), evaluated in double."""
    _, _, vmin, vmax = stats(data, mask)
    return data.dtype.type(0.5 * np.float64(vmin) + 0.5 * np.float64(vmax))


def fill(data, mask, c):
    """Rows along the last dimension, cut into segments of 1024 that restart at every row. A masked element takes the
    nearest valid element with a smaller index in its segment, else the nearest with a larger one, else c."""
    shape = data.shape if data.ndim else (1,)
    nf = shape[-1]
    out = np.array(data, copy=True).reshape(-1, nf)
    rows_mask = np.ascontiguousarray(mask).reshape(-1, nf)
    c = data.dtype.type(c)
    for r in range(out.shape[0]):
        if not rows_mask[r].any():
            continue
        for a in range(0, nf, SEGMENT):
            b = min(a + SEGMENT, nf)
            m = rows_mask[r, a:b]
            if not m.any():
                continue
            seg = out[r, a:b]
            valid = np.flatnonzero(~m)
            if valid.size == 0:
                seg[:] = c
                continue
            idx = np.flatnonzero(m)
            below = np.searchsorted(valid, idx)  # valid elements with a smaller index
            # the last of those; with none, every valid element lies above and the nearest is the first
            seg[idx] = seg[np.where(below > 0, valid[np.maximum(below, 1) - 1], valid[0])]
    return out.reshape(data.shape)


def restore(data, mask, value):
    out = np.array(data, copy=True)
    out[mask] = data.dtype.type(value)
    return out


def segments(shape):
    """[(flat start, length)] of every segment, row by row."""
    nf = shape[-1]
    rows = int(np.prod(shape[:-1], dtype=np.int64)) if len(shape) > 1 else 1
    return [(r * nf + a, min(SEGMENT, nf - a)) for r in range(rows) for a in range(0, nf, SEGMENT)]


def segment_words(start, length):
    """(first word, bit of its first element in that word, words it touches)"""
    return start >> 6, start & 63, ((start & 63) + length + 63) // 64


def int_view(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def value_bits(dtype, value):
    """The bits of (T)value, zero-extended."""
    v = np.array([value], dtype=dtype)
    return int(v.view(np.uint32 if v.dtype == np.float32 else np.uint64)[0])


# ---- trailer ------------------------------------------------------------------------------------------------
def footer(container, record, n_masked, restore_bits, kind):
    """u64 C | u64 R | u64 n_masked | u64 restore_bits | u32 kind | u32 crc32(record) | "MGHMASK1", little-endian."""
    return struct.pack("<QQQQII", container, len(record), n_masked, restore_bits, kind,
                       zlib.crc32(bytes(record)) & 0xffffffff) + MAGIC


def parse_footer(buf):
    """dict of the footer's fields, or None without the magic."""
    buf = bytes(buf[-FOOTER_BYTES:]) if len(buf) >= FOOTER_BYTES else b""
    if len(buf) < FOOTER_BYTES or buf[40:] != MAGIC:
        return None
    c, r, nm, bits, kind, crc = struct.unpack("<QQQQII", buf[:40])
    return dict(container=c, record=r, n_masked=nm, restore_bits=bits, kind=kind, crc=crc)
