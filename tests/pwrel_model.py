"""NumPy / Python restatement of the pointwise relative error bound (mgard_amd/csrc/pwrel_plan.hpp and the passes of
kernels_pwrel.hpp), written from the text of the interface: the classes of an element, the two bitmaps, the decode
rule, the tolerance delta and the trailer. Nothing here looks at the library."""
import math
import struct
import zlib

import numpy as np

from tests import mask_model as mm

FOOTER_BYTES = 56
MAGIC = b"MGHPWRL1"
VALID, ZEROED, NONFINITE = 0, 1, 2


def floor_eff(dtype, abs_floor):
    return max(float(abs_floor), float(np.finfo(dtype).tiny))


def classify(x, abs_floor=0.0):
    """int8 array of the data's shape: NONFINITE (NaN, +-Inf), ZEROED (|x| < floor_eff, in double), else VALID."""
    a = np.abs(x.astype(np.float64))
    cls = np.full(x.shape, VALID, dtype=np.int8)
    cls[a < floor_eff(x.dtype, abs_floor)] = ZEROED
    cls[~np.isfinite(x)] = NONFINITE
    return cls


def bitmaps(x, abs_floor=0.0):
    """(mask, flag) as boolean arrays: mask = not valid; flag = non-finite, or a negative valid element."""
    cls = classify(x, abs_floor)
    return cls != VALID, (cls == NONFINITE) | ((cls == VALID) & np.signbit(x))


def forward(x, abs_floor=0.0):
    """y = T(log2(float64(|x|))) at valid positions, 0 elsewhere."""
    cls = classify(x, abs_floor)
    y = np.zeros(x.shape, dtype=x.dtype)
    v = cls == VALID
    y[v] = np.log2(np.abs(x[v].astype(np.float64))).astype(x.dtype)
    return y


def inverse(y, mask, flag):
    """NaN (mask and flag), +0.0 (mask), else +-T(exp2(float64(y))) clamped to [smallest normal, largest finite]."""
    fi = np.finfo(y.dtype)
    with np.errstate(over="ignore", under="ignore"):
        mag = np.exp2(y.astype(np.float64))
    mag = np.clip(mag, float(fi.tiny), float(fi.max)).astype(y.dtype)
    out = np.where(flag, -mag, mag)
    out[mask] = 0.0
    out[mask & flag] = np.nan
    return out.astype(y.dtype)


def filled(x, abs_floor=0.0):
    """The array the container holds: y with the masked writer's fill (tests/mask_model.py) at the masked positions."""
    mask, _ = bitmaps(x, abs_floor)
    y = forward(x, abs_floor)
    return mm.fill(y, mask, mm.fill_constant(y, mask))


def ybound(x, abs_floor=0.0):
    """max |y| over the valid elements; -1 when there is none."""
    mask, _ = bitmaps(x, abs_floor)
    y = forward(x, abs_floor)
    return float(np.max(np.abs(y[~mask]))) if (~mask).any() else -1.0


# ---- tolerance -----------------------------------------------------------------------------------------------
def ulp(dtype, v):
    v = abs(v)
    if np.dtype(dtype) == np.float64:
        return math.nextafter(v, math.inf) - v
    f = np.float32(v)
    return float(np.nextafter(f, np.float32(np.inf))) - float(f)


def e2(dtype):
    return 2.0 ** -52 if np.dtype(dtype) == np.float64 else 2.0 ** -23


def log2_1p(eps):
    return math.log1p(eps) / 0.6931471805599453 * (1.0 - 2.0 ** -50)


K_MIN = 64.0     # the smallest delta the container is handed, in ulp_T(ybound)


def budget(dtype, eps, yb):
    """B = log2(1 + eps) - ulp_T(ybound) - 1.5 E2 rounded down: what |y' - y| may use."""
    d = log2_1p(eps) - ulp(dtype, yb) - 1.5 * e2(dtype)
    return math.nextafter(math.nextafter(d, -math.inf), -math.inf)


def abs_tolerance(dtype, eps, yb, k_min=K_MIN):
    """delta = B, or None where the call is refused: delta < k_min ulp_T(ybound) (the container's own rounding, measured
    in tests/test_pwrel_rounding_cpu.py) or delta < 0.5 log2(1 + eps). yb < 0: nothing is valid and delta =
    log2(1 + eps). k_min=0 is the rule before the container's rounding was measured."""
    if not (math.isfinite(eps) and 0.0 < eps < 1.0):
        return None
    L = log2_1p(eps)
    if yb < 0:
        return L
    d = budget(dtype, eps, yb)
    return None if d < k_min * ulp(dtype, yb) or d < 0.5 * L else d


def smallest_accepted_eps(dtype, yb, rel=0.01):
    """An eps abs_tolerance accepts at this ybound, no more than `rel` above the smallest one it accepts (bisection;
    acceptance is monotone in eps)."""
    lo, hi = 2.0 ** -60, 0.5
    assert abs_tolerance(dtype, lo, yb) is None and abs_tolerance(dtype, hi, yb) is not None
    while hi > lo * (1.0 + rel):
        mid = math.sqrt(lo * hi)
        lo, hi = (lo, mid) if abs_tolerance(dtype, mid, yb) is not None else (mid, hi)
    return hi


# ---- the writer's path for y, through the CPU oracle ------------------------------------------------------------
def oracle_y_errors(x, deltas, abs_floor=0.0):
    """The container's part of the writer, restated with oracle.Hierarchy (which tests/test_gpu_parity.py pins the GPU
    transform to, bit for bit): y = the filled T(log2|x|) -> decompose -> for every delta in `deltas`: quantize (ABS,
    s = inf, norm 1, dictionary 8192) -> dequantize -> recompose. Everything runs in T; the differences are taken in
    float64, where they are exact. Returns (ybound, [max |y' - y| over the VALID elements, one per delta]); a delta
    of None leaves the quantizer out (decompose -> recompose alone)."""
    import oracle
    dt = x.dtype.type
    mask, _ = bitmaps(x, abs_floor)
    y = filled(x, abs_floor)
    h = oracle.Hierarchy(x.shape, x.dtype)
    c = h.decompose(y)
    yd = y.astype(np.float64)
    errs = []
    for delta in deltas:
        back = c
        if delta is not None:
            args = (oracle.ABS, dt(delta), dt(np.inf), dt(1))
            q, oi, ov, _ = h.quantize(c, *args, dict_size=8192)
            back = h.dequantize(q, *args, dict_size=8192, outlier_idx=oi, outlier_val=ov)
        errs.append(float(np.max(np.abs(h.recompose(back).astype(np.float64) - yd)[~mask])))
    return ybound(x, abs_floor), errs


# ---- trailer -------------------------------------------------------------------------------------------------
def footer(masked, record, n_flag, eps, abs_floor, kind):
    """u64 M | u64 S | u64 n_flag | f64 eps | f64 abs_floor | u32 kind | u32 crc32(record) | "MGHPWRL1", little-endian."""
    return struct.pack("<QQQddII", masked, len(record), n_flag, eps, abs_floor, kind,
                       zlib.crc32(bytes(record)) & 0xffffffff) + MAGIC


def parse_footer(buf):
    """dict of the footer's fields, or None without the magic."""
    buf = bytes(buf[-FOOTER_BYTES:]) if len(buf) >= FOOTER_BYTES else b""
    if len(buf) < FOOTER_BYTES or buf[48:] != MAGIC:
        return None
    m, s, nf, eps, floor, kind, crc = struct.unpack("<QQQddII", buf[:48])
    return dict(masked=m, record=s, n_flag=nf, eps=eps, abs_floor=floor, kind=kind, crc=crc)


# ---- compare -------------------------------------------------------------------------------------------------
def compare(x, r, abs_floor=0.0):
    """dict of mgh_pwrel_compare's fields for the original x and the reconstruction r, in float64."""
    x, r = x.reshape(-1), r.reshape(-1)
    cls = classify(x, abs_floor)
    xd, rd = x.astype(np.float64), r.astype(np.float64)
    valid, zeroed, nonfin = cls == VALID, cls == ZEROED, cls == NONFINITE
    ok = np.isfinite(r) & (r != 0)
    plus_zero = (r == 0) & ~np.signbit(r)
    meas = valid & np.isfinite(r)
    with np.errstate(all="ignore"):
        rel = np.where(meas, np.abs(rd - xd) / np.where(meas, np.abs(xd), 1.0), -1.0)
    return dict(n=x.size, n_valid=int(valid.sum()), n_zeroed=int(zeroed.sum()), n_nonfinite=int(nonfin.sum()),
                max_rel_err=float(rel.max()) if meas.any() else 0.0, argmax=int(np.argmax(rel)) if meas.any() else 0,
                rel=rel, max_zeroed_abs=float(np.abs(xd[zeroed]).max()) if zeroed.any() else 0.0,
                n_class_mismatch=int((zeroed & ~plus_zero).sum() + (nonfin & ~np.isnan(r)).sum() + (valid & ~ok).sum()),
                n_sign_mismatch=int((valid & ok & (np.signbit(r) != np.signbit(x))).sum()))


# ---- test fields ---------------------------------------------------------------------------------------------
def specials(dtype, abs_floor):
    """The planted values: +-0, a denormal, +-smallest normal, +-largest finite, NaN, +-Inf, one value just below and one
    exactly at abs_floor."""
    fi = np.finfo(dtype)
    t = np.dtype(dtype).type
    below = np.nextafter(t(abs_floor), t(0)) if abs_floor else t(0)
    return np.array([0.0, -0.0, fi.smallest_subnormal * 3, fi.tiny, -fi.tiny, fi.max, -fi.max, np.nan, np.inf, -np.inf,
                     below, t(abs_floor)], dtype=dtype)


def plant(x, abs_floor):
    """x with the special values at fixed flat indices: the first and the last element and both sides of every word
    boundary that exists, cycling through the values."""
    flat = x.reshape(-1)
    n = flat.size
    sp = specials(x.dtype, abs_floor)
    where = [i for i in (0, n - 1, 63, 64, 65, 127, 128, 1, 2, 3, 5, 8, 13, 21, 34, 55, 62, 66) if 0 <= i < n]
    where = list(dict.fromkeys(where))
    for k, i in enumerate(where):
        flat[i] = sp[k % len(sp)]
    return x


def decades_field(shape, dtype, seed=0, abs_floor=0.0, planted=True):
    """Magnitudes 10^U(-30, 30) (float32) or 10^U(-300, 300) (float64) with random signs, the special values planted
    (planted=False: every element is valid)."""
    rng = np.random.default_rng(seed)
    span = 30 if np.dtype(dtype) == np.float32 else 300
    x = (10.0 ** rng.uniform(-span, span, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(dtype)
    return plant(x, abs_floor) if planted else x


def smooth_field(shape, dtype, abs_floor=0.0, negative=True, planted=True):
    """exp of a few sine modes (smooth in the exponent, many decades) times a blocky sign pattern."""
    span = 25.0 if np.dtype(dtype) == np.float32 else 200.0
    g = np.meshgrid(*[np.linspace(0.0, 1.0, e) for e in shape], indexing="ij")
    e = sum(np.sin(2 * np.pi * (k + 1) * a + 0.3 * k) / (k + 1) for k, a in enumerate(g))
    e = e / max(1e-30, np.max(np.abs(e)))
    x = 10.0 ** (span * e)
    if negative:
        x = x * np.where(sum(np.floor(4 * a) for a in g) % 2 == 0, 1.0, -1.0)
    x = x.astype(dtype)
    return plant(x, abs_floor) if planted else x
