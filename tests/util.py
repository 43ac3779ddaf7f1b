"""Shared helpers for the tests: seeded synthetic fields."""
import numpy as np


def smooth_field(shape, dtype=np.float32, seed=20260101, noise=1e-3):
    """u = sin(2*pi*3x) cos(2*pi*2y) + 0.5 sin(2*pi*5z) + noise*xi on the unit cube; for other
    dimensionalities the same recipe is applied to the trailing dims that exist."""
    rng = np.random.default_rng(seed)
    D = len(shape)
    ax = [np.arange(n, dtype=np.float64) / max(n - 1, 1) for n in shape]
    grids = np.meshgrid(*ax, indexing="ij", sparse=True)
    f = [3.0, 2.0, 5.0, 1.0, 4.0]
    u = np.zeros(shape, dtype=np.float64)
    u = u + np.sin(2 * np.pi * f[0] * grids[D - 1])
    if D >= 2:
        u = u * np.cos(2 * np.pi * f[1] * grids[D - 2])
    if D >= 3:
        u = u + 0.5 * np.sin(2 * np.pi * f[2] * grids[D - 3])
    for d in range(D - 3):
        u = u + 0.25 * np.cos(2 * np.pi * f[3 + (d % 2)] * grids[d])
    u = u + noise * rng.uniform(-1, 1, size=shape)
    return np.ascontiguousarray(u.astype(dtype))


def nonuniform_coords(shape, dtype=np.float64, seed=7):
    """x_i = (i + 0.3*zeta_i)/(n-1), zeta ~ U(-1,1): strictly increasing."""
    rng = np.random.default_rng(seed)
    out = []
    for n in shape:
        z = rng.uniform(-1, 1, size=n)
        out.append(((np.arange(n) + 0.3 * z) / (n - 1)).astype(dtype))
    return out


def inside_field(shape, dtype=np.float32, seed=1):
    """A field whose quantized coefficients stay inside an 8192-entry dictionary at 1e-3 in 4-D / 5-D and on
    short extents too (the quantizer's bins shrink with 1 + 3^D; smooth_field puts whole periods across
    extents of a few nodes): one period of a sine across every extent of 32 and more points, 1 % of that
    across the short ones, 1e-3 uniform noise."""
    ax = np.meshgrid(*[np.arange(n, dtype=np.float64) / max(n - 1, 1) for n in shape], indexing="ij", sparse=True)
    g = sum((1.0 if shape[k] >= 32 else 0.01) * np.sin(2 * np.pi * a + 0.3 * k) for k, a in enumerate(ax))
    g = g + 1e-3 * np.random.default_rng(seed).uniform(-1, 1, size=shape)
    return np.ascontiguousarray(g.astype(dtype))


def huffman_symbols(n, seed=3, width=6.0, dict_size=8192):
    """Quantizer-like symbols for the lossless stage: a rounded normal of the given width about the middle of
    the dictionary, clipped into [0, dict_size). int64."""
    rng = np.random.default_rng(seed)
    q = np.rint(rng.normal(0, width, n)).astype(np.int64) + dict_size // 2
    return np.clip(q, 0, dict_size - 1)


MAXDIM, BLOCK, VARIABLE = 0, 1, 2  # mgh_domain_decomposition


def blocks(shape, dd, sizes=None):
    """Per dimension the list of (offset, extent) of the decomposition grid. dd = (method, dim, size) or None."""
    out = [[(0, n)] for n in shape]
    if dd is None:
        return out
    method, dim, size = dd

    def cut(n):
        full, rest = divmod(n, size)
        ext = [size] * full + ([rest] if rest else [])
        return [(j * size, e) for j, e in enumerate(ext)]

    if method == MAXDIM:
        out[dim] = cut(shape[dim])
    elif method == BLOCK:
        out = [cut(n) for n in shape]
    else:
        assert sum(sizes) == shape[dim]
        out[dim] = [(int(sum(sizes[:j])), e) for j, e in enumerate(sizes)]
    return out


def reference_footprint(shape, elem, ratio=1.0, dict_size=8192, block=20480, prefetch=False):
    """DomainDecomposer::EstimateMemoryFootprint (DomainDecomposer.hpp:24-69 and the estimators it
    calls), runtime-independent terms -- restated here independently of the library."""
    D = len(shape)
    n = float(np.prod(shape, dtype=np.float64))
    ws = float(np.prod([e + 2 for e in shape], dtype=np.float64))
    def levels(e):
        k = 0
        while e > 2:
            e = e // 2 + 1
            k += 1
        return k
    L = min(levels(e) for e in shape)
    hier = 0.0
    for l in range(L + 1):
        for e in shape:
            m = e
            for _ in range(L - l):
                m = m // 2 + 1
            hier += 6.0 * (m + 1) * elem
        hier += D * 8 * 2
    b = n * elem + n * 8 + ratio * 8 + hier
    if prefetch:
        b *= 2
    nchunk = np.floor((n - 1) / block) + 1
    lossless = (8 + n * ratio * 16 + dict_size * 4 + dict_size * 8 + (8 * 128 + 8 * dict_size) + n * 8 +
                3 * nchunk * 8 + 4 + dict_size * 4 + dict_size * 8 + 16 * dict_size + 24 * dict_size +
                8 * dict_size + 64)
    comp = ws * elem * (2 if D > 3 else 1) + elem + (L + 1) * elem + lossless + elem
    if 8 > elem:
        comp += 8 * n
    return int(b + comp)


# ---- quantizer decision points planted through the finest level (tests/test_value_regimes_cpu.py) ----
def planted_sites(shape):
    """Every position planted_field may use: at least one odd index, and in a dimension of even extent
    n an index < n - 2 (clear of the ghost-node rule at the far end). An (N, D) array, row-major order."""
    ax = [np.arange(n - 2 if n % 2 == 0 else n) for n in shape]
    pos = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, len(shape))
    return pos[(pos % 2 == 1).any(axis=1)]


def planted_field(shape, dt, values, seed):
    """(u, positions): a zero array with values[k] at positions[k], seeded random distinct rows of
    planted_sites(shape). Every such node is a finest-level coefficient node whose interpolation
    neighbours all have even indices only: while those hold 0, its coefficient is the planted value."""
    values = np.asarray(values, dtype=dt)
    sites = planted_sites(shape)
    if len(values) > len(sites):
        raise ValueError("%d values for the %d sites of %r" % (len(values), len(sites), tuple(shape)))
    pick = np.random.default_rng(seed).choice(len(sites), size=len(values), replace=False)
    pos = sites[pick]
    u = np.zeros(shape, dtype=dt)
    u[tuple(pos.T)] = values
    return u, pos


def quantizer_targets(dt, dict_size):
    """Products t * quantizer (* volume) at which the quantizer decides something, both signs of each:
    rounding ties k + 0.5 and the integers k (k = 0 .. 39; k = 0 gives +-0.0), the dictionary edges
    half - 2 .. half + 1 and the ties next to them, the representable neighbours of 2^31 (where a 32-bit
    conversion saturates), 2^40, and in float64 2^20 + 0.5, 2^31 +- 1 and 2^53 + 2. All below 2^62."""
    dt = np.dtype(dt).type
    half = dict_size // 2
    t = []
    for k in range(40):
        t += [k + 0.5, float(k)]
    for k in range(half - 2, half + 2):
        t += [float(k), k + 0.5]
    two31 = dt(2.0 ** 31)
    t += [2147483520.0, float(two31), float(np.nextafter(two31, dt(np.inf))), 2.0 ** 40]
    if dt is np.float64:
        t += [2.0 ** 20 + 0.5, 2.0 ** 31 - 1, 2.0 ** 31 + 1, 2.0 ** 53 + 2]
    t = np.array(t, dtype=dt)
    assert np.all(np.abs(t.astype(np.float64)) < 2.0 ** 62)
    return np.concatenate([t, -t])


def solve_targets(dt, targets, qz, vol):
    """For each target a value c with dt(dt(c * qz) * vol) == target (quantize_one's operand order), searched
    among target / (qz * vol) and its +-4 ulp neighbours. Returns (values, mask of exact hits); where
    nothing hits, the value is the rounded quotient."""
    dt = np.dtype(dt).type
    targets = np.asarray(targets, dtype=dt)
    qz, vol = dt(qz), dt(vol)
    vals = np.empty_like(targets)
    hit = np.zeros(len(targets), dtype=bool)
    for k, t in enumerate(targets):
        if t == 0:
            vals[k], hit[k] = t, True  # (+-0.0: the product keeps the sign)
            continue
        c0 = dt(np.float64(t) / (np.float64(qz) * np.float64(vol)))
        cand = [c0]
        lo = hi = c0
        for _ in range(4):
            lo, hi = np.nextafter(lo, dt(-np.inf)), np.nextafter(hi, dt(np.inf))
            cand += [lo, hi]
        vals[k] = c0
        for c in cand:
            if dt(dt(c * qz) * vol) == t:
                vals[k], hit[k] = c, True
                break
    return vals, hit


def level_volume(level_shape, dt):
    """sqrt of the product of 1 / (n - 1) over the level's extents, in the order and precision of the
    quantizer (LinearQuantization.hpp: the fastest dimension first, every step rounded to dt)."""
    dt = np.dtype(dt).type
    v = dt(1)
    for n in reversed(level_shape):
        v = dt(v * dt(1.0 / np.float64(dt(n - 1))))
    return dt(np.sqrt(v))


def rule_integer(target, dt, dict_size):
    """(int64) copysign(0.5 + |target|, target) + dict_size / 2 with the sum rounded to dt as the
    kernels round it, and whether that leaves [0, dict_size): the quantizer's rule, evaluated by hand."""
    dt = np.dtype(dt).type
    m = int(dt(0.5) + abs(dt(target)))
    q = (-m if np.signbit(target) else m) + dict_size // 2
    return q, not 0 <= q < dict_size


def reordered_position(pos, shape, coarse_shape):
    """Place of the finest-grid nodes `pos` ((N, D), as planted_sites gives them) in the reordered layout:
    an even index p sits at p / 2 inside the corner box `coarse_shape` of the level below, an odd one at
    coarse extent + (p - 1) / 2."""
    pos = np.asarray(pos)
    nc = np.asarray(coarse_shape)
    return np.where(pos % 2 == 0, pos // 2, nc + (pos - 1) // 2)
