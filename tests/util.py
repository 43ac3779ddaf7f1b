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
