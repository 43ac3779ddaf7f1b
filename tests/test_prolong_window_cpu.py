"""Windowed full-grid preview on the CPU: which nodes of every level a window of the full grid depends on.

mgard_amd/csrc/prolong_window_plan.hpp gives, for a hierarchy's level shapes, a start level and a window, the closed
range of node indices per level and dimension (the chain). This module
  - restates the chain rule in NumPy and holds the header against it: tests/cpp/prolong_window_dump.cpp is compiled
    with g++ against the header alone (no HIP) -- with -fsanitize=address,undefined where the host compiler links
    that, plain where it does not (the fixture tries the sanitized build first) -- and run over EVERY window of the
    1-D extents 2 .. 40 at every start level, and over corner, plane and random windows of the CASES_3D shapes;
  - checks the chain against the oracle-pinned level step of tests/test_prolong_cpu.py (prolong_step): with NaN
    written everywhere OUTSIDE the chain's range at EVERY level on the way, the window comes out bit for bit as the
    crop of prolong_numpy of the whole array (sufficiency: nothing outside is used), and in 1-D a NaN AT either end
    of a range reaches the window (the ranges are tight);
  - checks that the library exports the new entries and the headers declare them.

windows_of() is shared with tests/test_gpu_prolong_window.py.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from tests.test_prolong_cpu import (CASES_3D, assert_same_bits, coefficients, hierarchy_kw, level_of, prolong_numpy,
                                    prolong_step, zeroed)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgard_amd", "csrc")


# ---- the chain rule, restated ---------------------------------------------------------------------
def padded(i, n):
    """Real index i of an extent n in padded coordinates: the last node of an even n sits at P = n."""
    return n if (n % 2 == 0 and i == n - 1) else i


def chain_numpy(shapes, level, lo, ext):
    """shapes[l][d], l = 0 .. L. Returns [[(first, last) per dimension] for l = level .. L]."""
    L = len(shapes) - 1
    rng = [(int(a), int(a + e - 1)) for a, e in zip(lo, ext)]
    made = {L: rng}
    for l in range(L, level, -1):
        nxt = []
        for d, (a, b) in enumerate(rng):
            n, m = shapes[l][d], shapes[l - 1][d]
            nxt.append((a, b) if m == n else (padded(a, n) // 2, (padded(b, n) + 1) // 2))
        rng = made[l - 1] = nxt
    return [made[l] for l in range(level, L + 1)]


def windows_of(shape, seed=0):
    """The windows the window tests use, as (name, lo, ext): the full array, the eight single-node corners, one plane
    per dimension at the first, the last and an odd interior index, boxes that start and end on odd indices, the last
    two nodes of every dimension separately and together, five seeded random boxes."""
    D = len(shape)
    w = [("full", (0,) * D, tuple(shape))]
    for corner in np.ndindex(*(2,) * D):
        w.append(("corner%r" % (corner,), tuple((n - 1) * c for n, c in zip(shape, corner)), (1,) * D))
    for d in range(D):
        odd = (shape[d] // 2) | 1
        odd = odd if odd < shape[d] - 1 else 1
        for at in (0, shape[d] - 1, odd):
            w.append(("plane d%d @%d" % (d, at), tuple(at if k == d else 0 for k in range(D)),
                      tuple(1 if k == d else shape[k] for k in range(D))))
    last_odd = [n - 2 if (n - 2) % 2 else n - 3 for n in shape]
    w.append(("odd..odd wide", (1,) * D, tuple(max(b, 1) for b in last_odd)))          # [1, last odd index]
    w.append(("odd..odd short", tuple(min(3, b) for b in last_odd), tuple(min(3, b - min(3, b) + 1) for b in last_odd)))
    for d in range(D):
        for a, e in ((shape[d] - 2, 1), (shape[d] - 1, 1), (shape[d] - 2, 2)):
            w.append(("tail d%d [%d,+%d)" % (d, a, e), tuple(a if k == d else 0 for k in range(D)),
                      tuple(e if k == d else shape[k] for k in range(D))))
    rng = np.random.default_rng(1000 + seed + sum(shape))
    for i in range(5):
        lo = [int(rng.integers(0, n)) for n in shape]
        ext = [int(rng.integers(1, n - a + 1)) for n, a in zip(shape, lo)]
        w.append(("random%d" % i, tuple(lo), tuple(ext)))
    for name, lo, ext in w:
        assert all(e >= 1 and a >= 0 and a + e <= n for a, e, n in zip(lo, ext, shape)), (name, lo, ext, shape)
    return w


def crop(a, lo, ext):
    return np.ascontiguousarray(a[tuple(slice(o, o + e) for o, e in zip(lo, ext))])


def oracle_of(name, dt):
    shape, _, opts, _, _ = CASES_3D[name]
    return oracle.Hierarchy(shape, dt, **hierarchy_kw(shape, dt, opts))


def shapes_of(H):
    return [tuple(int(e) for e in H.level_shape(l)) for l in range(H.l_target + 1)]


# ---- the header against the restatement -----------------------------------------------------------
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prolong_window") / "prolong_window_dump")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC,
            os.path.join(ROOT, "tests", "cpp", "prolong_window_dump.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True,
                         text=True)
    if san.returncode != 0:
        print("no sanitizer build (%s): plain" % san.stderr.strip().splitlines()[-1:])
        subprocess.check_call(base)

    def run(queries):
        """queries: (shapes, level, lo, ext) -> the chains, in chain_numpy's form (None for a refused query)."""
        text = ""
        for shapes, level, lo, ext in queries:
            D, L = len(shapes[0]), len(shapes) - 1
            text += " ".join(map(str, [D, L, level] + [e for s in shapes for e in s] + list(lo) + list(ext))) + "\n"
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(queries)
        out = []
        for (shapes, level, _, _), line in zip(queries, lines):
            if line == "bad":
                out.append(None)
                continue
            v = [int(x) for x in line.split()]
            D = len(shapes[0])
            assert len(v) == (len(shapes) - level) * 2 * D
            out.append([[(v[k * 2 * D + 2 * d], v[k * 2 * D + 2 * d + 1]) for d in range(D)]
                        for k in range(len(shapes) - level)])
        return out
    run.exe = exe
    return run


def test_header_compiles_alone_without_hip(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "prolong_window_plan.hpp"\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", CSRC, str(src)])


def shapes_1d(n):
    if n == 2:
        return [(2,)]
    return shapes_of(oracle.Hierarchy((n,), np.float32))


def test_chain_of_every_1d_window(dump):
    queries = []
    for n in range(2, 41):
        shapes = shapes_1d(n)
        assert shapes[-1] == (n,) and all(s[0] // 2 + 1 == c[0] for s, c in zip(shapes[1:], shapes[:-1]))
        for level in range(len(shapes)):
            for a in range(n):
                for b in range(a, n):
                    queries.append((shapes, level, (a,), (b - a + 1,)))
    got = dump(queries)
    print("%d windows" % len(queries))
    for q, g in zip(queries, got):
        assert g == chain_numpy(*q), q
        # (every range lies inside its level and is ordered)
        for l, r in zip(range(q[1], len(q[0])), g):
            assert 0 <= r[0][0] <= r[0][1] < q[0][l][0], (q, g)


def test_chain_of_the_3d_cases(dump):
    queries = []
    for name in CASES_3D:
        H = oracle_of(name, CASES_3D[name][1][0])
        shapes = shapes_of(H)
        for level in range(H.l_target + 1):
            for _, lo, ext in windows_of(shapes[-1]):
                queries.append((shapes, level, lo, ext))
    got = dump(queries)
    for q, g in zip(queries, got):
        assert g == chain_numpy(*q), q


def test_chain_refuses_bad_windows(dump):
    shapes = shapes_of(oracle.Hierarchy((9, 9, 9), np.float32))
    L = len(shapes) - 1
    bad = [(shapes, -1, (0, 0, 0), (1, 1, 1)), (shapes, L + 1, (0, 0, 0), (1, 1, 1)), (shapes, 0, (0, 0, 0), (1, 0, 1)),
           (shapes, 0, (0, 5, 0), (1, 5, 1)), (shapes, 0, (9, 0, 0), (1, 1, 1))]
    assert dump(bad) == [None] * len(bad)
    assert dump([(shapes, L, (8, 8, 8), (1, 1, 1))]) == [[[(8, 8)] * 3]]


def test_window_plan_covers_the_cells(dump):
    """The launch plan of a step: the cells under the range, tiles and chunks by prolong_plan's rule for as many
    coarse nodes as there are cells (the full window of a level step gives prolong_plan's own figures)."""
    text = "plan 129 255 33 0 0 0 128 254 32 1\nplan 16 16 16 15 14 3 15 15 8 1\nplan 34 21 18 33 1 17 33 19 17 1\n"
    r = subprocess.run([dump.exe], input=text, capture_output=True, text=True, check=True)
    rows = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    assert rows[0][:2] == [4, 64] and rows[0][4] >= 2 and rows[0][6:] == [0, 0, 0, 65, 128, 17]
    assert rows[0][5] == -(-65 // rows[0][4])
    assert rows[1][6:] == [8, 7, 1, 1, 2, 4]   # (P(15) = 16 of the even extent 16: cell 8, alone)
    assert rows[2][6:] == [17, 0, 9, 1, 10, 1]  # (34 and 18 even: their last nodes are cells 17 and 9)


# ---- the chain against the oracle-pinned level step -------------------------------------------------
def prolong_boxes(level_array, H, level, chain):
    """The window from the chain's boxes alone: at every level everything outside the chain's range is NaN before the
    (whole, oracle-pinned) level step runs; returns the chain's box of l_target, i.e. the window."""
    a = level_array
    for l in range(level, H.l_target + 1):
        sl = tuple(slice(f, t + 1) for f, t in chain[l - level])
        masked = np.full_like(a, np.nan)
        masked[sl] = a[sl]
        a = prolong_step(masked, H, l + 1) if l < H.l_target else masked
    return np.ascontiguousarray(a[tuple(slice(f, t + 1) for f, t in chain[-1])])


@pytest.mark.parametrize("name", list(CASES_3D))
def test_chain_boxes_give_the_crop(name):
    shape, dts, _, _, _ = CASES_3D[name]
    dt = dts[0]
    H = oracle_of(name, dt)
    shapes = shapes_of(H)
    wins = windows_of(shape)
    if np.prod(shape) > 200000:  # (the level step in NumPy is slow there: corners and random boxes only)
        wins = [w for w in wins if w[0].startswith(("corner", "random"))]
    c = coefficients(H, shape, dt, "smooth")
    for level in range(H.l_target + 1):
        lvl = level_of(H.recompose(zeroed(H, c, level)), H, level)
        whole = prolong_numpy(lvl, H, level)
        assert not np.isnan(whole).any()
        for wname, lo, ext in wins:
            chain = chain_numpy(shapes, level, lo, ext)
            got = prolong_boxes(lvl, H, level, chain)
            assert_same_bits(got, crop(whole, lo, ext), "%s level %d window %s" % (name, level, wname))


def test_chain_ranges_are_tight_in_1d():
    """Every end of every range is used: a NaN there reaches the window (n = 3 .. 24, every window, every level)."""
    for n in range(3, 25):
        H = oracle.Hierarchy((n,), np.float32)
        shapes = shapes_of(H)
        for level in range(H.l_target):
            lvl = np.linspace(1, 2, shapes[level][0]).astype(np.float32)
            for a in range(n):
                for b in range(a, n):
                    r = chain_numpy(shapes, level, (a,), (b - a + 1,))[0][0]
                    for end in set(r):
                        x = lvl.copy()
                        x[end] = np.nan
                        assert np.isnan(prolong_numpy(x, H, level)[a:b + 1]).any(), (n, level, a, b, r, end)


# ---- the entries ----------------------------------------------------------------------------------
NEW_ENTRIES = ("mgh_prolong_window", "mgh_debug_prolong_window_ranges", "mgh_decompress_preview_window",
               "mgh_progressive_preview_window")


def test_library_exports_the_window_entries():
    import mgard_amd
    L = mgard_amd.load_library()
    for sym in NEW_ENTRIES:
        assert hasattr(L, sym), sym


def test_headers_declare_the_window_entries():
    def text(name):
        txt = open(os.path.join(ROOT, "include", name)).read()
        return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    low = text("mgard_hip.h")
    assert ("int mgh_prolong_window(mgh_hierarchy *h, int level, const void *d_level, const uint64_t *lo, "
            "const uint64_t *ext, void *d_out, void *stream);") in low
    assert ("int mgh_debug_prolong_window_ranges(const mgh_hierarchy *h, int level, const uint64_t *lo, "
            "const uint64_t *ext, int64_t *out, uint64_t cap);") in low
    hl = text("mgard_hip_compress.h")
    assert ("int mgh_decompress_preview_window(const void *compressed_data, size_t compressed_size, int halvings, "
            "const uint64_t *lo, const uint64_t *ext, void **decompressed_data, const mgh_config *config, "
            "int output_pre_allocated);") in hl
    assert ("int mgh_progressive_preview_window(mgh_progressive *p, const uint64_t *lo, const uint64_t *ext, "
            "void **data, int output_pre_allocated);") in hl
    # the C++ mirrors
    assert "mgh_prolong_window(" in text("mgard_hip.hpp")
    assert "mgh_decompress_preview_window(" in text("compress_hip.hpp")
    assert "mgh_progressive_preview_window(" in text("compress_hip.hpp")
    assert "mgh_decompress_preview_window(" in text("compress_x_hip.hpp")
