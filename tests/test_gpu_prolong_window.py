"""mgh_prolong_window on the GPU: Hierarchy.prolong(..., window=(lo, ext)) against the crop of the oracle's recomposition.

For every case, data type, field and level L0 in 0 .. l_target (those of tests/test_gpu_prolong.py): z = the
reordered coefficients with everything outside the corner box of L0 zero, want = oracle.Hierarchy.recompose(z)[W],
got = Hierarchy.prolong(want's nodes of L0, L0, window=W); also against Hierarchy.prolong(...)[W]. Bit patterns, no
tolerance. The windows are windows_of() of tests/test_prolong_window_cpu.py: the full array, the eight corners,
planes at the first, the last and an odd index, boxes from odd to odd indices, the last two nodes of every dimension
separately and together, five seeded random boxes.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from tests.test_gpu_prolong import FALLBACK
from tests.test_prolong_cpu import (CASES_3D, FIELDS, assert_same_bits, coefficients, hierarchy_kw, level_of, zeroed)
from tests.test_prolong_window_cpu import crop, windows_of

pytestmark = pytest.mark.gpu


def _int_view(t):
    import torch
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _run_case(name, dt, which):
    import torch
    import mgard_amd as mg
    shape, _, opts, kernel, _ = CASES_3D[name]
    kw = hierarchy_kw(shape, dt, opts)
    O = oracle.Hierarchy(shape, dt, **kw)
    h = mg.Hierarchy(shape, dt, **kw)
    wins = windows_of(shape)
    try:
        c = coefficients(O, shape, dt, which)
        for level in range(h.l_target + 1):
            want = O.recompose(zeroed(O, c, level))
            lvl = torch.from_numpy(level_of(want, O, level)).cuda()
            keep = lvl.clone()
            full = h.prolong(lvl, level).cpu().numpy()
            for wname, lo, ext in wins:
                what = "%s %s %s level %d of %d window %s" % (name, np.dtype(dt).name, which, level, h.l_target, wname)
                got = h.prolong(lvl, level, window=(lo, ext))
                assert tuple(got.shape) == tuple(ext), what
                got = got.cpu().numpy()
                assert_same_bits(got, crop(want, lo, ext), what + " against the oracle")
                assert_same_bits(got, crop(full, lo, ext), what + " against the crop of Hierarchy.prolong")
            assert torch.equal(_int_view(lvl), _int_view(keep)), "%s level %d: d_level changed" % (name, level)
            if kernel and level < h.l_target:  # the plan of a window step exists exactly where the kernel runs
                h.prolong_window_plan(level, (0, 0, 0), shape, level + 1)
    finally:
        h.close()


@pytest.mark.parametrize("which", FIELDS)
@pytest.mark.parametrize("name", list(CASES_3D))
def test_window_3d_against_the_oracle(name, which):
    for dt in CASES_3D[name][1]:
        _run_case(name, dt, which)


def test_the_full_width_window_marches_in_chunks():
    import mgard_amd as mg
    shape = CASES_3D["129x255x33-chunks"][0]
    h = mg.Hierarchy(shape, np.float32)
    L = h.l_target
    p = h.prolong_window_plan(0, (0, 0, 0), shape, L)
    print(p)
    assert p == dict(h.prolong_plan(L), J0_r=0, J0_c=0, J0_f=0, cells_r=65, cells_c=128, cells_f=17)
    assert p["rch"] >= 2 and p["nchunk"] >= 2
    # a window of full width but a few planes only: more, shorter chunks
    q = h.prolong_window_plan(0, (40, 0, 0), (7, 255, 33), L)
    assert (q["J0_r"], q["cells_r"]) == (20, 4) and q["rch"] == 1 and q["nchunk"] == 4, q
    h.close()


@pytest.mark.parametrize("name", ["16", "34x21x18", "9x129x9-tall+1", "129x255x33-chunks"])
def test_locality_on_the_device(name):
    """NaN everywhere outside the range the library says the window depends on: the same bits come out."""
    import torch
    import mgard_amd as mg
    shape, dts, opts, _, _ = CASES_3D[name]
    dt = dts[0]
    h = mg.Hierarchy(shape, dt, **hierarchy_kw(shape, dt, opts))
    rng = np.random.default_rng(3)
    try:
        for level in range(h.l_target + 1):
            lvl = torch.from_numpy(rng.standard_normal(h.level_shape(level)).astype(dt)).cuda()
            for wname, lo, ext in windows_of(shape):
                ranges = h.prolong_window_ranges(level, lo, ext)
                assert len(ranges) == h.l_target - level + 1
                assert ranges[-1] == [(a, a + e - 1) for a, e in zip(lo, ext)]
                sl = tuple(slice(a, b + 1) for a, b in ranges[0])
                poisoned = torch.full_like(lvl, float("nan"))
                poisoned[sl] = lvl[sl]
                keep = poisoned.clone()
                clean = h.prolong(lvl, level, window=(lo, ext))
                got = h.prolong(poisoned, level, window=(lo, ext))
                what = "%s level %d window %s" % (name, level, wname)
                assert_same_bits(got.cpu().numpy(), clean.cpu().numpy(), what)
                assert torch.equal(_int_view(poisoned), _int_view(keep)), what + ": d_level changed"
    finally:
        h.close()


@pytest.mark.parametrize("name", ["16", "34x21x18", "17x101x18-tall", "5"])
def test_guarded_output(name):
    """d_out between two poisoned guards: the call writes the window and nothing else."""
    import torch
    import mgard_amd as mg
    shape, dts, opts, _, _ = CASES_3D[name]
    tdt = torch.float32
    h = mg.Hierarchy(shape, np.float32, **hierarchy_kw(shape, np.float32, opts))
    G = 4096
    try:
        for level in (0, h.l_target - 1, h.l_target):
            lvl = torch.rand(h.level_shape(level), dtype=tdt, device="cuda")
            for wname, lo, ext in windows_of(shape):
                n = int(np.prod(ext))
                for shift in (0, 1):  # (an odd element offset: the paired stores must look at the address)
                    buf = torch.full((G + shift + n + G,), -77.0, dtype=tdt, device="cuda")
                    out = buf[G + shift:G + shift + n]
                    got = h.prolong(lvl, level, out=out, window=(lo, ext))
                    want = h.prolong(lvl, level, window=(lo, ext))
                    what = "%s level %d window %s shift %d" % (name, level, wname, shift)
                    assert torch.equal(_int_view(got.reshape(-1)), _int_view(want.reshape(-1))), what
                    assert bool(torch.all(buf[:G + shift] == -77.0)) and bool(torch.all(buf[G + shift + n:] == -77.0)), what
    finally:
        h.close()


def test_route():
    """A window call on a fused 3-D shape launches the window kernel once per level above `level` and nothing else;
    a call without `window` still launches prolong3 only."""
    import torch
    import mgard_amd as mg
    h = mg.Hierarchy((33, 33, 33), np.float32)
    for level in range(h.l_target + 1):
        lvl = torch.rand(h.level_shape(level), dtype=torch.float32, device="cuda")
        for lo, ext in (((0, 0, 0), (33, 33, 33)), ((7, 9, 30), (5, 1, 3))):
            h.profile(True)
            h.prolong(lvl, level, window=(lo, ext))
            torch.cuda.synchronize()
            prof = h.profile_read()
            h.profile(False)
            ran = {k: v[1] for k, v in prof.items() if v[1]}
            want = {"prolong3_win": h.l_target - level} if level < h.l_target else {"copy_box": 1}
            assert ran == want, (level, lo, ext, prof)
        h.profile(True)
        h.prolong(lvl, level)
        torch.cuda.synchronize()
        prof = h.profile_read()
        h.profile(False)
        ran = {k: v[1] for k, v in prof.items() if v[1]}
        assert ran == ({"prolong3": h.l_target - level} if level < h.l_target else {}), (level, prof)
    # the intermediates of a small window are window-sized: the handle grows, by far less than the array of level
    # l_target - 1 (65^3 floats) that the full call keeps
    small = mg.Hierarchy((129, 129, 129), np.float32)
    before = small.device_bytes()
    lvl = torch.rand(small.level_shape(0), dtype=torch.float32, device="cuda")
    small.prolong(lvl, 0, window=((60, 60, 60), (4, 4, 4)))
    torch.cuda.synchronize()
    grown = small.device_bytes() - before
    print("device bytes grown by a 4^3 window of 129^3:", grown)
    assert 0 < grown < 65 ** 3 * 4 // 8, grown
    small.close()
    h.close()


@pytest.mark.parametrize("name", list(FALLBACK))
def test_fallback_shapes(name):
    import torch
    import mgard_amd as mg
    shape, dts = FALLBACK[name]
    for dt in dts:
        h = mg.Hierarchy(shape, dt)
        with pytest.raises(mg.MgardHipError):
            h.prolong_window_plan(0, (0,) * len(shape), shape, 1)
        rng = np.random.default_rng(11)
        for level in (0, h.l_target - 1, h.l_target):
            lvl = torch.from_numpy(rng.standard_normal(h.level_shape(level)).astype(dt)).cuda()
            full = h.prolong(lvl, level).cpu().numpy()
            lo = tuple(n // 3 for n in shape)
            for lo, ext in ((lo, tuple(n - a - 1 for n, a in zip(shape, lo))),
                            (tuple(n - 2 for n in shape), (2,) * len(shape))):
                got = h.prolong(lvl, level, window=(lo, ext)).cpu().numpy()
                assert_same_bits(got, crop(full, lo, ext), "%s %s level %d window %r+%r" % (name, np.dtype(dt).name,
                                                                                           level, lo, ext))
        h.close()


def test_bad_arguments():
    import torch
    import mgard_amd as mg
    h = mg.Hierarchy((33, 33, 33), np.float32)
    L = mg.load_library()
    lvl = torch.zeros(h.level_shape(1), dtype=torch.float32, device="cuda")
    out = torch.full((33, 33, 33), 7.0, dtype=torch.float32, device="cuda")
    p, o = C.c_void_p(lvl.data_ptr()), C.c_void_p(out.data_ptr())
    u3 = C.c_uint64 * 3
    lo, ext = u3(1, 2, 3), u3(4, 5, 6)
    for level in (-1, h.l_target + 1):
        assert L.mgh_prolong_window(h._h, level, p, lo, ext, o, None) == -1
    assert L.mgh_prolong_window(h._h, 1, None, lo, ext, o, None) == -1
    assert L.mgh_prolong_window(h._h, 1, p, None, ext, o, None) == -1
    assert L.mgh_prolong_window(h._h, 1, p, lo, None, o, None) == -1
    assert L.mgh_prolong_window(h._h, 1, p, lo, ext, None, None) == -1
    assert L.mgh_prolong_window(None, 1, p, lo, ext, o, None) == -1
    assert L.mgh_prolong_window(h._h, 1, p, lo, u3(4, 0, 6), o, None) == -1
    assert L.mgh_prolong_window(h._h, 1, p, u3(30, 0, 0), u3(4, 1, 1), o, None) == -1
    assert L.mgh_prolong_window(h._h, 1, p, u3(0, 33, 0), u3(1, 1, 1), o, None) == -1
    assert L.mgh_prolong_window(h._h, 1, p, u3(0, 0, 2 ** 64 - 1), u3(1, 1, 2), o, None) == -1
    r = (C.c_int64 * 64)()
    assert L.mgh_debug_prolong_window_ranges(h._h, 1, u3(30, 0, 0), u3(4, 1, 1), r, 64) == -1
    assert L.mgh_debug_prolong_window_ranges(h._h, 1, lo, ext, r, 3) == -1
    torch.cuda.synchronize()
    assert bool(torch.all(out == 7.0))
    with pytest.raises(mg.MgardHipError):
        h.prolong(lvl, 1, window=((0, 0, 0), (34, 1, 1)))
    assert L.mgh_prolong_window(h._h, 1, p, lo, ext, o, None) == 0  # (the handle works afterwards)
    h.close()
