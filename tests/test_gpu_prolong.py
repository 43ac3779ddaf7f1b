"""mgh_prolong on the GPU: Hierarchy.prolong against the recomposition of the zeroed coefficient array.

For every case, data type, field and level L0 in 0 .. l_target: z = the reordered coefficients with everything
outside the corner box of L0 zero, want = oracle.Hierarchy.recompose(z) (and ref.Hierarchy.recompose(z) where
oracle/_ref is built), got = Hierarchy.prolong(want[nodes of L0], L0). Bit patterns, no tolerance. The cases, the
fields and the NumPy restatement of the level step are those of tests/test_prolong_cpu.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from oracle import ref
from tests.test_prolong_cpu import (CASES_3D, FIELDS, assert_same_bits, coefficients, hierarchy_kw, level_of, zeroed)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# shapes that run the existing level loops over zeros (no kernel of the call's own)
FALLBACK = {
    "1000": ((1000,), (np.float32, np.float64)),
    "70x45": ((70, 45), (np.float32, np.float64)),
    "300x5x7-thin": ((300, 5, 7), (np.float32, np.float64)),
    "9x17x17x17": ((9, 17, 17, 17), (np.float32, np.float64)),
    "4x3x10x5x9": ((4, 3, 10, 5, 9), (np.float32, np.float64)),
}


def _run_case(shape, dt, opts, which, expect_kernel, with_ref):
    import torch
    import mgard_amd as mg
    kw = hierarchy_kw(shape, dt, opts)
    O = oracle.Hierarchy(shape, dt, **kw)
    R = ref.Hierarchy(shape, dt, **kw) if with_ref else None
    h = mg.Hierarchy(shape, dt, **kw)
    try:
        assert h.l_target == O.l_target
        if expect_kernel is not None:
            try:
                h.prolong_plan(1)
                runs_kernel = True
            except mg.MgardHipError:
                runs_kernel = False
            assert runs_kernel == expect_kernel, (shape, runs_kernel)
        c = coefficients(O, shape, dt, which)
        for level in range(h.l_target + 1):
            z = zeroed(O, c, level)
            want = O.recompose(z)
            lvl = torch.from_numpy(level_of(want, O, level)).cuda()
            keep = lvl.clone()
            got = h.prolong(lvl, level)
            what = "%r %s %s level %d of %d" % (shape, np.dtype(dt).name, which, level, h.l_target)
            assert tuple(got.shape) == tuple(shape)
            assert_same_bits(got.cpu().numpy(), want, what + " against the oracle")
            assert torch.equal(lvl.view(torch.int32 if dt == np.float32 else torch.int64),
                               keep.view(torch.int32 if dt == np.float32 else torch.int64)), what + ": d_level changed"
            if R is not None:
                assert_same_bits(got.cpu().numpy(), R.recompose(z), what + " against the reference")
            if level == h.l_target:
                assert_same_bits(got.cpu().numpy(), lvl.cpu().numpy(), what + ": level == l_target is a copy")
    finally:
        h.close()


@pytest.mark.parametrize("which", FIELDS)
@pytest.mark.parametrize("name", list(CASES_3D))
def test_prolong_3d_against_the_oracle(name, which):
    shape, dts, opts, kernel, _ = CASES_3D[name]
    for dt in dts:
        _run_case(shape, dt, opts, which, kernel, False)


@pytest.mark.skipif(not ref.available(), reason="%s is not built (oracle.build_ref())" % ref.LIB_PATH)
@pytest.mark.parametrize("which", FIELDS)
@pytest.mark.parametrize("name", list(CASES_3D))
def test_prolong_3d_against_the_reference(name, which):
    shape, dts, opts, kernel, _ = CASES_3D[name]
    for dt in dts:
        _run_case(shape, dt, opts, which, kernel, True)


@pytest.mark.parametrize("name", list(FALLBACK))
def test_prolong_fallback_shapes(name):
    shape, dts = FALLBACK[name]
    for dt in dts:
        for which in FIELDS:
            # (the reference on the smooth field only: for D > 3 the oracle and the reference disagree on the sign
            # of a -0.0 written into a corner of the coarsest box, and the fallback is the oracle's level loop)
            _run_case(shape, dt, {}, which, False, ref.available() and which == "smooth")


def test_the_march_takes_two_chunk_lengths():
    import mgard_amd as mg
    shape = CASES_3D["129x255x33-chunks"][0]
    h = mg.Hierarchy(shape, np.float32)
    p = h.prolong_plan(h.l_target)
    print(p)
    m_r = h.level_shape(h.l_target - 1)[0]
    assert (p["TC"], p["TF"]) == (4, 64)
    assert p["rch"] >= 2 and p["nchunk"] >= 2 and p["nchunk"] * p["rch"] >= m_r
    last = m_r - (p["nchunk"] - 1) * p["rch"]
    assert 1 <= last < p["rch"], (p, m_r)
    h.close()


def test_tile_shapes_of_the_cases():
    import mgard_amd as mg
    for name, tile in (("17x101x18-tall", (64, 4)), ("9x129x9-tall+1", (64, 4)), ("9x9x129-wide+1", (4, 64))):
        shape = CASES_3D[name][0]
        h = mg.Hierarchy(shape, np.float32)
        p = h.prolong_plan(h.l_target)
        m = h.level_shape(h.l_target - 1)
        assert (p["TC"], p["TF"]) == tile, (name, p)
        if name.endswith("+1"):
            assert m[1] % p["TC"] == 1 and m[2] % p["TF"] == 1, (name, m, p)
        h.close()


def test_bad_arguments():
    import ctypes as C
    import torch
    import mgard_amd as mg
    h = mg.Hierarchy((33, 33, 33), np.float32)
    L = mg.load_library()
    lvl = torch.zeros(h.level_shape(1), dtype=torch.float32, device="cuda")
    out = torch.full((33, 33, 33), 7.0, dtype=torch.float32, device="cuda")
    p, o = C.c_void_p(lvl.data_ptr()), C.c_void_p(out.data_ptr())
    for level in (-1, h.l_target + 1):
        assert L.mgh_prolong(h._h, level, p, o, None) == -1
    assert L.mgh_prolong(h._h, 1, None, o, None) == -1
    assert L.mgh_prolong(h._h, 1, p, None, None) == -1
    assert L.mgh_prolong(None, 1, p, o, None) == -1
    torch.cuda.synchronize()
    assert bool(torch.all(out == 7.0))
    with pytest.raises(mg.MgardHipError):
        h.prolong(lvl, h.l_target + 1)
    h.close()


def test_profile_only_prolong3_launches():
    import torch
    import mgard_amd as mg
    h = mg.Hierarchy((33, 33, 33), np.float32)
    for level in range(h.l_target):
        lvl = torch.rand(h.level_shape(level), dtype=torch.float32, device="cuda")
        h.profile(True)
        h.prolong(lvl, level)
        torch.cuda.synchronize()
        prof = h.profile_read()
        h.profile(False)
        ran = {k: v[1] for k, v in prof.items() if v[1]}
        assert ran == {"prolong3": h.l_target - level}, (level, prof)
    h.close()


_WORKER = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
import torch
import mgard_amd as mg
import oracle
from oracle import ref
from tests.test_prolong_cpu import assert_same_bits, coefficients, level_of, zeroed
shape, dt = (33, 33, 33), np.float32
O = oracle.Hierarchy(shape, dt)
R = ref.Hierarchy(shape, dt) if ref.available() else None
h = mg.Hierarchy(shape, dt)
try:
    h.prolong_plan(1)
    raise SystemExit("the switch did not take the call off the fused route")
except mg.MgardHipError:
    pass
for which in ("smooth", "zeros"):
    c = coefficients(O, shape, dt, which)
    for level in range(h.l_target + 1):
        z = zeroed(O, c, level)
        want = O.recompose(z)
        got = h.prolong(torch.from_numpy(level_of(want, O, level)).cuda(), level)
        assert_same_bits(got.cpu().numpy(), want, "%%s level %%d" %% (which, level))
        if R is not None:
            assert_same_bits(got.cpu().numpy(), R.recompose(z), "%%s level %%d against the reference" %% (which, level))
print("WORKER OK" + (" (reference compared)" if R is not None else " (no reference build)"))
"""


@pytest.mark.parametrize("switch", ["MGH_FORCE_V1", "MGH_FORCE_ND"])
def test_prolong_under_the_cross_check_switches(switch):
    """The developer switches are read once per process: a child process, as tests/crosscheck_worker.py is run."""
    env = dict(os.environ)
    env[switch] = "1"
    r = subprocess.run([sys.executable, "-c", _WORKER % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "WORKER OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
