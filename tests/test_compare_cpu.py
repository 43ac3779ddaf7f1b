"""CPU tests of the error statistics (mgh_compare / mgh_verify): the host-only planner and fold of
mgard_amd/csrc/compare_plan.hpp through tests/cpp/compare_plan_dump.cpp (g++ against the header alone, no
HIP), and the ABI of the new entry points.

The plan: workgroup b of the reduction kernel takes the slab [b * S, min(n, (b + 1) * S)); the slabs
partition [0, n) in ascending order, S is a whole number of 16-byte vectors times 256 lanes, and the number
of workgroups is capped by a constant, so the order of every addition depends on n alone.
merge(): every part of an array reduced on its own and folded must give what tests/compare_ref.py computes
for the whole array -- counters, extremes and argmax (the LOWEST index among equals, whichever order the
parts are folded in) exactly, the sums within tests/compare_ref.py's sum_tolerance.
The same program is also built with -fsanitize=address,undefined and run once as a stand-alone binary."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.compare_ref import assert_stats, ref_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgard_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "compare_plan_dump.cpp")
NS = [0, 1, 3, 1023, 1024, 1025, 2**20 + 7, 2**31 + 5, 2**33]
FIELDS = ("n", "nonfinite", "max_abs_err", "argmax", "sum_sq_err", "ref_min", "ref_max", "ref_abs_max", "ref_sum_sq")
INTS = ("n", "nonfinite", "argmax")


def _build(tmp_path_factory, name, extra=()):
    exe = str(tmp_path_factory.mktemp(name) / "compare_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", CSRC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return _build(tmp_path_factory, "compare_plan")


def _run(exe, text):
    return subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=120).stdout


def _parse(out):
    """[(stats dict, derived dict)] of the "stats" / "derived" lines."""
    res, cur = [], None
    for line in out.splitlines():
        f = line.split()
        if f[0] == "stats":
            cur = {k: (int(v) if k in INTS else float.fromhex(v)) for k, v in zip(FIELDS, f[1:])}
        elif f[0] == "derived":
            d = dict(zip(("mse", "rmse", "l2n", "l2", "psnr"), [float.fromhex(v) for v in f[1:]]))
            res.append((cur, d))
            cur = None
    return res


def test_header_compiles_alone_without_hip(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "compare_plan.hpp"\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", CSRC, str(src)])


@pytest.mark.parametrize("esz", [4, 8])
def test_plan_partitions_the_array(dump, esz):
    out = _run(dump, "".join("plan %d %d\n" % (n, esz) for n in NS)).splitlines()
    vec = 16 // esz
    at = 0
    for n in NS:
        f = out[at].split()
        assert f[0] == "plan"
        groups, slab, unit, cap = map(int, f[1:])
        at += 1
        assert unit == vec * 256 and slab % unit == 0 and slab > 0
        assert groups <= cap == 2048
        assert groups == (0 if n == 0 else -(-n // slab))  # n = 0: nothing is launched
        if n:  # no workgroup is empty, and (where the cap allows) none takes more than it must
            assert (groups - 1) * slab < n <= groups * slab
            assert slab == -(-(-(-n // cap)) // unit) * unit
        shown = []
        while at < len(out) and out[at].startswith("slab"):
            shown.append(tuple(map(int, out[at].split()[1:])))
            at += 1
        assert [b for b, _, _ in shown] == sorted({b for b in (0, 1, groups - 2, groups - 1) if 0 <= b < groups})
        for b, lo, hi in shown:
            assert lo == b * slab and lo % vec == 0 and lo < hi  # starts on a whole vector; ascending, contiguous:
            assert hi == (n if b == groups - 1 else (b + 1) * slab)
    assert at == len(out)


def _case(dt, n, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(n).astype(dt)
    b = (a + (rng.standard_normal(n) * 1e-3).astype(dt)).astype(dt)
    return a, b


def _merge_cmd(tmp_path, tag, a, b, cuts, order="fwd"):
    fa, fb = str(tmp_path / (tag + ".a")), str(tmp_path / (tag + ".b"))
    a.tofile(fa)
    b.tofile(fb)
    return "merge %s %s %s %d %s %d %s\n" % ("f32" if a.dtype == np.float32 else "f64", fa, fb, a.size, order,
                                             len(cuts), " ".join(map(str, cuts)))


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_merge_equals_the_one_shot_statistics(dump, tmp_path, dt):
    n = 5000
    cases = []
    a, b = _case(dt, n, 1)
    cases.append(("plain", a, b, [1, 17, 18, 2500, 4999]))
    cases.append(("one-part", a, b, []))
    cases.append(("empty-parts", a, b, [0, 0, 1000, 1000, n]))
    # the same largest error at the first and the last element: a tie that spans two parts
    a2, b2 = a.copy(), b.copy()
    a2[0] = a2[-1] = dt(1)
    b2[0] = b2[-1] = dt(-7)
    assert a2[0] - b2[0] == a2[-1] - b2[-1] == dt(8)
    cases.append(("tie", a2, b2, [100, 3000]))
    # ... and a tie of a zero error everywhere
    cases.append(("all-equal", a, a.copy(), [7, 4000]))
    # non-finite positions, one part made of nothing else
    a3, b3 = a.copy(), b.copy()
    a3[10] = np.nan
    b3[20] = np.inf
    a3[30] = b3[30] = np.inf
    a3[2000:2100] = np.nan
    cases.append(("nonfinite", a3, b3, [15, 2000, 2100]))
    # the extremes of the reference in different parts, all values negative
    a4 = (-np.abs(a) - dt(1)).astype(dt)
    cases.append(("negative", a4, (a4 + dt(0.25)).astype(dt), [1234]))
    text = ""
    for tag, x, y, cuts in cases:
        text += _merge_cmd(tmp_path, tag, x, y, cuts, "fwd") + _merge_cmd(tmp_path, tag, x, y, cuts, "rev")
    res = _parse(_run(dump, text))
    assert len(res) == 2 * len(cases)
    for k, (tag, x, y, cuts) in enumerate(cases):
        want = ref_stats(x, y)
        for got, _ in res[2 * k:2 * k + 2]:
            assert_stats(got, want, what=tag)
    tie = res[2 * 3][0]
    assert tie["argmax"] == 0 and tie["max_abs_err"] == 8.0
    assert res[2 * 3 + 1][0]["argmax"] == 0  # folded last part first: still the lower index
    assert res[2 * 4][0]["argmax"] == 0 and res[2 * 4][1]["psnr"] == math.inf
    assert res[2 * 5][0]["nonfinite"] == 103


def test_finalisers_on_known_answers(dump):
    hexf = float.hex
    lines = [
        # n nonfinite max argmax sse rmin rmax ramax rss
        "derive 8 0 %s 3 %s %s %s %s %s" % (hexf(2.0), hexf(8.0), hexf(-1.0), hexf(3.0), hexf(3.0), hexf(20.0)),
        "derive 8 0 %s 0 %s %s %s %s %s" % (hexf(0.0), hexf(0.0), hexf(-1.0), hexf(3.0), hexf(3.0), hexf(20.0)),
        "derive 8 8 %s 0 %s %s %s %s %s" % (hexf(0.0), hexf(0.0), hexf(0.0), hexf(0.0), hexf(0.0), hexf(0.0)),
        "derive 10 2 %s 3 %s %s %s %s %s" % (hexf(2.0), hexf(8.0), hexf(-1.0), hexf(3.0), hexf(3.0), hexf(20.0)),
        "derive 0 0 %s 0 %s %s %s %s %s" % (hexf(0.0), hexf(0.0), hexf(0.0), hexf(0.0), hexf(0.0), hexf(0.0)),
    ]
    res = [d for _, d in _parse(_run(dump, "\n".join(lines) + "\n"))]
    assert res[0] == {"mse": 1.0, "rmse": 1.0, "l2n": 1.0, "l2": math.sqrt(8.0), "psnr": 20 * math.log10(4.0)}
    assert res[1]["mse"] == 0 and res[1]["psnr"] == math.inf  # a zero error
    # nothing finite, nothing at all: no division by zero
    for r in (res[2], res[4]):
        assert r["mse"] == 0 and r["rmse"] == 0 and r["l2n"] == 0 and r["l2"] == 0 and r["psnr"] == math.inf
    assert res[3] == res[0]  # the divisor is n - nonfinite


def test_program_is_clean_under_address_and_undefined_sanitizers(tmp_path_factory, tmp_path):
    exe = _build(tmp_path_factory, "compare_plan_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    a, b = _case(np.float32, 3000, 2)
    a[5] = np.nan
    text = "".join("plan %d %d\n" % (n, e) for n in NS for e in (4, 8))
    text += _merge_cmd(tmp_path, "san", a, b, [0, 5, 6, 2999, 3000]) + _merge_cmd(tmp_path, "san", a, b, [1500], "rev")
    text += "derive 8 8 0x0p+0 0 0x0p+0 0x0p+0 0x0p+0 0x0p+0 0x0p+0\n"
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr
    assert_stats(_parse(p.stdout)[0][0], ref_stats(a, b))


# ---- ABI -------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points():
    import mgard_amd
    from mgard_amd import highlevel
    L = mgard_amd.load_library()
    assert "mgh_compare" in mgard_amd.SYMBOLS and "mgh_verify" in highlevel.HL_SYMBOLS
    for name in ("mgh_compare", "mgh_verify"):
        assert hasattr(L, name), name


def test_ctypes_structs_match_the_c_structs(tmp_path):
    """A C program prints sizeof / offsetof from the public headers; the ctypes mirrors must agree."""
    import mgard_amd
    from mgard_amd import highlevel
    stats_fields = [f for f, _ in mgard_amd.ErrorStats._fields_]
    result_fields = [f for f, _ in highlevel.VerifyResult._fields_]
    assert stats_fields == list(FIELDS)
    src = tmp_path / "layout.c"
    body = ['#include <stddef.h>', '#include <stdio.h>', '#include "mgard_hip_compress.h"', 'int main(void) {',
            '  printf("mgh_error_stats %zu\\n", sizeof(mgh_error_stats));',
            '  printf("mgh_verify_result %zu\\n", sizeof(mgh_verify_result));']
    body += ['  printf("s.%s %%zu\\n", offsetof(mgh_error_stats, %s));' % (f, f) for f in stats_fields]
    body += ['  printf("r.%s %%zu\\n", offsetof(mgh_verify_result, %s));' % (f, f) for f in result_fields]
    body += ['  return 0;', '}']
    src.write_text("\n".join(body) + "\n")
    exe = str(tmp_path / "layout")
    cc = shutil.which("gcc") or shutil.which("cc")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(got["mgh_error_stats"]) == ctypes.sizeof(mgard_amd.ErrorStats) == 72
    assert int(got["mgh_verify_result"]) == ctypes.sizeof(highlevel.VerifyResult)
    for f in stats_fields:
        assert int(got["s." + f]) == getattr(mgard_amd.ErrorStats, f).offset, f
    for f in result_fields:
        assert int(got["r." + f]) == getattr(highlevel.VerifyResult, f).offset, f


def test_error_stats_properties():
    import mgard_amd
    s = mgard_amd.ErrorStats(n=10, nonfinite=2, max_abs_err=2.0, argmax=3, sum_sq_err=8.0, ref_min=-1.0, ref_max=3.0,
                             ref_abs_max=3.0, ref_sum_sq=20.0)
    assert s.mse == 1.0 and s.rmse == 1.0 and s.l2_error(True) == 1.0 and s.l2_error(False) == math.sqrt(8.0)
    assert s.psnr == 20 * math.log10(4.0)
    z = mgard_amd.ErrorStats(n=4, nonfinite=4)
    assert z.mse == 0 and z.rmse == 0 and z.psnr == math.inf
