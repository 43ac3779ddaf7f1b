"""CPU test of mgard_amd/csrc/target_plan.hpp: which figure of the statistics a target is held against, when
it is met, and the search for the largest tolerance that meets it.

tests/cpp/target_plan_dump.cpp is compiled with g++ against the header alone (no HIP) and once more with
-fsanitize=address,undefined as a stand-alone binary. The expectations are restated here from the text of
the walk: sqrt and one multiply are exact IEEE operations, so NumPy walks the same doubles and every
comparison is an equality of doubles or of integers."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgard_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "target_plan_dump.cpp")
INF, NAN = float("inf"), float("nan")
FOUND, NOTHING_MEETS, BAD_ARGUMENT = 0, 1, 2
MAX_ABS, RMSE, PSNR = 0, 1, 2


def _build(tmp_path_factory, name, extra=()):
    exe = str(tmp_path_factory.mktemp(name) / "target_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", CSRC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return _build(tmp_path_factory, "target_plan")


def _run(exe, text):
    return subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=300).stdout.splitlines()


def _hex(x):
    return float(x).hex()


def test_header_compiles_alone_without_hip(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "target_plan.hpp"\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", CSRC, str(src)])


# ---- the search ------------------------------------------------------------------------------------------
def walk(meets, tol_min, tol_max, rounds):
    """The walk as the issue states it: (end, tol, coarser, candidates evaluated in order)."""
    if not (tol_min > 0) or not (tol_min <= tol_max) or not np.isfinite(tol_max) or not (1 <= rounds <= 16):
        return BAD_ARGUMENT, 0.0, 0.0, []
    seen = [tol_max]
    if meets(tol_max):
        return FOUND, tol_max, 0.0, seen
    seen.append(tol_min)
    if not meets(tol_min):
        return NOTHING_MEETS, 0.0, 0.0, seen
    a, b = np.float64(tol_min), np.float64(tol_max)
    for _ in range(rounds):
        m = np.sqrt(a) * np.sqrt(b)
        seen.append(float(m))
        if meets(m):
            a = m
        else:
            b = m
    return FOUND, float(a), float(b), seen


def _stub(t1, t2, t3):
    return lambda tol: bool(tol <= t1 or (t2 <= tol <= t3))


# (tol_min, tol_max, rounds, t1, t2, t3): meets(tol) = tol <= t1 or t2 <= tol <= t3; t2 > t3: monotone
SEARCH_CASES = {
    "monotone": (1e-6, 1e-1, 8, 3.3e-4, 1.0, 0.0),
    "monotone-1-round": (1e-6, 1e-1, 1, 3.3e-4, 1.0, 0.0),
    "monotone-16-rounds": (1e-6, 1e-1, 16, 3.3e-4, 1.0, 0.0),
    "monotone-threshold-is-a-candidate": (1e-4, 1e-2, 6, float(np.sqrt(np.float64(1e-4)) * np.sqrt(np.float64(1e-2))), 1.0, 0.0),
    # an island of tolerances that meet the target above ones that do not: the walk may or may not land on it
    "island-hit": (1e-6, 1e-1, 8, 2e-5, 2e-4, 5e-4),
    "island-missed": (1e-6, 1e-1, 8, 2e-5, 4e-3, 5e-3),
    "island-16-rounds": (1e-7, 1e1, 16, 3e-6, 9e-4, 1.1e-3),
    "tol-max-meets": (1e-6, 1e-1, 8, 1e-1, 1.0, 0.0),
    "tol-max-meets-on-an-island": (1e-6, 1e-1, 8, 1e-9, 5e-2, 1e-1),
    "tol-min-fails": (1e-6, 1e-1, 8, 9e-7, 1.0, 0.0),
    "tol-min-fails-island-inside": (1e-6, 1e-1, 8, 9e-7, 1e-3, 1e-2),
    "one-point": (1e-3, 1e-3, 4, 1e-3, 1.0, 0.0),
    "one-point-fails": (1e-3, 1e-3, 4, 1e-4, 1.0, 0.0),
    "denormal-to-huge": (5e-324, 1e300, 16, 1e-20, 1.0, 0.0),
}


@pytest.mark.parametrize("name", sorted(SEARCH_CASES))
def test_search_walks_the_restated_doubles(dump, name):
    tol_min, tol_max, rounds, t1, t2, t3 = SEARCH_CASES[name]
    meets = _stub(t1, t2, t3)
    end, tol, coarser, seen = walk(meets, tol_min, tol_max, rounds)
    (line,) = _run(dump, "search %s %s %d %s %s %s\n" % (_hex(tol_min), _hex(tol_max), rounds, _hex(t1), _hex(t2), _hex(t3)))
    got = line.split()
    assert int(got[0]) == end
    assert int(got[3]) == len(seen)
    assert [_hex(float.fromhex(g)) for g in got[4:]] == [_hex(t) for t in seen]
    assert _hex(float.fromhex(got[1])) == _hex(tol) and _hex(float.fromhex(got[2])) == _hex(coarser)
    if name.startswith("tol-max-meets"):
        assert end == FOUND and tol == tol_max and len(seen) == 1
    elif name.startswith("tol-min-fails") or name == "one-point-fails":
        assert end == NOTHING_MEETS and len(seen) == 2
    elif name == "one-point":
        assert end == FOUND and len(seen) == 1
    else:
        assert end == FOUND and len(seen) == 2 + rounds
        # whatever the curve: the result meets the target, the bracket's other end does not
        assert meets(tol) and not meets(coarser) and tol_min <= tol < coarser <= tol_max
        # the bracket is the 2^rounds-th root of the range (in log), up to the rounding of the square roots
        assert abs(np.log(coarser / tol) - np.log(tol_max / tol_min) / 2 ** rounds) <= 1e-9 * np.log(tol_max / tol_min)


def test_search_uses_the_island_when_it_lands_on_it(dump):
    """Not monotone: the result of "island-hit" lies ON the island, above tolerances that fail -- it meets the
    target by measurement -- and "island-missed" ends below its island: compression lost, never the target."""
    for name, on_island in (("island-hit", True), ("island-missed", False)):
        tol_min, tol_max, rounds, t1, t2, t3 = SEARCH_CASES[name]
        _, tol, _, _ = walk(_stub(t1, t2, t3), tol_min, tol_max, rounds)
        assert (t2 <= tol <= t3) == on_island and (tol <= t1) == (not on_island), (name, tol)


@pytest.mark.parametrize("tol_min,tol_max,rounds", [
    (0.0, 1e-1, 4), (-1e-3, 1e-1, 4), (NAN, 1e-1, 4), (1e-1, 1e-3, 4), (1e-3, NAN, 4), (1e-3, INF, 4),
    (1e-6, 1e-1, 0), (1e-6, 1e-1, -1), (1e-6, 1e-1, 17),
])
def test_bad_arguments_have_their_own_end_state(dump, tol_min, tol_max, rounds):
    (line,) = _run(dump, "search %s %s %d %s %s %s\n" % (_hex(tol_min), _hex(tol_max), rounds, _hex(1.0), _hex(1.0), _hex(0.0)))
    got = line.split()
    assert int(got[0]) == BAD_ARGUMENT and int(got[3]) == 0 and len(got) == 4  # (nothing was evaluated)
    assert walk(lambda t: True, tol_min, tol_max, rounds)[0] == BAD_ARGUMENT


# ---- achieved figure and meets ---------------------------------------------------------------------------
def _stats(n=1000, nonfinite=0, max_abs_err=1e-3, argmax=7, sum_sq_err=2.5e-5, ref_min=-1.0, ref_max=3.0,
           ref_abs_max=3.0, ref_sum_sq=1234.5):
    return dict(n=n, nonfinite=nonfinite, max_abs_err=max_abs_err, argmax=argmax, sum_sq_err=sum_sq_err, ref_min=ref_min,
                ref_max=ref_max, ref_abs_max=ref_abs_max, ref_sum_sq=ref_sum_sq)


def _achieved(s, metric):
    """The figures as include/mgard_hip.h defines them (the Python mirror ErrorStats restates the same)."""
    m = s["n"] - s["nonfinite"]
    rmse = float(np.sqrt(np.float64(s["sum_sq_err"]) / m)) if m else 0.0
    if metric == MAX_ABS:
        return s["max_abs_err"]
    if metric == RMSE:
        return rmse
    if rmse == 0:
        return INF
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(20.0 * np.log10(np.float64(s["ref_max"] - s["ref_min"]) / rmse))


def _meets_line(s, metric, target):
    return "meets %d %s %d %d %s %d %s %s %s %s %s\n" % (
        metric, _hex(target), s["n"], s["nonfinite"], _hex(s["max_abs_err"]), s["argmax"], _hex(s["sum_sq_err"]),
        _hex(s["ref_min"]), _hex(s["ref_max"]), _hex(s["ref_abs_max"]), _hex(s["ref_sum_sq"]))


def test_target_meets_in_both_directions(dump):
    s = _stats()
    rmse, psnr = _achieved(s, RMSE), _achieved(s, PSNR)
    assert rmse == float(np.sqrt(2.5e-8)) and 80.0 < psnr < 100.0
    up, down = (lambda x: float(np.nextafter(x, INF))), (lambda x: float(np.nextafter(x, -INF)))
    cases = [
        # an error must not exceed its target ...
        (s, MAX_ABS, 1e-3, 1), (s, MAX_ABS, down(1e-3), 0), (s, MAX_ABS, up(1e-3), 1), (s, MAX_ABS, 0.0, 0),
        (s, MAX_ABS, INF, 1), (s, RMSE, rmse, 1), (s, RMSE, down(rmse), 0), (s, RMSE, up(rmse), 1),
        # ... a PSNR must reach it
        (s, PSNR, psnr, 1), (s, PSNR, up(psnr), 0), (s, PSNR, down(psnr), 1), (s, PSNR, -INF, 1), (s, PSNR, INF, 0),
        # non-finite positions meet nothing, however loose the target
        (_stats(nonfinite=1), MAX_ABS, INF, 0), (_stats(nonfinite=1), RMSE, INF, 0), (_stats(nonfinite=1), PSNR, -INF, 0),
        (_stats(nonfinite=1000, max_abs_err=0.0, sum_sq_err=0.0), MAX_ABS, 1.0, 0),
        # a zero error: infinite PSNR meets any PSNR target, and zero targets are met
        (_stats(max_abs_err=0.0, sum_sq_err=0.0), PSNR, 1e308, 1), (_stats(max_abs_err=0.0, sum_sq_err=0.0), PSNR, INF, 1),
        (_stats(max_abs_err=0.0, sum_sq_err=0.0), MAX_ABS, 0.0, 1), (_stats(max_abs_err=0.0, sum_sq_err=0.0), RMSE, 0.0, 1),
        (_stats(max_abs_err=0.0, sum_sq_err=0.0, ref_min=2.0, ref_max=2.0), PSNR, 300.0, 1),
        # a constant reference with an error: PSNR is -inf and reaches only -inf
        (_stats(ref_min=2.0, ref_max=2.0), PSNR, -1e308, 0), (_stats(ref_min=2.0, ref_max=2.0), PSNR, -INF, 1),
        # a NaN figure meets nothing
        (_stats(max_abs_err=NAN), MAX_ABS, INF, 0), (_stats(sum_sq_err=NAN), RMSE, INF, 0), (_stats(sum_sq_err=NAN), PSNR, -INF, 0),
    ]
    out = _run(dump, "".join(_meets_line(st, metric, target) for st, metric, target, _ in cases))
    assert len(out) == len(cases)
    for (st, metric, target, want), line in zip(cases, out):
        got, meets = line.split()
        got, expect = float.fromhex(got) if "nan" not in got else NAN, _achieved(st, metric)
        assert (np.isnan(got) and np.isnan(expect)) or got == expect or \
            (metric == PSNR and abs(got - expect) <= 1e-12 * abs(expect)), (st, metric, got, expect)  # (log10: not exact IEEE)
        assert int(meets) == want, (st, metric, target, got)


def test_metric_range_and_roundtrip_refusal(dump):
    out = _run(dump, "".join("metric %d\n" % m for m in (-1, 0, 1, 2, 3)) +
               "".join("refusal %d\n" % t for t in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40)))
    assert [int(x) for x in out] == [0, 1, 1, 1, 0, 1, 0, 0, 1, 1]


def test_sanitized_build_agrees(dump, tmp_path_factory):
    """The same program under AddressSanitizer and UBSan, stand-alone: the same output on every search case."""
    san = _build(tmp_path_factory, "target_plan_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    text = ""
    for name in sorted(SEARCH_CASES):
        tol_min, tol_max, rounds, t1, t2, t3 = SEARCH_CASES[name]
        text += "search %s %s %d %s %s %s\n" % (_hex(tol_min), _hex(tol_max), rounds, _hex(t1), _hex(t2), _hex(t3))
    text += _meets_line(_stats(), PSNR, 80.0) + _meets_line(_stats(nonfinite=3), MAX_ABS, 1.0)
    assert _run(san, text) == _run(dump, text)
