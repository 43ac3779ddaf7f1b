"""CPU test of mgard_amd/csrc/size_plan.hpp: the record and container brackets, the rule for the
synchronisation points, the split of tolerances into histogram launches, and the budget search.

tests/cpp/size_plan_dump.cpp is compiled with g++ against the header alone (no HIP) and once more with
-fsanitize=address,undefined as a stand-alone binary. The expectations are tests/size_model.py, a
restatement from the format and from the text of the search."""
import os
import subprocess

import numpy as np
import pytest

from tests import size_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgard_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "size_plan_dump.cpp")


def _build(tmp_path_factory, name, extra=()):
    exe = str(tmp_path_factory.mktemp(name) / "size_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", CSRC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return _build(tmp_path_factory, "size_plan")


def _run(exe, text):
    return subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=300).stdout.splitlines()


def test_header_compiles_alone_without_hip(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "size_plan.hpp"\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", CSRC, str(src)])


# ---- brackets ----------------------------------------------------------------------------------------
def _record_cases():
    rng = np.random.default_rng(20240611)
    cases = []
    for chunk in (7, 1023, 1024, 1025, 20480, 20481):
        for dict_size in (2, 64, 256, 8192, 16384):
            for n in (1, chunk - 1, chunk, chunk + 1, 3 * chunk, 3 * chunk + 77, 40 * chunk + 5):
                if n < 1:
                    continue
                for _ in range(3):
                    bits = int(rng.integers(0, 33 * n + 1))
                    nout = int(rng.integers(0, n + 1)) if rng.random() < 0.5 else 0
                    cases.append((n, dict_size, chunk, bits, nout))
                # whole units, and both sides of the 4-bits-per-symbol threshold of the synchronisation points
                cases += [(n, dict_size, chunk, 64 * (n // 7), 0), (n, dict_size, chunk, 4 * n, 3),
                          (n, dict_size, chunk, max(4 * n - 1, 0), 3), (n, dict_size, chunk, 0, 0)]
    return cases


def test_record_bracket_and_sync_rule_against_the_restatement(dump):
    cases = _record_cases()
    text = ""
    for n, d, c, bits, nout in cases:
        for env in (0, 1):
            text += "sync 0 %d %d %d %d %d\n" % (d, c, bits, n, env)
        text += "sync 2 %d %d %d %d 1\n" % (d, c, bits, n)
        for sync in (0, 1):
            text += "record %d %d %d %d %d %d\n" % (n, d, c, bits, nout, sync)
    out = iter(_run(dump, text))
    seen_sync = set()
    for n, d, c, bits, nout in cases:
        for env in (0, 1):
            want = sm.has_sync(sm.HUFFMAN, d, c, bits, n, env)
            assert int(next(out)) == int(want), (n, d, c, bits, env)
            seen_sync.add((c >= 1024, bits >= 4 * n, bool(want)))
        assert int(next(out)) == 0  # Huffman_Zstd never carries them
        for sync in (0, 1):
            lo, hi = map(int, next(out).split())
            assert (lo, hi) == sm.record_bracket(n, d, c, bits, nout, bool(sync)), (n, d, c, bits, nout, sync)
            assert lo <= hi and hi - lo <= 8 * sm.nchunks(n, c)
    # both sides of the threshold in the bits and of chunk = 1024 were there, with both answers
    assert {(True, True, True), (True, False, False), (False, True, False)} <= seen_sync


def test_exact_size_lies_inside_the_bracket(dump):
    """Per-chunk bit counts drawn at random: min <= the size with every chunk padded on its own <= max;
    both ends are reached (all chunks whole units: min; every chunk one bit over: max)."""
    rng = np.random.default_rng(7)
    text, want = "", []
    for chunk, n in ((7, 5), (7, 7), (7, 50), (1024, 1024 * 6), (1024, 1024 * 6 + 1), (20480, 20480 * 9 + 3)):
        nc = sm.nchunks(n, chunk)
        draws = [rng.integers(0, 32 * chunk, nc) for _ in range(20)]
        draws += [64 * rng.integers(0, chunk // 2 + 1, nc), 64 * rng.integers(0, chunk // 2 + 1, nc) + 1]
        for cb in draws:
            nout = int(rng.integers(0, 4))
            text += "record %d 256 %d %d %d 1\n" % (n, chunk, int(cb.sum()), nout)
            want.append((sm.record_exact(n, 256, chunk, cb, nout, True), nc))
    out = _run(dump, text)
    hit_lo = hit_hi = 0
    for line, (exact, nc) in zip(out, want):
        lo, hi = map(int, line.split())
        assert lo <= exact <= hi and hi - lo <= 8 * nc
        hit_lo += exact == lo
        hit_hi += exact == hi
    assert hit_lo >= 6 and hit_hi >= 6


def test_container_bracket_and_the_raw_threshold(dump):
    rng = np.random.default_rng(11)
    cases = []
    for elem in (4, 8):
        for n in (1, 100, 11220, 1 << 20):
            dense = n * elem
            # record == n * elem counts as raw (a reader takes a record of that size for the array itself;
            # the container has the same bytes either way), eight bytes less does not
            for rec in ((dense, dense), (dense - 8, dense), (dense, dense + 8), (dense + 8, dense + 16),
                        (dense - 16, dense - 8), (dense - 8, dense + 8)):
                if rec[0] > 0:
                    cases.append((int(rng.integers(40, 4000)), n, elem, rec))
            for _ in range(10):
                lo = int(rng.integers(1, 3 * dense + 2))
                cases.append((int(rng.integers(40, 4000)), n, elem, (lo, lo + 8 * int(rng.integers(0, 50)))))
    out = _run(dump, "".join("container %d %d %d %d %d\n" % (m, n, e, r[0], r[1]) for m, n, e, r in cases))
    raws = set()
    for line, (m, n, e, r) in zip(out, cases):
        got = tuple(map(int, line.split()))
        assert got == sm.container_bracket(m, n, e, r), (m, n, e, r)
        assert got[1] <= m + 8 + n * e
        raws.add(got[2])
    assert raws == {1, 0, -1}
    # the threshold itself
    (a,), (b,) = [[tuple(map(int, l.split())) for l in _run(dump, "container 100 10 4 %d %d\n" % r)] for r in ((32, 32), (40, 40))]
    assert a == (140, 140, 0) and b == (148, 148, 1)


# ---- histogram launches --------------------------------------------------------------------------------
def test_launch_split_covers_every_tolerance_within_128_kb(dump):
    cases = [(d, k) for d in (2, 64, 8192, 16384) for k in range(1, 65)]
    out = _run(dump, "".join("split %d %d\n" % c for c in cases))
    for line, (d, k) in zip(out, cases):
        launches = list(map(int, line.split()))
        assert sum(launches) == k and min(launches) >= 1
        assert all(4 * d * x <= 128 * 1024 and x <= 8 for x in launches)
        per = min(8, 128 * 1024 // (4 * d))
        assert launches == [per] * (k // per) + ([k % per] if k % per else [])
    assert _run(dump, "split 16384 5\nsplit 8192 9\nsplit 64 9\n") == ["2 2 1 ", "4 4 1 ", "8 1 "]


def test_argument_check_of_the_histogram_call(dump):
    rows = [((1, 1, 2), 0), (((1 << 32) - 1, 64, 16384), 0), ((1 << 32, 1, 8192), 1), ((1 << 40, 1, 8192), 1),
            ((0, 1, 8192), 1), ((100, 0, 8192), 1), ((100, 65, 8192), 1), ((100, 1, 1), 1), ((100, 1, 16385), 1)]
    out = _run(dump, "".join("refuse %d %d %d\n" % r for r, _ in rows))
    assert [int(x) for x in out] == [w for _, w in rows]


# ---- the search ----------------------------------------------------------------------------------------
INF = float("inf")


def _search_cmd(tol_min, tol_max, rounds, intervals):
    flat = [float(x).hex() for iv in intervals for x in iv]
    return "search %s %s %d %d %s\n" % (float(tol_min).hex(), float(tol_max).hex(), rounds, len(intervals), " ".join(flat))


def _fits(intervals):
    return lambda t: any(lo <= float(t) <= hi for lo, hi in intervals)


def _search_cases():
    lo, hi = 1e-7, 1e-1
    m1, m2, m3 = (float(x) for x in sm.quartiles(lo, hi))
    n1, n2, n3 = (float(x) for x in sm.quartiles(lo, m1))
    cases = []
    for rounds in range(1, 9):
        cases += [
            ("monotone", lo, hi, rounds, [(3.3e-4, INF)]),
            ("monotone, early", 3e-9, 2e3, rounds, [(4.1e-9, INF)]),
            ("step exactly at a candidate", lo, hi, rounds, [(m2, INF)]),
            ("step exactly at a second-round candidate", lo, hi, rounds, [(n3, INF)]),
            ("step just above a candidate", lo, hi, rounds, [(np.nextafter(m1, 1.0), INF)]),
            ("not monotone: a hole above the first fit", lo, hi, rounds, [(2e-5, 5e-4), (3e-3, INF)]),
            ("not monotone: islands", lo, hi, rounds, [(n1, n1), (m3, m3), (hi, hi)]),
            ("only tol_max fits", lo, hi, rounds, [(hi, hi)]),
            ("tol_min fits", lo, hi, rounds, [(lo, INF)]),
            ("tol_min fits, nothing else", lo, hi, rounds, [(lo, lo)]),
            ("nothing fits", lo, hi, rounds, []),
            ("nothing fits but the middle", lo, hi, rounds, [(m2, m2)]),
            ("one point", 1e-3, 1e-3, rounds, [(1e-3, INF)]),
        ]
    return cases


def test_search_is_bit_equal_to_the_restatement_and_its_result_fits(dump):
    cases = _search_cases()
    out = _run(dump, "".join(_search_cmd(a, b, r, iv) for _, a, b, r, iv in cases))
    ends = set()
    for line, (name, a, b, rounds, iv) in zip(out, cases):
        end, tol, finer, index, evals = line.split()
        fits = _fits(iv)
        want, want_finer = sm.search(fits, a, b, rounds)
        ends.add(end)
        if want is None:
            assert end == "nothing" and int(evals) == 2, name
            continue
        assert end == "found", name
        got = float.fromhex(tol)
        assert got.hex() == float(want).hex(), (name, rounds, got, want)
        assert fits(got), name
        if want_finer is None:
            assert got == a and int(index) == 0 and int(evals) == 1, name
        else:
            assert float.fromhex(finer).hex() == float(want_finer).hex(), name
            assert not fits(float.fromhex(finer)), name
            assert int(evals) == 2 + 3 * rounds, name
        if name == "monotone":
            # the bracket shrinks to a quarter (in log) per round and still holds the step
            assert float.fromhex(finer) < 3.3e-4 <= got
            assert np.log(got / float.fromhex(finer)) <= np.log(b / a) / 4 ** rounds * (1 + 1e-9)
    assert ends == {"found", "nothing"}


def test_search_refuses_bad_arguments(dump):
    rows = [(0.0, 1.0, 4), (-1.0, 1.0, 4), (2.0, 1.0, 4), (1e-3, 1.0, 0), (1e-3, 1.0, 9), (float("nan"), 1.0, 4),
            (1e-3, INF, 4)]
    out = _run(dump, "".join(_search_cmd(a, b, r, [(0.0, INF)]) for a, b, r in rows))
    assert [l.split()[0] for l in out] == ["bad"] * len(rows)


def test_program_is_clean_under_address_and_undefined_sanitizers(tmp_path_factory):
    exe = _build(tmp_path_factory, "size_plan_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    text = "".join("record %d %d %d %d %d 1\n" % c for c in _record_cases()[:400])
    text += "".join(_search_cmd(a, b, r, iv) for _, a, b, r, iv in _search_cases())
    text += "".join("split %d %d\n" % (d, k) for d in (2, 64, 8192, 16384) for k in (1, 5, 64))
    text += "container 100 10 4 40 48\nrefuse 4294967296 1 8192\nsync 0 8192 20480 81920 20480 1\n"
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-4000:]
    assert len(p.stdout.splitlines()) == text.count("\n")
