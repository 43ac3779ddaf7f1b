"""The table of small streaming-solve cases (tests/ipk_stream_cases.py) against the planner
(mgard_amd/csrc/ipk_plan.hpp through tests/cpp/ipk_plan_dump.cpp, compiled without HIP): every solve
of the table is planned as k_ipk_stream with the attributes the table gives, and the table as a
whole reaches every class of the kernel it is there for. tests/test_gpu_ipk_stream.py runs the same
table on the GPU and checks the library's own plan log against it."""
import os
import subprocess

import pytest

from tests.ipk_stream_cases import CASES, RANGE_CASES, tuning

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [(c, s, add) for c in CASES + RANGE_CASES for s in c["solves"] for add in s["add"]]
MB = 1 << 20


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipk_stream_cases") / "ipk_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mgard_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ipk_plan_dump.cpp"), "-o", exe])
    text = ""
    for c, s, add in ROWS:
        text += " ".join(map(str, [s["elem"], s["axis"], *s["m"], s["nbatch"], s["batch_stride"], add] +
                             ["%s=%d" % kv for kv in sorted(tuning(c["env"]).items())])) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    got = []
    for line in out.splitlines():
        f = line.split("\t")
        if f[0] == "plan":
            got.append(dict(kv.split("=") for kv in f[1:]))
        elif f[0] == "dispatch":
            got[-1].update(kernel=f[1], grid=int(f[2]), lds=int(f[4]))
    assert len(got) == len(ROWS)
    return got


def _facts(c, s, p):
    """What a planned solve exercises in k_ipk_stream, from the table row and the plan."""
    U = 64 // s["elem"]
    n = s["m"][s["axis"]]
    W, n_glob, KR, npencil = int(p["W"]), int(p["n_glob"]), int(p["KR"]), int(p["npencil"])
    parked = (n // U - KR) * U
    tiles = -(-npencil // W)
    n_inner = {0: s["m"][1] * s["m"][2], 1: s["m"][2], 2: npencil}[s["axis"]]
    return dict(elem=s["elem"], axis=s["axis"], n=n, U=U, rem=n % U, nb=n // U, KR=KR, W=W, n_glob=n_glob, parked=parked,
                lds=p["lds"], last_rows=npencil - (tiles - 1) * W, tiles=tiles, grid=p["grid"], n_inner=n_inner,
                nbatch=s["nbatch"], nonuniform=c["nonuniform"], narrowed_by_switch="MGH_IPK_W" in c["env"],
                v1=c["env"].get("MGH_FORCE_V1") == "1", ndim=len(c["shape"]), fine=c["shape"])


@pytest.mark.parametrize("i", range(len(ROWS)), ids=["%s-ax%d-add%d" % (c["id"], s["axis"], add) for c, s, add in ROWS])
def test_planner_takes_the_streaming_kernel_with_the_attributes_of_the_table(plans, i):
    (c, s, add), p = ROWS[i], plans[i]
    if s["W"] is None:  # (a range case on the device's own CU count: whatever kernel solves it)
        return
    assert p["fam"] == "Stream"
    assert (int(p["W"]), int(p["n_glob"]), int(p["KR"])) == (s["W"], s["n_glob"], s["KR"])
    f = _facts(c, s, p)
    # dynamic LDS = what the kernel indexes: W columns of the parked elements that are not in global
    # memory, + TileIO's staging area of 64 rows of U + 1 for contiguous pencils
    assert p["lds"] == f["W"] * (f["parked"] - f["n_glob"]) * s["elem"] + (64 * (f["U"] + 1) * s["elem"] if s["axis"] == 2 else 0)
    assert p["grid"] % 8 == 0 and p["grid"] >= f["tiles"]
    assert f["n_glob"] % f["U"] == 0 and 0 <= f["n_glob"] <= f["parked"]
    assert p["kernel"] == "k_ipk_stream<%s, %d, %d, 1, %s, false>" % (
        "float" if s["elem"] == 4 else "double", f["U"], f["KR"], "true" if s["axis"] == 2 else "false")


def test_cases_are_small_and_their_boxes_come_from_their_shapes():
    for c in CASES + RANGE_CASES:
        size = 1
        for e in c["shape"]:
            size *= e
        assert size <= 8 << 20, c["id"]
        assert size <= 5 << 20 or c["id"] == "range-empty", c["id"]  # (3 x 600 x 600: the smallest with m[0] < ranges at 1 MB)
        coarse = tuple(e // 2 + 1 for e in c["shape"][-3:])
        for s in c["solves"]:
            assert s["elem"] == {"f32": 4, "f64": 8}[c["dtype"]]
            assert s["m"][1:] == coarse[1:], c["id"]
            if "ranges" in c:
                assert s["m"][0] in c["ranges"] and s["m"][0] > 0
            else:
                assert s["m"] == coarse, c["id"]
            if s["nbatch"] > 1:
                assert len(c["shape"]) == 4 and s["nbatch"] == c["shape"][0] // 2 + 1
                assert s["batch_stride"] == coarse[0] * coarse[1] * coarse[2]
    for c in RANGE_CASES:
        elem = {"f32": 4, "f64": 8}[c["dtype"]]
        m = tuple(e // 2 + 1 for e in c["shape"])
        assert m == c["coarse"]
        box_b, range_b = m[0] * m[1] * m[2] * elem, int(c["env"]["MGH_IPK_RANGE_MB"]) * MB
        assert 2 * range_b < box_b <= 5 * range_b
        nrange = -(-box_b // range_b)
        assert tuple(m[0] * (k + 1) // nrange - m[0] * k // nrange for k in range(nrange)) == c["ranges"]
        # (ipk_plane_fits_lds)
        assert c["plane_in_lds"] == (m[1] * (m[2] | 1) * elem <= 150 * 1024 and m[1] <= 1024 and m[2] <= 1024)
    assert any(m0 == 0 for c in RANGE_CASES for m0 in c["ranges"])           # an empty range
    assert any(len(set(c["ranges"])) > 1 and 0 not in c["ranges"] for c in RANGE_CASES)  # m[0] not a multiple of the ranges
    assert {c["dtype"] for c in RANGE_CASES} == {"f32", "f64"}
    assert any("MGH_IPK_PLAN_CU" in c["env"] for c in RANGE_CASES)


def test_table_covers_every_class(plans):
    F = [_facts(c, s, p) for (c, s, add), p in zip(ROWS, plans) if s["W"] is not None and c in CASES]
    adds = {(s["axis"], add) for c, s, add in ROWS if c in CASES}

    def some(pred):
        return any(pred(f) for f in F)

    strided = lambda f: f["axis"] != 2  # noqa: E731
    contig = lambda f: f["axis"] == 2   # noqa: E731
    classes = {
        # types and registers
        "KR 8 f32": lambda f: f["KR"] == 8 and f["elem"] == 4,
        "KR 8 f64": lambda f: f["KR"] == 8 and f["elem"] == 8,
        "KR 16 f32": lambda f: f["KR"] == 16 and f["elem"] == 4 and f["n"] >= 512,
        "KR 8 on a KR 16 box (MGH_IPK_KR16=0): many batches parked": lambda f: f["KR"] == 8 and f["n"] >= 512 and f["nb"] - 8 >= 24,
        # axes
        "strided, axis 0": lambda f: f["axis"] == 0,
        "strided, axis 1, tiles straddle planes": lambda f: f["axis"] == 1 and f["n_inner"] % f["W"] != 0,
        "contiguous, axis 2": contig,
        # global parking
        "strided n_glob == 0 < parked": lambda f: strided(f) and f["n_glob"] == 0 < f["parked"],
        "strided 0 < n_glob < parked": lambda f: strided(f) and 0 < f["n_glob"] < f["parked"],
        "strided nothing parked, LDS 0": lambda f: strided(f) and f["parked"] == 0 and f["lds"] == 0,
        "contiguous n_glob == 0 < parked": lambda f: contig(f) and f["n_glob"] == 0 < f["parked"],
        "contiguous 0 < n_glob < parked": lambda f: contig(f) and 0 < f["n_glob"] < f["parked"],
        "contiguous LDS = the staging area alone": lambda f: contig(f) and f["lds"] == 64 * (f["U"] + 1) * f["elem"],
        # tile width
        "W 64": lambda f: f["W"] == 64,
        "W < 64 through MGH_IPK_W": lambda f: f["W"] < 64 and f["narrowed_by_switch"],
        "W < 64 through residency": lambda f: f["W"] < 64 and not f["narrowed_by_switch"],
        "contiguous W < 64: lanes beyond W shadow the last row": lambda f: contig(f) and f["W"] < 64,
        # last tile, empty tiles
        "strided last tile partial": lambda f: strided(f) and f["last_rows"] < f["W"],
        "contiguous last tile of 2..15 rows": lambda f: contig(f) and 1 < f["last_rows"] < 16,
        "contiguous last tile of 1 row": lambda f: contig(f) and f["last_rows"] == 1,
        "contiguous last tile of 16+ rows, partial": lambda f: contig(f) and 16 <= f["last_rows"] < f["W"],
        "empty tiles": lambda f: f["grid"] > f["tiles"],
        # batches, grids, paths
        "nbatch > 1 on the 4-D slice-by-slice path": lambda f: f["nbatch"] > 1 and f["ndim"] == 4 and not f["v1"],
        "non-uniform f32": lambda f: f["nonuniform"] and f["elem"] == 4,
        "non-uniform f64": lambda f: f["nonuniform"] and f["elem"] == 8,
        "non-uniform contiguous": lambda f: f["nonuniform"] and contig(f),
        "without MGH_FORCE_V1 (r-solves only)": lambda f: not f["v1"] and f["ndim"] == 3,
        "with MGH_FORCE_V1": lambda f: f["v1"],
        "fine extent 2n - 1 along the pencil": lambda f: f["fine"][f["axis"] - 3] == 2 * f["n"] - 1,
        "fine extent 2n - 2 along the pencil (ghost node)": lambda f: f["fine"][f["axis"] - 3] == 2 * f["n"] - 2,
    }
    for elem, U in ((4, 16), (8, 8)):
        for name, rem in (("0", 0), ("1", 1), ("U - 1", U - 1)):
            classes["n mod U == %s, elem %d" % (name, elem)] = lambda f, e=elem, r=rem: f["elem"] == e and f["rem"] == r
        classes["1 < n mod U < U - 1, elem %d" % elem] = lambda f, e=elem: f["elem"] == e and 1 < f["rem"] < f["U"] - 1
        classes["n / U == KR, elem %d" % elem] = lambda f, e=elem: f["elem"] == e and f["nb"] == f["KR"]
        classes["n / U == KR + 1, elem %d" % elem] = lambda f, e=elem: f["elem"] == e and f["nb"] == f["KR"] + 1
    missing = [name for name, pred in classes.items() if not some(pred)]
    assert not missing, missing
    assert {f["W"] for f in F} >= {64, 60, 48, 32}
    # add: plain (f- and c-solves), + (r-solve of decompose), - (r-solve of recompose)
    assert {(0, +1), (0, -1)} <= adds and {(1, 0), (2, 0)} <= adds
