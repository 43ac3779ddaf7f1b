"""CPU test of the planner of the fused level passes (mgard_amd/csrc/fused_plan.hpp): tile shape,
face tiles, size class, march length, r-chunks and grid of a level box.

tests/cpp/fused_plan_dump.cpp is compiled with g++ against the header alone (no HIP).

(a) tests/golden/fused_plans.json is NOT a print-out of the planner: its rows were computed from a
Python transcription of the launch arithmetic of the commit BEFORE the planner existed (capi.hip:
level_class, fused_wide_tiles, fused_tall_tiles, fused_rch, fused_nchunk, launch_fused2_t,
launch_fused4_t) with the default switches, for the coarse boxes of 512^3 f32 and f64, 1024^3,
the slices of the 8 x 512^3 slab (nz: even / odd slices), 16395 x 39 x 39 f64, 2048 x 2048 x 17 and
130 x 67 x 35. `wide` is MGH_FUSED_WIDE as the data type sets it (1 floats, 0 doubles). With the
marches pinned the planner must give exactly these launches. Checked by hand: 129^3 coarse is
4 x 16 main tiles + 3 + 2 face tiles = 69, padded to 72 under XCD ranges, 32 chunks of 4.

(b) any box, any slot count: the chunks tile the coarse planes once, none is longer than the
kernel's 16 (the last: 17), the last carries the extra plane.

(c) the policy: rounds x (march + S), S = 1.5, over the launch's own workgroups."""
import itertools
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "fused_plans.json")))
MAX_MARCH = 16


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fused_plan") / "fused_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mgard_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "fused_plan_dump.cpp"), "-o", exe])

    def run(rows):
        """rows: (m, nz_class, nz, slots, switches) -> one dict per row"""
        text = ""
        for m, nzc, nz, slots, sw in rows:
            nz = list(nz) + [0] * (2 - len(nz))
            sl = list(slots) + [0] * (2 - len(slots))
            text += " ".join(map(str, list(m) + [nzc, 2 if nz[1] else 1] + nz + sl +
                                 ["%s=%s" % kv for kv in sorted(sw.items())])) + "\n"
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
        got = []
        for line in out.splitlines():
            d = dict(kv.split("=") for kv in line.split())
            planes = [int(x) for x in d.pop("planes").split(",")]
            d = {k: int(v) for k, v in d.items()}
            d["planes"] = planes
            got.append(d)
        assert len(got) == len(rows)
        return got
    return run


def test_header_compiles_alone_without_hip(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "fused_plan.hpp"\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "mgard_amd", "csrc"), str(src)])


def test_golden_covers_the_shape_classes():
    assert {r["from"] for r in GOLD} == {"512f32", "512f64", "1024f32", "slab4d", "16395x39x39", "2048x2048x17",
                                         "130x67x35"}
    assert {(r["plan"]["TC"], r["plan"]["TF"]) for r in GOLD} == {(8, 32), (4, 64), (64, 4)}
    assert {r["plan"]["cls"] for r in GOLD} == {0, 1, 2}
    assert {r["plan"]["xcd_ranges"] for r in GOLD} == {0, 1} and {r["plan"]["faces"] for r in GOLD} == {0, 1}


@pytest.mark.parametrize("slots", [0, 768, 1024])
def test_pinned_marches_give_the_launches_of_the_previous_code(dump, slots):
    rows = [(r["m"], r["nz_class"], r.get("nz", [1]), [slots, slots], {"wide": r["wide"], "pinned": 1}) for r in GOLD]
    for r, got in zip(GOLD, dump(rows)):
        assert {k: got[k] for k in r["plan"]} == r["plan"], r
        assert got["by_policy"] == 0


def test_unknown_residency_and_the_top_class_keep_the_class_constants(dump):
    rows = [(r["m"], r["nz_class"], r.get("nz", [1]), [0, 0], {"wide": r["wide"]}) for r in GOLD]
    rows += [(r["m"], r["nz_class"], r.get("nz", [1]), [768, 768], {"wide": r["wide"]}) for r in GOLD
             if r["plan"]["cls"] == 2]
    want = GOLD + [r for r in GOLD if r["plan"]["cls"] == 2]
    for r, got in zip(want, dump(rows)):
        assert {k: got[k] for k in r["plan"]} == r["plan"], r
        assert got["by_policy"] == 0


def test_the_tiles_do_not_depend_on_the_residency(dump):
    tiles = ("cls", "TC", "TF", "gxm", "n_main", "ff_F0", "n_ff", "cf_C0", "n_cf", "faces", "ntile", "xcd_ranges",
             "grid_x")
    rows = [(r["m"], r["nz_class"], r.get("nz", [1]), [s, s], {"wide": r["wide"]}) for r in GOLD for s in (8, 768)]
    got = dump(rows)
    for i, r in enumerate(GOLD):
        for g in got[2 * i:2 * i + 2]:
            assert {k: g[k] for k in tiles} == {k: r["plan"][k] for k in tiles}


BOXES = [(m0, m1, m2) for m0 in (2, 3, 5, 9, 16, 17, 18, 33, 34, 65, 66, 129, 130, 257, 1000)
         for (m1, m2) in ((33, 33), (21, 19), (34, 18), (129, 129), (65, 9))]


def test_any_plan_is_valid(dump):
    rows, meta = [], []
    for m, slots in itertools.product(BOXES, (0, 1, 8, 64, 300, 768, 1024, 100000)):
        for sw in ({}, {"box": 0}, {"pinned": 1, "rch0": 16, "rch1": 16}, {"pinned": 1, "rch1": 7, "rch0": 5}):
            rows.append((m, 1, [1], [slots], sw))
            meta.append((m, slots))
        rows.append((m, 3, [5, 3], [slots, max(0, slots - 256)], {}))
        meta.append((m, slots))
    for (m, slots), p in zip(meta, dump(rows)):
        planes = p["planes"]
        assert 1 <= p["rch"] <= MAX_MARCH and len(planes) == p["nchunk"] >= 1
        assert sum(planes) == m[0]  # every coarse plane once: chunk k starts at k * rch
        assert all(x == p["rch"] for x in planes[:-1])
        assert 1 <= planes[-1] <= p["rch"] + 1 <= MAX_MARCH + 1
        if (m[0] - 1) % p["rch"] == 0 and m[0] > 1:  # 2^k + 1 extents: the last chunk owns one plane more
            assert planes[-1] == p["rch"] + 1
        assert p["grid_x"] >= p["ntile"] and (p["grid_x"] % 8 == 0 if p["xcd_ranges"] else p["grid_x"] == p["ntile"])


def cost(p, S=1.5):
    return (p["rounds0"] + p["rounds1"]) * (p["rch"] + S)


def by_hand(m_r, grid_x, slots, S=1.5, nz=1):
    """rounds x (march + S) over the marches 1 .. 16, the longer of equal ones"""
    best = None
    for r in range(1, MAX_MARCH + 1):
        nchunk = max(1, (m_r - 1 + r - 1) // r)
        c = -(-grid_x * nchunk * nz // slots) * (r + S)
        if best is None or c <= best[0]:
            best = (c, r, nchunk)
    return best


def test_policy_512_cube_levels(dump):
    l8, l7 = (129, 129, 129), (65, 65, 65)
    p8, p7, q8, q7 = dump([(l8, 1, [1], [768], {}), (l7, 1, [1], [768], {}),
                           (l8, 1, [1], [1024], {}), (l7, 1, [1], [1024], {})])
    # 768 slots: 72 x 10 chunks of 13 fit one round (72 x 11 chunks of 12 = 792 do not); level 7 marches 2
    assert (p8["by_policy"], p8["rounds0"], p8["rch"], p8["nchunk"], p8["wg0"]) == (1, 1, 13, 10, 720)
    assert (p7["by_policy"], p7["rounds0"], p7["rch"], p7["nchunk"], p7["wg0"]) == (1, 1, 2, 32, 608)
    assert p7["rch"] < 4
    # 1024 slots: 13 chunks of 10 (936 workgroups) fit; 15 of 9 (1080) do not
    assert (q8["rounds0"], q8["rch"], q8["nchunk"], q8["wg0"]) == (1, 10, 13, 936)
    assert (q7["rounds0"], q7["rch"]) == (1, 2)
    for p, (m, slots) in zip((p8, p7, q8, q7), ((l8, 768), (l7, 768), (l8, 1024), (l7, 1024))):
        assert (cost(p), p["rch"], p["nchunk"]) == by_hand(m[0], p["grid_x"], slots)


def test_policy_flips_one_slot_below_the_plan(dump):
    for m in ((129, 129, 129), (65, 65, 65), (130, 67, 35)):
        for slots in (768, 1024):
            p, = dump([(m, 1, [1], [slots], {})])
            if p["rounds0"] != 1:
                continue
            at, below = dump([(m, 1, [1], [p["wg0"]], {}), (m, 1, [1], [p["wg0"] - 1], {})])
            assert (at["rch"], at["rounds0"]) == (p["rch"], 1)
            assert below["rch"] != p["rch"]
            assert (cost(below), below["rch"], below["nchunk"]) == by_hand(m[0], p["grid_x"], p["wg0"] - 1)


def test_policy_counts_slices_and_follows_S(dump):
    m = (129, 129, 129)
    one, two = dump([(m, 1, [1], [768], {}), (m, 2, [3, 2], [768, 512], {})])
    assert two["wg0"] == 3 * 72 * two["nchunk"] and two["wg1"] == 2 * 72 * two["nchunk"]
    assert two["rounds0"] == -(-two["wg0"] // 768) and two["rounds1"] == -(-two["wg1"] // 512)
    s0, s8 = dump([(m, 1, [1], [768], {"S": 0}), (m, 1, [1], [768], {"S": 8})])
    assert s0["rch"] <= one["rch"] <= s8["rch"]
    ov, = dump([(m, 1, [1], [768], {"slots_override": 1024})])
    assert (ov["rch"], ov["wg0"]) == (10, 936)
    # a best plan of more than two rounds of a launch is not taken: the class constant marches
    many, few = dump([(m, 1, [1], [64], {}), (m, 1, [1], [512], {})])
    assert (many["by_policy"], many["rch"], many["nchunk"]) == (0, 4, 32) and many["rounds0"] == 36
    assert (few["by_policy"], few["rch"], few["rounds0"]) == (1, 10, 2)
    # the box-kernel levels are not marched at all, whatever the plan says
    small, = dump([((33, 33, 33), 1, [1], [768], {})])
    assert small["cls"] == 0 and small["box_kernel"] == 1
