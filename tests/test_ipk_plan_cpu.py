"""CPU test of the Thomas-solve planner (mgard_amd/csrc/ipk_plan.hpp): which kernel family a solve
gets, and with which grid, workgroup, LDS and launch arguments.

tests/cpp/ipk_plan_dump.cpp is compiled with g++ against the header alone (no HIP) and run over the
solves of tests/golden/ipk_plans.json. The golden is NOT a print-out of the planner: its rows were
recorded on an MI355X from the commit BEFORE the planner existed (the 300-line ipk_launch), one
process per shape running mgh_decompose_quantize and mgh_dequantize_recompose once each under
rocprofv3 --kernel-trace, and converted by tools/ipk_trace_to_plans.py. `dispatches` (kernel name
with template arguments, grid in workgroups, workgroup size, LDS bytes) are the trace's. The LDS
column of that profiler holds the kernel's STATIC LDS only (`lds_static`: 0 but for the chunked
solve), so the dynamic LDS of a launch is NOT in the trace: the test computes what the KERNEL
indexes (`kernel_lds`, written from the kernels' sources) from the recorded `args` and the solve and
asserts that the plan asks for exactly that. The solve
(`elem`, `axis`, `m`, `nbatch`, `batch_stride`, `add`, the tables' `chunk_need`) and `args` (W,
n_glob, K, KR, P, S, nchunk) are that commit's own launch-argument log, printed by a development
build at each of its launch sites. Every row fixes num_cu = 256 (the MI355X) and the default
switches, but for the rows `from` the three cases that ran with MGH_IPK_SPEC=0, MGH_IPK_CHUNK=0 and
MGH_IPK_STREAM=0 (`tuning`).

One row is NOT from the trace and is marked `awaiting_trace`: 512^3 f32 with MGH_IPK_CHUNK=0, whose
top-level f-solve reaches ipk_launch (at 129 x 129 x 257, the recorded chunk = 0 case, every f- and
c-solve runs in k_ipk_plane_fc and the switch decides nothing). It is derived by hand from the
previous ipk_launch: m = 257^3, axis 2, 66049 pencils of 1028 bytes (n odd: no pad). Rounds of
resident workgroups for w = 64 / 48 / 32 / 16: tiles of 65792 / 49344 / 32896 / 16448 bytes, 2 / 3 /
4 / 8 per CU, 1033 / 1377 / 2065 / 4129 tiles over 256 CUs = 3 / 2 / 3 / 3 rounds, so best_w = 48 with
2 rounds. Not Spec (66049 > 64 pencils), chunk off, not Dma (axis 2), no KR = 16 (257 / 16 < 32), no
KR = 8 (2 rounds < MGH_IPK_CONTIG = 4): k_ipk_lds_contig<float, false>, grid ceil(66049 / 48) = 1377
of 256 threads, P = 48. The case is in tools/ipk_trace_case.py for the next recording.
Not pinned by any row here: the Thread family with nbatch > 1 (one call per box; the case
thread_batches_4d of tools/ipk_trace_case.py is meant to record it). tests/ipk_family_cases.py pins it
on a small 4-D array ("thread-4d-batches"), on the CPU and through the plan log on the GPU.

Shapes (`from`): 512^3 f32 and f64 (non-uniform), 1024^3 f32, the 8 x 512^3 4-D slab, 129^3, 257^3,
16395 x 64 x 64, a 2^24-element 1-D array, 4194304 x 9, 100 x 100 x 6000, 64^4, 8 x 8 x 64^3; with
switches: a 2^20-element 1-D array (spec = 0), 512^3 (chunk = 0), 1024^3 (stream = 0),
129 x 129 x 257 (chunk = 0). tools/ipk_trace.md: how the rows are regenerated."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "ipk_plans.json")))
FAMILIES = ["Spec", "LdsContigChunked", "Dma", "Stream", "LdsContig", "LdsStrided", "Thread"]
CASES = ["512f32", "512f64", "1024f32", "slab4d", "129f32", "257f32", "16395x64x64", "1d_2p24", "4194304x9",
         "100x100x6000", "64p4", "5d", "spec0_1d_2p20", "chunk0_129x129x257", "chunk0_512f32", "stream0_1024f32"]
LDS_PER_CU = 160 * 1024  # kLdsPerCU; the margins of the families: kLdsMarginWave, kLdsMarginChunked
LDS_LIMIT = {"Spec": 0, "LdsContigChunked": LDS_PER_CU - 8192, "Dma": LDS_PER_CU - 4096, "Stream": LDS_PER_CU - 4096,
             "LdsContig": LDS_PER_CU, "LdsStrided": LDS_PER_CU, "Thread": 0}


def kernel_lds(r, pad):
    """Bytes of dynamic LDS the kernel of a golden row indexes, from its recorded launch arguments:
    k_ipk_stream parks W columns of the (n / U - KR) * U - n_glob elements that are neither in
    registers nor left in global memory, and contiguous pencils add TileIO's staging area of
    64 rows of U + 1 (kernels_ipk_stream.hpp); k_ipk_lds_contig keeps P rows of n + pad elements,
    k_ipk_lds_strided W columns of n (kernels_ipk.hpp); k_ipk_dma 64 columns of the n - KR * U
    elements outside the registers (kernels_ipk_dma.hpp); the others use none."""
    a, elem, n = r["args"], r["elem"], r["m"][r["axis"]]
    U = 64 // elem
    return {"Stream": lambda: a["W"] * ((n // U - a["KR"]) * U - a["n_glob"]) * elem +
                              (64 * (U + 1) * elem if r["axis"] == 2 else 0),
            "LdsContig": lambda: a["P"] * (n + pad) * elem, "LdsContigChunked": lambda: a["P"] * (n + pad) * elem,
            "LdsStrided": lambda: a["W"] * n * elem, "Dma": lambda: (n - a["KR"] * U) * 64 * elem,
            "Spec": lambda: 0, "Thread": lambda: 0}[r["family"]]()


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipk_plan") / "ipk_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mgard_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ipk_plan_dump.cpp"), "-o", exe])
    text = ""
    for r in GOLD:
        text += " ".join(map(str, [r["elem"], r["axis"]] + r["m"] + [r["nbatch"], r["batch_stride"], r["add"]] +
                             ["%s=%d" % kv for kv in sorted(r["tuning"].items())])) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    got, cur = [], None
    for line in out.splitlines():
        f = line.split("\t")
        if f[0] == "plan":
            cur = {"plan": dict(kv.split("=") for kv in f[1:]), "dispatches": []}
        elif f[0] == "dispatch":
            cur["dispatches"].append({"kernel": f[1], "grid": int(f[2]), "workgroup": int(f[3]), "lds": int(f[4])})
        elif f[0] == "end":
            got.append(cur)
    assert len(got) == len(GOLD)
    return got


def test_header_compiles_alone_without_hip(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "ipk_plan.hpp"\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "mgard_amd", "csrc"), str(src)])


def test_golden_covers_every_family_and_every_case():
    assert sorted({r["family"] for r in GOLD}) == sorted(FAMILIES)
    assert sorted({c for r in GOLD for c in r["from"]}) == sorted(CASES)
    assert {16, 8} <= {r["args"]["KR"] for r in GOLD if r["family"] == "Stream"}
    assert any(r["nbatch"] > 1 and r["family"] == "Dma" for r in GOLD)
    assert any(r["tuning"].get("chunk") == 0 and r["family"] == "LdsContig" and r["m"][2] >= 64 for r in GOLD)


@pytest.mark.parametrize("i", range(len(GOLD)), ids=["%s-ax%d-%s-b%d-add%d" % (
    r["from"][0], r["axis"], "x".join(map(str, r["m"])), r["nbatch"], r["add"]) for r in GOLD])
def test_plan_is_what_the_trace_of_the_previous_dispatcher_shows(plans, i):
    want, got = GOLD[i], plans[i]
    assert got["plan"]["fam"] == want["family"]
    assert [(d["kernel"], d["grid"], d["workgroup"]) for d in got["dispatches"]] == \
        [(d["kernel"], d["grid"], d["workgroup"]) for d in want["dispatches"]]
    assert {k: int(got["plan"][k]) for k in want["args"]} == want["args"]
    # LDS rows are padded by one element where n is even (kernels_ipk.hpp: k_ipk_lds_contig)
    pad = int(got["plan"]["pad"])
    if want["family"] in ("LdsContig", "LdsContigChunked"):
        assert pad == (1 if want["m"][want["axis"]] % 2 == 0 else 0)
    assert [d["lds"] for d in got["dispatches"]] == [kernel_lds(want, pad)] * len(got["dispatches"])


@pytest.mark.parametrize("i", range(len(GOLD)), ids=[str(i) for i in range(len(GOLD))])
def test_plan_properties(plans, i):
    """Whatever the golden says: LDS within the budget of the family, the grid covers the pencils,
    grids rounded to 8 are multiples of 8, and the families with preconditions keep them."""
    r, p, d = GOLD[i], plans[i]["plan"], plans[i]["dispatches"]
    fam, npencil = p["fam"], int(p["npencil"])
    for x in d:
        assert x["lds"] <= LDS_LIMIT[fam]
    assert int(p["lds_attr"]) <= LDS_PER_CU
    g = d[0]["grid"]
    tile = {"Spec": None, "LdsContigChunked": int(p["P"]), "LdsContig": int(p["P"]), "Dma": 64, "Stream": int(p["W"]),
            "LdsStrided": int(p["W"]), "Thread": None}[fam]
    if tile:
        assert tile > 0 and g * tile >= npencil
    if fam == "Spec":  # one wave per 64 (chunk, pencil) pairs; one lane per pencil in the repair
        assert g * 64 >= npencil * int(p["nchunk"]) and int(p["nchunk"]) * int(p["S"]) >= r["m"][r["axis"]]
        assert d[2]["grid"] * 64 >= npencil and d[1]["grid"] * 256 >= npencil * int(p["nchunk"])
        assert r["tuning"].get("spec", 1) == 1
    if fam == "Thread":  # a call per box, a lane per pencil of the box
        assert len(d) == r["nbatch"] and g * 64 * r["nbatch"] >= npencil
    if fam in ("Dma", "Stream", "LdsStrided"):
        assert g % 8 == 0
    if fam == "Dma":
        assert r["elem"] == 4 and r["axis"] != 2
