"""The table of small cases for the Dma, LdsContigChunked, LdsContig, LdsStrided, Spec and Thread
solves (tests/ipk_family_cases.py) against the planner (mgard_amd/csrc/ipk_plan.hpp through
tests/cpp/ipk_plan_dump.cpp, compiled without HIP): every solve of the table is planned as the family
the table names with the table's arguments, and the table as a whole reaches every class it is there
for. tests/test_gpu_ipk_families.py runs the same table on the GPU and checks the library's own plan
log against it."""
import os
import subprocess

import pytest

from tests.ipk_family_cases import CASES, LARGER, MAX_ELEMS, NEED
from tests.ipk_stream_cases import tuning

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [(c, s, add) for c in CASES for s in c["solves"] for add in s["add"]]
ELEM = {"f32": 4, "f64": 8}
ARGS = {"Dma": ("KR",), "LdsContigChunked": ("P", "K"), "LdsContig": ("P",), "LdsStrided": ("W",), "Spec": ("K",),
        "Thread": ()}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipk_family_cases") / "ipk_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mgard_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ipk_plan_dump.cpp"), "-o", exe])
    text = ""
    for c, s, add in ROWS:
        t = dict(tuning(c["env"]), chunk_need=c["chunk_need"])
        text += " ".join(map(str, [s["elem"], s["axis"], *s["m"], s["nbatch"], s["batch_stride"], add] +
                             ["%s=%d" % kv for kv in sorted(t.items())])) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    got = []
    for line in out.splitlines():
        f = line.split("\t")
        if f[0] == "plan":
            got.append(dict((kv.split("=") for kv in f[1:]), kernels=[], grid=0, lds=0))
        elif f[0] == "dispatch":
            got[-1]["kernels"].append(f[1])
            got[-1].update(grid=int(f[2]), lds=int(f[4]))
    assert len(got) == len(ROWS)
    return got


def _facts(c, s, add, p):
    """What a planned solve exercises, from the table row and the plan."""
    n, npencil = s["m"][s["axis"]], int(p["npencil"])
    n_inner = {0: s["m"][1] * s["m"][2], 1: s["m"][2], 2: npencil}[s["axis"]]
    width = {"Dma": 64, "LdsStrided": s["W"], "LdsContig": s["P"], "LdsContigChunked": s["P"]}.get(s["family"], 64)
    tiles = -(-npencil // width)
    fits = ELEM[c["dtype"]] * s["m"][1] * (s["m"][2] | 1) <= 150 * 1024 and s["m"][1] <= 1024 and s["m"][2] <= 1024
    return dict(fam=s["family"], elem=s["elem"], axis=s["axis"], n=n, add=add, npencil=npencil, n_inner=n_inner,
                last=npencil - (tiles - 1) * width, width=width, W=s["W"], K=s["K"], nbatch=s["nbatch"], env=c["env"],
                v1=c["env"].get("MGH_FORCE_V1") == "1", ndim=len(c["shape"]), plane_fits=fits, per_batch=s["per_batch"],
                nonuniform=c["nonuniform"], pad=int(p["pad"]),
                too_long=16 * (n + (s["axis"] == 2 and n % 2 == 0)) * s["elem"] > 160 * 1024)


@pytest.mark.parametrize("i", range(len(ROWS)), ids=["%s-ax%d-add%d" % (c["id"], s["axis"], add) for c, s, add in ROWS])
def test_planner_takes_the_family_with_the_arguments_of_the_table(plans, i):
    (c, s, add), p = ROWS[i], plans[i]
    assert p["fam"] == s["family"]
    for a in ARGS[s["family"]]:
        assert s[a] > 0, "the table leaves %s of a %s solve open" % (a, s["family"])
    # (members a family does not use are 0 in the plan and in the table)
    assert {a: int(p[a]) for a in ("W", "P", "K", "KR")} == {a: s[a] for a in ("W", "P", "K", "KR")}
    assert int(p["n_glob"]) == 0 and int(p["per_batch"]) == int(s["per_batch"])
    T = "float" if s["elem"] == 4 else "double"
    n, npencil = s["m"][s["axis"]], int(p["npencil"])
    if s["family"] == "Dma":
        assert s["elem"] == 4 and s["axis"] != 2 and n >= 160
        assert p["kernels"] == ["k_ipk_dma<float, 16, 10, %d, true>" % add]
        assert p["lds"] == (n - 160) * 64 * 4 and p["grid"] % 8 == 0 and p["grid"] * 64 >= npencil
    elif s["family"] == "LdsStrided":
        assert p["kernels"] == ["k_ipk_lds_strided<%s, %d>" % (T, s["W"])]
        assert p["lds"] == s["W"] * n * s["elem"] <= 160 * 1024 and p["grid"] * s["W"] >= npencil
        assert s["W"] == 64 or (s["W"] + 16) * n * s["elem"] > 160 * 1024  # (the widest tile that fits)
    elif s["family"] in ("LdsContig", "LdsContigChunked"):
        assert p["kernels"] == ["k_ipk_lds_contig<%s, %s>" % (T, "true" if s["family"] == "LdsContigChunked" else "false")]
        assert int(p["pad"]) == (n % 2 == 0) and p["lds"] == s["P"] * (n + int(p["pad"])) * s["elem"]
        assert p["grid"] == -(-npencil // s["P"])
        if s["family"] == "LdsContigChunked":
            assert s["K"] == int(c["env"].get("MGH_IPK_CHUNK_K", c["chunk_need"])) <= n // 2 and n >= 64
    elif s["family"] == "Spec":
        assert s["K"] == int(c["env"].get("MGH_IPK_SPEC_K", 64 if s["elem"] == 4 else 128))
        assert ("k_ipk_spec_apply<%s>" % T in p["kernels"]) == (add != 0)
        assert int(p["S"]) == 128 and int(p["nchunk"]) == -(-n // 128)
    else:
        assert p["kernels"] == ["k_ipk<%s, %d>" % (T, s["axis"])] * (s["nbatch"] if s["per_batch"] else 1)


def _boxes(shape):
    """The coarse boxes of the top level that ipk_launch is given for an array: {axis: (m, nbatch, stride)}."""
    mc = tuple(e // 2 + 1 for e in shape)
    if len(shape) == 4:
        m3a = (mc[0] * mc[1], mc[2], mc[3])
        return {2: (m3a, 1, 0), 1: (m3a, 1, 0), 0: (mc[1:], mc[0], mc[1] * mc[2] * mc[3])}
    m = (1,) * (3 - len(shape)) + mc
    return {axis: (m, 1, 0) for axis in range(3)}


def test_cases_are_small_and_their_boxes_come_from_their_shapes():
    ids = [c["id"] for c in CASES]
    assert len(ids) == len(set(ids))
    assert set(LARGER) <= set(ids)
    for c in CASES:
        size = 1
        for e in c["shape"]:
            size *= e
        assert size <= MAX_ELEMS or LARGER.get(c["id"]), c["id"]
        assert c["chunk_need"] == (NEED[c["dtype"]] if len(c["shape"]) <= 3 else 0)
        assert "MGH_IPK_PLAN_CU" not in c["env"]  # (Stream has its own table)
        for s in c["solves"]:
            m, nbatch, stride = _boxes(c["shape"])[s["axis"]]
            assert s["elem"] == ELEM[c["dtype"]], c["id"]
            assert (s["m"], s["nbatch"]) == (m, nbatch), c["id"]
            assert nbatch == 1 or s["batch_stride"] == stride, c["id"]
            v1 = c["env"].get("MGH_FORCE_V1") == "1" or len(c["shape"]) < 3
            if len(c["shape"]) == 4:
                assert s["add"] == (0,), c["id"]
            elif s["axis"] == 0 or (v1 and len(c["shape"]) - 3 + s["axis"] == 0):
                assert s["add"] == (+1, -1), c["id"]  # (the last solve of a level is added to the coarse nodes)
            else:
                assert s["add"] == (0,), c["id"]
                # (reaches the planner at all: not the plane kernel of the fused 3-D route)
                fits = s["elem"] * m[1] * (m[2] | 1) <= 150 * 1024 and m[1] <= 1024 and m[2] <= 1024
                assert v1 or not fits, c["id"]
            if len(c["shape"]) == 3 and not v1:
                assert m[0] * m[1] * m[2] >= (16384 if s["elem"] == 4 else 8192), c["id"]  # (beyond the tail kernel)
        # the fastest extent is no multiple of 64
        assert c["shape"][-1] % 64, c["id"]
    # arrays shared between cases agree on their coordinates: one oracle run serves them
    for a in CASES:
        for b in CASES:
            assert (a["shape"], a["dtype"]) != (b["shape"], b["dtype"]) or a["nonuniform"] == b["nonuniform"]


def test_table_covers_every_class(plans):
    F = [_facts(c, s, add, p) for (c, s, add), p in zip(ROWS, plans)]
    is_ = lambda fam: (lambda f: f["fam"] == fam)  # noqa: E731
    both = lambda *preds: (lambda f: all(p(f) for p in preds))  # noqa: E731
    dma, chk, ctg, std, spc, thr = (is_(x) for x in ("Dma", "LdsContigChunked", "LdsContig", "LdsStrided", "Spec", "Thread"))
    fused3 = lambda f: f["ndim"] == 3 and not f["v1"]  # noqa: E731
    fused4 = lambda f: f["ndim"] == 4 and not f["v1"]  # noqa: E731
    env = lambda k, v=None: (lambda f: k in f["env"] and (v is None or f["env"][k] == v))  # noqa: E731
    classes = {
        "Dma axis 0 add +1": both(dma, lambda f: f["axis"] == 0 and f["add"] == +1),
        "Dma axis 0 add -1": both(dma, lambda f: f["axis"] == 0 and f["add"] == -1),
        "Dma n == 160: no LDS part": both(dma, lambda f: f["n"] == 160),
        "Dma n a little over 160": both(dma, lambda f: 160 < f["n"] <= 256),
        "Dma n over 400": both(dma, lambda f: f["n"] > 400),
        "Dma last tile of ONE pencil": both(dma, lambda f: f["npencil"] % 64 == 1),
        "Dma nbatch > 1, fused 4-D": both(dma, fused4, lambda f: f["nbatch"] > 1),
        "Dma axis 1, fused 3-D, plane not in LDS": both(dma, fused3, lambda f: f["axis"] == 1 and not f["plane_fits"]),
        "Dma axis 1, MGH_FORCE_V1": both(dma, lambda f: f["axis"] == 1 and f["v1"]),
        "Dma axis 1, tiles straddle planes": both(dma, lambda f: f["axis"] == 1 and f["n_inner"] % 64 != 0),
        "Dma axis 1, n_inner < 64": both(dma, lambda f: f["axis"] == 1 and f["n_inner"] < 64),
        "Dma non-uniform": both(dma, lambda f: f["nonuniform"]),
        "Chunked f32": both(chk, lambda f: f["elem"] == 4),
        "Chunked f64": both(chk, lambda f: f["elem"] == 8),
        "Chunked n odd": both(chk, lambda f: f["n"] % 2 == 1 and f["pad"] == 0),
        "Chunked n even (pad 1)": both(chk, lambda f: f["n"] % 2 == 0 and f["pad"] == 1),
        "Chunked partial last tile": both(chk, lambda f: f["last"] < f["width"]),
        "Chunked K from the tables, f32": both(chk, lambda f: f["elem"] == 4 and f["K"] == NEED["f32"] and "MGH_IPK_CHUNK_K" not in f["env"]),
        "Chunked K from the tables, f64": both(chk, lambda f: f["elem"] == 8 and f["K"] == NEED["f64"] and "MGH_IPK_CHUNK_K" not in f["env"]),
        "Chunked MGH_IPK_CHUNK_K=3, f32": both(chk, env("MGH_IPK_CHUNK_K", "3"), lambda f: f["elem"] == 4 and f["K"] == 3),
        "Chunked MGH_IPK_CHUNK_K=3, f64": both(chk, env("MGH_IPK_CHUNK_K", "3"), lambda f: f["elem"] == 8 and f["K"] == 3),
        "Chunked MGH_FORCE_V1": both(chk, lambda f: f["v1"]),
        "Chunked fused 4-D": both(chk, fused4),
        "Chunked fused 3-D, plane not in LDS": both(chk, fused3, lambda f: not f["plane_fits"]),
        "LdsContig with MGH_IPK_CHUNK=0": both(ctg, env("MGH_IPK_CHUNK", "0"), lambda f: f["n"] >= 64),
        "LdsContig n < 64": both(ctg, lambda f: f["n"] < 64),
        "LdsContig K > n / 2": both(ctg, lambda f: f["n"] >= 64 and NEED["f64" if f["elem"] == 8 else "f32"] > f["n"] // 2
                                    and "MGH_IPK_CHUNK" not in f["env"]),
        "LdsContig n even": both(ctg, lambda f: f["n"] % 2 == 0 and f["pad"] == 1),
        "LdsContig n odd": both(ctg, lambda f: f["n"] % 2 == 1 and f["pad"] == 0),
        "LdsContig partial last tile": both(ctg, lambda f: f["last"] < f["width"]),
        "LdsContig f32": both(ctg, lambda f: f["elem"] == 4),
        "LdsContig f64": both(ctg, lambda f: f["elem"] == 8),
        "LdsStrided axis 0 add +1": both(std, lambda f: f["axis"] == 0 and f["add"] == +1),
        "LdsStrided axis 0 add -1": both(std, lambda f: f["axis"] == 0 and f["add"] == -1),
        "LdsStrided axis 1": both(std, lambda f: f["axis"] == 1),
        "LdsStrided axis 1, W < 64": both(std, lambda f: f["axis"] == 1 and f["W"] < 64),
        "LdsStrided partial last tile": both(std, lambda f: f["last"] < f["width"]),
        "LdsStrided non-uniform": both(std, lambda f: f["nonuniform"]),
        "LdsStrided W 16 with MGH_IPK_SPEC_LONG=0": both(std, env("MGH_IPK_SPEC_LONG", "0"), lambda f: f["W"] == 16 and f["n"] >= 1024),
        "Spec axis 2, npencil <= 64 (1-D array)": both(spc, lambda f: f["axis"] == 2 and f["npencil"] <= 64 and f["ndim"] == 1),
        "Spec strided by the MGH_IPK_SPEC_LONG rule": both(spc, lambda f: f["axis"] != 2 and not f["too_long"] and f["n"] >= 1024),
        "Spec strided pencils too long for LDS": both(spc, lambda f: f["axis"] != 2 and f["too_long"] and f["n"] >= 2048),
        "Spec contiguous pencils too long for LDS": both(spc, lambda f: f["axis"] == 2 and f["too_long"] and f["npencil"] > 64),
        "Spec add +1 (k_ipk_spec_apply)": both(spc, lambda f: f["add"] == +1),
        "Spec add -1 (k_ipk_spec_apply)": both(spc, lambda f: f["add"] == -1),
        "Spec default K, f32": both(spc, lambda f: f["K"] == 64 and f["elem"] == 4),
        "Spec default K, f64": both(spc, lambda f: f["K"] == 128 and f["elem"] == 8),
        "Spec MGH_IPK_SPEC_K=2, contiguous": both(spc, env("MGH_IPK_SPEC_K", "2"), lambda f: f["K"] == 2 and f["axis"] == 2),
        "Spec MGH_IPK_SPEC_K=2, strided": both(spc, env("MGH_IPK_SPEC_K", "2"), lambda f: f["K"] == 2 and f["axis"] != 2),
        "Spec nbatch > 1": both(spc, lambda f: f["nbatch"] > 1),
        "Thread axis 0": both(thr, env("MGH_IPK_SPEC", "0"), lambda f: f["axis"] == 0 and f["too_long"]),
        "Thread axis 1": both(thr, env("MGH_IPK_SPEC", "0"), lambda f: f["axis"] == 1 and f["too_long"]),
        "Thread axis 2": both(thr, env("MGH_IPK_SPEC", "0"), lambda f: f["axis"] == 2 and f["too_long"]),
        "Thread add +1": both(thr, lambda f: f["add"] == +1),
        "Thread add -1": both(thr, lambda f: f["add"] == -1),
        "Thread nbatch > 1 (per_batch), fused 4-D": both(thr, fused4, lambda f: f["nbatch"] > 1 and f["per_batch"]),
    }
    for elem in (4, 8):
        for W in (64, 48, 32, 16):
            classes["LdsStrided W %d, elem %d" % (W, elem)] = both(std, lambda f, e=elem, w=W: f["elem"] == e and f["W"] == w)
    missing = [name for name, pred in classes.items() if not any(pred(f) for f in F)]
    assert not missing, missing
    assert {f["fam"] for f in F} == set(ARGS)
