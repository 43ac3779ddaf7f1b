"""k_ipk_stream (mgard_amd/csrc/kernels_ipk_stream.hpp) on small arrays. The planner takes this
kernel for arrays of tens of megabytes only; MGH_IPK_PLAN_CU makes it plan for a device of one or
two CUs, and the cases of tests/ipk_stream_cases.py then reach every path of the kernel (register /
LDS / global parking, tile widths, partial and empty tiles, remainders, the wave-cooperative
contiguous loads, AddND / SubtractND, batches of boxes) on boxes of a few hundred thousand elements.
The library's plan log (Hierarchy.ipk_plans, filled while profiling is on) must show the solves of
the table with the table's plan -- a case that no longer reaches the kernel fails -- and everything
computed is compared bit by bit with the CPU oracle.

Second part: the r-plane ranges of the f- and c-solve (MGH_IPK_RANGE_MB), which the default of
128 MB leaves to 1024^3."""
import numpy as np
import pytest

import oracle
from tests.ipk_stream_cases import CASES, RANGE_CASES
from tests.test_gpu_parity import _outlier_set, assert_bit_equal
from tests.util import nonuniform_coords, smooth_field

pytestmark = pytest.mark.gpu

DT = {"f32": np.float32, "f64": np.float64}
TOL, DICT = 1e-3, 512
_REF = {}


def _gpu():
    import torch
    import mgard_amd
    return torch, mgard_amd


def _reference(c):
    """Input and the oracle's results for a case: computed once per array, shared by the cases (and
    tests) on the same array, never written to."""
    key = (c["shape"], c["dtype"], c["nonuniform"])
    if key not in _REF:
        dt = DT[c["dtype"]]
        coords = nonuniform_coords(c["shape"], dt, seed=sum(c["shape"])) if c["nonuniform"] else None
        u = smooth_field(c["shape"], dt, seed=sum(c["shape"]), noise=3e-3)
        o = oracle.Hierarchy(c["shape"], dt, coords=coords)
        coef = o.decompose(u)
        nrm = float(oracle.norm(u, dt(np.inf)))
        rq, roi, rov, rn = o.quantize(coef, oracle.REL, dt(TOL), dt(np.inf), dt(nrm), dict_size=DICT, outlier_cap=u.size)
        rback = o.recompose(o.dequantize(rq, oracle.REL, dt(TOL), dt(np.inf), dt(nrm), dict_size=DICT,
                                         outlier_idx=roi, outlier_val=rov))
        assert 0 < rn < u.size  # (the dictionary leaves outliers, and not only outliers)
        r = dict(u=u, coords=coords, coef=coef, back=o.recompose(coef), nrm=nrm, rq=rq, rn=rn, routl=_outlier_set(roi, rov),
                 rback=rback)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _find(log, s, add):
    """Records of the log for the solve s of the table with this `add`."""
    return [r for r in log if (r["elem"], r["axis"], r["m"], r["nbatch"], r["add"]) ==
            (s["elem"], s["axis"], s["m"], s["nbatch"], add) and (s["nbatch"] == 1 or r["batch_stride"] == s["batch_stride"])]


def _assert_planned_as_in_the_table(log, solves, what):
    assert len(log) < 512, "the plan log is full: records may be missing"
    for s in solves:
        for add in s["add"]:
            recs = _find(log, s, add)
            assert recs, "%s: no solve elem %d axis %d m %r add %d in the plan log" % (what, s["elem"], s["axis"], s["m"], add)
            if s["W"] is None:
                continue
            for r in recs:
                assert (r["family"], r["W"], r["n_glob"], r["KR"]) == ("Stream", s["W"], s["n_glob"], s["KR"]), (what, r)
                assert r["n"] == s["m"][s["axis"]]


def _assert_oracle_bits(torch, mg, h, ref, what):
    """decompose / recompose out of place and in place, decompose_quantize / dequantize_recompose:
    the oracle's bits, integers and outlier set."""
    ud = torch.tensor(ref["u"], device="cuda")
    c = h.decompose(ud)
    assert_bit_equal(c.cpu().numpy(), ref["coef"], what + ": decompose")
    back = h.recompose(c)
    assert_bit_equal(back.cpu().numpy(), ref["back"], what + ": recompose")
    w = ud.clone()
    h.decompose(w, out=w)
    assert_bit_equal(w.cpu().numpy(), ref["coef"], what + ": decompose in place")
    h.recompose(w, out=w)
    assert_bit_equal(w.cpu().numpy(), ref["back"], what + ": recompose in place")
    q, oi, ov, cnt, _ = h.decompose_quantize(ud, mg.REL, TOL, np.inf, norm=ref["nrm"], dict_size=DICT,
                                             outlier_cap=ref["u"].size)
    assert cnt == ref["rn"]
    assert np.array_equal(q.cpu().numpy(), ref["rq"]), what + ": quantized integers"
    gi, gv = _outlier_set(oi.cpu().numpy(), ov.cpu().numpy())
    assert np.array_equal(gi, ref["routl"][0]) and np.array_equal(gv, ref["routl"][1]), what + ": outlier set"
    rec = h.dequantize_recompose(q, mg.REL, TOL, np.inf, ref["nrm"], dict_size=DICT, outlier_idx=oi, outlier_val=ov)
    assert_bit_equal(rec.cpu().numpy(), ref["rback"], what + ": dequantize_recompose")
    return c, back


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_streaming_solves_on_small_shapes(c, monkeypatch):
    torch, mg = _gpu()
    ref = _reference(c)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    h = mg.Hierarchy(c["shape"], DT[c["dtype"]], coords=ref["coords"])
    assert h.ipk_plans() == []  # (nothing is recorded before profiling is on)
    h.decompose(torch.tensor(ref["u"], device="cuda"))
    assert h.ipk_plans() == []
    h.profile(True)
    coef, back = _assert_oracle_bits(torch, mg, h, ref, c["id"])
    _assert_planned_as_in_the_table(h.ipk_plans(), c["solves"], c["id"])
    assert h.ipk_plans() == []  # (reading resets)
    h.close()
    # the switch changes the plan, never the result
    monkeypatch.delenv("MGH_IPK_PLAN_CU")
    g = mg.Hierarchy(c["shape"], DT[c["dtype"]], coords=ref["coords"])
    g.profile(True)
    c2 = g.decompose(torch.tensor(ref["u"], device="cuda"))
    assert torch.equal(c2.view(torch.uint8), coef.view(torch.uint8))
    assert torch.equal(g.recompose(c2).view(torch.uint8), back.view(torch.uint8))
    # (and on the device's own CU count no solve of these small boxes is a streaming one)
    assert not any(r["family"] == "Stream" for s in c["solves"] for add in s["add"] for r in _find(g.ipk_plans(), s, add))
    g.close()


@pytest.mark.parametrize("c", RANGE_CASES, ids=[c["id"] for c in RANGE_CASES])
def test_f_and_c_solves_in_ranges_of_r_planes(c, monkeypatch):
    """MGH_IPK_RANGE_MB=1 on coarse boxes of a little over 2 MB: the f- and c-solve of the top level
    of decompose / decompose_quantize run range by range (planes per range: c["ranges"], unequal where
    the planes do not divide; an empty range is skipped). Where the planes of the box fit in LDS a
    range is ONE launch of the plane kernel, "ipk_fc" in the profile: its launches are counted against
    a hierarchy with the ranges off. Else the plan log shows the f- and the c-solve of every sub-box,
    alternating, and none of the whole box."""
    torch, mg = _gpu()
    ref = _reference(c)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    h = mg.Hierarchy(c["shape"], DT[c["dtype"]], coords=ref["coords"])
    h.profile(True)
    ud = torch.tensor(ref["u"], device="cuda")
    coef = h.decompose(ud)
    log, prof = h.ipk_plans(), h.profile_read()
    assert_bit_equal(coef.cpu().numpy(), ref["coef"], c["id"] + ": decompose")
    m = c["coarse"]
    live = [k for k in c["ranges"] if k > 0]
    if c["plane_in_lds"]:
        assert not [r for r in log if r["axis"] != 0 and r["m"][1:] == m[1:]]
    else:
        top = [(r["axis"], r["m"][0]) for r in log if r["axis"] != 0 and r["m"][1:] == m[1:]]
        assert top == [(axis, k) for k in live for axis in (2, 1)]
        _assert_planned_as_in_the_table([r for r in log if r["axis"] != 0], c["solves"], c["id"])
    _assert_oracle_bits(torch, mg, h, ref, c["id"])
    h.close()
    monkeypatch.setenv("MGH_IPK_RANGE_MB", "0")
    g = mg.Hierarchy(c["shape"], DT[c["dtype"]], coords=ref["coords"])
    g.profile(True)
    c0 = g.decompose(ud)
    log0, prof0 = g.ipk_plans(), g.profile_read()
    assert torch.equal(c0.view(torch.uint8), coef.view(torch.uint8))
    if c["plane_in_lds"]:
        assert prof["ipk_fc"][1] - prof0["ipk_fc"][1] == len(live) - 1
    else:
        assert [(r["axis"], r["m"]) for r in log0 if r["axis"] != 0 and r["m"][1:] == m[1:]] == [(2, m), (1, m)]
    g.close()
