"""The march length of the fused level passes (mgard_amd/csrc/fused_plan.hpp) changes the launch,
never the result. Small arrays with everything a march length can break: 65 x 41 x 37 and 33^3
(2^k + 1 along r: the last r-chunk owns one plane more), 130 x 67 x 35 (non-dyadic, coarse boxes
66 x 34 x 18 and 34 x 18 x 10: face tiles on both axes, a last chunk with and without the extra plane) and the 4-D
20 x 40 x 40 x 40 (even and odd slices in one plan).

MGH_BOX=0 sends every level to the marching kernel (these boxes are all of the smallest class,
which the box kernel runs by default). Marches of 1, 2, 3, 5, 7, 12, 16 forced through MGH_RCH,
and the planner's own choice for a device of MGH_FUSED_SLOTS = 8, 64, 768 resident workgroups:
quantized integers and the outlier set are the CPU oracle's in every setting (so equal between
the settings), dequantize + recompose comes back within the tolerance, and the plan log
(Hierarchy.fused_plans, filled while profiling is on) shows the march that ran."""
import numpy as np
import pytest

import oracle
from tests.test_gpu_parity import _outlier_set
from tests.util import smooth_field

pytestmark = pytest.mark.gpu

SHAPES = [(65, 41, 37), (33, 33, 33), (130, 67, 35), (20, 40, 40, 40)]
FORCED = [1, 2, 3, 5, 7, 12, 16]
SLOTS = [8, 64, 768]
TOL, DICT = 1e-3, 512
MAX_MARCH = 16
_REF = {}


def _reference(shape):
    """Input and the oracle's results, computed once per shape and never written to."""
    if shape not in _REF:
        dt = np.float32
        u = smooth_field(shape, dt, seed=sum(shape), noise=3e-3)
        o = oracle.Hierarchy(shape, dt)
        nrm = float(oracle.norm(u, dt(np.inf)))
        rq, roi, rov, rn = o.quantize(o.decompose(u), oracle.REL, dt(TOL), dt(np.inf), dt(nrm), dict_size=DICT,
                                      outlier_cap=u.size)
        assert 0 < rn < u.size  # (the dictionary leaves outliers, and not only outliers)
        r = dict(u=u, nrm=nrm, rq=rq, rn=rn, routl=_outlier_set(roi, rov))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[shape] = r
    return _REF[shape]


def _nchunk(m_r, rch):
    return max(1, (m_r - 1 + rch - 1) // rch)


def _run(shape, monkeypatch, env):
    import torch
    import mgard_amd as mg
    ref = _reference(shape)
    monkeypatch.setenv("MGH_BOX", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h = mg.Hierarchy(shape, np.float32)
    h.profile(True)
    ud = torch.tensor(ref["u"], device="cuda")
    q, oi, ov, cnt, _ = h.decompose_quantize(ud, mg.REL, TOL, np.inf, norm=ref["nrm"], dict_size=DICT,
                                             outlier_cap=ref["u"].size)
    plans = h.fused_plans()
    what = "%r %r" % (shape, env)
    assert cnt == ref["rn"], what
    assert np.array_equal(q.cpu().numpy(), ref["rq"]), what + ": quantized integers"
    gi, gv = _outlier_set(oi.cpu().numpy(), ov.cpu().numpy())
    assert np.array_equal(gi, ref["routl"][0]) and np.array_equal(gv, ref["routl"][1]), what + ": outlier set"
    back = h.dequantize_recompose(q, mg.REL, TOL, np.inf, ref["nrm"], dict_size=DICT, outlier_idx=oi, outlier_val=ov)
    err = float(np.max(np.abs(back.cpu().numpy().astype(np.float64) - ref["u"])))
    assert err <= TOL * ref["nrm"], (what, err)
    h.close()
    # the log: at least the top level marched, 4-D levels as an even and an odd launch of one plan
    assert plans and len(plans) < 512, what
    top = tuple(n // 2 + 1 for n in shape[-3:])
    assert plans[0]["m"] == top and plans[0]["elem"] == 4, (what, plans[0])
    for p in plans:
        assert 1 <= p["rch"] <= MAX_MARCH and p["nchunk"] == _nchunk(p["m"][0], p["rch"]), (what, p)
        nz = (p["nz0"], p["nz1"])
        assert (nz[1] > 0) == (len(shape) == 4) and nz[0] >= 1, (what, p)
        assert p["workgroups0"] == p["grid_x"] * p["nchunk"] * nz[0], (what, p)
        assert p["workgroups1"] == p["grid_x"] * p["nchunk"] * nz[1], (what, p)
    return plans


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("rch", FORCED)
def test_forced_march(shape, rch, monkeypatch):
    plans = _run(shape, monkeypatch, {"MGH_RCH": "%d,%d,%d" % (rch, rch, rch)})
    for p in plans:
        assert (p["rch"], p["by_policy"]) == (rch, 0), p
    if shape == (130, 67, 35):  # coarse planes 66, 34: the extra plane only where rch divides m_r - 1
        assert [p["m"][0] for p in plans[:2]] == [66, 34]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("slots", SLOTS)
def test_planned_march(shape, slots, monkeypatch):
    plans = _run(shape, monkeypatch, {"MGH_FUSED_SLOTS": str(slots)})
    for p in plans:
        assert p["cls"] == 0 and p["slots"] == slots, p
        assert p["rounds"] == max(-(-p["workgroups0"] // slots), -(-p["workgroups1"] // slots)), p
        # (a plan of more than two rounds is not the policy's: the class constant, 1, marches)
        assert p["by_policy"] == 1 and p["rounds"] <= 2 or (p["by_policy"], p["rch"]) == (0, 1), p
    # a device that holds every workgroup of the shortest march at once runs marches of 1
    for p in plans:
        if p["grid_x"] * _nchunk(p["m"][0], 1) * max(p["nz0"], p["nz1"]) <= slots:
            assert p["rch"] == 1, p
