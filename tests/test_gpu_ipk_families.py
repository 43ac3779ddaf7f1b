"""The Thomas-solve kernels beside k_ipk_stream -- k_ipk_dma, k_ipk_lds_contig (chunked and not),
k_ipk_lds_strided<W>, k_ipk_spec_* and k_ipk -- on the small arrays of tests/ipk_family_cases.py.
Which kernel a solve gets depends on the planner, the developer switches and the route, so per case
the library's plan log (Hierarchy.ipk_plans, filled while profiling is on) must show every solve of
the table with the table's family and arguments -- a case that no longer reaches its kernel fails --
and everything computed is compared bit by bit with the CPU oracle. The logged K of an
LdsContigChunked solve without MGH_IPK_CHUNK_K is the warm-up length of the hierarchy's own tables:
the table's `chunk_need`, which the CPU test plans with, is confirmed here.

The verified-chunk solves (Spec) count the chunks they had to repair (Hierarchy.spec_repairs): with
MGH_IPK_SPEC_K=2 the repair must have run; the count is bounded by the chunks of the logged solves."""
import pytest

from tests.ipk_family_cases import CASES
from tests.test_gpu_ipk_stream import DT, _assert_oracle_bits, _find, _gpu, _reference

pytestmark = pytest.mark.gpu

ARGS = ("W", "P", "K", "KR")


def _records(log, s, add):
    """Records of the log for the solve s of the table: of the launch, or (a Thread plan with batches
    runs its boxes one call each) of its boxes."""
    if s["per_batch"]:
        return _find(log, dict(s, nbatch=1), add)
    return _find(log, s, add)


def assert_planned_as_in_the_table(log, solves, what):
    """-> {family: solves of the table found in the log}"""
    assert len(log) < 512, "the plan log is full: records may be missing"
    found = {}
    for s in solves:
        for add in s["add"]:
            recs = _records(log, s, add)
            assert recs, "%s: no solve elem %d axis %d m %r add %d in the plan log" % (what, s["elem"], s["axis"], s["m"], add)
            assert not s["per_batch"] or len(recs) % s["nbatch"] == 0
            for r in recs:
                assert (r["family"],) + tuple(r[a] for a in ARGS) == (s["family"],) + tuple(s[a] for a in ARGS), (what, r)
                assert r["n"] == s["m"][s["axis"]] and r["n_glob"] == 0
            found[s["family"]] = found.get(s["family"], 0) + 1
    return found


def spec_chunks(log):
    """Most repairs the Spec solves of a log can count: every chunk of every pencil in both sweeps
    (ipk_plan.hpp: chunks of S = 128 for pencils of fewer than 2^21 + 2^14 elements)."""
    total = 0
    for r in log:
        if r["family"] == "Spec":
            assert r["n"] < 129 * 16384
            total += 2 * r["npencil"] * -(-r["n"] // 128)
    return total


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_solves_of_every_family_on_small_shapes(c, monkeypatch):
    torch, mg = _gpu()
    ref = _reference(c)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    h = mg.Hierarchy(c["shape"], DT[c["dtype"]], coords=ref["coords"])
    assert h.spec_repairs() == 0  # (no solve so far: nothing allocated, nothing counted)
    h.profile(True)
    _assert_oracle_bits(torch, mg, h, ref, c["id"])
    log = h.ipk_plans()
    found = assert_planned_as_in_the_table(log, c["solves"], c["id"])
    print("%s: table solves in the plan log: %r" % (c["id"], found))
    for s in c["solves"]:
        if s["family"] == "LdsContigChunked" and "MGH_IPK_CHUNK_K" not in c["env"]:
            assert s["K"] == c["chunk_need"]  # (so the log has just confirmed chunk_need)
    repairs, most = h.spec_repairs(), spec_chunks(log)
    assert h.spec_repairs() == 0  # (reading resets)
    if any(s["family"] == "Spec" for s in c["solves"]):
        print("%s: %d chunks repaired of at most %d" % (c["id"], repairs, most))
        assert most > 0
    assert 0 <= repairs <= most
    if c["env"].get("MGH_IPK_SPEC_K") == "2":
        assert repairs > 0, "a warm-up of 2 elements and no chunk repaired"
    if not any(r["family"] == "Spec" for r in log):
        assert repairs == 0
    h.close()
