"""mgh_verify on the GPU (mgard_amd.highlevel.verify): the error statistics of the original against a
container's reconstruction, subdomain by subdomain, without the reconstruction ever being an array.

verify(buf, x).stats must be compare(x, decompress(buf)) (tests/test_gpu_compare.py holds compare to NumPy) in
counters, extremes and argmax (the index in the WHOLE array), exactly. The two sums are held against the
NumPy statistics of the same two arrays (compare_ref.ref_stats: math.fsum), within compare_ref.sum_tolerance
-- n 2^-52, the bound of the sums everywhere -- and so against nothing the library computed. Containers: one subdomain (33 x 17 x 65, f32 and f64, REL 1e-3, s = inf) and
the decomposed cases of tests/test_gpu_coarsened.py (MaxDim, Block, Variable; 3-D and 4-D, uniform and not),
reorder 0 and 1, container and original each on the host and on the device."""
import re

import numpy as np
import pytest

from tests.compare_ref import EXACT, SUMS, bits, ref_stats, sum_tolerance
from tests.test_gpu_coarsened import CASES as DD_CASES, _cfg as dd_cfg
from tests.util import nonuniform_coords, smooth_field

pytestmark = pytest.mark.gpu

TOL = 1e-3
# (the small ones do not shrink at this tolerance and are stored raw, error 0; the large one is the shape whose halves
# tests/test_gpu_coarsened.py knows to be Huffman records, so it reconstructs with an error)
ONE = {"one-f32": ((33, 17, 65), np.float32), "one-f64": ((33, 17, 65), np.float64),
       "one-f32-large": ((129, 64, 65), np.float32)}
NAMES = list(ONE) + list(DD_CASES)


class Case:
    """Data, coordinates and configuration of a container: made once per name and reorder."""

    def __init__(self, name, reorder):
        import mgard_amd as mg
        from mgard_amd import highlevel as hl
        if name in ONE:
            self.shape, self.dt = ONE[name]
            self.coords, self.s, self.rel = None, np.inf, True
            self.cfg = hl.Config(reorder=reorder)
            self.subdomains = 1
        else:
            self.shape, self.dt, nonuniform, _, _, _, _, self.rel, self.s = DD_CASES[name]
            self.coords = nonuniform_coords(self.shape, self.dt, seed=sum(self.shape)) if nonuniform else None
            self.cfg = dd_cfg(name, reorder=reorder)
            self.subdomains = 2
        self.x = smooth_field(self.shape, self.dt)
        self.buf = hl.compress(self.x, TOL, self.s, mg.REL if self.rel else mg.ABS, coords=self.coords, config=self.cfg)
        self.meta = hl.metadata_parse(bytes(self.buf[:65536]))
        assert self.meta["domain_decomposed"] == (name not in ONE)
        self.dec = hl.decompress(self.buf, config=self.cfg)
        self.ref = ref_stats(self.x, self.dec)


_CASES = {}


def case(name, reorder):
    if (name, reorder) not in _CASES:
        _CASES[(name, reorder)] = Case(name, reorder)
    return _CASES[(name, reorder)]


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def assert_same(got, want, ref, what):
    """got: ErrorStats of verify; want: ErrorStats of compare on the same two arrays, for the exact fields;
    ref: their NumPy statistics, for the sums."""
    for k in EXACT:
        assert bits(getattr(got, k)) == bits(getattr(want, k)), "%s %s: %r / %r" % (what, k, getattr(got, k), getattr(want, k))
        assert bits(getattr(got, k)) == bits(ref[k]), "%s %s: %r / %r" % (what, k, getattr(got, k), ref[k])
    for k in SUMS:
        g, w = getattr(got, k), ref[k]
        assert abs(g - w) <= sum_tolerance(ref["n"]) * w, "%s %s: %r / %r" % (what, k, g, w)


@pytest.mark.parametrize("reorder", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_verify_equals_compare_of_the_decompressed_array(name, reorder):
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    c = case(name, reorder)
    want = mg.compare(c.x, c.dec)
    n = c.x.size
    assert want.n == n and want.nonfinite == 0
    if name == "one-f32-large" or name.startswith("maxdim0"):
        assert want.max_abs_err > 0  # (lossy records: the comparison is not one of equal arrays)
    for buf_dev in (False, True):
        for x_dev in (False, True):
            what = "%s reorder %d, container on %s, original on %s" % (name, reorder, "device" if buf_dev else "host",
                                                                      "device" if x_dev else "host")
            r = hl.verify(dev(c.buf) if buf_dev else c.buf, dev(c.x) if x_dev else c.x, config=c.cfg)
            print(what, r)
            assert_same(r.stats, want, c.ref, what)
            assert r.bound == TOL * c.meta["norm"]
            if np.isinf(c.s):
                # (the round-trip tests hold these containers to the bound: the compressor alone satisfies it)
                assert r.bound_kind == 0 and r.achieved == r.stats.max_abs_err and r.within == 1, what
            else:
                assert c.s == 0 and r.bound_kind == 1
                l2 = np.sqrt(c.ref["sum_sq_err"] / n)  # (normalize_coordinates is on)
                assert abs(r.achieved - l2) <= sum_tolerance(n) * l2, (what, r.achieved, l2)
                assert r.within == int(r.achieved <= r.bound), what


def test_a_bound_in_an_s_norm_is_not_evaluated():
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    x = smooth_field((33, 17, 65), np.float32)
    buf = hl.compress(x, TOL, 1.0, mg.REL)
    r = hl.verify(buf, x)
    assert r.bound_kind == -1 and r.within == -1
    dec = hl.decompress(buf)
    assert_same(r.stats, mg.compare(x, dec), ref_stats(x, dec), "s = 1")
    # (stats is filled whatever the bound is in; the error itself may be 0: a record that does not shrink is stored raw)
    assert r.stats.n == x.size and r.stats.ref_abs_max == float(np.abs(x).max()) and r.achieved == 0


@pytest.mark.parametrize("name", ["one-f64", "one-f32-large", "maxdim0", "block", "variable-f64-nonuniform", "variable-4d"])
def test_a_corrupted_element_is_found(name):
    """4 x bound added to one element of the original (in a subdomain that is not the first, where there is
    more than one): the bound is missed, and the element is where the largest error is."""
    from mgard_amd import highlevel as hl
    c = case(name, 1)
    pos = tuple(e - 2 for e in c.shape)
    bound = TOL * c.meta["norm"]
    x = c.x.copy()
    x[pos] = x[pos] + c.dt(4 * bound)
    for x_dev in (False, True):
        r = hl.verify(c.buf, dev(x) if x_dev else x, config=c.cfg)
        assert r.within == 0 and r.bound == bound
        assert r.stats.argmax == int(np.ravel_multi_index(pos, c.shape))
        assert bits(r.stats.max_abs_err) == bits(float(np.abs(x[pos] - c.dec[pos])))  # (the difference in T)
        assert r.achieved == r.stats.max_abs_err > 2 * bound
    # ... and a NaN in the original misses the bound whatever the rest does
    x = c.x.copy()
    x[pos] = np.nan
    r = hl.verify(c.buf, x, config=c.cfg)
    assert r.stats.nonfinite == 1 and r.within == 0 and r.stats.max_abs_err <= bound


def _status(exc):
    return int(re.search(r"error (-?\d+)", str(exc.value)).group(1))


@pytest.mark.parametrize("name", ["one-f32", "one-f32-large", "block", "variable-f64-nonuniform"])
def test_verify_of_a_preview(name):
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    c = case(name, 1)
    pre = hl.decompress_preview(c.buf, 1, config=c.cfg)
    want, ref = mg.compare(c.x, pre), ref_stats(c.x, pre)
    for x_dev in (False, True):
        r = hl.verify(c.buf, dev(c.x) if x_dev else c.x, config=c.cfg, coarsen=1)
        assert r.within == -1
        assert_same(r.stats, want, ref, name)
    assert r.stats.max_abs_err > hl.verify(c.buf, c.x, config=c.cfg).stats.max_abs_err
    _, K = hl.infer_coarsened(c.buf, None, c.cfg)
    with pytest.raises(hl.MgardHipError) as preview:
        hl.decompress_preview(c.buf, K + 1, config=c.cfg)
    with pytest.raises(hl.MgardHipError) as verify:
        hl.verify(c.buf, c.x, config=c.cfg, coarsen=K + 1)
    assert _status(verify) == _status(preview) == -1
    assert hl.verify(c.buf, c.x, config=c.cfg, coarsen=K).within == -1


def test_wrong_size_or_type_of_the_original_is_refused_before_any_work():
    from mgard_amd import highlevel as hl
    c = case("one-f32", 0)
    for bad in (c.x[:-1], c.x.astype(np.float64), dev(c.x)[:, :-1]):
        with pytest.raises(hl.MgardHipError) as e:
            hl.verify(c.buf, bad, config=c.cfg)
        assert _status(e) == -1 and "mgh_verify" in str(e.value)
        assert hl.last_decompress_stats()["subdomains"] == 0  # (nothing was opened)
    assert hl.verify(c.buf, c.x, config=c.cfg).within == 1
