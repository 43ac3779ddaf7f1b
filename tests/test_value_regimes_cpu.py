"""The construction behind tests/test_gpu_value_regimes.py, proved with the CPU oracle alone.

The finest-level coefficients are computed from the input by interpolation alone, before any
correction is added. With 0 at every node whose indices are all even, the coefficient at a node with
an odd index is the input value there, bit for bit; so a product t * quantizer that sits exactly on a
decision point of the quantizer (a rounding tie, a dictionary edge, -0.0, the neighbours of 2^31) can
be planted through decompose + quantize. Checked here: every planted value is found at the planted
node's place in the reordered layout, enough targets are hit exactly, and the oracle's integers at the
exact hits are the ones the rule (int64) copysign(0.5 + |t|, t) + dict / 2 gives by hand -- which pins
the oracle against the rule itself, not only against the kernels.
"""
import numpy as np
import pytest

import oracle
from tests.util import (planted_field, planted_sites, quantizer_targets, reordered_position, rule_integer,
                        solve_targets)

SHAPES = [(17, 17, 17), (33, 40, 36), (34, 33, 32), (9, 10, 17, 12), (3, 4, 5, 6, 7), (300,), (33, 20)]
TOL = 1e-3
MIN_HITS = 150  # of the 184 (float32) / 192 (float64) targets of one dictionary size; 158 to 184 are hit here


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("dict_size", [64, 8192, 65536])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_planted_values_are_the_finest_coefficients_and_quantize_by_the_rule(shape, dt, dict_size):
    o = oracle.Hierarchy(shape, dt)
    L = o.l_target
    args = (oracle.ABS, dt(TOL), dt(np.inf), dt(1))
    qz = o.quantizers(*args, reciprocal=True)[L]
    assert np.isfinite(qz) and qz > 0
    targets = quantizer_targets(dt, dict_size)
    vals, hit = solve_targets(dt, targets, qz, dt(1))
    assert np.all(_bits(dt(vals * qz))[hit] == _bits(targets)[hit])
    assert int(hit.sum()) >= MIN_HITS, "%d of %d targets hit exactly" % (hit.sum(), len(targets))
    # (300,) has 149 sites: the values go into as many fields as that takes
    cap = len(planted_sites(shape))
    for first in range(0, len(vals), cap):
        sl = slice(first, min(first + cap, len(vals)))
        u, pos = planted_field(shape, dt, vals[sl], seed=len(shape) * 1000 + first)
        c = o.decompose(u)
        # the place of each planted node in the reordered layout: on the finest level by the hierarchy's marks
        at = reordered_position(pos, shape, o.level_shape(L - 1))
        marks = np.stack([o.marks(d)[at[:, d]] for d in range(len(shape))], axis=1)
        assert np.all(marks.max(axis=1) == L)
        idx = tuple(at.T)
        assert np.array_equal(_bits(c[idx]), _bits(vals[sl])), "planted values are not the coefficients there"
        q, oi, ov, n = o.quantize(c, *args, dict_size=dict_size)
        outl = dict(zip(oi.tolist(), ov.tolist()))
        assert len(outl) == n
        lin = np.ravel_multi_index(idx, shape)
        for k in np.flatnonzero(hit[sl]):
            want, out = rule_integer(targets[sl][k], dt, dict_size)
            if out:
                assert q[tuple(at[k])] == 0 and outl.get(int(lin[k])) == want, (targets[sl][k], want)
            else:
                assert q[tuple(at[k])] == want and int(lin[k]) not in outl, (targets[sl][k], want)


def test_the_targets_are_the_decision_points():
    """Ties and dictionary edges of both signs, both zeros, and the saturation boundary are in the list."""
    for dt in (np.float32, np.float64):
        for dict_size in (64, 8192, 65536):
            t = quantizer_targets(dt, dict_size)
            half = dict_size // 2
            have = set(t.astype(np.float64).tolist())
            for x in (0.5, 1.5, 2.5, 39.5, half - 1, half, half - 0.5, half + 0.5, 2147483520.0, 2.0 ** 31, 2.0 ** 40):
                assert x in have and -x in have
            assert np.any((t == 0) & np.signbit(t)) and np.any((t == 0) & ~np.signbit(t))
            assert (rule_integer(dt(half - 1), dt, dict_size), rule_integer(dt(half), dt, dict_size)) == (
                (dict_size - 1, False), (dict_size, True))
            assert (rule_integer(dt(-half), dt, dict_size), rule_integer(dt(-half - 1), dt, dict_size)) == (
                (0, False), (-1, True))
            assert rule_integer(dt(-0.0), dt, dict_size) == (half, False)
    assert rule_integer(np.float64(2.0 ** 53 + 2), np.float64, 64)[0] == 2 ** 53 + 2 + 32  # (0.5 + x rounds back to x)
