"""Developer tool: what measuring the achieved error of tolerances costs against compressing and verifying at
them. 512^3 float32 on the device, REL, s = inf; medians of `reps` runs, in milliseconds:
  (a) mgh_achieved_errors for K = 1, 4, 12 tolerances (one decomposition; per tolerance one streaming pass, one
      recomposition, one comparison);
  (b) mgh_compress_target with 8 rounds (10 candidates evaluated, then mgh_compress);
  (c) the loop a caller writes without it: mgh_compress + mgh_verify per candidate, at (b)'s candidates.
Usage: python tools/exp_target.py [n] [reps]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgard_amd  # noqa: E402
from mgard_amd import highlevel as hl  # noqa: E402
from tests.util import smooth_field  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
d = torch.from_numpy(smooth_field((n, n, n), np.float32)).cuda()
INF = float("inf")
REL = mgard_amd.REL


def median_ms(fn):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


for K in (1, 4, 12):
    tols = [float(t) for t in np.logspace(-5, -2, K)] if K > 1 else [1e-3]
    a = median_ms(lambda: hl.achieved_errors(d, tols, INF, REL))
    print("K = %2d   (a) achieved_errors %8.2f ms" % (K, a))
    if K == 12:
        st = hl.achieved_errors(d, tols, INF, REL)
        norm = st[0].ref_abs_max
        print("        bound / achieved max error: " + " ".join("%.1f" % (t * norm / max(s.max_abs_err, 1e-300)) for t, s in zip(tols, st)))

TOL_MIN, TOL_MAX, ROUNDS = 1e-6, 1e-1, 8
target = 1e-3 * float(d.abs().max())  # max error: a thousandth of the range's half


def caller_loop():
    """The same walk with what exists without the call: compress + verify per candidate."""
    def meets(tol):
        buf = hl.compress(d, float(tol), INF, REL)
        return hl.verify(buf, d).stats.max_abs_err <= target, buf
    ok, buf = meets(TOL_MAX)
    if ok:
        return buf, TOL_MAX
    ok, buf = meets(TOL_MIN)
    assert ok
    a, b = np.float64(TOL_MIN), np.float64(TOL_MAX)
    for _ in range(ROUNDS):
        m = np.sqrt(a) * np.sqrt(b)
        ok, cand = meets(m)
        if ok:
            a, buf = m, cand
        else:
            b = m
    return buf, float(a)


b = median_ms(lambda: hl.compress_target(d, hl.TARGET_MAX_ABS, target, TOL_MIN, TOL_MAX, rounds=ROUNDS, s=INF, mode=REL))
buf, tol, stats, cand = hl.compress_target(d, hl.TARGET_MAX_ABS, target, TOL_MIN, TOL_MAX, rounds=ROUNDS, s=INF, mode=REL)
c = median_ms(caller_loop)
buf_c, tol_c = caller_loop()
print("(b) compress_target, %d rounds, max error <= %.3e: %8.2f ms   -> tol %.3e, %d candidates, %d bytes, achieved %.3e"
      % (ROUNDS, target, b, tol, cand, buf.numel(), stats.max_abs_err))
print("(c) compress + verify per candidate:              %8.2f ms   -> tol %.3e, %d bytes%s"
      % (c, tol_c, buf_c.numel(), "" if tol_c == tol else "   (ANOTHER tolerance than (b))"))
plain = hl.compress(d, target / float(d.abs().max()), INF, REL)
print("    passing the target as the tolerance instead: %d bytes (%.2f x the container of (b))" % (plain.numel(), plain.numel() / buf.numel()))
