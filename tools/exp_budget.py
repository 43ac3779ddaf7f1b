"""Developer tool: what pricing tolerances costs against compressing at them. 512^3 float32 on the device,
REL 1e-3-ish tolerances, s = inf; medians of `reps` runs, in milliseconds:
  (a) mgh_estimate_sizes for K = 1, 4, 12 tolerances (one decomposition + one read of the coefficients per
      launch of four);
  (b) mgh_compress_budget with 4 rounds (14 candidates priced, then mgh_compress);
  (c) K separate mgh_compress calls -- what a caller without the estimates has to do.
Usage: python tools/exp_budget.py [n] [reps]"""
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
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
d = torch.from_numpy(smooth_field((n, n, n), np.float32)).cuda()
INF = float("inf")


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
    a = median_ms(lambda: hl.estimate_sizes(d, tols, INF, mgard_amd.REL))
    c = median_ms(lambda: [hl.compress(d, t, INF, mgard_amd.REL) for t in tols])
    print("K = %2d   (a) estimate_sizes %8.2f ms   (c) K x compress %8.2f ms" % (K, a, c))
budget = d.numel() * 4 // 10
b = median_ms(lambda: hl.compress_budget(d, budget, 1e-7, 1e-1, rounds=4, s=INF, mode=mgard_amd.REL))
buf, tol, est = hl.compress_budget(d, budget, 1e-7, 1e-1, rounds=4, s=INF, mode=mgard_amd.REL)
print("(b) compress_budget, 4 rounds, budget %d bytes: %8.2f ms   -> tol %.3e, %d bytes (%r)" % (budget, b, tol, buf.numel(), est))
