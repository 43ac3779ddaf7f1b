"""Timing of the progressive reader against starting over ("Refining level by level").

    python tools/exp_progressive.py [N] [reps]      # N^3 f32, reorder = 1, tol 1e-3 REL, device container

Prints, per level l, the median over `reps` of: the refine step l - 1 -> l, decompress(level = l) from
scratch, and at the end the whole walk 0 -> l_target and decompress(). HIP events on the default stream; the
first repetition (allocations, lazy state) is dropped."""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgard_amd as mg  # noqa: E402
from mgard_amd import highlevel as hl  # noqa: E402
from tests.util import smooth_field  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    u = torch.from_numpy(smooth_field((n, n, n), np.float32)).cuda()
    cfg = hl.Config(reorder=1)
    buf = hl.compress(u, 1e-3, np.inf, mg.REL, config=cfg)
    L = hl.infer_level(buf, None, cfg)[1]
    outs = [torch.empty(hl.infer_level(buf, l, cfg)[0], dtype=torch.float32, device="cuda") for l in range(L + 1)]
    step = [[] for _ in range(L + 1)]
    scratch = [[] for _ in range(L + 1)]
    walk, full = [], []
    for r in range(reps + 1):
        with hl.Progressive(buf, cfg) as p:
            ts = [timed(lambda l=l: p.refine(l, out=outs[l])) for l in range(L + 1)]
        fs = [timed(lambda l=l: hl.decompress(buf, config=cfg, level=l, out=outs[l])) for l in range(L + 1)]
        f = timed(lambda: hl.decompress(buf, config=cfg, out=outs[L]))
        if r == 0:
            continue
        for l in range(L + 1):
            step[l].append(ts[l])
            scratch[l].append(fs[l])
        walk.append(sum(ts))
        full.append(f)
    med = statistics.median
    print("%d^3 f32, container %d bytes, l_target %d, %d repetitions (ms, medians)" % (n, buf.numel(), L, reps))
    for l in range(L + 1):
        print("level %2d: refine step %8.3f   decompress(level) from scratch %8.3f" % (l, med(step[l]), med(scratch[l])))
    print("(a) step l_target-1 -> l_target %.3f  (b) whole walk %.3f  (c) decompress(level=l_target-1) %.3f  "
          "decompress() %.3f" % (med(step[L]), med(walk), med(scratch[L - 1]), med(full)))


if __name__ == "__main__":
    main()
