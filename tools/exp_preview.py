#!/usr/bin/env python3
"""Cost of the full-grid preview ("Full-grid preview").

512^3 f32, REL 1e-3, a reorder = 1 container resident on the device, outputs pre-allocated on the device.
Every figure is the median of HIP-event timings over `--calls` calls after `--warmup` calls:

  (a) the top-level prolong3 launch alone: Hierarchy.prolong(level l_target - 1 -> l_target)
  (b) mgh_decompress_preview for k = 1, 2, 3
  (c) mgh_decompress_coarsened for the same k
  (d) mgh_decompress
  (e) a plain device fill of the output's bytes: the floor of a pass that must write N * esz

(c), (d) and (e) are the yardsticks; the structural expectation is (b) ~ (c) + (a), well below (d).
Prints one line per figure and a JSON line at the end; sets no threshold.

    python tools/exp_preview.py [--n 512] [--calls 10] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, calls, warmup):
    """Median, min and max in ms of `calls` calls of fn() between two HIP events, after `warmup` calls."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=512, help="edge of the cube")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    from tests.util import smooth_field

    shape = (args.n,) * 3
    u = torch.from_numpy(smooth_field(shape, np.float32)).cuda()
    cfg = hl.Config(reorder=1)
    buf = hl.compress(u, 1e-3, np.inf, mg.REL, config=cfg)
    assert isinstance(buf, torch.Tensor) and buf.is_cuda
    _, K = hl.infer_coarsened(buf, None, cfg)
    full = torch.empty(shape, dtype=torch.float32, device="cuda")
    res = {"shape": list(shape), "dtype": "float32", "container_bytes": int(buf.numel()),
           "device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup}

    def report(key, what, t):
        res[key] = {"median_ms": t[0], "min_ms": t[1], "max_ms": t[2]}
        print("%-28s %-58s median %8.3f ms  (min %.3f, max %.3f)" % (key, what, t[0], t[1], t[2]), flush=True)

    # (e) first: the floor
    report("e_fill", "device fill of %d bytes" % (full.numel() * 4), timed(lambda: full.fill_(1.0), args.calls, args.warmup))

    # (a) the top-level launch alone
    h = mg.Hierarchy(shape, np.float32)
    L = h.l_target
    lvl = torch.rand(h.level_shape(L - 1), dtype=torch.float32, device="cuda")
    print("prolong plan of the top level: %r" % (h.prolong_plan(L),))
    report("a_prolong3_top", "Hierarchy.prolong(level %d -> %d): one prolong3 launch" % (L - 1, L),
           timed(lambda: h.prolong(lvl, L - 1, out=full), args.calls, args.warmup))
    # ... and the kernel on this shape (it marches in the longest chunks, which the small shapes of the tests do
    # not reach) against the library's own full recomposition: random coefficients in the corner box of level
    # l_target - 1, zeros outside; the level by mgh_recompose_to_level, prolonged, against mgh_recompose
    z = torch.zeros(shape, dtype=torch.float32, device="cuda")
    box = tuple(slice(0, m) for m in h.level_shape(L - 1))
    z[box] = torch.rand(h.level_shape(L - 1), dtype=torch.float32, device="cuda")
    got = h.prolong(h.recompose(z, level=L - 1), L - 1)
    same = bool(torch.equal(h.recompose(z).view(torch.int32), got.view(torch.int32)))
    print("top-level launch bit-equal to Hierarchy.recompose of the zeroed array: %r" % same)
    res["a_checked_against_recompose"] = same
    del got
    del z
    h.close()

    # (d) the whole decode
    report("d_decompress", "mgh_decompress", timed(lambda: hl.decompress(buf, config=cfg, out=full), args.calls, args.warmup))

    for k in range(1, min(3, K) + 1):
        cshape, _ = hl.infer_coarsened(buf, k, cfg)
        small = torch.empty(cshape, dtype=torch.float32, device="cuda")
        report("c_coarsened_k%d" % k, "mgh_decompress_coarsened(k = %d) -> %r" % (k, tuple(cshape)),
               timed(lambda: hl.decompress(buf, config=cfg, coarsen=k, out=small), args.calls, args.warmup))
        st = hl.last_decompress_stats()
        report("b_preview_k%d" % k, "mgh_decompress_preview(k = %d) -> %r" % (k, shape),
               timed(lambda: hl.decompress_preview(buf, k, config=cfg, out=full), args.calls, args.warmup))
        res["chunks_k%d" % k] = [hl.last_decompress_stats()["chunks_decoded"], st["chunks_total"]]
    res["a_over_e"] = res["a_prolong3_top"]["median_ms"] / res["e_fill"]["median_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
