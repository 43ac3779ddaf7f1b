#!/usr/bin/env python3
"""Cost of the windowed full-grid preview ("A window of the preview").

512^3 f32, REL 1e-3, a reorder = 1 container resident on the device, outputs pre-allocated on the device.
Every figure is the median of HIP-event timings over `--calls` calls after `--warmup` calls, as in
tools/exp_preview.py:

  (a) mgh_decompress_preview for k = 1, 2, 3 (the whole array)
  (b) mgh_decompress_preview_window for the same k and the windows: a 64^3 box, a 512 x 512 plane along each of the
      three dimensions, the full window
  (c) the last prolong3_win launch of the full window (Hierarchy.prolong(level l_target - 1, window = everything))
      against the prolong3 launch it mirrors (Hierarchy.prolong(level l_target - 1)), and the two bit for bit

The structural expectation: a small window costs the coarsened decode plus a few small launches; the full window's
last launch costs about what prolong3 costs. Prints one line per figure and a JSON line at the end; sets no threshold.

    python tools/exp_preview_window.py [--n 512] [--calls 10] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.exp_preview import timed  # noqa: E402


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

    n = args.n
    shape = (n,) * 3
    u = torch.from_numpy(smooth_field(shape, np.float32)).cuda()
    cfg = hl.Config(reorder=1)
    buf = hl.compress(u, 1e-3, np.inf, mg.REL, config=cfg)
    assert isinstance(buf, torch.Tensor) and buf.is_cuda
    del u
    _, K = hl.infer_coarsened(buf, None, cfg)
    full = torch.empty(shape, dtype=torch.float32, device="cuda")
    res = {"shape": list(shape), "dtype": "float32", "container_bytes": int(buf.numel()),
           "device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup}

    def report(key, what, t):
        res[key] = {"median_ms": t[0], "min_ms": t[1], "max_ms": t[2]}
        print("%-28s %-62s median %8.3f ms  (min %.3f, max %.3f)" % (key, what, t[0], t[1], t[2]), flush=True)

    b = min(64, n)
    at = (n - b) // 2 | 1
    windows = [("box%d" % b, (at,) * 3, (b,) * 3)]
    for d in range(3):
        windows.append(("plane_d%d" % d, tuple(n // 2 + 1 if k == d else 0 for k in range(3)),
                        tuple(1 if k == d else n for k in range(3))))
    windows.append(("full", (0, 0, 0), shape))

    # (c) the last launch of the full window against the prolong3 launch it mirrors
    h = mg.Hierarchy(shape, np.float32)
    L = h.l_target
    lvl = torch.rand(h.level_shape(L - 1), dtype=torch.float32, device="cuda")
    print("prolong plan of the top level: %r" % (h.prolong_plan(L),))
    print("window plan of the top level, full window: %r" % (h.prolong_window_plan(L - 1, (0, 0, 0), shape, L),))
    report("c_prolong3_top", "Hierarchy.prolong(level %d -> %d): one prolong3 launch" % (L - 1, L),
           timed(lambda: h.prolong(lvl, L - 1, out=full), args.calls, args.warmup))
    other = torch.empty(shape, dtype=torch.float32, device="cuda")
    report("c_prolong3_win_top", "... window = the whole array: one prolong3_win launch",
           timed(lambda: h.prolong(lvl, L - 1, out=other, window=((0, 0, 0), shape)), args.calls, args.warmup))
    res["c_win_equals_full"] = bool(torch.equal(full.view(torch.int32), other.view(torch.int32)))
    print("the two launches bit-equal: %r" % res["c_win_equals_full"])
    del other, lvl
    h.close()

    for k in range(1, min(3, K) + 1):
        report("a_preview_k%d" % k, "mgh_decompress_preview(k = %d) -> %r" % (k, shape),
               timed(lambda: hl.decompress_preview(buf, k, config=cfg, out=full), args.calls, args.warmup))
        for wname, lo, ext in windows:
            out = torch.empty(ext, dtype=torch.float32, device="cuda")
            report("b_window_k%d_%s" % (k, wname), "mgh_decompress_preview_window(k = %d, %r + %r)" % (k, lo, ext),
                   timed(lambda: hl.decompress_preview(buf, k, config=cfg, out=out, window=(lo, ext)), args.calls,
                         args.warmup))
            sl = tuple(slice(a, a + e) for a, e in zip(lo, ext))
            same = bool(torch.equal(full[sl].contiguous().view(torch.int32), out.view(torch.int32)))
            res["b_window_k%d_%s" % (k, wname)]["equals_crop"] = same
            if not same:
                print("  NOT the crop of the full preview")
            del out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
