"""Timing of the error statistics on the device ("Error statistics"): 512^3 f32 and f64,
device-resident, HIP-event timings of ten calls after three warm-ups each; median and min ... max.

  (a) mgh_compare(a, b)                                    one launch over both arrays (+ the fold)
  (b) two mgh_norm_device(s = inf) calls, one per array    the same bytes through the norm reduction
  (c) the torch expressions bench.py uses for its check    (b - a).abs().max() and a.abs().max()
  (d) mgh_verify of the reorder = 1 container              against mgh_decompress followed by (a)
  (e) the same two for a Block-decomposed container        (--block, default 129: 64 subdomains; the
      device-resident original is then read box by box through k_compare_ld)

    python tools/exp_compare.py [--n 512] [--out FILE.json]

The variants are timed in turns (one round = every variant once), so that a drift of the machine meets all
of them alike. Every timed call ends in a device synchronise of its own or is bracketed by events on the
stream it runs on."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # microseconds


def summary(us):
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "calls": len(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--block", type=int, default=129)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import mgard_amd as mg
    from mgard_amd import highlevel as hl
    from tests.util import smooth_field
    assert torch.cuda.is_available(), "exp_compare.py needs a GPU"
    shape = (args.n,) * 3
    result = {"device": torch.cuda.get_device_name(0), "shape": shape, "library": mg.lib_path(), "cases": {}}
    for dt in (np.float32, np.float64):
        u = smooth_field(shape, dt)
        d_a = torch.from_numpy(u).cuda()
        cfg = hl.Config(reorder=1)
        buf = hl.compress(d_a, 1e-3, float("inf"), mg.REL, config=cfg)
        d_b = hl.decompress(buf, config=cfg)
        bcfg = hl.Config(reorder=1, domain_decomposition=hl.DD_BLOCK, block_size=args.block)
        bbuf = hl.compress(d_a, 1e-3, float("inf"), mg.REL, config=bcfg)
        h = mg.Hierarchy(shape, dt)
        slot = torch.empty(1, dtype=d_a.dtype, device="cuda")
        out = torch.empty_like(d_a)

        def torch_check():
            return float((d_b - d_a).abs().max().item()), float(d_a.abs().max().item())

        def decompress_then_compare():
            hl.decompress(buf, config=cfg, out=out)
            return mg.compare(d_a, out)

        def block_decompress_then_compare():
            hl.decompress(bbuf, config=bcfg, out=out)
            return mg.compare(d_a, out)

        variants = {
            "a_mgh_compare": lambda: mg.compare(d_a, d_b),
            "b_two_norm_device": lambda: (h.norm_device(d_a, out=slot), h.norm_device(d_b, out=slot)),
            "c_torch_check": torch_check,
            "d_mgh_verify": lambda: hl.verify(buf, d_a, config=cfg),
            "d_decompress_then_compare": decompress_then_compare,
            "e_block_mgh_verify": lambda: hl.verify(bbuf, d_a, config=bcfg),
            "e_block_decompress_then_compare": block_decompress_then_compare,
        }
        times = {k: [] for k in variants}
        for r in range(args.warmup + args.calls):
            for k, fn in variants.items():
                t = timed(fn, torch)
                if r >= args.warmup:
                    times[k].append(t)
        s, v = mg.compare(d_a, d_b), hl.verify(buf, d_a, config=cfg)
        err, nrm = torch_check()
        assert s.max_abs_err == err == v.stats.max_abs_err and s.ref_abs_max == nrm, (s, v, err, nrm)
        case = {k: summary(t) for k, t in times.items()}
        case["bytes_read_by_a"] = 2 * d_a.numel() * d_a.element_size()
        case["a_over_b"] = case["a_mgh_compare"]["median_us"] / case["b_two_norm_device"]["median_us"]
        case["a_GBps"] = case["bytes_read_by_a"] / case["a_mgh_compare"]["median_us"] * 1e-3
        bv, bs = hl.verify(bbuf, d_a, config=bcfg), block_decompress_then_compare()
        assert bv.stats.max_abs_err == bs.max_abs_err and bv.stats.argmax == bs.argmax, (bv, bs)
        case["max_abs_err"], case["within"], case["block_within"] = s.max_abs_err, v.within, bv.within
        case["block_subdomains"] = hl.last_decompress_stats()["subdomains"]
        result["cases"][np.dtype(dt).name] = case
        h.close()
        for k, t in case.items():
            print(np.dtype(dt).name, k, t, flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
