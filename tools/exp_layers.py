"""Developer tool: what precision layers cost beside a tolerance ladder. n^3 float32 on the device (512 by
default), REL, s = inf; wall-clock medians of `reps` runs that end in a device synchronisation, in
milliseconds; outputs pre-allocated:
  (a) mgh_compress_layers with K = 1, 4, 12 tolerances against mgh_compress_ladder at the same tolerances,
      alternating in the same run;
  (b) Layers with k = 1..4 adds, then data(), against k mgh_decompress calls of the ladder's tiers;
  (c) the kernels of mgh_quantize_symbols_residual and mgh_dequantize_add alone at 1e-3, beside
      mgh_quantize_symbols and mgh_quantize_roundtrip, device events around each (every call with its table
      upload; the symbol kernels with their memset);
  (d) bytes of the layers, the ladder and the finest tier alone.
Usage: python tools/exp_layers.py [n] [reps]"""
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
u = smooth_field((n, n, n), np.float32)
d = torch.from_numpy(u).cuda()
INF = float("inf")
CAP = d.numel() * 4 + 1000000


def timed_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def medians_ms(*fns):
    """Medians of `reps` runs of every function, the functions alternating (one warm-up each)."""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ts[k].append(timed_ms(fn))
    return [float(np.median(t)) for t in ts]


def decades(K):
    return [float(t) for t in np.logspace(-2, -5, K)] if K > 1 else [1e-3]


# ---- (a), (d) --------------------------------------------------------------------------------------------------
outs = [torch.empty(CAP, dtype=torch.uint8, device="cuda") for _ in range(12)]
for K in (1, 4, 12):
    tols = decades(K)
    lay, lad = medians_ms(lambda: hl.compress_layers(d, tols, INF, mgard_amd.REL, outs=outs[:K]),
                          lambda: hl.compress_ladder(d, tols, INF, mgard_amd.REL, outs=outs[:K]))
    layers = hl.compress_layers(d, tols, INF, mgard_amd.REL, outs=outs[:K])
    st = hl.last_compress_stats()
    b_lay = [int(g.numel()) for g in layers]
    ladder = hl.compress_ladder(d, tols, INF, mgard_amd.REL, outs=outs[:K])
    b_lad = [int(g.numel()) for g in ladder]
    print("(a) K = %2d: layers %.2f ms, ladder %.2f ms; (d) bytes layers %d, ladder %d, finest tier alone %d; %s"
          % (K, lay, lad, sum(b_lay), sum(b_lad), b_lad[-1], st))

# ---- (b) -------------------------------------------------------------------------------------------------------
tols = decades(4)
layers = [g.clone() for g in hl.compress_layers(d, tols, INF, mgard_amd.REL)]
tiers = [g.clone() for g in hl.compress_ladder(d, tols, INF, mgard_amd.REL)]
out = torch.empty_like(d)
for k in range(1, 5):
    def read_layers():
        with hl.Layers(layers[0]) as r:
            for g in layers[1:k]:
                r.add(g)
            r.data(out=out)
    a, b = medians_ms(read_layers, lambda: [hl.decompress(g, out=out) for g in tiers[:k]])
    print("(b) k = %d: Layers open + %d adds + data %.2f ms, %d mgh_decompress calls %.2f ms" % (k, k - 1, a, k, b))

# ---- (c) -------------------------------------------------------------------------------------------------------
h = mgard_amd.Hierarchy((n, n, n), np.float32)
norm = h.norm(d, INF)
coeff = h.decompose(d)
res = torch.empty_like(coeff)
q, oi, ov, _ = h.quantize(coeff, mgard_amd.REL, 1e-3, INF, norm, dict_size=8192, prep_huffman=True)
acc = h.dequantize_add(q, mgard_amd.REL, 1e-3, INF, norm, outlier_idx=oi, outlier_val=ov)


def events_ms(fn, calls=20):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


for name, fn in (
        ("quantize_symbols_residual (histogram)", lambda: h.quantize_symbols_residual(coeff, mgard_amd.REL, 1e-3, INF, norm, out=res)),
        ("quantize_symbols (histogram)", lambda: h.quantize_symbols(coeff, mgard_amd.REL, 1e-3, INF, norm)),
        ("quantize_roundtrip", lambda: h.quantize_roundtrip(coeff, mgard_amd.REL, 1e-3, INF, norm, out=res)),
        ("dequantize_add (first)", lambda: h.dequantize_add(q, mgard_amd.REL, 1e-3, INF, norm, outlier_idx=oi, outlier_val=ov)),
        ("dequantize_add (add)", lambda: h.dequantize_add(q, mgard_amd.REL, 1e-3, INF, norm, outlier_idx=oi, outlier_val=ov, acc=acc))):
    print("(c) %-40s %.3f ms per call (the Python wrapper's allocations and count read-back included)" % (name, events_ms(fn)))
h.close()
hl.release_cache()
