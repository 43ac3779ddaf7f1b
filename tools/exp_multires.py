"""Reconstruction at a coarser level against the FULL call, in the same run on the same box: HIP events,
warm-up, several alternations (full, l_target-1, -2, -3, full, ...). For n^3 f32 (default 512; 1024):
dequantize_recompose from int64 and from 16-bit symbols, highlevel.decompress device to device and host to
host of a reorder = 0 and of a reorder = 1 (level-linearised) container -- below l_target only the head of the
latter is decoded; where the library has mgh_last_decompress_stats the chunks decoded are printed, so the
tool runs on an older tree too -- the box_from_linear kernel on its own, and the
full call's top-level kernels (profile) -- the structural claim is
    time(level = l_target - 1) < time(full) - time(top-level kernels of the full call) + spread.
Dev tool; the table goes into DESIGN.md section 6 and profiles/NOTES.md."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgard_amd as mg
from bench import gpu_field
from mgard_amd import highlevel as hl

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
reps = 5
dev = torch.device("cuda:0")
d = gpu_field(torch, (n, n, n), torch.float32, dev)
h = mg.Hierarchy((n, n, n), np.float32)
L = h.l_target
INF = float("inf")
q, oi, ov, cnt, nrm = h.decompose_quantize(d, mg.REL, 1e-3, INF)
sym, si, sv, scnt, _ = h.decompose_quantize_sym16(d, mg.REL, 1e-3, INF, nrm)
stream = hl.compress(d, 1e-3, INF, mg.REL)
cfg1 = hl.Config(reorder=1)
stream1 = hl.compress(d, 1e-3, INF, mg.REL, config=cfg1)
host0, host1 = stream.cpu().numpy(), stream1.cpu().numpy()
levels = [None, L - 1, L - 2, L - 3]
outs = {lv: torch.empty(h.shape if lv is None else h.level_shape(lv), dtype=torch.float32, device=dev) for lv in levels}
houts = {lv: np.empty(h.shape if lv is None else h.level_shape(lv), dtype=np.float32) for lv in levels}


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


legs = {
    "int64": lambda lv: h.dequantize_recompose(q, mg.REL, 1e-3, INF, nrm, outlier_idx=oi, outlier_val=ov,
                                               out=outs[lv], level=lv),
    "sym16": lambda lv: h.dequantize_recompose_sym16(sym, mg.REL, 1e-3, INF, nrm, outlier_idx=si, outlier_val=sv,
                                                     out=outs[lv], level=lv),
    "decompress": lambda lv: hl.decompress(stream, out=outs[lv], level=lv),
    "decompress r1": lambda lv: hl.decompress(stream1, config=cfg1, out=outs[lv], level=lv),
    "decompress h2h": lambda lv: hl.decompress(host0, out=houts[lv], level=lv),
    "decompress r1 h2h": lambda lv: hl.decompress(host1, config=cfg1, out=houts[lv], level=lv),
}
print("%d^3 f32, l_target %d, %d alternations x %d calls; ms per call: min / median / max" % (n, L, rounds, reps))
for name, f in legs.items():
    for lv in levels:  # warm-up: every level once (allocations, first launches)
        f(lv)
    torch.cuda.synchronize()
    t = {lv: [] for lv in levels}
    for _ in range(rounds):
        for lv in levels:
            t[lv].append(timed(lambda: f(lv)))
    for lv in levels:
        v = sorted(t[lv])
        print("  %-18s %-14s %8.3f / %8.3f / %8.3f" % (name, "full" if lv is None else "l_target-%d" % (L - lv),
                                                          v[0], v[len(v) // 2], v[-1]))
    if name.startswith("decompress"):
        if hasattr(hl, "last_decompress_stats"):
            for lv in levels:
                f(lv)
                print("     %-14s %s" % ("full" if lv is None else "l_target-%d" % (L - lv), hl.last_decompress_stats()))
        continue
    # per-kernel events of the full call and of level l_target - 1 (3 calls each): every kernel of both, their
    # sums, and the kernel time of the full call beyond that level. Beside the whole-call times above, the sums
    # tell how much of a call is NOT kernel time (launch gaps, memsets): whole - sum.
    prof = {}
    for lv in (None, L - 1):
        h.profile(True)
        for _ in range(3):
            f(lv)
        torch.cuda.synchronize()
        prof[lv] = h.profile_read(reset=True)
        h.profile(False)
    top = 0.0
    sums = {None: 0.0, L - 1: 0.0}
    for k in sorted(set(prof[None]) | set(prof[L - 1])):
        ms, cntk = prof[None].get(k, (0.0, 0))
        ms1, cnt1 = prof[L - 1].get(k, (0.0, 0))
        if not cntk and not cnt1:
            continue
        print("     %-18s full %8.1f us (%2d launches)   l_target-1 %8.1f us (%2d)" % (
            k, ms / 3 * 1e3, cntk // 3, ms1 / 3 * 1e3, cnt1 // 3))
        top += (ms - ms1) / 3
        sums[None] += ms / 3
        sums[L - 1] += ms1 / 3
    med = {lv: sorted(t[lv])[len(t[lv]) // 2] for lv in (None, L - 1)}
    print("     kernel sums: full %.3f ms, l_target-1 %.3f ms; beyond level l_target-1: %.3f ms" % (
        sums[None], sums[L - 1], top))
    print("     not kernel time (whole call - kernel sum): full %.3f ms, l_target-1 %.3f ms" % (
        med[None] - sums[None], med[L - 1] - sums[L - 1]))
    print("     structural check: l_target-1 %.3f ms against full - beyond = %.3f ms" % (med[L - 1], med[None] - top))

# k_box_from_linear on its own: the box of level l_target - 1 (and - 2) from the head of the linearised integers
if hasattr(h, "level_box_from_linear"):
    lin = h.level_linearize(q).reshape(-1)
    for lv in (L - 1, L - 2):
        n_l = int(np.prod(h.level_shape(lv)))
        head, box = lin[:n_l].clone(), torch.empty(n_l, dtype=torch.int64, device=dev)
        h.level_box_from_linear(head, lv, out=box)
        v = sorted(timed(lambda: h.level_box_from_linear(head, lv, out=box)) for _ in range(rounds))
        print("  box_from_linear %s: %.4f / %.4f / %.4f ms, %.0f GB/s at the median (16 bytes per element)" % (
            "x".join(map(str, h.level_shape(lv))), v[0], v[len(v) // 2], v[-1], 16 * n_l / v[len(v) // 2] / 1e6))
