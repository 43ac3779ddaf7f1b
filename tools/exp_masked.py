"""Developer tool: what a missing-value mask costs. n^3 float32 on the device (512 by default) with a ball mask of
about 30 % (NaN), REL 1e-3, s = inf; wall-clock medians of `reps` runs that end in a device synchronisation, in
milliseconds; outputs pre-allocated:
  (1) compress_masked / decompress_masked beside compress / decompress of the pre-filled array, alternating in the
      same run -- the structural expectation is the plain call plus three streams of the array (scan; the fill's
      read and write) and one of n / 8 bytes -- and the three kernels alone under device events;
  (2) bytes of the mask record, kind 0 against kind 1, and the container's size under the hold rule against a
      constant fill with c.
Usage: python tools/exp_masked.py [n] [reps]"""
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
INF = float("inf")
TOL = 1e-3
shape = (n, n, n)
u = smooth_field(shape, np.float32)
ax = [(np.arange(n, dtype=np.float32) - (n - 1) / 2) ** 2 for _ in range(3)]
mask = (ax[0][:, None, None] + ax[1][None, :, None] + ax[2][None, None, :]) < (0.415 * n) ** 2  # 4/3 pi r^3 = 0.30
u[mask] = np.nan
d = torch.from_numpy(u).cuda()
print("%d^3 float32, ball mask %.1f %%" % (n, 100.0 * mask.mean()))


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


def events_ms(fn, calls=20):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


# ---- the kernels alone, and the two fills ---------------------------------------------------------------------
words, st = mgard_amd.mask_scan(d)
c = 0.5 * st.vmin + 0.5 * st.vmax
hold = mgard_amd.mask_fill(d, words, c)
const = torch.where(torch.isfinite(d), d, torch.tensor(c, dtype=d.dtype, device=d.device))
tmp = torch.empty_like(d)
nbytes = d.numel() * 4
for name, fn, moved in (
        ("mask_scan", lambda: mgard_amd.mask_scan(d), nbytes + nbytes // 32),
        ("mask_fill", lambda: mgard_amd.mask_fill(d, words, c, out=tmp), 2 * nbytes + nbytes // 32),
        ("mask_restore", lambda: mgard_amd.mask_restore(tmp, words, float("nan")), nbytes // 32 + int(mask.sum()) * 4)):
    ms = events_ms(fn)
    print("(1) %-12s %.3f ms per call, %.2f TB/s of the bytes it must move (the Python wrapper's allocations included)"
          % (name, ms, moved / ms * 1e-9))

# ---- (1) the whole calls ---------------------------------------------------------------------------------------
cap = nbytes + 1000000 + 8 * ((d.numel() + 63) // 64) + 48
out_m = torch.empty(cap, dtype=torch.uint8, device="cuda")
out_p = torch.empty(cap, dtype=torch.uint8, device="cuda")
cm, cp = medians_ms(lambda: hl.compress_masked(d, TOL, INF, mgard_amd.REL, out=out_m),
                    lambda: hl.compress(hold, TOL, INF, mgard_amd.REL, out=out_p))
buf = hl.compress_masked(d, TOL, INF, mgard_amd.REL, out=out_m).clone()
plain = hl.compress(hold, TOL, INF, mgard_amd.REL, out=out_p).clone()
back = torch.empty_like(d)
dm, dp = medians_ms(lambda: hl.decompress_masked(buf, out=back), lambda: hl.decompress(plain, out=back))
print("(1) compress_masked %.2f ms, compress of the pre-filled array %.2f ms; decompress_masked %.2f ms, decompress %.2f ms"
      % (cm, cp, dm, dp))

# ---- (2) bytes ---------------------------------------------------------------------------------------------------
info = hl.masked_info(buf)
packed = 8 * ((d.numel() + 63) // 64)
held = int(info.container_size)
constant = int(hl.compress(const, TOL, INF, mgard_amd.REL, out=out_p).numel())
print("(2) mask record: kind %d, %d bytes (kind 0 would be %d); container under the hold rule %d bytes, under a "
      "constant fill with c %d bytes (%+.2f %%)" % (info.kind, info.record_size, packed, held, constant,
                                                    100.0 * (constant - held) / held))
hl.release_cache()
