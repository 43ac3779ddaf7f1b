"""Developer tool: what writing several tolerances of one array costs from ONE decomposition. n^3 float32 on
the device (512 by default), REL, s = inf; wall-clock medians of `reps` runs that end in a device
synchronisation, in milliseconds; outputs pre-allocated on both sides:
  (a) mgh_compress_ladder with K = 1, 4, 12 tolerances against K separate mgh_compress calls at the same
      tolerances, alternating in the same run;
  (b) mgh_compress_budget (4 rounds, budget 10 % of the array, tolerances 1e-7 .. 1e-1) and mgh_compress_target
      (8 rounds, max error <= a thousandth of max|x|, tolerances 1e-6 .. 1e-1) -- the arguments of DESIGN.md
      section 8 -- and, when `other_lib` names a second build of libmgard_hip.so (the parent commit's), the same
      calls through it, alternating in the same process;
  (c) the kernel of mgh_quantize_symbols alone at 1e-3: with the fused histogram, against d_freq = NULL followed
      by the lossless stage's own histogram kernel (mgh_histogram_sym16), device events around each.
Usage: python tools/exp_ladder.py [n] [reps] [other_lib]"""
import ctypes as C
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
other_lib = sys.argv[3] if len(sys.argv) > 3 else None
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


# ---- (a) -------------------------------------------------------------------------------------------------------
outs = [torch.empty(CAP, dtype=torch.uint8, device="cuda") for _ in range(12)]
for K in (1, 4, 12):
    tols = [float(t) for t in np.logspace(-5, -2, K)] if K > 1 else [1e-3]
    lad, sep = medians_ms(lambda: hl.compress_ladder(d, tols, INF, mgard_amd.REL, outs=outs[:K]),
                          lambda: [hl.compress(d, t, INF, mgard_amd.REL, out=outs[k]) for k, t in enumerate(tols)])
    got = hl.compress_ladder(d, tols, INF, mgard_amd.REL, outs=outs[:K])
    st = hl.last_compress_stats()
    sizes = [int(g.numel()) for g in got]
    same = sizes == [int(hl.compress(d, t, INF, mgard_amd.REL, out=outs[0]).numel()) for t in tols]
    print("(a) K = %2d   compress_ladder %8.2f ms   K x compress %8.2f ms   sizes equal: %s   stats %r"
          % (K, lad, sep, same, st))
del outs


# ---- (b) -------------------------------------------------------------------------------------------------------
class Cfg(C.Structure):
    _fields_ = hl.Config._fields_


def bind(path):
    """mgh_compress_budget / _target of a build of the library, bound by hand (an older build lacks what
    mgard_amd.highlevel binds)."""
    L = C.CDLL(path)
    vp, u64 = C.c_void_p, C.c_uint64
    L.mgh_config_default.argtypes = [C.POINTER(Cfg)]
    L.mgh_config_default.restype = None
    L.mgh_compress_budget.argtypes = [C.c_int, C.c_int, C.POINTER(u64), C.c_size_t, C.c_double, C.c_double, C.c_int,
                                      C.c_double, C.c_int, vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp),
                                      C.POINTER(Cfg), C.c_int, C.POINTER(C.c_double), vp]
    L.mgh_compress_target.argtypes = [C.c_int, C.c_int, C.POINTER(u64), C.c_int, C.c_double, C.c_double, C.c_double,
                                      C.c_int, C.c_double, C.c_int, vp, C.POINTER(vp), C.POINTER(C.c_size_t),
                                      C.POINTER(vp), C.POINTER(Cfg), C.c_int, C.POINTER(C.c_double), vp, C.POINTER(C.c_int)]
    cfg = Cfg()
    L.mgh_config_default(C.byref(cfg))
    return L, cfg


out = torch.empty(CAP, dtype=torch.uint8, device="cuda")
shp = (C.c_uint64 * 3)(n, n, n)
budget = d.numel() * 4 // 10
target = 1e-3 * float(np.max(np.abs(u)))


def budget_call(lib):
    L, cfg = lib
    optr, size, used = C.c_void_p(out.data_ptr()), C.c_size_t(CAP), C.c_double()
    rc = L.mgh_compress_budget(3, 0, shp, budget, 1e-7, 1e-1, 4, INF, mgard_amd.REL, C.c_void_p(d.data_ptr()),
                               C.byref(optr), C.byref(size), None, C.byref(cfg), 1, C.byref(used), None)
    assert rc == 0, rc
    return used.value, size.value


def target_call(lib):
    L, cfg = lib
    optr, size, used, cand = C.c_void_p(out.data_ptr()), C.c_size_t(CAP), C.c_double(), C.c_int()
    rc = L.mgh_compress_target(3, 0, shp, 0, target, 1e-6, 1e-1, 8, INF, mgard_amd.REL, C.c_void_p(d.data_ptr()),
                               C.byref(optr), C.byref(size), None, C.byref(cfg), 1, C.byref(used), None, C.byref(cand))
    assert rc == 0, rc
    return used.value, size.value, cand.value


libs = [("this build", bind(mgard_amd.lib_path()))]
if other_lib:
    libs.append(("other build", bind(other_lib)))
for name, call in (("compress_budget", budget_call), ("compress_target", target_call)):
    ms = medians_ms(*[lambda lib=lib: call(lib) for _, lib in libs])
    for (which, lib), t in zip(libs, ms):
        print("(b) %s, %s: %8.2f ms   -> %r" % (name, which, t, call(lib)))

# ---- (c) -------------------------------------------------------------------------------------------------------
L = mgard_amd.load_library()
H = hl._hl()
h = mgard_amd.Hierarchy((n, n, n), np.float32)
coeff = h.decompose(d)
norm = h.norm(d, INF)
dict_size = 8192
sym = torch.empty(d.numel(), dtype=torch.uint16, device="cuda")
freq = torch.zeros(dict_size, dtype=torch.int32, device="cuda")
cnt, idx, val = h._outlier_bufs(d.numel() // 8)


def qsym(with_freq):
    rc = L.mgh_quantize_symbols(h._h, C.c_void_p(coeff.data_ptr()), mgard_amd.REL, 1e-3, INF, norm, dict_size,
                                C.c_void_p(sym.data_ptr()), C.c_void_p(freq.data_ptr()) if with_freq else None,
                                C.c_void_p(cnt.data_ptr()), C.c_void_p(idx.data_ptr()), C.c_void_p(val.data_ptr()),
                                int(idx.numel()), None)
    assert rc == 0, rc


def fused():
    freq.zero_()
    cnt.zero_()
    qsym(True)


def separate():
    freq.zero_()
    cnt.zero_()
    qsym(False)
    assert H.mgh_histogram_sym16(C.c_void_p(sym.data_ptr()), d.numel(), dict_size, C.c_void_p(freq.data_ptr()), None) == 0


def event_ms(fn):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(20):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 20


ts = [[], []]
for _ in range(reps):
    ts[0].append(event_ms(fused))
    ts[1].append(event_ms(separate))
fused()
f1 = freq.clone()
separate()
print("(c) quantize_symbols at 1e-3, dict %d, per call (two memsets included): fused histogram %7.3f ms   "
      "d_freq = NULL + k_histogram %7.3f ms   histograms equal: %s   outliers %d"
      % (dict_size, float(np.median(ts[0])), float(np.median(ts[1])), bool((f1 == freq).all()), int(cnt.item())))
h.close()
