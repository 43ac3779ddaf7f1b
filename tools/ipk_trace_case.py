"""One case of the Thomas-solve plan list (tests/golden/ipk_plans.json): mgh_decompose_quantize and
mgh_dequantize_recompose once each on one shape, in a process of its own. Run under
rocprofv3 --kernel-trace with a development build that logs its solves; tools/ipk_trace.md has the
recipe, tools/ipk_trace_to_plans.py turns the result into golden rows.

  python tools/ipk_trace_case.py NAME      (--list prints the names)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    "512f32": ((512, 512, 512), "float32", False, {}),
    "512f64": ((512, 512, 512), "float64", True, {}),
    "1024f32": ((1024, 1024, 1024), "float32", False, {}),
    "slab4d": ((8, 512, 512, 512), "float32", False, {}),
    "129f32": ((129, 129, 129), "float32", False, {}),
    "257f32": ((257, 257, 257), "float32", False, {}),
    "16395x64x64": ((16395, 64, 64), "float32", False, {}),
    "1d_2p24": ((1 << 24,), "float32", False, {}),
    "4194304x9": ((4194304, 9), "float32", False, {}),
    "100x100x6000": ((100, 100, 6000), "float32", False, {}),
    "64p4": ((64, 64, 64, 64), "float32", False, {}),
    "5d": ((8, 8, 64, 64, 64), "float32", False, {}),
    "spec0_1d_2p20": ((1 << 20,), "float32", False, {"MGH_IPK_SPEC": "0"}),
    "chunk0_129x129x257": ((129, 129, 257), "float32", False, {"MGH_IPK_CHUNK": "0"}),
    # (512^3: the 257 x 257 coarse plane does not fit LDS, so the top level's f-solve reaches ipk_launch)
    "chunk0_512f32": ((512, 512, 512), "float32", False, {"MGH_IPK_CHUNK": "0"}),
    "stream0_1024f32": ((1024, 1024, 1024), "float32", False, {"MGH_IPK_STREAM": "0"}),
    # batched strided pencils too long for LDS with streaming and verified chunks off: a call per box
    "thread_batches_4d": ((5, 6001, 17, 17), "float32", False, {"MGH_IPK_STREAM": "0", "MGH_IPK_SPEC": "0"}),
}


def main():
    name = sys.argv[1]
    if name == "--list":
        print(" ".join(CASES))
        return
    shape, dt, nonuniform, env = CASES[name]
    os.environ.update(env)
    import numpy as np
    import torch
    import mgard_amd
    import bench
    from tests.util import nonuniform_coords
    dev = torch.device("cuda:0")
    np_dt = np.dtype(dt)
    t_dt = torch.float32 if np_dt.itemsize == 4 else torch.float64
    S = 0.0 if nonuniform else float("inf")
    coords = nonuniform_coords(shape, np_dt) if nonuniform else None
    if len(shape) == 4 and shape[0] == 8:
        base = bench.gpu_field(torch, shape[1:], t_dt, dev)
        u = torch.stack([base * (1.0 + 0.002 * t) + 1e-4 * t for t in range(shape[0])])
        del base
    else:
        u = bench.gpu_field(torch, shape, t_dt, dev)
    h = mgard_amd.Hierarchy(shape, np_dt, coords=coords)
    cap = max(h.total // 8, 1024)
    torch.cuda.synchronize()
    sys.stderr.write("IPKCASE %s decompose\n" % name)
    sys.stderr.flush()
    q, oi, ov, n, nrm = h.decompose_quantize(u, mgard_amd.REL, 1e-3, S, outlier_cap=cap)
    torch.cuda.synchronize()
    sys.stderr.write("IPKCASE %s recompose\n" % name)
    sys.stderr.flush()
    back = h.dequantize_recompose(q, mgard_amd.REL, 1e-3, S, nrm, outlier_idx=oi, outlier_val=ov, out=u)
    torch.cuda.synchronize()
    sys.stderr.write("IPKCASE %s done outliers=%d cap=%d\n" % (name, n, cap))
    h.close()


if __name__ == "__main__":
    main()
