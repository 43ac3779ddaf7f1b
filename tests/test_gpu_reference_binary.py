"""The HIP kernels against a build of the reference itself, bit for bit, with no oracle in between.

oracle/_ref/libmgx_ref.so is the reference MGARD-X's own SERIAL code path (oracle/ref_driver.cpp,
built by oracle.build_ref()); a misreading that the CPU oracle and the kernels share cannot hide
here. Every case runs decompose, recompose, quantize, dequantize, the fused decompose_quantize and
dequantize_recompose of mgard_amd.Hierarchy, and compares each with the reference's
DataRefactor / LinearQuantizer on the same input: floats through their bit patterns, integers
exactly, outliers as sorted (index, value) sets. The norm is injected.

The shapes are chosen so that every kernel family of DESIGN.md's kernel table runs at least once;
each case says which path it targets. max_level and normalize_coordinates = False run here too.
"""
import numpy as np
import pytest

from oracle import ref
from tests.util import nonuniform_coords, smooth_field

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ref.available(),
                                 reason="%s is not built (oracle.build_ref())" % ref.LIB_PATH)]

REL, ABS = ref.REL, ref.ABS

# (shape, dtype, options, the path the case targets). options: coords ("nonuniform"), normalize,
# max_level ("top-1" = l_target - 1), ebtype, tol, s, dict_size, prep_huffman.
CASES = [
    ((17, 17, 17), np.float32, dict(),
     "every level fits in LDS: k_tail (decompose) and k_recompose_head (recompose)"),
    ((65, 70, 129), np.float64, dict(coords="nonuniform", ebtype=ABS, s=0.0, dict_size=64),
     "fused 3-D level kernel, 8 x 32 tiles, mid-size march class; LDS-staged Thomas solves"),
    ((40, 130, 9), np.float32, dict(normalize=False, s=1.0),
     "fused 3-D level kernel with 64 x 4 main tiles (coarse f <= 16 under coarse c >= 48)"),
    ((70, 300, 5), np.float64, dict(max_level=1, s=-1.0, dict_size=1001),
     "64 x 4 main tiles, hierarchy cut by max_level"),
    ((1025, 130, 257), np.float32, dict(s=np.inf),
     "long-march class (>= 2048 tiles x marches at the top level): 4 x 64 float tiles, RCH = 16"),
    ((5000, 5, 7), np.float32, dict(s=0.5, dict_size=1001, prep_huffman=False),
     "thin array (plane fills < 1/8 of its tiles): the one-thread-per-element simple kernels"),
    ((3000, 17, 17), np.float64, dict(coords="nonuniform", max_level="top-1"),
     "chunked strided solves (r-pencils of 3000 nodes), fused tiles on a small cross-section"),
    ((8, 66, 70, 129), np.float32, dict(s=0.0),
     "fused 4-D slice path (even / odd t-slices, k_tsweep, ipk_t, k_head_in4_q)"),
    ((20, 40, 40, 40), np.float64, dict(normalize=False, max_level=1, ebtype=ABS, s=1.0),
     "fused 4-D slice path, normalize_coordinates = False, max_level"),
    ((9, 8, 10, 17), np.float32, dict(coords="nonuniform", dict_size=64),
     "4-D outside the fused kernels: generic N-D kernels"),
    ((4, 3, 70, 5, 131), np.float32, dict(ebtype=ABS, s=1.0),
     "D = 5: generic N-D row kernels (k_nd_coeff_rows, k_nd_lpk_fast / _mid)"),
    ((6, 7, 5, 3, 10), np.float64, dict(coords="nonuniform", max_level=0, s=0.0),
     "D = 5 with a single level (max_level = 0)"),
    ((300001,), np.float32, dict(s=np.inf),
     "1-D long pencil: chunked speculative Thomas sweeps (k_ipk_spec_*)"),
    ((257, 130), np.float64, dict(normalize=False, s=0.5, max_level="top-1"),
     "D = 2: the one-thread-per-element kernels"),
]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_bit_equal(got, want, what):
    gb, wb = _bits(got), _bits(want)
    assert gb.shape == wb.shape, (what, gb.shape, wb.shape)
    if not np.array_equal(gb, wb):
        bad = np.argwhere(gb != wb)
        i = tuple(bad[0])
        raise AssertionError("%s: %d/%d elements differ; first at %s: HIP %r reference %r" % (
            what, len(bad), gb.size, i, got[i], want[i]))


def _outliers(idx, val):
    idx, val = np.asarray(idx).astype(np.int64), np.asarray(val).astype(np.int64)
    order = np.argsort(idx, kind="stable")
    return list(zip(idx[order].tolist(), val[order].tolist()))


def _cpu(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])) + "-" + np.dtype(c[1]).name)
def test_hip_equals_reference(case):
    import torch
    import mgard_amd as mg

    shape, dt, opt, _path = case
    coords = nonuniform_coords(shape, dt, seed=sum(shape)) if opt.get("coords") else None
    normalize = opt.get("normalize", True)
    ml = opt.get("max_level")
    if ml == "top-1":
        ml = ref.Hierarchy(shape, dt).l_target - 1
    r = ref.Hierarchy(shape, dt, coords=coords, normalize_coordinates=normalize,
                      **({} if ml is None else dict(max_level=ml)))
    h = mg.Hierarchy(shape, dt, coords=coords, normalize_coordinates=normalize, max_level=ml)
    assert h.l_target == r.l_target
    for l in range(r.l_target + 1):
        assert h.level_shape(l) == r.level_shape(l)

    ebtype, s = opt.get("ebtype", REL), opt.get("s", np.inf)
    tol, dict_size, prep = opt.get("tol", 1e-4), opt.get("dict_size", 8192), opt.get("prep_huffman", True)
    u = smooth_field(shape, dt, seed=int(np.prod(shape)) % 100003, noise=1e-2)
    norm = ref.norm(u, s, normalize)
    qargs = (ebtype, dt(tol), dt(s), dt(norm), dict_size, prep)
    gargs = (ebtype, tol, float(s), float(dt(norm)), dict_size, prep)
    du = torch.from_numpy(u).cuda()

    # decompose / recompose
    cr = r.decompose(u)
    assert_bit_equal(_cpu(h.decompose(du)), cr, "decompose")
    dcr = torch.from_numpy(cr).cuda()
    assert_bit_equal(_cpu(h.recompose(dcr)), r.recompose(cr), "recompose")

    # quantize / dequantize
    qr, oir, ovr, nr = r.quantize(cr, *qargs)
    q, oi, ov, n = h.quantize(dcr, *gargs)
    assert n == nr, ("quantize outlier count", n, nr)
    assert np.array_equal(_cpu(q), qr), "quantize: %d values differ" % int(np.sum(_cpu(q) != qr))
    assert _outliers(_cpu(oi), _cpu(ov)) == _outliers(oir, ovr), "quantize outliers"
    dqr = torch.from_numpy(qr).cuda()
    doi = torch.from_numpy(oir.astype(np.int64)).cuda()
    dov = torch.from_numpy(ovr).cuda()
    vr = r.dequantize(qr, *qargs, outlier_idx=oir, outlier_val=ovr)
    assert_bit_equal(_cpu(h.dequantize(dqr.clone(), *gargs, outlier_idx=doi, outlier_val=dov)), vr,
                     "dequantize")

    # the fused paths
    q2, oi2, ov2, n2, _ = h.decompose_quantize(du, ebtype, tol, float(s), float(dt(norm)),
                                                dict_size=dict_size, prep_huffman=prep)
    assert n2 == nr, ("decompose_quantize outlier count", n2, nr)
    assert np.array_equal(_cpu(q2), qr), "decompose_quantize: %d values differ" % int(
        np.sum(_cpu(q2) != qr))
    assert _outliers(_cpu(oi2), _cpu(ov2)) == _outliers(oir, ovr), "decompose_quantize outliers"
    back = h.dequantize_recompose(dqr, ebtype, tol, float(s), float(dt(norm)), dict_size=dict_size,
                                  prep_huffman=prep, outlier_idx=doi, outlier_val=dov)
    assert_bit_equal(_cpu(back), r.recompose(vr), "dequantize_recompose")
