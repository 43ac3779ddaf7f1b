"""CPU test of what the region of interest adds to the ABI: the four public entry points are declared (and compile as
C), exported and bound; the two streaming passes over a box are exported and bound and declared in no header; the
C++ mirror compiles on the host; and the refusals that need no device -- NULL arguments and every rule of the boxes
(mgard_amd/csrc/roi_plan.hpp) -- come back before any device work, with nothing allocated and nothing cleared."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIGH = ["mgh_compress_roi", "mgh_decompress_roi", "mgh_roi_info", "mgh_verify_roi"]
LOW = ["mgh_box_scratch_bytes_", "mgh_box_residual_", "mgh_box_add_"]
MGH_ERR_INVALID_ARGUMENT = -1


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_new_symbols_are_declared_exported_and_bound():
    import mgard_amd
    from mgard_amd import highlevel
    L = mgard_amd.load_library()
    for name in HIGH + LOW:
        assert hasattr(L, name), name
    declared = set(re.findall(r"\b(mgh_[a-z_0-9]+)\s*\(", _header("mgard_hip_compress.h")))
    assert set(HIGH) <= declared and set(HIGH) <= set(highlevel.HL_SYMBOLS)
    # (the passes over a box are internal: exported and bound, declared in no public header)
    assert mgard_amd.ROI_INTERNAL_SYMBOLS == LOW
    assert not set(LOW) & (set(mgard_amd.SYMBOLS) | set(highlevel.HL_SYMBOLS) | set(mgard_amd.INTERNAL_SYMBOLS))
    for h in os.listdir(os.path.join(ROOT, "include")):
        for name in LOW:
            assert name not in _header(h), (h, name)
    assert callable(mgard_amd.box_residual) and callable(mgard_amd.box_add)
    for fn in ("compress_roi", "decompress_roi", "roi_info", "verify_roi"):
        assert callable(getattr(highlevel, fn))
    assert L.mgh_box_scratch_bytes_() == (1 + 2048) * 32 == (1 + 2048) * C.sizeof(mgard_amd.BoxStats)
    assert C.sizeof(highlevel.RoiBox) == 88 and C.sizeof(highlevel.RoiInfo) == 16 + 16 * 104


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "roi.c"
    src.write_text('#include "mgard_hip_compress.h"\n'
                   "int main(void) {\n"
                   "  mgh_roi_box b; struct mgh_roi_info i;\n"
                   "  int (*a)(int, int, const uint64_t *, double, double, int, const void *, int, const mgh_roi_box *, void **,\n"
                   "           size_t *, const void *const *, const mgh_config *, int) = mgh_compress_roi;\n"
                   "  int (*c)(const void *, size_t, void **, const mgh_config *, int) = mgh_decompress_roi;\n"
                   "  int (*d)(const void *, size_t, struct mgh_roi_info *) = mgh_roi_info;\n"
                   "  int (*e)(const void *, size_t, const void *, size_t, int, const mgh_config *, mgh_verify_result *,\n"
                   "           mgh_verify_result *) = mgh_verify_roi;\n"
                   "  b.lo[MGH_MAX_DIM - 1] = 0; b.ext[0] = 3; b.tol = 1e-4; i.box[15].tolres = b.tol; i.nbox = (int)b.ext[0];\n"
                   "  return !(a && c && d && e) + (int)i.box[15].tolres + i.nbox;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_cpp_mirror_compiles_on_host():
    src = ('#include "compress_hip.hpp"\n'
           'int main() { using namespace mgard_hip; void *buf = nullptr, *d = nullptr; size_t n = 0; HighLevelConfig c;\n'
           '  std::vector<mgh_roi_box> boxes(1); bool roi = false; struct mgh_roi_info info; mgh_verify_result w;\n'
           '  std::vector<mgh_verify_result> per;\n'
           '  return (int)compress_roi(3, data_type::Float, {9, 9, 9}, 1e-2, 1.0 / 0.0, error_bound_type::REL, d, boxes, buf, n, {}, c, false)\n'
           '    + (int)decompress_roi(buf, n, d, c, false) + (int)roi_info(buf, n, roi, info)\n'
           '    + (int)verify_roi(buf, n, d, 0, data_type::Float, c, w, per); }\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wno-div-by-zero", "-I", os.path.join(ROOT, "include"),
                        "-x", "c++", "-"], input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr


def test_refusals_that_need_no_device():
    from mgard_amd import highlevel as hl
    L = hl._hl()
    err = lambda: L.mgh_last_error()
    shape = (C.c_uint64 * 3)(33, 40, 65)
    data = (C.c_float * 8)()                      # (never read: every call below is refused first)
    cfg = hl.Config()
    inf = float("inf")

    def boxes_of(boxes):
        arr = (hl.RoiBox * max(len(boxes), 1))()
        for b, (lo, ext, tol) in zip(arr, boxes):
            b.lo[:3], b.ext[:3], b.tol = lo, ext, tol
        return arr

    def roi(boxes, tol=1e-2, s=inf, D=3, nbox=None, out=True, size=True, data_ptr=data, shp=shape, box_ptr=True):
        slot, sz = C.c_void_p(0xdead0), C.c_size_t(0)
        rc = L.mgh_compress_roi(D, 0, shp, tol, s, 1, data_ptr, len(boxes) if nbox is None else nbox,
                                boxes_of(boxes) if box_ptr else None, C.byref(slot) if out else None,
                                C.byref(sz) if size else None, None, C.byref(cfg), 0)
        assert slot.value == 0xdead0                # nothing allocated, nothing cleared
        return rc

    good = ((4, 5, 3), (17, 25, 57), 1e-4)
    for kw in (dict(out=False), dict(size=False), dict(data_ptr=None), dict(shp=None), dict(box_ptr=False)):
        assert roi([good], **kw) == MGH_ERR_INVALID_ARGUMENT and b"NULL" in err(), kw
    for boxes, kw, msg in (([], {}, b"nbox must be in 1 .. 16"), ([good], dict(nbox=17), b"nbox must be in 1 .. 16"),
                           ([good], dict(nbox=-1), b"nbox must be in 1 .. 16"),
                           ([((4, 5, 9), (17, 25, 57), 1e-4)], {}, b"leaves the array"),
                           ([((4, 5, 3), (17, 2, 57), 1e-4)], {}, b"at least 3"),
                           ([good, ((20, 29, 59), (3, 3, 3), 1e-3)], {}, b"pairwise disjoint"),
                           ([((4, 5, 3), (17, 25, 57), 1e-2)], {}, b"0 < tol_i < tol"),
                           ([((4, 5, 3), (17, 25, 57), 0.0)], {}, b"0 < tol_i < tol"),
                           ([good], dict(s=0.0), b"s must be infinite"), ([good], dict(s=1.0), b"s must be infinite"),
                           ([good], dict(tol=float("nan")), b"tol must be positive"),
                           ([good], dict(D=0), b"D must be 1 .. 5"), ([good], dict(D=6), b"D must be 1 .. 5"),
                           ([good], dict(shp=(C.c_uint64 * 3)(65536, 65536, 3)), b"2^32 - 1 elements")):
        assert roi(boxes, **kw) == MGH_ERR_INVALID_ARGUMENT and b"compress_roi: " in err() and msg in err(), (boxes, kw, err())
    # the readers: NULL
    p, info, res = C.c_void_p(), hl.RoiInfo(), hl.VerifyResult()
    assert L.mgh_decompress_roi(None, 8, C.byref(p), None, 0) == MGH_ERR_INVALID_ARGUMENT and b"NULL" in err()
    assert L.mgh_decompress_roi(data, 8, None, None, 0) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_decompress_roi(data, 8, C.byref(p), None, 1) == MGH_ERR_INVALID_ARGUMENT and b"pre-allocated" in err()
    assert L.mgh_roi_info(None, 8, C.byref(info)) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_roi_info(data, 8, None) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_verify_roi(None, 8, data, 32, 0, None, C.byref(res), None) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_verify_roi(data, 8, None, 32, 0, None, C.byref(res), None) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_verify_roi(data, 8, data, 32, 0, None, None, None) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_verify_roi(data, 8, data, 32, 7, None, C.byref(res), None) == MGH_ERR_INVALID_ARGUMENT and b"dtype" in err()
    # a host buffer too short for any footer is no buffer with boxes: 0, and no device was asked
    assert L.mgh_roi_info(data, 8, C.byref(info)) == 0
    # the passes over a box
    lo, ext = (C.c_uint64 * 3)(0, 0, 0), (C.c_uint64 * 3)(3, 3, 3)
    assert L.mgh_box_residual_(3, 0, shape, lo, ext, None, data, data, data, None) == MGH_ERR_INVALID_ARGUMENT and b"NULL" in err()
    assert L.mgh_box_residual_(3, 0, shape, None, ext, data, data, data, data, None) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_box_residual_(6, 0, shape, lo, ext, data, data, data, data, None) == MGH_ERR_INVALID_ARGUMENT
    assert L.mgh_box_residual_(3, 5, shape, lo, ext, data, data, data, data, None) == MGH_ERR_INVALID_ARGUMENT and b"dtype" in err()
    far = (C.c_uint64 * 3)(31, 0, 0)
    assert L.mgh_box_residual_(3, 0, shape, far, ext, data, data, data, data, None) == MGH_ERR_INVALID_ARGUMENT and b"leaves" in err()
    assert L.mgh_box_add_(3, 0, shape, far, ext, data, data, None) == MGH_ERR_INVALID_ARGUMENT and b"leaves" in err()
    none = (C.c_uint64 * 3)(3, 0, 3)             # (an extent of 0 is no box)
    assert L.mgh_box_residual_(3, 0, shape, lo, none, data, data, data, data, None) == MGH_ERR_INVALID_ARGUMENT and b"leaves" in err()
    assert L.mgh_box_add_(3, 0, shape, lo, ext, None, data, None) == MGH_ERR_INVALID_ARGUMENT and b"NULL" in err()
