"""mgard_amd -- MI355X-native MGARD-X hot path (multilevel decomposition + level-wise linear
quantizer) behind the C ABI of include/mgard_hip.h.

This module is the thin Python host side used by the tests and bench.py: torch supplies device
memory and streams, every computation goes through libmgard_hip.so (hand-written HIP kernels).
There is no CPU fallback: without the built library or without a GPU the calls raise.
"""
import ctypes as C
import os

import numpy as np

from . import _build

REL, ABS = 0, 1          # mgard_x::error_bound_type
LD_IN, LD_OUT = 0, 1     # mgh_set_ld
FLOAT, DOUBLE = 0, 1     # mgard_x::data_type
INF = float("inf")

_lib = None

SYMBOLS = [
    "mgh_last_error", "mgh_device_count", "mgh_hierarchy_create", "mgh_hierarchy_destroy",
    "mgh_l_target", "mgh_level_shape", "mgh_total_num_elems", "mgh_device_bytes", "mgh_norm_device_ptr",
    "mgh_hierarchy_table", "mgh_norm", "mgh_decompose", "mgh_recompose", "mgh_quantize",
    "mgh_dequantize", "mgh_decompose_quantize", "mgh_dequantize_recompose",
    "mgh_norm_device", "mgh_decompose_quantize_dn", "mgh_decompose_quantize_sym16",
    "mgh_dequantize_recompose_sym16", "mgh_sym16_supported",
    "mgh_profile_enable", "mgh_profile_filter", "mgh_profile_read", "mgh_stream_calibrate",
    "mgh_level_linearize", "mgh_outlier_restore", "mgh_norm_stream_begin", "mgh_norm_stream_add",
    "mgh_norm_stream_end", "mgh_quantize_histograms", "mgh_quantize_roundtrip",
    "mgh_quantize_symbols", "mgh_quantize_symbols_residual", "mgh_dequantize_add",
    "mgh_set_ld",
    "mgh_recompose_to_level", "mgh_dequantize_recompose_to_level",
    "mgh_dequantize_recompose_sym16_to_level", "mgh_level_nodes",
    "mgh_level_box_from_linear", "mgh_dequantize_recompose_linear_to_level",
    "mgh_refine_level", "mgh_debug_ipk_plans_read", "mgh_debug_spec_repairs_read", "mgh_debug_fused_plans_read",
    "mgh_prolong", "mgh_debug_prolong_plan",
    "mgh_prolong_window", "mgh_prolong_window_strided", "mgh_debug_prolong_window_ranges",
    "mgh_debug_prolong_window_plan",
    "mgh_compare",
    "mgh_mask_scan", "mgh_mask_fill", "mgh_mask_restore",
]
# declared in include/mgard_hip_level_layers.h (which mgard_hip.h includes): the low-level calls of the precision
# layers in level order
LEVEL_LAYERS_SYMBOLS = ["mgh_quantize_residual_linear", "mgh_dequantize_add_linear", "mgh_recompose_linear_to_level"]
# entry points of the library that no public header declares yet (trailing underscore): bound here for
# mask_sample / compare_masked and their tests
INTERNAL_SYMBOLS = ["mgh_mask_sample_", "mgh_compare_masked_"]
# ... and the three streaming passes of the pointwise relative bound (pwrel_forward / pwrel_inverse / compare_pwrel)
PWREL_INTERNAL_SYMBOLS = ["mgh_pwrel_forward_", "mgh_pwrel_inverse_", "mgh_compare_pwrel_"]
# ... and the inverse pass over a level array, a coarsened array or a window (pwrel_inverse_sampled)
PWREL_VIEW_INTERNAL_SYMBOLS = ["mgh_pwrel_inverse_sampled_"]
# ... and the two streaming passes of the region of interest over a box of an array (box_residual / box_add)
ROI_INTERNAL_SYMBOLS = ["mgh_box_scratch_bytes_", "mgh_box_residual_", "mgh_box_add_"]


class MgardHipError(RuntimeError):
    pass


class ErrorStats(C.Structure):
    """mgh_error_stats (include/mgard_hip.h): statistics of a reference array `a` against an array `b`.
    Positions whose difference is not finite are counted in `nonfinite` and take part in nothing else."""
    _fields_ = [("n", C.c_uint64), ("nonfinite", C.c_uint64), ("max_abs_err", C.c_double), ("argmax", C.c_uint64),
                ("sum_sq_err", C.c_double), ("ref_min", C.c_double), ("ref_max", C.c_double),
                ("ref_abs_max", C.c_double), ("ref_sum_sq", C.c_double)]

    @property
    def mse(self):
        m = self.n - self.nonfinite
        return self.sum_sq_err / m if m else 0.0

    @property
    def rmse(self):
        return float(np.sqrt(self.mse))

    @property
    def psnr(self):
        """20 log10((ref_max - ref_min) / rmse); +inf for a zero error."""
        r = self.rmse
        if r == 0:
            return INF
        with np.errstate(divide="ignore"):
            return float(20.0 * np.log10(np.float64(self.ref_max - self.ref_min) / r))

    def l2_error(self, normalize=True):
        return float(np.sqrt(self.mse if normalize else self.sum_sq_err))

    def __repr__(self):
        return "ErrorStats(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k, _ in self._fields_)


class PwrelStats(C.Structure):
    """mgh_pwrel_stats: element count, masked count (non-finite or below the floor), the non-finite among them, the
    set flag bits (non-finite, and negative valid elements), and the extremes of y = log2|x| over the valid elements
    (0, 0 when there is none)."""
    _fields_ = [("n", C.c_uint64), ("n_masked", C.c_uint64), ("n_nonfinite", C.c_uint64), ("n_flag", C.c_uint64),
                ("ymin", C.c_double), ("ymax", C.c_double)]

    def __repr__(self):
        return "PwrelStats(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k, _ in self._fields_)


class PwrelCompare(C.Structure):
    """mgh_pwrel_compare (include/mgard_hip.h): an original against a reconstruction under the pointwise relative
    bound -- max |x' - x| / |x| over the valid positions and where, the counts of the three classes, the largest |x|
    that was zeroed, and the positions whose class or sign did not come back."""
    _fields_ = [("n", C.c_uint64), ("n_valid", C.c_uint64), ("n_zeroed", C.c_uint64), ("n_nonfinite", C.c_uint64),
                ("max_rel_err", C.c_double), ("argmax", C.c_uint64), ("max_zeroed_abs", C.c_double),
                ("n_class_mismatch", C.c_uint64), ("n_sign_mismatch", C.c_uint64)]

    def __repr__(self):
        return "PwrelCompare(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k, _ in self._fields_)


def lib_path():
    return _build.LIB


def load_library():
    """Loads libmgard_hip.so (importing torch first so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_build.LIB):
        raise MgardHipError(
            "libmgard_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    import torch  # noqa: F401  (loads libamdhip64.so.7 that our library binds to)
    L = C.CDLL(_build.LIB)
    vp, u64, i64p, u64p = C.c_void_p, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
    L.mgh_last_error.restype = C.c_char_p
    L.mgh_device_count.restype = C.c_int
    L.mgh_hierarchy_create.argtypes = [C.POINTER(vp), C.c_int, u64p, C.c_int, C.POINTER(vp),
                                       C.c_int, u64, C.c_int]
    L.mgh_hierarchy_destroy.argtypes = [vp]
    L.mgh_hierarchy_destroy.restype = None
    L.mgh_l_target.argtypes = [vp]
    L.mgh_level_shape.argtypes = [vp, C.c_int, u64p]
    L.mgh_total_num_elems.argtypes = [vp]
    L.mgh_total_num_elems.restype = u64
    L.mgh_device_bytes.argtypes = [vp]
    L.mgh_device_bytes.restype = C.c_size_t
    L.mgh_hierarchy_table.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, u64]
    L.mgh_hierarchy_table.restype = C.c_int64
    L.mgh_norm.argtypes = [vp, vp, C.c_double, C.POINTER(C.c_double), vp]
    L.mgh_decompose.argtypes = [vp, vp, vp, vp]
    L.mgh_recompose.argtypes = [vp, vp, vp, vp]
    L.mgh_quantize.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, C.c_double, u64, C.c_int,
                               vp, vp, vp, vp, u64, vp]
    L.mgh_dequantize.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, C.c_double, u64,
                                 C.c_int, vp, vp, u64, vp, vp]
    L.mgh_decompose_quantize.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, C.c_double,
                                         C.POINTER(C.c_double), u64, C.c_int, vp, vp, vp, vp, u64,
                                         vp, vp]
    L.mgh_norm_device.argtypes = [vp, vp, C.c_double, vp, vp]
    L.mgh_norm_stream_begin.argtypes = [vp, vp]
    L.mgh_set_ld.argtypes = [vp, C.c_int, u64p]
    L.mgh_norm_stream_add.argtypes = [vp, vp, u64, C.c_double, C.c_int, vp]
    L.mgh_norm_stream_end.argtypes = [vp, C.c_double, C.POINTER(C.c_double), vp]
    L.mgh_quantize_histograms.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_double, C.c_double,
                                          u64, vp, vp, vp]
    L.mgh_quantize_roundtrip.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, C.c_double, vp, vp]
    L.mgh_quantize_symbols.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, C.c_double, u64, vp, vp, vp, vp, vp,
                                       u64, vp]
    L.mgh_quantize_symbols_residual.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, C.c_double, u64, vp, vp, vp, vp,
                                                vp, u64, vp, vp]
    L.mgh_dequantize_add.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, C.c_double, u64, C.c_int, vp, vp, u64,
                                     C.c_int, vp, vp]
    L.mgh_dequantize_recompose_sym16.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, C.c_double, u64,
                                                 vp, vp, u64, vp, vp]
    L.mgh_sym16_supported.argtypes = [vp]
    L.mgh_decompose_quantize_sym16.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, C.c_double,
                                               C.POINTER(C.c_double), u64, vp, vp, vp, vp, u64, vp]
    L.mgh_decompose_quantize_dn.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, vp, u64, u64,
                                            C.c_int, vp, vp, vp, vp, u64, vp]
    L.mgh_dequantize_recompose.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, C.c_double,
                                           u64, C.c_int, vp, vp, u64, vp, vp]
    L.mgh_profile_enable.argtypes = [vp, C.c_int]
    L.mgh_profile_filter.argtypes = [vp, C.c_char_p]
    L.mgh_profile_read.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_double), u64p,
                                   C.c_int, C.c_int]
    L.mgh_debug_ipk_plans_read.argtypes = [vp, i64p, C.c_int, C.c_int]
    L.mgh_debug_spec_repairs_read.argtypes = [vp, u64p, C.c_int]
    L.mgh_debug_fused_plans_read.argtypes = [vp, i64p, C.c_int, C.c_int]
    L.mgh_outlier_restore.argtypes = [vp, u64, vp, vp, u64, vp]
    L.mgh_level_linearize.argtypes = [vp, vp, vp, C.c_int, vp, vp, u64, u64, vp]
    L.mgh_recompose_to_level.argtypes = [vp, vp, C.c_int, vp, vp]
    L.mgh_recompose_linear_to_level.argtypes = [vp, vp, C.c_int, vp, vp]
    L.mgh_quantize_residual_linear.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, C.c_double, u64, vp, vp, vp, vp,
                                               u64, vp, vp]
    L.mgh_dequantize_add_linear.argtypes = [vp, vp, u64, u64, C.c_int, C.c_double, C.c_double, C.c_double, u64, C.c_int,
                                            vp, vp, u64, C.c_int, vp, vp]
    L.mgh_dequantize_recompose_to_level.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, C.c_double,
                                                    u64, C.c_int, vp, vp, u64, C.c_int, vp, vp]
    L.mgh_dequantize_recompose_sym16_to_level.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double,
                                                          C.c_double, u64, vp, vp, u64, C.c_int, vp, vp]
    L.mgh_level_box_from_linear.argtypes = [vp, vp, C.c_int, vp, vp]
    L.mgh_dequantize_recompose_linear_to_level.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, C.c_double,
                                                           u64, C.c_int, vp, vp, u64, C.c_int, vp, vp]
    L.mgh_refine_level.argtypes = [vp, vp, vp, C.c_int, C.c_double, C.c_double, C.c_double, u64, C.c_int, vp, vp, u64,
                                   C.c_int, vp, vp]
    L.mgh_level_nodes.argtypes = [vp, C.c_int, C.c_int, u64p, u64]
    L.mgh_prolong.argtypes = [vp, C.c_int, vp, vp, vp]
    L.mgh_debug_prolong_plan.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    L.mgh_prolong_window.argtypes = [vp, C.c_int, vp, u64p, u64p, vp, vp]
    L.mgh_prolong_window_strided.argtypes = [vp, C.c_int, vp, u64p, u64p, vp, u64p, vp]
    L.mgh_debug_prolong_window_ranges.argtypes = [vp, C.c_int, u64p, u64p, i64p, u64]
    L.mgh_debug_prolong_window_plan.argtypes = [vp, C.c_int, u64p, u64p, C.c_int, C.POINTER(C.c_int)]
    L.mgh_stream_calibrate.argtypes = [C.c_int, vp, vp, vp, u64, C.c_int, C.POINTER(C.c_double), vp]
    L.mgh_compare.argtypes = [C.c_int, C.c_int, u64p, vp, u64p, vp, u64p, C.POINTER(ErrorStats), C.c_int, vp]
    L.mgh_mask_scan.argtypes = [C.c_int, C.c_int, u64p, vp, C.c_int, C.c_double, vp, vp, vp]
    L.mgh_mask_fill.argtypes = [C.c_int, C.c_int, u64p, vp, vp, C.c_double, vp, vp]
    L.mgh_mask_restore.argtypes = [C.c_int, C.c_int, u64p, vp, C.c_double, vp, vp]
    L.mgh_mask_sample_.argtypes = [C.c_int, u64p, vp, u64p, C.POINTER(vp), vp, vp, vp]
    L.mgh_compare_masked_.argtypes = [C.c_int, C.c_int, u64p, vp, u64p, vp, u64p, vp, u64p, u64, C.POINTER(ErrorStats),
                                     C.c_int, vp]
    L.mgh_pwrel_forward_.argtypes = [C.c_int, C.c_int, u64p, vp, C.c_double, vp, vp, vp, vp, vp]
    L.mgh_pwrel_inverse_.argtypes = [C.c_int, C.c_int, u64p, vp, vp, vp, vp]
    L.mgh_pwrel_inverse_sampled_.argtypes = [C.c_int, C.c_int, u64p, vp, vp, u64p, C.POINTER(vp), vp, vp]
    L.mgh_compare_pwrel_.argtypes = [C.c_int, C.c_int, u64p, vp, vp, C.c_double, C.POINTER(PwrelCompare), vp]
    L.mgh_box_scratch_bytes_.restype = C.c_size_t
    L.mgh_box_scratch_bytes_.argtypes = []
    L.mgh_box_residual_.argtypes = [C.c_int, C.c_int, u64p, u64p, u64p, vp, vp, vp, vp, vp]
    L.mgh_box_add_.argtypes = [C.c_int, C.c_int, u64p, u64p, u64p, vp, vp, vp]
    _lib = L
    return L


def _check(rc):
    if rc < 0:
        raise MgardHipError("mgard_hip error %d: %s" % (rc, load_library().mgh_last_error().decode()))
    return rc


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_NP = {FLOAT: np.float32, DOUBLE: np.float64}


def _leading_dims(t):
    """The leading dimensions (mgh_set_ld's convention) that describe the strides of a cuda tensor, or
    None where they cannot (the caller then compares a contiguous copy)."""
    shape, strides = tuple(t.shape), tuple(t.stride())
    D = len(shape)
    ld = list(shape)
    for d in range(D - 1, 0, -1):
        if shape[d - 1] > 1 and strides[d] > 0 and strides[d - 1] % strides[d] == 0:
            ld[d] = strides[d - 1] // strides[d]
    run = 1
    for d in range(D - 1, -1, -1):
        if shape[d] > 1 and strides[d] != run:
            return None
        if d > 0 and ld[d] < shape[d]:
            return None
        run *= ld[d]
    return ld


def compare(a, b, device=None):
    """mgh_compare: ErrorStats of `a` (the reference) against `b`, in one pass on the device. Each of the
    two is a cuda tensor or a NumPy array, float32 or float64 alike and of one shape. A cuda tensor whose
    rows are padded (a slice of a larger allocation: strides that leading dimensions describe) is read in
    place, its padding passed as `ld`; any other layout is compared through a contiguous copy. With a
    NumPy array in the call both are compared dense."""
    import torch
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError("compare: the arrays have different shapes")
    tensors = [x for x in (a, b) if isinstance(x, torch.Tensor)]
    if any(not x.is_cuda for x in tensors):
        raise ValueError("compare: tensors must be cuda tensors (pass host data as NumPy arrays)")
    if device is None:
        device = tensors[0].device.index if tensors else torch.cuda.current_device()
    host = len(tensors) < 2
    keep, ptrs, lds, dts = [], [], [], []
    for x in (a, b):
        if isinstance(x, torch.Tensor):
            ld = None if host else _leading_dims(x)
            if ld is None and not x.is_contiguous():
                x = x.contiguous()
            dts.append({torch.float32: FLOAT, torch.float64: DOUBLE}.get(x.dtype))
            ptrs.append(C.c_void_p(x.data_ptr()))
        else:
            x = np.ascontiguousarray(x)
            ld = None
            dts.append({np.dtype(np.float32): FLOAT, np.dtype(np.float64): DOUBLE}.get(x.dtype))
            ptrs.append(C.c_void_p(x.ctypes.data))
        keep.append(x)
        lds.append(None if ld is None or list(ld) == list(x.shape) else (C.c_uint64 * len(ld))(*ld))
    if dts[0] is None or dts[0] != dts[1]:
        raise ValueError("compare: float32 or float64 arrays of one type expected")
    shape = tuple(int(e) for e in a.shape)
    out = ErrorStats()
    with torch.cuda.device(device):
        stream = _stream()
    _check(load_library().mgh_compare(len(shape), dts[0], (C.c_uint64 * max(len(shape), 1))(*shape), ptrs[0], lds[0],
                                      ptrs[1], lds[1], C.byref(out), int(device), stream))
    return out


# ---- missing-value masks (mgh_mask_*) ---------------------------------------------------------------------
MASK_NONFINITE, MASK_VALUE = 1, 2


class MaskStats(C.Structure):
    """mgh_mask_stats: element count, masked count, and the extremes of the valid elements (0, 0 when none)."""
    _fields_ = [("n", C.c_uint64), ("n_masked", C.c_uint64), ("vmin", C.c_double), ("vmax", C.c_double)]

    def __repr__(self):
        return "MaskStats(n=%d, n_masked=%d, vmin=%r, vmax=%r)" % (self.n, self.n_masked, self.vmin, self.vmax)


def _mask_array(data, what):
    """(dtype code, shape array, D) of a contiguous float32 / float64 cuda tensor."""
    import torch
    if not (isinstance(data, torch.Tensor) and data.is_cuda and data.is_contiguous() and
            data.dtype in (torch.float32, torch.float64)):
        raise ValueError("%s: a contiguous float32 / float64 cuda tensor expected" % what)
    shape = tuple(int(e) for e in data.shape) or (1,)
    return FLOAT if data.dtype == torch.float32 else DOUBLE, (C.c_uint64 * len(shape))(*shape), len(shape)


def _mask_words(words, n, what):
    import torch
    if not (isinstance(words, torch.Tensor) and words.is_cuda and words.is_contiguous() and words.dtype == torch.int64 and
            words.numel() == (n + 63) // 64):
        raise ValueError("%s: `words` must be the int64 cuda tensor of ceil(n / 64) words mask_scan returns" % what)
    return C.c_void_p(words.data_ptr())


def mask_flags(nonfinite=True, fill_value=None):
    return (MASK_NONFINITE if nonfinite else 0) | (MASK_VALUE if fill_value is not None else 0)


def mask_scan(data, nonfinite=True, fill_value=None):
    """mgh_mask_scan of a cuda tensor: (words, stats). words: int64 cuda tensor of ceil(n / 64) words, bit i % 64 of
    word i / 64 set when flat element i is NaN / +-Inf (`nonfinite`) or equals `fill_value` in the data's type;
    stats: MaskStats over the valid elements."""
    import torch
    dt, shp, D = _mask_array(data, "mask_scan")
    n = data.numel()
    words = torch.empty((n + 63) // 64, dtype=torch.int64, device=data.device)
    d_stats = torch.empty(4, dtype=torch.int64, device=data.device)
    with torch.cuda.device(data.device):
        _check(load_library().mgh_mask_scan(D, dt, shp, C.c_void_p(data.data_ptr()), mask_flags(nonfinite, fill_value),
                                            0.0 if fill_value is None else float(fill_value),
                                            C.c_void_p(words.data_ptr()), C.c_void_p(d_stats.data_ptr()), _stream()))
    return words, MaskStats.from_buffer_copy(d_stats.cpu().numpy().tobytes())


def mask_fill(data, words, c, out=None):
    """mgh_mask_fill: `data` with every masked element replaced by the nearest valid element below it in its
    segment of 1024 of its row, else the nearest above, else `c` (in the data's type). out may be data."""
    import torch
    dt, shp, D = _mask_array(data, "mask_fill")
    if out is None:
        out = torch.empty_like(data)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.dtype == data.dtype and
            out.shape == data.shape):
        raise ValueError("mask_fill: `out` must be a contiguous cuda tensor of the data's shape and type")
    with torch.cuda.device(data.device):
        _check(load_library().mgh_mask_fill(D, dt, shp, C.c_void_p(data.data_ptr()), _mask_words(words, data.numel(), "mask_fill"),
                                            float(c), C.c_void_p(out.data_ptr()), _stream()))
    return out


def mask_restore(data, words, value):
    """mgh_mask_restore, in place: `value` (in the data's type; may be NaN) at every masked position of `data`."""
    import torch
    dt, shp, D = _mask_array(data, "mask_restore")
    with torch.cuda.device(data.device):
        _check(load_library().mgh_mask_restore(D, dt, shp, _mask_words(words, data.numel(), "mask_restore"), float(value),
                                               C.c_void_p(data.data_ptr()), _stream()))
    return data


# ---- pointwise relative error bound (mgh_pwrel_forward_ / mgh_pwrel_inverse_ / mgh_compare_pwrel_) -----------------
def pwrel_forward(data, abs_floor=0.0, out=None):
    """mgh_pwrel_forward_ of a cuda tensor: (y, mask_words, flag_words, stats). y = (T)log2((double)|x|) at valid
    positions and 0 at the others (`out` may be `data`: in place); mask bit: NaN / +-Inf or |x| < max(abs_floor,
    smallest normal); flag bit: NaN / +-Inf, or a negative valid element; stats: PwrelStats."""
    import torch
    dt, shp, D = _mask_array(data, "pwrel_forward")
    n = data.numel()
    if out is None:
        out = torch.empty_like(data)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.dtype == data.dtype and
            out.shape == data.shape):
        raise ValueError("pwrel_forward: `out` must be a contiguous cuda tensor of the data's shape and type")
    mwords = torch.empty((n + 63) // 64, dtype=torch.int64, device=data.device)
    fwords = torch.empty((n + 63) // 64, dtype=torch.int64, device=data.device)
    d_stats = torch.empty(6, dtype=torch.int64, device=data.device)
    with torch.cuda.device(data.device):
        _check(load_library().mgh_pwrel_forward_(D, dt, shp, C.c_void_p(data.data_ptr()), float(abs_floor),
                                                 C.c_void_p(out.data_ptr()), C.c_void_p(mwords.data_ptr()),
                                                 C.c_void_p(fwords.data_ptr()), C.c_void_p(d_stats.data_ptr()), _stream()))
    return out, mwords, fwords, PwrelStats.from_buffer_copy(d_stats.cpu().numpy().tobytes())


def pwrel_inverse(data, mask_words, flag_words):
    """mgh_pwrel_inverse_, in place over y': quiet NaN where mask and flag are set, +0.0 where only the mask is, else
    +-exp2(y') (the flag bit is the sign) with the magnitude clamped to [smallest normal, largest finite]."""
    import torch
    dt, shp, D = _mask_array(data, "pwrel_inverse")
    with torch.cuda.device(data.device):
        _check(load_library().mgh_pwrel_inverse_(D, dt, shp, _mask_words(mask_words, data.numel(), "pwrel_inverse"),
                                                 _mask_words(flag_words, data.numel(), "pwrel_inverse"),
                                                 C.c_void_p(data.data_ptr()), _stream()))
    return data


def compare_pwrel(original, reconstructed, abs_floor=0.0):
    """mgh_compare_pwrel_: PwrelCompare of the cuda tensor `original` against `reconstructed` (same shape and type)."""
    import torch
    dt, shp, D = _mask_array(original, "compare_pwrel")
    if not (isinstance(reconstructed, torch.Tensor) and reconstructed.is_cuda and reconstructed.is_contiguous() and
            reconstructed.dtype == original.dtype and reconstructed.shape == original.shape and
            reconstructed.device == original.device):
        raise ValueError("compare_pwrel: `reconstructed` must be a contiguous cuda tensor of the original's shape and type")
    out = PwrelCompare()
    with torch.cuda.device(original.device):
        _check(load_library().mgh_compare_pwrel_(D, dt, shp, C.c_void_p(original.data_ptr()),
                                                 C.c_void_p(reconstructed.data_ptr()), float(abs_floor), C.byref(out), _stream()))
    return out


# ---- region of interest (mgh_box_residual_ / mgh_box_add_) -----------------------------------------------------------
class BoxStats(C.Structure):
    """What mgh_box_residual_ reduces over a box: max |r| and max |x| over the finite values, and the number of
    positions whose x or r is not finite."""
    _fields_ = [("max_abs_r", C.c_double), ("max_abs_x", C.c_double), ("n_nonfinite", C.c_uint64), ("pad", C.c_uint64)]

    def __repr__(self):
        return "BoxStats(max_abs_r=%r, max_abs_x=%r, n_nonfinite=%d)" % (self.max_abs_r, self.max_abs_x, self.n_nonfinite)


def _box_args(data, lo, ext, what):
    dt, shp, D = _mask_array(data, what)
    lo, ext = tuple(int(v) for v in lo), tuple(int(v) for v in ext)
    if len(lo) != D or len(ext) != D:
        raise ValueError("%s: `lo` and `ext` must have the data's number of dimensions" % what)
    return dt, shp, D, (C.c_uint64 * D)(*lo), (C.c_uint64 * D)(*ext), ext


def box_residual(x, b, lo, ext, sync=True):
    """mgh_box_residual_ of two cuda tensors of the same shape and type: (r, stats). r: the dense tensor of `ext`,
    fl(x[box] - b[box]) for the box lo .. lo + ext; stats: BoxStats. sync=False: stats is the cuda int64 tensor the
    kernel leaves it in (four words: the struct's), and nothing waits for the stream."""
    import torch
    dt, shp, D, clo, cext, ext = _box_args(x, lo, ext, "box_residual")
    if not (isinstance(b, torch.Tensor) and b.is_cuda and b.is_contiguous() and b.dtype == x.dtype and b.shape == x.shape and
            b.device == x.device):
        raise ValueError("box_residual: `b` must be a contiguous cuda tensor of x's shape and type")
    with torch.cuda.device(x.device):
        L = load_library()
        r = torch.empty(ext, dtype=x.dtype, device=x.device)
        scratch = torch.empty(int(L.mgh_box_scratch_bytes_()) // 8, dtype=torch.int64, device=x.device)
        _check(L.mgh_box_residual_(D, dt, shp, clo, cext, C.c_void_p(x.data_ptr()), C.c_void_p(b.data_ptr()),
                                   C.c_void_p(r.data_ptr()), C.c_void_p(scratch.data_ptr()), _stream()))
    if not sync:
        return r, scratch[:4]
    return r, BoxStats.from_buffer_copy(scratch[:4].cpu().numpy().tobytes())


def box_add(data, r, lo):
    """mgh_box_add_, in place: data[box] = fl(data[box] + r) for the box lo .. lo + r.shape; nothing else is touched."""
    import torch
    if not (isinstance(r, torch.Tensor) and r.is_cuda and r.is_contiguous() and isinstance(data, torch.Tensor) and
            r.dtype == data.dtype and r.device == data.device):
        raise ValueError("box_add: `r` must be a contiguous cuda tensor of the data's type")
    dt, shp, D, clo, cext, ext = _box_args(data, lo, tuple(r.shape) or (1,), "box_add")
    with torch.cuda.device(data.device):
        _check(load_library().mgh_box_add_(D, dt, shp, clo, cext, C.c_void_p(r.data_ptr()), C.c_void_p(data.data_ptr()),
                                           _stream()))
    return data


def _sample_lists(idx_lists, shape, out_shape, device, what):
    """(keepalive, pointers, lengths) of one index list per dimension as mgh_mask_sample_ takes them: an int sequence,
    a cuda int32 / uint32 tensor, or None for the identity 0 .. out_shape[d] - 1."""
    import torch
    if len(idx_lists) != len(shape):
        raise ValueError("%s: one index list (or None) per dimension" % what)
    keep, ptrs, lens = [], [], []
    for d, lst in enumerate(idx_lists):
        if lst is None:
            ptrs.append(None)
            lens.append(shape[d] if out_shape is None else int(out_shape[d]))
            continue
        if isinstance(lst, torch.Tensor):
            if not (lst.is_cuda and lst.is_contiguous() and lst.dim() == 1 and lst.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))):
                raise ValueError("%s: an index tensor must be a contiguous 1-D cuda int32 / uint32 tensor" % what)
            t = lst
        else:
            a = np.asarray(lst, dtype=np.int64).reshape(-1)
            if a.size and (a.min() < 0 or a.max() > 0xffffffff):
                raise ValueError("%s: index outside 0 .. 2^32 - 1" % what)
            t = torch.from_numpy(a.astype(np.uint32).view(np.int32)).to(device)
        keep.append(t)
        ptrs.append(t.data_ptr())
        lens.append(int(t.numel()))
    if out_shape is not None and tuple(int(e) for e in out_shape) != tuple(lens):
        raise ValueError("%s: out_shape disagrees with the lengths of the lists" % what)
    return keep, ptrs, lens


def mask_sample(words, shape, idx_lists, out_shape=None):
    """mgh_mask_sample_: (out_words, count) -- the packed mask of the dense array whose element (i_0 ...) is element
    (idx_0[i_0] ...) of the array of `shape` that `words` is the packed mask of. idx_lists: one entry per dimension,
    an int sequence, a cuda int32 / uint32 tensor, or None for the identity 0 .. out_shape[d] - 1 (out_shape is then
    needed for that dimension; by default it is the lists' lengths, and shape[d] for None). An entry >= shape[d]
    reads nothing and gives 0. count: the number of set output bits."""
    import torch
    shape = tuple(int(e) for e in shape)
    D = len(shape)
    keep, ptrs, lens = _sample_lists(idx_lists, shape, out_shape, words.device, "mask_sample")
    n = int(np.prod(shape, dtype=np.int64))
    wp = _mask_words(words, n, "mask_sample")
    n_out = int(np.prod(lens, dtype=np.int64))
    out_words = torch.empty((n_out + 63) // 64, dtype=torch.int64, device=words.device)
    d_count = torch.empty(1, dtype=torch.int64, device=words.device)
    with torch.cuda.device(words.device):
        _check(load_library().mgh_mask_sample_(D, (C.c_uint64 * D)(*shape), wp, (C.c_uint64 * D)(*lens),
                                              (C.c_void_p * D)(*ptrs), C.c_void_p(out_words.data_ptr()),
                                              C.c_void_p(d_count.data_ptr()), _stream()))
    del keep
    return out_words, int(d_count.item())


def pwrel_inverse_sampled(data, mask_words, flag_words, shape, idx_lists):
    """mgh_pwrel_inverse_sampled_, in place over y' of a VIEW: pwrel_inverse with the two bits of element (i_0 ...) of
    `data` taken from element (idx_0[i_0] ...) of the array of `shape` that mask_words / flag_words are the packed maps
    of -- pwrel_inverse(data, mask_sample(mask_words, ...)[0], mask_sample(flag_words, ...)[0]) in one pass. idx_lists
    as for mask_sample, with the data's shape as out_shape; an entry >= shape[d] reads nothing and gives a valid,
    positive element."""
    import torch
    dt, oshp, D = _mask_array(data, "pwrel_inverse_sampled")
    shape = tuple(int(e) for e in shape)
    if len(shape) != D:
        raise ValueError("pwrel_inverse_sampled: `shape` must have the data's number of dimensions")
    keep, ptrs, lens = _sample_lists(idx_lists, shape, tuple(int(e) for e in oshp), data.device, "pwrel_inverse_sampled")
    n = int(np.prod(shape, dtype=np.int64))
    with torch.cuda.device(data.device):
        _check(load_library().mgh_pwrel_inverse_sampled_(D, dt, (C.c_uint64 * D)(*shape),
                                                         _mask_words(mask_words, n, "pwrel_inverse_sampled"),
                                                         _mask_words(flag_words, n, "pwrel_inverse_sampled"), oshp,
                                                         (C.c_void_p * D)(*ptrs), C.c_void_p(data.data_ptr()), _stream()))
    del keep
    return data


def compare_masked(a, b, words, ld_m=None, bit0=0):
    """mgh_compare_masked_: ErrorStats of the cuda tensor `a` (the reference) against `b` over the positions whose
    bit of the packed mask `words` (int64 cuda tensor) is NOT set; `n` counts those positions. Element (i_0 ...) has
    bit bit0 + its offset in an array of leading dimensions ld_m (None: dense, the arrays' shape) -- a box of a
    larger array is held against that array's mask with ld_m = the array's shape and bit0 = the flat index of the
    box's first element. Tensors with padded rows are read in place like compare's; other layouts through a copy."""
    import torch
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError("compare_masked: the arrays have different shapes")
    if not all(isinstance(x, torch.Tensor) and x.is_cuda for x in (a, b, words)):
        raise ValueError("compare_masked: a, b and words must be cuda tensors")
    if not (words.is_contiguous() and words.dtype == torch.int64):
        raise ValueError("compare_masked: `words` must be a contiguous int64 cuda tensor")
    keep, ptrs, lds, dts = [], [], [], []
    for x in (a, b):
        ld = _leading_dims(x)
        if ld is None and not x.is_contiguous():
            x = x.contiguous()
        dts.append({torch.float32: FLOAT, torch.float64: DOUBLE}.get(x.dtype))
        ptrs.append(C.c_void_p(x.data_ptr()))
        keep.append(x)
        lds.append(None if ld is None or list(ld) == list(x.shape) else (C.c_uint64 * len(ld))(*ld))
    if dts[0] is None or dts[0] != dts[1]:
        raise ValueError("compare_masked: float32 or float64 arrays of one type expected")
    shape = tuple(int(e) for e in a.shape)
    D = len(shape)
    ldm = None
    if ld_m is not None:
        if len(ld_m) != D:
            raise ValueError("compare_masked: ld_m needs one entry per dimension")
        ldm = (C.c_uint64 * D)(*[int(e) for e in ld_m])
    # the last bit the view reaches must lie inside `words`
    lead = [int(e) for e in ld_m] if ld_m is not None else list(shape)
    last, run = int(bit0), 1
    for d in range(D - 1, -1, -1):
        last += (shape[d] - 1) * run
        run *= lead[d]
    if int(bit0) < 0 or (a.numel() and last >= 64 * words.numel()):
        raise ValueError("compare_masked: the view of the mask leaves `words`")
    out = ErrorStats()
    device = a.device.index
    with torch.cuda.device(device):
        stream = _stream()
    _check(load_library().mgh_compare_masked_(D, dts[0], (C.c_uint64 * max(D, 1))(*shape), ptrs[0], lds[0], ptrs[1], lds[1],
                                             C.c_void_p(words.data_ptr()), ldm, int(bit0), C.byref(out), int(device), stream))
    del keep
    return out


class Hierarchy:
    """Host mirror of mgard_x::Hierarchy<D,T,HIP> + the stages of mgard_x::Compressor<D,T,HIP>
    (reference include/mgard-x/CompressionLowLevel/Compressor.h:39-78): norm, decompose,
    quantize, dequantize, recompose on torch device tensors."""

    def __init__(self, shape, dtype="float32", coords=None, normalize_coordinates=True,
                 max_level=None, device=0):
        import torch
        L = load_library()
        if not torch.cuda.is_available():
            raise MgardHipError("no HIP device visible: mgard_amd has no CPU fallback")
        self.shape = tuple(int(s) for s in shape)
        self.D = len(self.shape)
        self.np_dtype = np.dtype(dtype)
        self.dtype = {np.dtype(np.float32): FLOAT, np.dtype(np.float64): DOUBLE}[self.np_dtype]
        self.torch_dtype = torch.float32 if self.dtype == FLOAT else torch.float64
        self.device = int(device)
        shp = (C.c_uint64 * self.D)(*self.shape)
        cptr = None
        if coords is not None:
            self._coords = [np.ascontiguousarray(c, dtype=self.np_dtype) for c in coords]
            cptr = (C.c_void_p * self.D)(*[c.ctypes.data for c in self._coords])
        h = C.c_void_p()
        _check(L.mgh_hierarchy_create(C.byref(h), self.D, shp, self.dtype, cptr,
                                      int(normalize_coordinates),
                                      2**64 - 1 if max_level is None else int(max_level),
                                      self.device))
        self._h = h
        self._ld = {LD_IN: None, LD_OUT: None}
        self.l_target = L.mgh_l_target(h)
        self.total = int(L.mgh_total_num_elems(h))

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            try:
                _lib.mgh_hierarchy_destroy(self._h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None

    __del__ = close

    # ---- introspection ----
    def level_shape(self, l):
        out = (C.c_uint64 * self.D)()
        _check(load_library().mgh_level_shape(self._h, l, out))
        return tuple(int(x) for x in out)

    def level_nodes(self, level, dim):
        """mgh_level_nodes: index in the finest grid of every node of `level` along `dim`."""
        n = self.shape[dim] if 0 <= dim < self.D else 1
        out = (C.c_uint64 * n)()
        k = _check(load_library().mgh_level_nodes(self._h, int(level), int(dim), out, n))
        return np.array(out[:k], dtype=np.int64)

    def device_bytes(self):
        return int(load_library().mgh_device_bytes(self._h))

    def table(self, kind, level, dim):
        kinds = {"dist": 0, "ratio": 1, "am": 2, "bm": 3, "marks": 4}
        n = max(self.shape) + 1
        buf = np.zeros(n, dtype=np.int32 if kind == "marks" else self.np_dtype)
        k = _check(load_library().mgh_hierarchy_table(self._h, kinds[kind], level, dim,
                                                      buf.ctypes.data, n))
        return buf[:k].copy()

    # ---- stages ----
    def _chk(self, t, dtype=None):
        import torch
        ok = {self.total}
        if dtype is None:  # (a T array may be a pitched allocation: mgh_set_ld)
            for ld in self._ld.values():
                if ld is not None:
                    n = self.shape[0]
                    for x in ld[1:]:
                        n *= x
                    ok.add(n)
        assert t.is_cuda and t.is_contiguous() and t.numel() in ok, "bad tensor"
        assert t.dtype == (dtype or self.torch_dtype), "bad dtype"
        assert t.device.index == self.device
        return C.c_void_p(t.data_ptr())

    def norm(self, data, s=INF):
        out = C.c_double()
        _check(load_library().mgh_norm(self._h, self._chk(data), s, C.byref(out), _stream()))
        return out.value

    def _new_out(self, device):
        """A T array for the calls to write: dense, or the pitched allocation LD_OUT describes."""
        import torch
        ld = self._ld[LD_OUT]
        shape = self.shape if ld is None else (self.shape[0],) + tuple(ld[1:])
        return torch.empty(shape, dtype=self.torch_dtype, device=device)

    def decompose(self, data, out=None):
        out = self._new_out(data.device) if out is None else out
        _check(load_library().mgh_decompose(self._h, self._chk(data), self._chk(out), _stream()))
        return out

    def _level_out(self, level, out, device):
        """The dense array of level_shape(level) the *_to_level calls write (LD_OUT does not apply)."""
        import torch
        if out is None:
            shape = self.level_shape(level)  # (raises on a level outside 0 .. l_target)
            return torch.empty(shape, dtype=self.torch_dtype, device=device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == self.torch_dtype, "bad tensor"
        assert out.device.index == self.device
        if 0 <= level <= self.l_target:
            assert out.numel() == int(np.prod(self.level_shape(level))), "bad tensor"
        return out

    def recompose(self, coeff, out=None, level=None):
        """level = None: the full array. Else mgh_recompose_to_level: the nodal values of that level
        of the hierarchy (0 = coarsest), a dense array of level_shape(level)."""
        if level is not None:
            out = self._level_out(level, out, coeff.device)
            _check(load_library().mgh_recompose_to_level(self._h, self._chk(coeff), int(level),
                                                         C.c_void_p(out.data_ptr()), _stream()))
            return out
        out = self._new_out(coeff.device) if out is None else out
        _check(load_library().mgh_recompose(self._h, self._chk(coeff), self._chk(out), _stream()))
        return out

    def _outlier_bufs(self, cap):
        import torch
        dev = torch.device("cuda", self.device)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        idx = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        val = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        return cnt, idx, val

    def quantize(self, coeff, ebtype, tol, s, norm, dict_size=8192, prep_huffman=True,
                 outlier_cap=None, out=None):
        """Returns (q int64 tensor, outlier_idx, outlier_val, outlier_count)."""
        import torch
        cap = self.total if outlier_cap is None else int(outlier_cap)
        q = torch.empty(self.shape, dtype=torch.int64, device=coeff.device) if out is None else out
        cnt, idx, val = self._outlier_bufs(cap)
        _check(load_library().mgh_quantize(
            self._h, self._chk(coeff), ebtype, tol, s, norm, dict_size, int(prep_huffman),
            self._chk(q, torch.int64), C.c_void_p(cnt.data_ptr()), C.c_void_p(idx.data_ptr()),
            C.c_void_p(val.data_ptr()), cap, _stream()))
        n = int(cnt.item())
        k = min(n, cap)
        return q, idx[:k], val[:k], n

    def dequantize(self, q, ebtype, tol, s, norm, dict_size=8192, prep_huffman=True,
                   outlier_idx=None, outlier_val=None, out=None):
        import torch
        out = self._new_out(q.device) if out is None else out
        n = 0 if outlier_idx is None else int(outlier_idx.numel())
        _check(load_library().mgh_dequantize(
            self._h, self._chk(q, torch.int64), ebtype, tol, s, norm, dict_size, int(prep_huffman),
            C.c_void_p(outlier_idx.data_ptr() if n else 0),
            C.c_void_p(outlier_val.data_ptr() if n else 0), n, self._chk(out), _stream()))
        return out

    def norm_device(self, data, s=INF, out=None):
        """Asynchronous norm: returns a 1-element device tensor of the hierarchy's dtype."""
        import torch
        out = torch.empty(1, dtype=self.torch_dtype, device=data.device) if out is None else out
        _check(load_library().mgh_norm_device(self._h, self._chk(data), s,
                                              C.c_void_p(out.data_ptr()), _stream()))
        return out

    def decompose_quantize_dn(self, data, ebtype, tol, s, d_norm, num_subdomains, bufs,
                              dict_size=8192, prep_huffman=True):
        """Fused hot path with a device-resident GLOBAL norm (decomposed domain); fully async."""
        import torch
        q, cnt, idx, val = bufs
        _check(load_library().mgh_decompose_quantize_dn(
            self._h, self._chk(data), ebtype, tol, s, C.c_void_p(d_norm.data_ptr()),
            int(num_subdomains), dict_size, int(prep_huffman), self._chk(q, torch.int64),
            C.c_void_p(cnt.data_ptr()), C.c_void_p(idx.data_ptr()), C.c_void_p(val.data_ptr()),
            int(idx.numel()), _stream()))
        return q, idx, val, cnt

    def decompose_quantize(self, data, ebtype, tol, s, norm=0.0, dict_size=8192,
                           prep_huffman=True, outlier_cap=None, bufs=None, coeff_out=None,
                           want_norm=True):
        """The fused hot path (Compressor::Compress up to the lossless stage). Returns
        (q, outlier_idx, outlier_val, outlier_count, norm). `bufs` = (q, cnt, idx, val) lets a
        caller reuse output buffers; then no host sync happens and outlier_count is the device
        tensor."""
        import torch
        cap = self.total if outlier_cap is None else int(outlier_cap)
        if bufs is None:
            q = torch.empty(self.shape, dtype=torch.int64, device=data.device)
            cnt, idx, val = self._outlier_bufs(cap)
        else:
            q, cnt, idx, val = bufs
            cap = int(idx.numel())
        nout = C.c_double()
        _check(load_library().mgh_decompose_quantize(
            self._h, self._chk(data), ebtype, tol, s, norm,
            C.byref(nout) if want_norm else None, dict_size,
            int(prep_huffman), self._chk(q, torch.int64), C.c_void_p(cnt.data_ptr()),
            C.c_void_p(idx.data_ptr()), C.c_void_p(val.data_ptr()), cap,
            C.c_void_p(coeff_out.data_ptr()) if coeff_out is not None else None, _stream()))
        if bufs is not None:
            return q, idx, val, cnt, nout.value
        n = int(cnt.item())
        k = min(n, cap)
        return q, idx[:k], val[:k], n, nout.value

    def sym16_supported(self):
        return bool(load_library().mgh_sym16_supported(self._h))

    def set_ld(self, which, ld):
        """mgh_set_ld: leading dimensions (len D, or None = dense) of the T arrays the calls read
        (which = LD_IN) or write (LD_OUT). Arrays are then passed as tensors whose STORAGE is the
        pitched allocation (any shape with enough elements)."""
        arr = None if ld is None else (C.c_uint64 * len(ld))(*[int(x) for x in ld])
        _check(load_library().mgh_set_ld(self._h, int(which), arr))
        self._ld[which] = None if ld is None else tuple(int(x) for x in ld)

    def norm_stream(self, data, s, parts):
        """mgh_norm_stream_begin + one mgh_norm_stream_add per part of the (flattened) array: the next
        fused decompose_quantize* call with a REL bound and norm = 0 takes the accumulated norm.
        `parts`: element counts that add up to the array."""
        flat = data.reshape(-1)
        assert sum(parts) == flat.numel()
        L = load_library()
        _check(L.mgh_norm_stream_begin(self._h, _stream()))
        off = 0
        for k, cnt in enumerate(parts):
            _check(L.mgh_norm_stream_add(self._h, C.c_void_p(flat.data_ptr() + off * flat.element_size()),
                                         int(cnt), s, int(k + 1 < len(parts)), _stream()))
            off += cnt

    def norm_stream_end(self, s):
        """mgh_norm_stream_end: the norm accumulated by norm_stream(), instead of the fused call that
        would have taken it."""
        out = C.c_double()
        _check(load_library().mgh_norm_stream_end(self._h, s, C.byref(out), _stream()))
        return out.value

    def quantize_histograms(self, coeff, tols, ebtype, s, norm, dict_size=8192):
        """mgh_quantize_histograms: (freq int32 tensor [len(tols), dict_size], outliers int64 tensor
        [len(tols)]) -- per tolerance the histogram of the symbols quantize(prep_huffman=True) would
        store (outliers in bin 0) and its outlier count, from one read of `coeff`."""
        import torch
        tols = [float(t) for t in tols]
        k = len(tols)
        freq = torch.empty((k, int(dict_size)), dtype=torch.int32, device=coeff.device)
        outl = torch.empty(k, dtype=torch.int64, device=coeff.device)
        _check(load_library().mgh_quantize_histograms(
            self._h, self._chk(coeff), ebtype, k, (C.c_double * k)(*tols), s, norm, int(dict_size),
            C.c_void_p(freq.data_ptr()), C.c_void_p(outl.data_ptr()), _stream()))
        return freq, outl

    def quantize_roundtrip(self, coeff, error_bound_type, tol, s, norm, out=None):
        """mgh_quantize_roundtrip: what dequantize() gives for the integers quantize() makes from `coeff`,
        bit for bit, in one pass and without the integers. `out`: a dense tensor of the hierarchy's shape and
        type (LD_OUT does not apply); it may be `coeff` itself (in place)."""
        import torch
        if out is None:
            out = torch.empty(self.shape, dtype=self.torch_dtype, device=coeff.device)
        assert out.is_cuda and out.is_contiguous() and out.numel() == self.total, "bad tensor"
        assert out.dtype == self.torch_dtype and out.device.index == self.device, "bad tensor"
        _check(load_library().mgh_quantize_roundtrip(
            self._h, self._chk(coeff), int(error_bound_type), tol, s, norm, C.c_void_p(out.data_ptr()), _stream()))
        return out

    def quantize_symbols(self, coeff, ebtype, tol, s, norm, dict_size=8192, histogram=True, outlier_cap=None):
        """mgh_quantize_symbols: (symbols uint16, freq int32 [dict_size] or None, outlier_idx, outlier_val)
        -- what quantize(prep_huffman=True) stores, as 16-bit symbols with 0 at the outliers' positions, the
        outlier list (its length is the count; at most `outlier_cap` pairs, the whole array by default) and,
        with `histogram`, the histogram of the stored symbols, all from one pass over `coeff`."""
        import torch
        cap = self.total if outlier_cap is None else int(outlier_cap)
        sym = torch.empty(self.shape, dtype=torch.uint16, device=coeff.device)
        freq = torch.zeros(int(dict_size), dtype=torch.int32, device=coeff.device) if histogram else None
        cnt, idx, val = self._outlier_bufs(cap)
        _check(load_library().mgh_quantize_symbols(
            self._h, self._chk(coeff), int(ebtype), tol, s, norm, int(dict_size), C.c_void_p(sym.data_ptr()),
            C.c_void_p(freq.data_ptr()) if histogram else None, C.c_void_p(cnt.data_ptr()),
            C.c_void_p(idx.data_ptr()), C.c_void_p(val.data_ptr()), cap, _stream()))
        k = min(int(cnt.item()), cap)
        return sym, freq, idx[:k], val[:k]

    def quantize_symbols_residual(self, coeff, ebtype, tol, s, norm, dict_size=8192, histogram=True, outlier_cap=None,
                                  out=None):
        """mgh_quantize_symbols_residual: quantize_symbols' (symbols, freq or None, outlier_idx, outlier_val) and,
        fifth, the residual `coeff - dequantize(those integers)`, bit for bit, from the same pass -- what the
        next precision layer quantizes. `out`: a dense tensor of the hierarchy's shape and type for the
        residual; it may be `coeff` itself (in place)."""
        import torch
        cap = self.total if outlier_cap is None else int(outlier_cap)
        sym = torch.empty(self.shape, dtype=torch.uint16, device=coeff.device)
        freq = torch.zeros(int(dict_size), dtype=torch.int32, device=coeff.device) if histogram else None
        if out is None:
            out = torch.empty(self.shape, dtype=self.torch_dtype, device=coeff.device)
        assert out.is_cuda and out.is_contiguous() and out.numel() == self.total, "bad tensor"
        assert out.dtype == self.torch_dtype and out.device.index == self.device, "bad tensor"
        cnt, idx, val = self._outlier_bufs(cap)
        _check(load_library().mgh_quantize_symbols_residual(
            self._h, self._chk(coeff), int(ebtype), tol, s, norm, int(dict_size), C.c_void_p(sym.data_ptr()),
            C.c_void_p(freq.data_ptr()) if histogram else None, C.c_void_p(cnt.data_ptr()),
            C.c_void_p(idx.data_ptr()), C.c_void_p(val.data_ptr()), cap, C.c_void_p(out.data_ptr()), _stream()))
        k = min(int(cnt.item()), cap)
        return sym, freq, idx[:k], val[:k], out

    def dequantize_add(self, q, ebtype, tol, s, norm, dict_size=8192, prep_huffman=True, outlier_idx=None,
                       outlier_val=None, acc=None):
        """mgh_dequantize_add: acc = None -- a new tensor that holds dequantize(q, ...), bit for bit; else
        `acc` (dense, the hierarchy's shape and type) with that value added to it in place. Like dequantize
        the call writes the outliers back into `q`."""
        import torch
        first = acc is None
        if first:
            acc = torch.empty(self.shape, dtype=self.torch_dtype, device=q.device)
        assert acc.is_cuda and acc.is_contiguous() and acc.numel() == self.total, "bad tensor"
        assert acc.dtype == self.torch_dtype and acc.device.index == self.device, "bad tensor"
        n = 0 if outlier_idx is None else int(outlier_idx.numel())
        _check(load_library().mgh_dequantize_add(
            self._h, self._chk(q, torch.int64), int(ebtype), tol, s, norm, int(dict_size), int(prep_huffman),
            C.c_void_p(outlier_idx.data_ptr() if n else 0), C.c_void_p(outlier_val.data_ptr() if n else 0), n,
            int(first), C.c_void_p(acc.data_ptr()), _stream()))
        return acc

    def quantize_residual_linear(self, coeff, ebtype, tol, s, norm, dict_size=8192, outlier_cap=None, out=None):
        """mgh_quantize_residual_linear: (integers, outlier_idx, outlier_val, residual) -- the level-linearised
        integers (flat int64) and the outlier pairs at linearised positions that quantize(prep_huffman=True) +
        level_linearize(outlier_idx=...) give, and quantize_symbols_residual's residual in array order. `out`: a
        dense tensor for the residual; it may be `coeff` itself."""
        import torch
        cap = self.total if outlier_cap is None else int(outlier_cap)
        lin = torch.empty(self.total, dtype=torch.int64, device=coeff.device)
        if out is None:
            out = torch.empty(self.shape, dtype=self.torch_dtype, device=coeff.device)
        assert out.is_cuda and out.is_contiguous() and out.numel() == self.total, "bad tensor"
        assert out.dtype == self.torch_dtype and out.device.index == self.device, "bad tensor"
        cnt, idx, val = self._outlier_bufs(cap)
        _check(load_library().mgh_quantize_residual_linear(
            self._h, self._chk(coeff), int(ebtype), tol, s, norm, int(dict_size), C.c_void_p(lin.data_ptr()),
            C.c_void_p(cnt.data_ptr()), C.c_void_p(idx.data_ptr()), C.c_void_p(val.data_ptr()), cap,
            C.c_void_p(out.data_ptr()), _stream()))
        k = min(int(cnt.item()), cap)
        return lin, idx[:k], val[:k], out

    def dequantize_add_linear(self, window, first, acc, ebtype, tol, s, norm, dict_size=8192, prep_huffman=True,
                              outlier_idx=None, outlier_val=None, store=False):
        """mgh_dequantize_add_linear: `window` (contiguous int64, any view) holds the integers [first, first +
        window.numel()) of the level-linearised array; `acc` (flat, total elements of the hierarchy's type) is the
        whole accumulator in that order. Inside the window acc is stored (store=True) or added to; outside it
        nothing is touched. The outliers of the window are written into `window`. Returns acc."""
        import torch
        assert window.is_cuda and window.dtype == torch.int64 and window.is_contiguous(), "bad tensor"
        assert acc.is_cuda and acc.is_contiguous() and acc.numel() == self.total, "bad tensor"
        assert acc.dtype == self.torch_dtype and acc.device.index == self.device, "bad tensor"
        n = 0 if outlier_idx is None else int(outlier_idx.numel())
        _check(load_library().mgh_dequantize_add_linear(
            self._h, C.c_void_p(window.data_ptr()), int(first), int(window.numel()), int(ebtype), tol, s, norm,
            int(dict_size), int(prep_huffman), C.c_void_p(outlier_idx.data_ptr() if n else 0),
            C.c_void_p(outlier_val.data_ptr() if n else 0), n, int(store), C.c_void_p(acc.data_ptr()), _stream()))
        return acc

    def recompose_linear_to_level(self, acc, level, out=None):
        """mgh_recompose_linear_to_level: the dense array of `level` from the head of a level-linearised coefficient
        array (at least prod(level_shape(level)) elements are read, nothing behind them)."""
        need = 1
        for e in self.level_shape(level):
            need *= int(e)
        assert acc.is_cuda and acc.is_contiguous() and acc.dtype == self.torch_dtype and acc.numel() >= need, "bad tensor"
        out = self._level_out(level, out, acc.device)
        _check(load_library().mgh_recompose_linear_to_level(self._h, C.c_void_p(acc.data_ptr()), int(level),
                                                            C.c_void_p(out.data_ptr()), _stream()))
        return out

    def decompose_quantize_sym16(self, data, ebtype, tol, s, norm=0.0, dict_size=8192, outlier_cap=None):
        """mgh_decompose_quantize_sym16: (symbols uint16, outlier_idx, outlier_val, count, norm)."""
        import torch
        cap = self.total if outlier_cap is None else int(outlier_cap)
        sym = torch.empty(self.shape, dtype=torch.uint16, device=data.device)
        cnt, idx, val = self._outlier_bufs(cap)
        nout = C.c_double()
        _check(load_library().mgh_decompose_quantize_sym16(
            self._h, self._chk(data), ebtype, tol, s, norm, C.byref(nout), dict_size,
            C.c_void_p(sym.data_ptr()), C.c_void_p(cnt.data_ptr()), C.c_void_p(idx.data_ptr()),
            C.c_void_p(val.data_ptr()), cap, _stream()))
        n = int(cnt.item())
        k = min(n, cap)
        return sym, idx[:k], val[:k], n, nout.value

    def dequantize_recompose_sym16(self, sym, ebtype, tol, s, norm, dict_size=8192, outlier_idx=None,
                                   outlier_val=None, out=None, level=None):
        import torch
        n = 0 if outlier_idx is None else int(outlier_idx.numel())
        if level is not None:
            out = self._level_out(level, out, sym.device)
            _check(load_library().mgh_dequantize_recompose_sym16_to_level(
                self._h, C.c_void_p(sym.data_ptr()), ebtype, tol, s, norm, dict_size,
                C.c_void_p(outlier_idx.data_ptr() if n else 0), C.c_void_p(outlier_val.data_ptr() if n else 0),
                n, int(level), C.c_void_p(out.data_ptr()), _stream()))
            return out
        out = self._new_out(sym.device) if out is None else out
        _check(load_library().mgh_dequantize_recompose_sym16(
            self._h, C.c_void_p(sym.data_ptr()), ebtype, tol, s, norm, dict_size,
            C.c_void_p(outlier_idx.data_ptr() if n else 0), C.c_void_p(outlier_val.data_ptr() if n else 0),
            n, self._chk(out), _stream()))
        return out

    def dequantize_recompose(self, q, ebtype, tol, s, norm, dict_size=8192, prep_huffman=True,
                             outlier_idx=None, outlier_val=None, out=None, level=None):
        import torch
        n = 0 if outlier_idx is None else int(outlier_idx.numel())
        if level is not None:
            out = self._level_out(level, out, q.device)
            _check(load_library().mgh_dequantize_recompose_to_level(
                self._h, self._chk(q, torch.int64), ebtype, tol, s, norm, dict_size, int(prep_huffman),
                C.c_void_p(outlier_idx.data_ptr() if n else 0),
                C.c_void_p(outlier_val.data_ptr() if n else 0), n, int(level),
                C.c_void_p(out.data_ptr()), _stream()))
            return out
        out = self._new_out(q.device) if out is None else out
        _check(load_library().mgh_dequantize_recompose(
            self._h, self._chk(q, torch.int64), ebtype, tol, s, norm, dict_size, int(prep_huffman),
            C.c_void_p(outlier_idx.data_ptr() if n else 0),
            C.c_void_p(outlier_val.data_ptr() if n else 0), n, self._chk(out), _stream()))
        return out

    def level_linearize(self, q, inverse=False, outlier_idx=None):
        """mgh_level_linearize: the quantized array level by level (config.reorder == 1) or back;
        forward, `outlier_idx` (int64/uint64 device tensor) is rewritten in place."""
        import torch
        out = torch.empty_like(q)
        n = 0 if outlier_idx is None else int(outlier_idx.numel())
        _check(load_library().mgh_level_linearize(
            self._h, self._chk(q, torch.int64), C.c_void_p(out.data_ptr()), int(inverse),
            C.c_void_p(outlier_idx.data_ptr() if n else 0), None, n, 0, _stream()))
        return out

    def _linear_head(self, lin, level):
        import torch
        need = 1
        for e in self.level_shape(level):
            need *= int(e)
        if not (lin.is_cuda and lin.dtype == torch.int64 and lin.is_contiguous() and lin.numel() >= need):
            raise ValueError("expected a contiguous cuda int64 tensor of at least %d elements "
                             "(the head of the level-linearised array)" % need)
        return need

    def level_box_from_linear(self, lin, level, out=None):
        """mgh_level_box_from_linear: the compact corner box of `level` (reordered layout, dense in
        level_shape(level)) out of the first prod(level_shape(level)) integers of a level-linearised
        array; `lin` need not be longer than that."""
        import torch
        need = self._linear_head(lin, level)
        if out is None:
            out = torch.empty(tuple(int(e) for e in self.level_shape(level)), dtype=torch.int64, device=lin.device)
        elif not (out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and out.numel() >= need):
            raise ValueError("out: expected a contiguous cuda int64 tensor of at least %d elements" % need)
        _check(load_library().mgh_level_box_from_linear(
            self._h, C.c_void_p(lin.data_ptr()), int(level), C.c_void_p(out.data_ptr()), _stream()))
        return out

    def dequantize_recompose_linear(self, lin, ebtype, tol, s, norm, dict_size=8192, prep_huffman=True,
                                    outlier_idx=None, outlier_val=None, out=None, level=None):
        """mgh_dequantize_recompose_linear_to_level: `lin` holds (at least) the head of the
        level-linearised array that is the box of `level` (default: l_target); the outlier indices are
        linearised positions, those inside the head are written into `lin`."""
        level = self.l_target if level is None else int(level)
        self._linear_head(lin, level)
        n = 0 if outlier_idx is None else int(outlier_idx.numel())
        out = self._level_out(level, out, lin.device)
        _check(load_library().mgh_dequantize_recompose_linear_to_level(
            self._h, C.c_void_p(lin.data_ptr()), ebtype, tol, s, norm, dict_size, int(prep_huffman),
            C.c_void_p(outlier_idx.data_ptr() if n else 0), C.c_void_p(outlier_val.data_ptr() if n else 0),
            n, level, C.c_void_p(out.data_ptr()), _stream()))
        return out

    def refine_level(self, coarse, segment, ebtype, tol, s, norm, level, dict_size=8192, prep_huffman=True,
                     outlier_idx=None, outlier_val=None, out=None):
        """mgh_refine_level: one level step. `coarse`: the dense array of level_shape(level - 1) (not
        modified); `segment`: the prod(level_shape(level)) - prod(level_shape(level - 1)) integers of
        `level` in the level-linearised array (outliers of the level are written into it; the indices
        are linearised positions of the whole array). Returns the dense array of `level`."""
        import torch
        level = int(level)
        if not 1 <= level <= self.l_target:
            raise ValueError("level must be in 1 .. l_target")
        lo = hi = 1
        for e in self.level_shape(level - 1):
            lo *= int(e)
        for e in self.level_shape(level):
            hi *= int(e)
        if not (coarse.is_cuda and coarse.is_contiguous() and coarse.dtype == self.torch_dtype and
                coarse.numel() == lo):
            raise ValueError("coarse: expected the contiguous cuda array of level %d (%d elements)" % (level - 1, lo))
        if not (segment.is_cuda and segment.dtype == torch.int64 and segment.is_contiguous() and
                segment.numel() >= hi - lo):
            raise ValueError("segment: expected a contiguous cuda int64 tensor of at least %d elements" % (hi - lo))
        n = 0 if outlier_idx is None else int(outlier_idx.numel())
        out = self._level_out(level, out, coarse.device)
        _check(load_library().mgh_refine_level(
            self._h, C.c_void_p(coarse.data_ptr()), C.c_void_p(segment.data_ptr()), ebtype, tol, s, norm, dict_size,
            int(prep_huffman), C.c_void_p(outlier_idx.data_ptr() if n else 0),
            C.c_void_p(outlier_val.data_ptr() if n else 0), n, level, C.c_void_p(out.data_ptr()), _stream()))
        return out

    def prolong(self, level_array, level, out=None, window=None):
        """mgh_prolong: the dense array of `level` (level_shape(level), not modified) prolonged to the
        full grid -- recompose() of the coefficient array with everything outside the level's corner
        box zero. Returns the dense array of the hierarchy's shape (LD_OUT does not apply).
        window = (lo, ext): mgh_prolong_window -- the box [lo, lo + ext) of that array alone, a dense
        array of shape ext; on the fused 3-D route the work is that of the window, not of the array."""
        import torch
        level = int(level)
        if 0 <= level <= self.l_target:
            need = int(np.prod(self.level_shape(level)))
            if not (level_array.is_cuda and level_array.is_contiguous() and level_array.dtype == self.torch_dtype
                    and level_array.numel() == need):
                raise ValueError("level_array: expected the contiguous cuda array of level %d (%d elements)"
                                 % (level, need))
        if window is not None:
            lo, ext = self._window(window)
            shape = tuple(int(e) for e in ext)
            if out is None:
                out = torch.empty(shape, dtype=self.torch_dtype, device=level_array.device)
            elif not (out.is_cuda and out.is_contiguous() and out.dtype == self.torch_dtype and
                      out.numel() == int(np.prod(shape))):
                raise ValueError("out: expected a contiguous cuda array of the window's shape")
            _check(load_library().mgh_prolong_window(self._h, level, C.c_void_p(level_array.data_ptr()), lo, ext,
                                                     C.c_void_p(out.data_ptr()), _stream()))
            return out
        if out is None:
            out = torch.empty(self.shape, dtype=self.torch_dtype, device=level_array.device)
        elif not (out.is_cuda and out.is_contiguous() and out.dtype == self.torch_dtype and
                  out.numel() == self.total):
            raise ValueError("out: expected a contiguous cuda array of the hierarchy's shape")
        _check(load_library().mgh_prolong(self._h, level, C.c_void_p(level_array.data_ptr()),
                                          C.c_void_p(out.data_ptr()), _stream()))
        return out

    def _window(self, window):
        """(lo, ext) as two uint64 arrays of the hierarchy's dimension (the library checks the values)."""
        lo, ext = window
        D = len(self.shape)
        if len(lo) != D or len(ext) != D or min(lo) < 0 or min(ext) < 0:
            raise ValueError("window: (lo, ext) with one non-negative integer per dimension each")
        return (C.c_uint64 * D)(*[int(x) for x in lo]), (C.c_uint64 * D)(*[int(x) for x in ext])

    def prolong_window_ranges(self, level, lo, ext):
        """mgh_debug_prolong_window_ranges (host only): the nodes prolong(..., window=(lo, ext)) depends on --
        a list over the levels level .. l_target of D pairs (first, last) of node indices of that level."""
        lo, ext = self._window((lo, ext))
        D = len(self.shape)
        cap = (self.l_target + 1) * 2 * D
        out = (C.c_int64 * cap)()
        n = _check(load_library().mgh_debug_prolong_window_ranges(self._h, int(level), lo, ext, out, cap))
        return [[(int(out[k * 2 * D + 2 * d]), int(out[k * 2 * D + 2 * d + 1])) for d in range(D)]
                for k in range(n // (2 * D))]

    PROLONG_WINDOW_PLAN_FIELDS = ("TC", "TF", "tiles_f", "tiles", "rch", "nchunk", "J0_r", "J0_c", "J0_f",
                                  "cells_r", "cells_c", "cells_f")

    def prolong_window_plan(self, level, lo, ext, step):
        """The launch plan of the window kernel for the step `step` - 1 -> `step` of that window
        (mgh_debug_prolong_window_plan): a dict with the keys PROLONG_WINDOW_PLAN_FIELDS."""
        lo, ext = self._window((lo, ext))
        out = (C.c_int * 12)()
        _check(load_library().mgh_debug_prolong_window_plan(self._h, int(level), lo, ext, int(step), out))
        return dict(zip(self.PROLONG_WINDOW_PLAN_FIELDS, [int(x) for x in out]))

    PROLONG_PLAN_FIELDS = ("TC", "TF", "tiles_f", "tiles", "rch", "nchunk")

    def prolong_plan(self, level):
        """The launch plan of prolong()'s kernel for the level step level - 1 -> level
        (mgh_debug_prolong_plan): a dict with the keys PROLONG_PLAN_FIELDS."""
        out = (C.c_int * 6)()
        _check(load_library().mgh_debug_prolong_plan(self._h, int(level), out))
        return dict(zip(self.PROLONG_PLAN_FIELDS, [int(x) for x in out]))

    FUSED_PLAN_FIELDS = ("cls", "elem", "m0", "m1", "m2", "TC", "TF", "faces", "ntile", "grid_x", "rch", "nchunk",
                         "by_policy", "nz0", "nz1", "workgroups0", "workgroups1", "slots", "rounds", "slots1")

    def fused_plans(self, reset=True):
        """The levels that went through the planner of the fused level passes (csrc/fused_plan.hpp)
        while profile() was on, in launch order: one dict per level with the keys FUSED_PLAN_FIELDS
        (`m` as a tuple instead of m0..m2)."""
        cap, nf = 512, len(self.FUSED_PLAN_FIELDS)
        buf = (C.c_int64 * (cap * nf))()
        n = _check(load_library().mgh_debug_fused_plans_read(self._h, buf, cap, int(reset)))
        out = []
        for i in range(min(n, cap)):
            r = dict(zip(self.FUSED_PLAN_FIELDS, buf[i * nf:(i + 1) * nf]))
            r["m"] = (r.pop("m0"), r.pop("m1"), r.pop("m2"))
            out.append(r)
        return out

    def spec_repairs(self, reset=True):
        """Chunks that the solves in verified chunks (family Spec of ipk_plans) had to recompute on this
        hierarchy since it was created or since the last read that reset the count. Waits for the device."""
        n = C.c_uint64(0)
        _check(load_library().mgh_debug_spec_repairs_read(self._h, C.byref(n), int(reset)))
        return int(n.value)

    # ---- per-kernel timing (HIP events on the launch stream) ----
    def profile(self, enable=True, only=None):
        _check(load_library().mgh_profile_filter(self._h, only.encode() if only else None))
        _check(load_library().mgh_profile_enable(self._h, int(enable)))

    def profile_read(self, reset=True):
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        cnt = (C.c_uint64 * cap)()
        n = _check(load_library().mgh_profile_read(self._h, names, ms, cnt, cap, int(reset)))
        return {names[i].decode(): (ms[i], int(cnt[i])) for i in range(min(n, cap))}

    IPK_FAMILIES = ("Spec", "LdsContigChunked", "Dma", "Stream", "LdsContig", "LdsStrided", "Thread")
    IPK_PLAN_FIELDS = ("family", "axis", "elem", "m0", "m1", "m2", "nbatch", "n", "npencil", "W", "n_glob", "KR",
                       "P", "K", "add", "batch_stride")

    def ipk_plans(self, reset=True):
        """The Thomas solves that went through the planner (csrc/ipk_plan.hpp) while profile() was
        on, in launch order: one dict per solve with the keys IPK_PLAN_FIELDS (`family` by name, `m`
        as a tuple instead of m0..m2)."""
        cap, nf = 512, len(self.IPK_PLAN_FIELDS)
        buf = (C.c_int64 * (cap * nf))()
        n = _check(load_library().mgh_debug_ipk_plans_read(self._h, buf, cap, int(reset)))
        out = []
        for i in range(min(n, cap)):
            r = dict(zip(self.IPK_PLAN_FIELDS, buf[i * nf:(i + 1) * nf]))
            r["family"] = self.IPK_FAMILIES[r["family"]]
            r["m"] = (r.pop("m0"), r.pop("m1"), r.pop("m2"))
            out.append(r)
        return out
