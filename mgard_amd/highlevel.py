"""Python host side of the high-level path (include/mgard_hip_compress.h): whole-array
compress / decompress, the container header and the lossless stage, all through the C ABI.

    buf = mgard_amd.highlevel.compress(u, tol=1e-3, s=inf, mode=REL)     # numpy or cuda tensor
    v = mgard_amd.highlevel.decompress(buf)

mirrors mgard_x::compress / decompress (reference include/compress_x.hpp:31-154).

Streams. The container calls of the C ABI run on pipeline streams of their own, which are ordered against
the NULL stream only (include/mgard_hip_compress.h, above mgh_pin_memory): work in flight on a NON-BLOCKING
stream is not waited for, and torch's side streams are non-blocking. So every function here that is given a
cuda tensor -- the array, the container, `out=`, `outs=` -- first synchronises the CURRENT stream of that
tensor's device when it is not the device's default stream (_wait_for_current_stream): inside
`with torch.cuda.stream(S)` a tensor that S is still producing is complete before the library reads it.
Results are complete when a call returns, so a consumer on S needs nothing further. On the default stream
nothing is synchronised here: the library's own ordering against the NULL stream holds.
"""
import ctypes as C

import numpy as np

from . import ABS, DOUBLE, FLOAT, INF, REL, ErrorStats, MgardHipError, _check, load_library  # noqa: F401

MAX_DIM = 5
DD_MAXDIM, DD_BLOCK, DD_VARIABLE = 0, 1, 2
HUFFMAN, HUFFMAN_LZ4, HUFFMAN_ZSTD, CPU_LOSSLESS = 0, 1, 2, 3
TARGET_MAX_ABS, TARGET_RMSE, TARGET_PSNR = 0, 1, 2  # mgh_target_metric

HL_SYMBOLS = [
    "mgh_config_default", "mgh_compress", "mgh_decompress", "mgh_infer_shape",
    "mgh_infer_data_type", "mgh_free_device", "mgh_release_cache", "mgh_metadata_serialize",
    "mgh_metadata_parse", "mgh_lossless_create", "mgh_lossless_destroy", "mgh_lossless_compress",
    "mgh_lossless_decompress", "mgh_lossless_compress_device", "mgh_memcpy", "mgh_huffman_codebook",
    "mgh_compress_multi", "mgh_decompress_multi", "mgh_pin_memory", "mgh_check_memory_pinned",
    "mgh_unpin_memory", "mgh_dist_use_library", "mgh_compress_dist", "mgh_decompress_dist",
    "mgh_decompress_into",
    "mgh_infer_level_shape", "mgh_infer_level_nodes", "mgh_decompress_level",
    "mgh_lossless_decompress_prefix", "mgh_last_decompress_stats",
    "mgh_lossless_decompress_range", "mgh_infer_level_range", "mgh_progressive_open",
    "mgh_progressive_level", "mgh_progressive_refine", "mgh_progressive_close",
    "mgh_infer_coarsened_shape", "mgh_infer_coarsened_nodes", "mgh_decompress_coarsened",
    "mgh_decompress_preview", "mgh_progressive_preview",
    "mgh_decompress_preview_window", "mgh_progressive_preview_window",
    "mgh_verify",
    "mgh_estimate_sizes", "mgh_compress_budget",
    "mgh_achieved_errors", "mgh_compress_target",
    "mgh_compress_ladder", "mgh_last_compress_stats", "mgh_histogram_sym16",
    "mgh_compress_layers", "mgh_layers_open", "mgh_layers_add", "mgh_layers_count", "mgh_layers_tolerance",
    "mgh_layers_data", "mgh_layers_close", "mgh_decompress_layers", "mgh_layers_data_level",
    "mgh_compress_level_layers", "mgh_level_layers_open", "mgh_level_layers_add", "mgh_level_layers_extend",
    "mgh_level_layers_count", "mgh_level_layers_depth", "mgh_level_layers_tolerance", "mgh_level_layers_data",
    "mgh_level_layers_close", "mgh_decompress_level_layers",
    "mgh_compress_masked", "mgh_masked_info", "mgh_decompress_masked", "mgh_decompress_mask",
    "mgh_decompress_masked_level", "mgh_decompress_masked_coarsened", "mgh_decompress_masked_preview",
    "mgh_decompress_masked_preview_window", "mgh_decompress_mask_level", "mgh_decompress_mask_coarsened",
    "mgh_decompress_mask_window", "mgh_verify_masked",
    "mgh_compress_pwrel", "mgh_decompress_pwrel", "mgh_pwrel_info", "mgh_verify_pwrel",
    "mgh_decompress_pwrel_level", "mgh_decompress_pwrel_coarsened", "mgh_decompress_pwrel_preview",
    "mgh_decompress_pwrel_preview_window",
    "mgh_compress_roi", "mgh_decompress_roi", "mgh_roi_info", "mgh_verify_roi",
    "mgh_lossless_compress_sym16", "mgh_lossless_compress_device_sym16", "mgh_lossless_decompress_sym16",
]


class Config(C.Structure):
    """mgh_config (subset of mgard_x::Config)."""
    _fields_ = [
        ("dev_id", C.c_int),
        ("domain_decomposition", C.c_int),
        ("domain_decomposition_dim", C.c_int),
        ("domain_decomposition_sizes", C.POINTER(C.c_uint64)),
        ("num_domain_decomposition_sizes", C.c_uint64),
        ("block_size", C.c_uint64),
        ("estimate_outlier_ratio", C.c_double),
        ("huff_dict_size", C.c_uint64),
        ("huff_block_size", C.c_uint64),
        ("lossless", C.c_int),
        ("zstd_compress_level", C.c_int),
        ("normalize_coordinates", C.c_int),
        ("max_larget_level", C.c_uint64),
        ("max_memory_footprint", C.c_uint64),
        ("auto_pin_host_buffers", C.c_int),
        ("reorder", C.c_int),
        ("mirror_reference_coord_cast", C.c_int),
    ]

    def __init__(self, **kw):
        super().__init__()
        _hl().mgh_config_default(C.byref(self))
        self._sizes = None
        for k, v in kw.items():
            if k == "domain_decomposition_sizes":
                self._sizes = (C.c_uint64 * len(v))(*v)
                self.domain_decomposition_sizes = C.cast(self._sizes, C.POINTER(C.c_uint64))
                self.num_domain_decomposition_sizes = len(v)
            else:
                setattr(self, k, v)


class DecompressStats(C.Structure):
    """mgh_decompress_stats: what the lossless stage of the last decompress* call of this thread did."""
    _fields_ = [("subdomains", C.c_uint64), ("chunks_total", C.c_uint64), ("chunks_decoded", C.c_uint64),
                ("symbols_decoded", C.c_uint64), ("record_bytes", C.c_uint64),
                ("record_bytes_moved", C.c_uint64)]


class CompressStats(C.Structure):
    """mgh_compress_stats: what the last compress / compress_budget / compress_target / compress_ladder / compress_layers call
    of this thread did."""
    _fields_ = [("decompositions", C.c_uint64), ("quantize_passes", C.c_uint64), ("histogram_launches", C.c_uint64),
                ("records", C.c_uint64), ("raw_records", C.c_uint64), ("outlier_retries", C.c_uint64)]


class VerifyResult(C.Structure):
    """mgh_verify_result: `stats` (ErrorStats) of the original against the container's reconstruction;
    bound_kind 0: L-infinity, 1: L2, -1: not evaluated; `bound` absolute; `achieved` the matching figure
    of stats; `within` 1 / 0 / -1 (not evaluated: a preview, or a bound in an s-norm)."""
    _fields_ = [("stats", ErrorStats), ("bound_kind", C.c_int), ("bound", C.c_double), ("achieved", C.c_double),
                ("within", C.c_int)]

    def __repr__(self):
        return "VerifyResult(stats=%r, bound_kind=%d, bound=%r, achieved=%r, within=%d)" % (
            self.stats, self.bound_kind, self.bound, self.achieved, self.within)


class SizeEstimate(C.Structure):
    """mgh_size_estimate: bytes_min <= len(compress(data, tol)) <= bytes_max; raw 1 / 0 / -1 (the
    bracket straddles the threshold at which the writer stores the array itself)."""
    _fields_ = [("tol", C.c_double), ("bytes_min", C.c_uint64), ("bytes_max", C.c_uint64), ("outliers", C.c_uint64),
                ("code_bits", C.c_uint64), ("raw", C.c_int)]

    def __repr__(self):
        return "SizeEstimate(tol=%r, bytes_min=%d, bytes_max=%d, outliers=%d, code_bits=%d, raw=%d)" % (
            self.tol, self.bytes_min, self.bytes_max, self.outliers, self.code_bits, self.raw)


class MaskSpec(C.Structure):
    """mgh_mask_spec: which elements do not count, and what they decode to."""
    _fields_ = [("flags", C.c_int), ("fill_value", C.c_double), ("restore_value", C.c_double)]


class MaskedInfo(C.Structure):
    """mgh_masked_info: the parts of a masked buffer -- [container][mask record][48-byte footer] -- and its
    footer's fields. kind 0: packed words, 1: one record of the lossless stage, 2: nothing masked."""
    _fields_ = [("container_size", C.c_uint64), ("record_size", C.c_uint64), ("n_masked", C.c_uint64),
                ("kind", C.c_int), ("restore_value", C.c_double)]

    def __repr__(self):
        return "MaskedInfo(container_size=%d, record_size=%d, n_masked=%d, kind=%d, restore_value=%r)" % (
            self.container_size, self.record_size, self.n_masked, self.kind, self.restore_value)


class PwrelInfo(C.Structure):
    """mgh_pwrel_info: the parts of a pointwise-relative buffer -- [masked buffer of y = log2|x|][flag record][56-byte
    footer] -- with the footer's eps and abs_floor, and delta, the ABS tolerance of y in the container's header."""
    _fields_ = [("eps", C.c_double), ("abs_floor", C.c_double), ("delta", C.c_double), ("n_masked", C.c_uint64),
                ("n_flag", C.c_uint64), ("container_size", C.c_uint64), ("masked_size", C.c_uint64),
                ("mask_record_size", C.c_uint64), ("flag_record_size", C.c_uint64), ("mask_kind", C.c_int),
                ("flag_kind", C.c_int)]

    def __repr__(self):
        return "PwrelInfo(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k, _ in self._fields_)


class RoiBox(C.Structure):
    """mgh_roi_box: a box lo .. lo + ext of an array (the first D entries of each) and its tolerance."""
    _fields_ = [("lo", C.c_uint64 * MAX_DIM), ("ext", C.c_uint64 * MAX_DIM), ("tol", C.c_double)]


class _RoiInfoBox(C.Structure):
    _fields_ = [("lo", C.c_uint64 * MAX_DIM), ("ext", C.c_uint64 * MAX_DIM), ("tol", C.c_double), ("tolres", C.c_double),
                ("record_size", C.c_uint64)]


class RoiInfo(C.Structure):
    """mgh_roi_info: the parts of a buffer with boxes -- [container][one record per box][box table][40-byte footer].
    `boxes`: per box (lo, ext, tol, tolres, record_size), lo and ext as tuples of the array's dimension."""
    _fields_ = [("container_size", C.c_uint64), ("nbox", C.c_int), ("D", C.c_int), ("box", _RoiInfoBox * 16)]

    @property
    def boxes(self):
        return [(tuple(b.lo[:self.D]), tuple(b.ext[:self.D]), b.tol, b.tolres, int(b.record_size))
                for b in self.box[:self.nbox]]

    def __repr__(self):
        return "RoiInfo(container_size=%d, boxes=%r)" % (self.container_size, self.boxes)


class HeaderInfo(C.Structure):
    """mgh_header_info."""
    _fields_ = [
        ("version", C.c_uint64 * 3),
        ("dtype", C.c_int),
        ("D", C.c_int),
        ("shape", C.c_uint64 * MAX_DIM),
        ("uniform", C.c_int),
        ("coords", C.POINTER(C.c_double) * MAX_DIM),
        ("error_bound_type", C.c_int),
        ("tol", C.c_double),
        ("s", C.c_double),
        ("norm", C.c_double),
        ("domain_decomposed", C.c_int),
        ("dd_method", C.c_int),
        ("dd_dim", C.c_uint64),
        ("dd_size", C.c_uint64),
        ("l_target", C.c_uint64),
        ("reorder", C.c_int),
        ("lossless", C.c_int),
        ("huff_dict_size", C.c_uint64),
        ("huff_block_size", C.c_uint64),
    ]


_declared = False


def _hl():
    global _declared
    L = load_library()
    if _declared:
        return L
    vp, u64 = C.c_void_p, C.c_uint64
    L.mgh_config_default.argtypes = [C.POINTER(Config)]
    L.mgh_config_default.restype = None
    L.mgh_compress.argtypes = [C.c_int, C.c_int, C.POINTER(u64), C.c_double, C.c_double, C.c_int, vp,
                               C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp),
                               C.POINTER(Config), C.c_int]
    L.mgh_decompress.argtypes = [vp, C.c_size_t, C.POINTER(vp), C.POINTER(Config), C.c_int]
    L.mgh_decompress_into.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_int, vp]
    L.mgh_infer_level_shape.argtypes = [vp, C.c_size_t, vp, C.c_int, vp, vp, vp]
    L.mgh_infer_level_nodes.argtypes = [vp, C.c_size_t, vp, C.c_int, C.c_int, vp, u64]
    L.mgh_decompress_level.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(vp), vp, C.c_int]
    L.mgh_infer_coarsened_shape.argtypes = [vp, C.c_size_t, vp, C.c_int, vp, vp, vp]
    L.mgh_infer_coarsened_nodes.argtypes = [vp, C.c_size_t, vp, C.c_int, C.c_int, vp, u64]
    L.mgh_decompress_coarsened.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(vp), vp, C.c_int]
    L.mgh_decompress_preview.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(vp), vp, C.c_int]
    L.mgh_decompress_preview_window.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                                C.POINTER(vp), vp, C.c_int]
    L.mgh_verify.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, vp, C.POINTER(VerifyResult)]
    L.mgh_estimate_sizes.argtypes = [C.c_int, C.c_int, C.POINTER(u64), C.c_int, C.POINTER(C.c_double), C.c_double,
                                     C.c_int, vp, C.POINTER(vp), C.POINTER(Config), C.POINTER(SizeEstimate)]
    L.mgh_compress_budget.argtypes = [C.c_int, C.c_int, C.POINTER(u64), C.c_size_t, C.c_double, C.c_double, C.c_int,
                                      C.c_double, C.c_int, vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp),
                                      C.POINTER(Config), C.c_int, C.POINTER(C.c_double), C.POINTER(SizeEstimate)]
    L.mgh_achieved_errors.argtypes = [C.c_int, C.c_int, C.POINTER(u64), C.c_int, C.POINTER(C.c_double), C.c_double,
                                      C.c_int, vp, C.POINTER(vp), C.POINTER(Config), C.POINTER(ErrorStats)]
    L.mgh_compress_target.argtypes = [C.c_int, C.c_int, C.POINTER(u64), C.c_int, C.c_double, C.c_double, C.c_double,
                                      C.c_int, C.c_double, C.c_int, vp, C.POINTER(vp), C.POINTER(C.c_size_t),
                                      C.POINTER(vp), C.POINTER(Config), C.c_int, C.POINTER(C.c_double),
                                      C.POINTER(ErrorStats), C.POINTER(C.c_int)]
    L.mgh_dist_use_library.argtypes = [C.c_char_p]
    L.mgh_compress_dist.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(u64), C.c_double,
                                    C.c_double, C.c_int, vp, C.POINTER(vp), C.POINTER(C.c_size_t), vp, vp, C.c_int]
    L.mgh_decompress_dist.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp, vp]
    L.mgh_pin_memory.argtypes = [vp, C.c_size_t]
    L.mgh_check_memory_pinned.argtypes = [vp]
    L.mgh_unpin_memory.argtypes = [vp]
    L.mgh_compress_multi.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(u64), C.c_double,
                                     C.c_double, C.c_int, vp, C.POINTER(vp), C.POINTER(C.c_size_t),
                                     C.POINTER(vp), C.POINTER(Config), C.c_int]
    L.mgh_decompress_multi.argtypes = [C.c_int, C.POINTER(C.c_int), vp, C.c_size_t, C.POINTER(vp),
                                       C.POINTER(Config), C.c_int]
    L.mgh_infer_shape.argtypes = [vp, C.c_size_t, C.POINTER(C.c_int), C.POINTER(u64)]
    L.mgh_infer_data_type.argtypes = [vp, C.c_size_t, C.POINTER(C.c_int)]
    L.mgh_free_device.argtypes = [vp]
    L.mgh_free_device.restype = None
    L.mgh_release_cache.restype = None
    L.mgh_metadata_serialize.argtypes = [C.POINTER(HeaderInfo), vp, u64]
    L.mgh_metadata_serialize.restype = C.c_int64
    L.mgh_metadata_parse.argtypes = [vp, u64, C.POINTER(HeaderInfo), C.POINTER(C.c_double), u64,
                                     C.POINTER(u64)]
    L.mgh_lossless_create.argtypes = [C.POINTER(vp), C.c_int]
    L.mgh_lossless_destroy.argtypes = [vp]
    L.mgh_lossless_destroy.restype = None
    L.mgh_lossless_compress.argtypes = [vp, vp, u64, u64, u64, C.c_int, C.c_int, vp, vp, u64,
                                        C.POINTER(vp), C.POINTER(u64), vp]
    L.mgh_lossless_compress_device.argtypes = [vp, vp, u64, u64, u64, vp, vp, u64, vp, u64, C.POINTER(u64), vp]
    L.mgh_lossless_decompress.argtypes = [vp, vp, u64, C.c_int, vp, u64, C.POINTER(vp), C.POINTER(vp),
                                          C.POINTER(u64), vp]
    L.mgh_lossless_decompress_prefix.argtypes = [vp, vp, u64, C.c_int, vp, u64, u64, C.POINTER(vp), C.POINTER(vp),
                                                 C.POINTER(u64), vp]
    L.mgh_lossless_decompress_range.argtypes = [vp, vp, u64, C.c_int, vp, u64, u64, u64, C.POINTER(vp),
                                                C.POINTER(vp), C.POINTER(u64), vp]
    L.mgh_lossless_compress_sym16.argtypes = L.mgh_lossless_compress.argtypes
    L.mgh_lossless_compress_device_sym16.argtypes = L.mgh_lossless_compress_device.argtypes
    L.mgh_lossless_decompress_sym16.argtypes = L.mgh_lossless_decompress_range.argtypes
    L.mgh_infer_level_range.argtypes = [vp, C.c_size_t, vp, C.c_int, C.POINTER(u64), C.POINTER(u64),
                                        C.POINTER(u64), C.POINTER(u64)]
    L.mgh_progressive_open.argtypes = [C.POINTER(vp), vp, C.c_size_t, vp]
    L.mgh_progressive_level.argtypes = [vp]
    L.mgh_progressive_refine.argtypes = [vp, C.c_int, C.POINTER(vp), C.c_int]
    L.mgh_progressive_preview.argtypes = [vp, C.POINTER(vp), C.c_int]
    L.mgh_progressive_preview_window.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(vp),
                                                 C.c_int]
    L.mgh_progressive_close.argtypes = [vp]
    L.mgh_progressive_close.restype = None
    L.mgh_last_decompress_stats.argtypes = [C.POINTER(DecompressStats)]
    L.mgh_last_compress_stats.argtypes = [C.POINTER(CompressStats)]
    L.mgh_compress_ladder.argtypes = [C.c_int, C.c_int, C.POINTER(u64), C.c_int, C.POINTER(C.c_double), C.c_double,
                                      C.c_int, vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp),
                                      C.POINTER(Config), C.c_int]
    L.mgh_histogram_sym16.argtypes = [vp, u64, u64, vp, vp]
    L.mgh_compress_layers.argtypes = L.mgh_compress_ladder.argtypes
    L.mgh_layers_open.argtypes = [C.POINTER(vp), vp, C.c_size_t, vp]
    L.mgh_layers_add.argtypes = [vp, vp, C.c_size_t]
    L.mgh_layers_count.argtypes = [vp]
    L.mgh_layers_tolerance.argtypes = [vp]
    L.mgh_layers_tolerance.restype = C.c_double
    L.mgh_layers_data.argtypes = [vp, C.POINTER(vp), C.c_int]
    L.mgh_layers_close.argtypes = [vp]
    L.mgh_layers_close.restype = None
    L.mgh_layers_data_level.argtypes = [vp, C.c_int, C.POINTER(vp), C.c_int]
    L.mgh_compress_level_layers.argtypes = L.mgh_compress_ladder.argtypes
    L.mgh_level_layers_open.argtypes = [C.POINTER(vp), vp, C.c_size_t, vp, C.c_int]
    L.mgh_level_layers_add.argtypes = [vp, vp, C.c_size_t, C.c_int]
    L.mgh_level_layers_extend.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_int]
    L.mgh_level_layers_count.argtypes = [vp]
    L.mgh_level_layers_depth.argtypes = [vp, C.c_int]
    L.mgh_level_layers_tolerance.argtypes = [vp, C.c_int]
    L.mgh_level_layers_tolerance.restype = C.c_double
    L.mgh_level_layers_data.argtypes = [vp, C.c_int, C.POINTER(vp), C.c_int]
    L.mgh_level_layers_close.argtypes = [vp]
    L.mgh_level_layers_close.restype = None
    L.mgh_decompress_level_layers.argtypes = [C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_int, C.POINTER(Config),
                                              C.POINTER(vp), C.c_int]
    L.mgh_decompress_layers.argtypes = [C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(Config), C.POINTER(vp),
                                        C.c_int]
    L.mgh_memcpy.argtypes = [vp, vp, C.c_size_t]
    L.mgh_huffman_codebook.argtypes = [vp, u64, vp, vp, vp, vp]
    L.mgh_compress_masked.argtypes = [C.c_int, C.c_int, C.POINTER(u64), C.c_double, C.c_double, C.c_int, vp,
                                      C.POINTER(MaskSpec), C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp),
                                      C.POINTER(Config), C.c_int]
    L.mgh_masked_info.argtypes = [vp, C.c_size_t, C.POINTER(MaskedInfo)]
    L.mgh_decompress_masked.argtypes = [vp, C.c_size_t, C.POINTER(Config), C.POINTER(vp), C.c_int]
    L.mgh_decompress_mask.argtypes = [vp, C.c_size_t, C.POINTER(Config), vp]
    for name in ("mgh_decompress_masked_level", "mgh_decompress_masked_coarsened", "mgh_decompress_masked_preview"):
        getattr(L, name).argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(vp), C.POINTER(Config), C.c_int]
    L.mgh_decompress_masked_preview_window.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(u64), C.POINTER(u64),
                                                       C.POINTER(vp), C.POINTER(Config), C.c_int]
    L.mgh_decompress_mask_level.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(Config), vp]
    L.mgh_decompress_mask_coarsened.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(Config), vp]
    L.mgh_decompress_mask_window.argtypes = [vp, C.c_size_t, C.POINTER(u64), C.POINTER(u64), C.POINTER(Config), vp]
    L.mgh_verify_masked.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, C.POINTER(Config),
                                    C.POINTER(VerifyResult), C.POINTER(u64)]
    from . import PwrelCompare
    L.mgh_compress_pwrel.argtypes = [C.c_int, C.c_int, C.POINTER(u64), C.c_double, C.c_double, vp, C.POINTER(vp),
                                     C.POINTER(C.c_size_t), C.POINTER(vp), C.POINTER(Config), C.c_int]
    L.mgh_decompress_pwrel.argtypes = [vp, C.c_size_t, C.POINTER(Config), C.POINTER(vp), C.c_int]
    for name in ("mgh_decompress_pwrel_level", "mgh_decompress_pwrel_coarsened", "mgh_decompress_pwrel_preview"):
        getattr(L, name).argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(vp), C.POINTER(Config), C.c_int]
    L.mgh_decompress_pwrel_preview_window.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(u64), C.POINTER(u64),
                                                      C.POINTER(vp), C.POINTER(Config), C.c_int]
    L.mgh_pwrel_info.argtypes = [vp, C.c_size_t, C.POINTER(PwrelInfo)]
    L.mgh_compress_roi.argtypes = [C.c_int, C.c_int, C.POINTER(u64), C.c_double, C.c_double, C.c_int, vp, C.c_int,
                                   C.POINTER(RoiBox), C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp),
                                   C.POINTER(Config), C.c_int]
    L.mgh_decompress_roi.argtypes = [vp, C.c_size_t, C.POINTER(vp), C.POINTER(Config), C.c_int]
    L.mgh_roi_info.argtypes = [vp, C.c_size_t, C.POINTER(RoiInfo)]
    L.mgh_verify_roi.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.POINTER(Config), C.POINTER(VerifyResult),
                                 C.POINTER(VerifyResult)]
    L.mgh_verify_pwrel.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.POINTER(Config), C.POINTER(PwrelCompare),
                                   C.POINTER(C.c_int)]
    _declared = True
    return L


# ---- header ---------------------------------------------------------------------------------
def metadata_serialize(dtype, shape, mode, tol, s, norm=0.0, coords=None, dd=None, lossless=HUFFMAN,
                       dict_size=8192, block_size=20480, reorder=0, l_target=0):
    """Bytes of preamble + header for the given description. dd = (method, dim, size) or None."""
    info = HeaderInfo()
    info.version[0], info.version[1], info.version[2] = 1, 0, 0
    info.dtype = dtype
    info.D = len(shape)
    for d, n in enumerate(shape):
        info.shape[d] = n
    keep = []
    info.uniform = 1 if coords is None else 0
    if coords is not None:
        for d, c in enumerate(coords):
            a = np.ascontiguousarray(c, dtype=np.float64)
            keep.append(a)
            info.coords[d] = a.ctypes.data_as(C.POINTER(C.c_double))
    info.error_bound_type = mode
    info.tol, info.s, info.norm = tol, s, norm
    if dd is None:
        info.domain_decomposed, info.dd_dim, info.dd_size = 0, 0, shape[0]
    else:
        info.domain_decomposed, info.dd_method, info.dd_dim, info.dd_size = 1, dd[0], dd[1], dd[2]
    info.l_target = l_target
    info.reorder = reorder
    info.lossless = lossless
    info.huff_dict_size, info.huff_block_size = dict_size, block_size
    L = _hl()
    n = _check(L.mgh_metadata_serialize(C.byref(info), None, 0))
    buf = (C.c_uint8 * n)()
    _check(L.mgh_metadata_serialize(C.byref(info), buf, n))
    return bytes(buf)


def metadata_parse(data):
    """dict of the header fields + 'metadata_size'."""
    L = _hl()
    raw = (C.c_uint8 * len(data)).from_buffer_copy(data)
    info = HeaderInfo()
    cap = 1 << 16
    while True:
        store = (C.c_double * cap)()
        ms = C.c_uint64()
        rc = L.mgh_metadata_parse(raw, len(data), C.byref(info), store, cap, C.byref(ms))
        if rc < 0 and b"coords_storage" in L.mgh_last_error() and cap < (1 << 28):
            cap *= 16
            continue
        _check(rc)
        break
    D = info.D
    out = dict(dtype=info.dtype, shape=[int(info.shape[d]) for d in range(D)], uniform=bool(info.uniform),
               mode=info.error_bound_type, tol=info.tol, s=info.s, norm=info.norm,
               domain_decomposed=bool(info.domain_decomposed), dd_method=info.dd_method,
               dd_dim=int(info.dd_dim), dd_size=int(info.dd_size), l_target=int(info.l_target),
               reorder=info.reorder, lossless=info.lossless, dict_size=int(info.huff_dict_size),
               block_size=int(info.huff_block_size), version=[int(v) for v in info.version],
               metadata_size=int(ms.value))
    if not info.uniform:
        out["coords"] = [np.array([info.coords[d][i] for i in range(out["shape"][d])]) for d in range(D)]
    return out


# ---- whole-array compress / decompress -------------------------------------------------------
def _wait_for_current_stream(*args):
    """The stream contract of this module (see its docstring): for every cuda tensor among `args` (lists of
    tensors are looked into; anything else is passed over), synchronise the current stream of the tensor's
    device unless it is that device's default stream."""
    import torch
    done = set()
    for a in args:
        for t in (a if isinstance(a, (list, tuple)) else (a,)):
            if isinstance(t, torch.Tensor) and t.is_cuda and t.device not in done:
                done.add(t.device)
                cur = torch.cuda.current_stream(t.device)
                if cur != torch.cuda.default_stream(t.device):
                    cur.synchronize()


def _as_ptr(a):
    """(pointer, dtype code, shape, keepalive) of a numpy array or a cuda tensor."""
    import torch
    if isinstance(a, torch.Tensor):
        if not a.is_contiguous():
            a = a.contiguous()  # (a copy on the current stream)
        _wait_for_current_stream(a)
        dt = FLOAT if a.dtype == torch.float32 else DOUBLE if a.dtype == torch.float64 else None
        if dt is None:
            raise MgardHipError("float32 or float64 data expected")
        return C.c_void_p(a.data_ptr()), dt, tuple(a.shape), a
    a = np.ascontiguousarray(a)
    dt = FLOAT if a.dtype == np.float32 else DOUBLE if a.dtype == np.float64 else None
    if dt is None:
        raise MgardHipError("float32 or float64 data expected")
    return C.c_void_p(a.ctypes.data), dt, a.shape, a


def _writer_out(data, out, cap):
    """(out, pointer, size word) of a writer's output: `out` where given (its size is the capacity), else a new uint8
    buffer of `cap` bytes -- a numpy array for host `data`, a cuda tensor beside device `data`."""
    import torch
    on_device = isinstance(data, torch.Tensor) and data.is_cuda
    if out is not None:
        cap = int(out.numel()) if on_device else int(out.size)
    elif on_device:
        out = torch.empty(cap, dtype=torch.uint8, device=data.device)
    else:
        out = np.empty(cap, dtype=np.uint8)
    return out, C.c_void_p(out.data_ptr() if on_device else out.ctypes.data), C.c_size_t(cap)


def compress(data, tol, s=INF, mode=REL, coords=None, config=None, out_capacity=None, out=None):
    """mgard_x::compress. `data`: numpy array (host) or cuda tensor (device). Returns the
    compressed stream as a numpy uint8 array (host input) or a cuda uint8 tensor (device input).
    `out`: optional pre-allocated uint8 buffer of the same kind to write into (its size is the
    capacity)."""
    L = _hl()
    cfg = config if config is not None else Config()
    ptr, dt, shape, keep = _as_ptr(data)
    _wait_for_current_stream(out)
    D = len(shape)
    shp = (C.c_uint64 * D)(*shape)
    cptr = None
    ckeep = []
    if coords is not None:
        npdt = np.float32 if dt == FLOAT else np.float64
        arr = (C.c_void_p * D)()
        for d in range(D):
            c = np.ascontiguousarray(coords[d], dtype=npdt)
            ckeep.append(c)
            arr[d] = c.ctypes.data
        cptr = arr
    nbytes = int(np.prod(shape)) * (4 if dt == FLOAT else 8)
    out, optr, size = _writer_out(data, out, int(out_capacity) if out_capacity is not None else nbytes + 1000000)
    _check(L.mgh_compress(D, dt, shp, float(tol), float(s), int(mode), ptr, C.byref(optr), C.byref(size),
                          cptr, C.byref(cfg), 1))
    return out[:size.value]


def _coords_ptr(coords, dt, D):
    """(void*[D] of host arrays of the data type or None, keepalive)"""
    if coords is None:
        return None, []
    npdt = np.float32 if dt == FLOAT else np.float64
    arr = (C.c_void_p * D)()
    keep = []
    for d in range(D):
        c = np.ascontiguousarray(coords[d], dtype=npdt)
        keep.append(c)
        arr[d] = c.ctypes.data
    return arr, keep


def estimate_sizes(data, tols, s=INF, mode=REL, coords=None, config=None):
    """mgh_estimate_sizes: one SizeEstimate per tolerance (1..64 of them) of what compress(data, tol, ...)
    would write, from one decomposition. Containers of one subdomain, Huffman only."""
    L = _hl()
    cfg = config if config is not None else Config()
    ptr, dt, shape, keep = _as_ptr(data)
    D = len(shape)
    tols = [float(t) for t in tols]
    k = len(tols)
    cptr, ckeep = _coords_ptr(coords, dt, D)
    out = (SizeEstimate * max(k, 1))()
    _check(L.mgh_estimate_sizes(D, dt, (C.c_uint64 * D)(*shape), k, (C.c_double * max(k, 1))(*tols), float(s), int(mode),
                                ptr, cptr, C.byref(cfg), out))
    return list(out)[:k]


def compress_budget(data, max_bytes, tol_min, tol_max, rounds=4, s=INF, mode=REL, coords=None, config=None):
    """mgh_compress_budget: the most accurate container of at most max_bytes, searching
    [tol_min, tol_max]. Returns (buf, tol_used, estimate): buf is compress(data, tol_used, ...) -- a numpy
    uint8 array (host input) or a cuda uint8 tensor (device input). Raises (MGH_ERR_OUTPUT_TOO_LARGE) when
    not even tol_max fits."""
    import torch
    L = _hl()
    cfg = config if config is not None else Config()
    ptr, dt, shape, keep = _as_ptr(data)
    D = len(shape)
    cptr, ckeep = _coords_ptr(coords, dt, D)
    on_device = isinstance(data, torch.Tensor) and data.is_cuda
    cap = int(np.prod(shape)) * (4 if dt == FLOAT else 8) + 1000000
    if on_device:
        out = torch.empty(cap, dtype=torch.uint8, device=data.device)
        optr = C.c_void_p(out.data_ptr())
    else:
        out = np.empty(cap, dtype=np.uint8)
        optr = C.c_void_p(out.ctypes.data)
    size = C.c_size_t(cap)
    used = C.c_double()
    est = SizeEstimate()
    _check(L.mgh_compress_budget(D, dt, (C.c_uint64 * D)(*shape), int(max_bytes), float(tol_min), float(tol_max),
                                 int(rounds), float(s), int(mode), ptr, C.byref(optr), C.byref(size), cptr,
                                 C.byref(cfg), 1, C.byref(used), C.byref(est)))
    return out[:size.value], used.value, est


def achieved_errors(data, tols, s=INF, mode=REL, coords=None, config=None):
    """mgh_achieved_errors: one ErrorStats per tolerance (1..64 of them) -- what verify(compress(data, tol, ...),
    data).stats would report, from one decomposition and without writing a container. Containers of one
    subdomain; any supported lossless type."""
    L = _hl()
    cfg = config if config is not None else Config()
    ptr, dt, shape, keep = _as_ptr(data)
    D = len(shape)
    tols = [float(t) for t in tols]
    k = len(tols)
    cptr, ckeep = _coords_ptr(coords, dt, D)
    out = (ErrorStats * max(k, 1))()
    _check(L.mgh_achieved_errors(D, dt, (C.c_uint64 * D)(*shape), k, (C.c_double * max(k, 1))(*tols), float(s), int(mode),
                                 ptr, cptr, C.byref(cfg), out))
    return list(out)[:k]


def compress_target(data, metric, target, tol_min, tol_max, rounds=8, s=INF, mode=REL, coords=None, config=None):
    """mgh_compress_target: the container of the LARGEST tolerance in [tol_min, tol_max] whose achieved error
    meets `target` in `metric` (TARGET_MAX_ABS / TARGET_RMSE: at most; TARGET_PSNR: at least). Returns
    (buf, tol_used, stats, candidates): buf is compress(data, tol_used, ...) -- a numpy uint8 array (host input)
    or a cuda uint8 tensor (device input) --, stats the ErrorStats of the chosen candidate, candidates the number
    evaluated. Raises (MGH_ERR_TARGET_NOT_MET) when not even tol_min meets the target."""
    import torch
    L = _hl()
    cfg = config if config is not None else Config()
    ptr, dt, shape, keep = _as_ptr(data)
    D = len(shape)
    cptr, ckeep = _coords_ptr(coords, dt, D)
    on_device = isinstance(data, torch.Tensor) and data.is_cuda
    cap = int(np.prod(shape)) * (4 if dt == FLOAT else 8) + 1000000
    if on_device:
        out = torch.empty(cap, dtype=torch.uint8, device=data.device)
        optr = C.c_void_p(out.data_ptr())
    else:
        out = np.empty(cap, dtype=np.uint8)
        optr = C.c_void_p(out.ctypes.data)
    size = C.c_size_t(cap)
    used = C.c_double()
    stats = ErrorStats()
    cand = C.c_int()
    _check(L.mgh_compress_target(D, dt, (C.c_uint64 * D)(*shape), int(metric), float(target), float(tol_min),
                                 float(tol_max), int(rounds), float(s), int(mode), ptr, C.byref(optr), C.byref(size), cptr,
                                 C.byref(cfg), 1, C.byref(used), C.byref(stats), C.byref(cand)))
    return out[:size.value], used.value, stats, cand.value


def compress_ladder(data, tols, s=INF, mode=REL, coords=None, config=None, outs=None, _call="mgh_compress_ladder"):
    """mgh_compress_ladder: [compress(data, tol, ...) for tol in tols] (1..64 tolerances, up to the order of
    the outlier lists) from ONE decomposition of `data` -- numpy uint8 arrays (host input) or cuda uint8
    tensors (device input). Containers of one subdomain. `outs`: optional pre-allocated uint8 buffers of
    the same kind, one per tolerance (their sizes are the capacities); when a tolerance fails the call
    raises, and the buffers of the tolerances before it hold their containers."""
    import torch
    L = _hl()
    cfg = config if config is not None else Config()
    ptr, dt, shape, keep = _as_ptr(data)
    D = len(shape)
    tols = [float(t) for t in tols]
    k = len(tols)
    cptr, ckeep = _coords_ptr(coords, dt, D)
    on_device = isinstance(data, torch.Tensor) and data.is_cuda
    cap = int(np.prod(shape)) * (4 if dt == FLOAT else 8) + 1000000
    if outs is None:
        outs = [torch.empty(cap, dtype=torch.uint8, device=data.device) if on_device else np.empty(cap, dtype=np.uint8)
                for _ in range(k)]
    assert len(outs) == k, "one output buffer per tolerance"
    _wait_for_current_stream(list(outs))
    optr = (C.c_void_p * max(k, 1))(*[o.data_ptr() if on_device else o.ctypes.data for o in outs])
    sizes = (C.c_size_t * max(k, 1))(*[int(o.numel()) if on_device else int(o.size) for o in outs])
    _check(getattr(L, _call)(D, dt, (C.c_uint64 * D)(*shape), k, (C.c_double * max(k, 1))(*tols), float(s),
                             int(mode), ptr, optr, sizes, cptr, C.byref(cfg), 1))
    return [o[:sizes[i]] for i, o in enumerate(outs)]


def compress_layers(data, tols, s=INF, mode=REL, coords=None, config=None, outs=None):
    """mgh_compress_layers: precision layers of `data` for the strictly decreasing tolerances `tols` (1..64) --
    container k holds what containers 0 .. k-1 left of the coefficients, quantized at tols[k], so
    decompress_layers(bufs[:k + 1]) is within tols[k] and the set is far smaller than a ladder. bufs[0] is
    compress(data, tols[0], ...)'s container; every layer is an ordinary container of one subdomain. The
    containers carry no layer index: keep them in order. Outputs, `outs` and a failure at layer k as in
    compress_ladder. Refused: a configuration that decomposes the domain, reorder = 1, a layer that would be
    stored raw."""
    return compress_ladder(data, tols, s, mode, coords, config, outs, _call="mgh_compress_layers")


def _container_ptr(buf):
    """(pointer, size, on_device, keepalive) of a container: numpy uint8 array or cuda uint8 tensor."""
    import torch
    if isinstance(buf, torch.Tensor) and buf.is_cuda:
        buf = buf.contiguous()
        _wait_for_current_stream(buf)
        return C.c_void_p(buf.data_ptr()), int(buf.numel()), True, buf
    buf = np.ascontiguousarray(buf)
    return C.c_void_p(buf.ctypes.data), int(buf.size), False, buf


def _layers_out(buf0, out, level=None, config=None):
    """The array layers of `buf0` reconstruct (level = None) or its level `level`, as (out, pointer): a cuda tensor
    for a device container, a numpy array for a host one."""
    import torch
    shape, dt = infer(buf0)
    if level is not None:
        shape = infer_level(buf0, level, config)[0]
    _wait_for_current_stream(out)
    on_dev = isinstance(buf0, torch.Tensor) and buf0.is_cuda
    n = int(np.prod(shape))
    if on_dev:
        want = torch.float32 if dt == FLOAT else torch.float64
        if out is None:
            out = torch.empty(shape, dtype=want, device=buf0.device)
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.dtype == want and
                out.numel() == n):
            raise ValueError("`out` must be a contiguous cuda tensor of the array's shape and the stream's type")
        return out, C.c_void_p(out.data_ptr())
    npdt = np.float32 if dt == FLOAT else np.float64
    if out is None:
        out = np.empty(shape, dtype=npdt)
    if not (isinstance(out, np.ndarray) and out.flags.c_contiguous and out.flags.writeable and out.dtype == npdt and
            out.size == n):
        raise ValueError("`out` must be a writeable C-contiguous numpy array of the array's shape and type")
    return out, C.c_void_p(out.ctypes.data)


def decompress_layers(bufs, config=None, out=None):
    """mgh_decompress_layers: the array after the layers `bufs` (compress_layers' containers, from layer 0 on, in
    order): one decode and one stream over the coefficients per layer, then one recomposition. A numpy array
    (host containers) or a cuda tensor. decompress_layers([b]) is decompress(b), bit for bit."""
    L = _hl()
    cfg = config if config is not None else Config()
    bufs = list(bufs)
    k = len(bufs)
    ptrs = [_container_ptr(b) for b in bufs]
    if k == 0:
        raise ValueError("decompress_layers needs at least layer 0")
    out, optr = _layers_out(bufs[0], out)
    _check(L.mgh_decompress_layers(k, (C.c_void_p * k)(*[p[0].value for p in ptrs]), (C.c_size_t * k)(*[p[1] for p in ptrs]),
                                   C.byref(cfg), C.byref(optr), 1))
    return out


def compress_level_layers(data, tols, s=INF, mode=REL, coords=None, config=None, outs=None):
    """mgh_compress_level_layers: compress_layers with level-linearised (reorder = 1) records, whatever
    config.reorder says -- a set that refines by tolerance AND by resolution: LevelLayers / decompress_level_layers
    read level L of layer k from the head of that layer's record. bufs[0] is compress(data, tols[0], reorder = 1)'s
    container; every layer is an ordinary container (decompress, decompress(level=), Progressive open it).
    Refused: a configuration that decomposes the domain, a layer that would be stored raw."""
    return compress_ladder(data, tols, s, mode, coords, config, outs, _call="mgh_compress_level_layers")


def decompress_level_layers(bufs, level, config=None, out=None):
    """mgh_decompress_level_layers: level `level` of the array after the layers `bufs` (compress_level_layers'
    containers, from layer 0 on, in order), every layer read up to that level: per layer a prefix decode and one
    stream over the head of the coefficients, then one recomposition of that head."""
    L = _hl()
    cfg = config if config is not None else Config()
    bufs = list(bufs)
    k = len(bufs)
    ptrs = [_container_ptr(b) for b in bufs]
    if k == 0:
        raise ValueError("decompress_level_layers needs at least layer 0")
    args = (k, (C.c_void_p * k)(*[p[0].value for p in ptrs]), (C.c_size_t * k)(*[p[1] for p in ptrs]), int(level), C.byref(cfg))
    try:
        known = int(level) >= 0 and infer_level(bufs[0], int(level), cfg)[0] is not None
    except MgardHipError:
        known = False
    if not known:
        # no such level, or no container that has levels: the call says which (it refuses before it allocates)
        _check(L.mgh_decompress_level_layers(*args, C.byref(C.c_void_p()), 0))
        raise MgardHipError("decompress_level_layers: the level's shape is unknown")
    out, optr = _layers_out(bufs[0], out, int(level), cfg)
    _check(L.mgh_decompress_level_layers(*args, C.byref(optr), 1))
    return out


# ---- arrays with missing values -------------------------------------------------------------------------------
def compress_masked(data, tol, s=INF, mode=REL, nonfinite=True, fill_value=None, restore_value=float("nan"), coords=None,
                    config=None, out=None):
    """mgh_compress_masked: compress(data) with the NaN / +-Inf (`nonfinite`) and / or the elements equal to
    `fill_value` left out of the bound. Returns [container][mask record][48-byte footer]: buf[:C], with C =
    masked_info(buf).container_size, is the ordinary container of the deterministically filled array and opens in
    every reader; decompress_masked puts `restore_value` at the masked positions. The bound holds at every valid
    position. Host array in, numpy buffer out; cuda tensor in, cuda buffer out. `out`: optional pre-allocated uint8
    buffer of the same kind (its size is the capacity)."""
    from . import mask_flags
    L = _hl()
    cfg = config if config is not None else Config()
    ptr, dt, shape, keep = _as_ptr(data)
    _wait_for_current_stream(out)
    D = len(shape)
    shp = (C.c_uint64 * D)(*shape)
    cptr, ckeep = _coords_ptr(coords, dt, D)
    n = int(np.prod(shape))
    out, optr, size = _writer_out(data, out, n * (4 if dt == FLOAT else 8) + 1000000 + 8 * ((n + 63) // 64) + 48)
    spec = MaskSpec(mask_flags(nonfinite, fill_value), 0.0 if fill_value is None else float(fill_value), float(restore_value))
    _check(L.mgh_compress_masked(D, dt, shp, float(tol), float(s), int(mode), ptr, C.byref(spec), C.byref(optr),
                                 C.byref(size), cptr, C.byref(cfg), 1))
    del keep, ckeep
    return out[:size.value]


def masked_info(buf):
    """mgh_masked_info: the MaskedInfo of a masked buffer, None for a buffer without the footer (a plain container);
    MgardHipError for a footer that fails a check."""
    p, n, _, keep = _container_ptr(buf)
    info = MaskedInfo()
    rc = _check(_hl().mgh_masked_info(p, n, C.byref(info)))
    del keep
    return info if rc == 1 else None


def _footed_full(call, info_of, buf, cfg, out):
    """The full array of a buffer with a footer (`info_of`: masked_info or pwrel_info; `call`: its C reader) into `out`
    or a new array shaped by the container part. A buffer without the footer: the library's own refusal is raised."""
    p, n, _, keep = _container_ptr(buf)
    info = info_of(keep)
    if info is None:
        _check(call(p, n, C.byref(cfg), C.byref(C.c_void_p()), 0))  # (raises: no footer)
    out, optr = _layers_out(keep[:info.container_size], out)
    _check(call(p, n, C.byref(cfg), C.byref(optr), 1))
    return out


def _masked_view(buf, cfg, level, coarsen, window, what):
    """(pointer, size, on_device, keepalive, container part, shape of the view) of a masked buffer and one of the
    views level / coarsen / window (at most one of them; none: the full array)."""
    if sum(x is not None for x in (level, coarsen, window)) > 1:
        raise ValueError("%s: pass at most one of `level`, `coarsen` and `window`" % what)
    p, n, on_dev, keep = _container_ptr(buf)
    info = masked_info(keep)
    if info is None:
        raise MgardHipError("mgard_hip error -8: %s: no mask footer (a plain container has the plain reader)" % what)
    cont = keep[:info.container_size]
    if level is not None:
        shape, _ = infer_level(cont, int(level), cfg)
    elif coarsen is not None:
        if int(coarsen) < 0:
            raise ValueError("coarsen must be >= 0")
        shape, _ = infer_coarsened(cont, int(coarsen), cfg)
    else:
        shape = infer(cont)[0]
    return p, n, on_dev, keep, cont, shape


def _masked_out(cont, shape, out):
    """`out`, or a new array of `shape`, for the array of the container `cont`, as (out, pointer): a cuda tensor for a
    device container, a numpy array for a host one."""
    import torch
    _, dt = infer(cont)
    _wait_for_current_stream(out)
    n = int(np.prod(shape))
    if isinstance(cont, torch.Tensor) and cont.is_cuda:
        want = torch.float32 if dt == FLOAT else torch.float64
        if out is None:
            out = torch.empty(tuple(shape), dtype=want, device=cont.device)
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.dtype == want and
                out.device == cont.device and out.numel() == n):
            raise ValueError("`out` must be a contiguous cuda tensor of the view's shape and the stream's type")
        return out, C.c_void_p(out.data_ptr())
    npdt = np.float32 if dt == FLOAT else np.float64
    if out is None:
        out = np.empty(tuple(shape), dtype=npdt)
    if not (isinstance(out, np.ndarray) and out.flags.c_contiguous and out.flags.writeable and out.dtype == npdt and
            out.size == n):
        raise ValueError("`out` must be a writeable C-contiguous numpy array of the view's shape and type")
    return out, C.c_void_p(out.ctypes.data)


def decompress_masked(buf, config=None, out=None, level=None, coarsen=None):
    """mgh_decompress_masked: the array of a masked buffer with restore_value at every masked position. A numpy array
    (host buffer) or a cuda tensor; `out` as for decompress_layers. A plain container is refused: it has decompress.
    `level` / `coarsen`: mgh_decompress_masked_level / _coarsened -- decompress(buf[:C], level=...) or (coarsen=...)
    with restore_value at every node whose element of the FULL array is masked (sampling: masked neighbours do not
    count). The valid nodes are those of the filled array's hierarchy: near masked regions they carry the fill's
    influence."""
    L = _hl()
    cfg = config if config is not None else Config()
    if level is None and coarsen is None:
        return _footed_full(L.mgh_decompress_masked, masked_info, buf, cfg, out)
    p, n, _, keep, cont, shape = _masked_view(buf, cfg, level, coarsen, None, "decompress_masked")
    out, optr = _masked_out(cont, shape, out)
    if level is not None:
        _check(L.mgh_decompress_masked_level(p, n, int(level), C.byref(optr), C.byref(cfg), 1))
    else:
        _check(L.mgh_decompress_masked_coarsened(p, n, int(coarsen), C.byref(optr), C.byref(cfg), 1))
    del keep
    return out


def decompress_masked_preview(buf, coarsen, config=None, out=None, window=None):
    """mgh_decompress_masked_preview(_window): decompress_preview(buf[:C], coarsen, window=window) with restore_value at
    every position of the array (of the window) that is masked in the full array. A preview carries no bound."""
    if coarsen is None:
        raise ValueError("decompress_masked_preview needs `coarsen`")
    if int(coarsen) < 0:
        raise ValueError("coarsen must be >= 0")
    L = _hl()
    cfg = config if config is not None else Config()
    p, n, _, keep, cont, shape = _masked_view(buf, cfg, None, None, None, "decompress_masked_preview")
    if window is None:
        out, optr = _masked_out(cont, shape, out)
        _check(L.mgh_decompress_masked_preview(p, n, int(coarsen), C.byref(optr), C.byref(cfg), 1))
    else:
        wlo, wext = _window_args(window, len(shape))
        out, optr = _masked_out(cont, tuple(int(e) for e in wext), out)
        _check(L.mgh_decompress_masked_preview_window(p, n, int(coarsen), wlo, wext, C.byref(optr), C.byref(cfg), 1))
    del keep
    return out


def decompress_mask(buf, config=None, level=None, coarsen=None, window=None):
    """mgh_decompress_mask: the mask of a masked buffer as a bool array of the data's shape (numpy for a host buffer, a
    cuda tensor for a device one). `level` / `coarsen` / window = (lo, ext): mgh_decompress_mask_level / _coarsened /
    _window -- the mask sampled at the nodes of that level array or coarsened array, or the box of it."""
    import torch
    L = _hl()
    cfg = config if config is not None else Config()
    p, n, on_dev, keep, cont, shape = _masked_view(buf, cfg, level, coarsen, window, "decompress_mask")
    if window is not None:
        wlo, wext = _window_args(window, len(shape))
        shape = tuple(int(e) for e in wext)
    if on_dev:
        mask = torch.empty(tuple(shape), dtype=torch.uint8, device=keep.device)
        mp = C.c_void_p(mask.data_ptr())
    else:
        mask = np.empty(tuple(shape), dtype=np.uint8)
        mp = C.c_void_p(mask.ctypes.data)
    if level is not None:
        _check(L.mgh_decompress_mask_level(p, n, int(level), C.byref(cfg), mp))
    elif coarsen is not None:
        _check(L.mgh_decompress_mask_coarsened(p, n, int(coarsen), C.byref(cfg), mp))
    elif window is not None:
        _check(L.mgh_decompress_mask_window(p, n, wlo, wext, C.byref(cfg), mp))
    else:
        _check(L.mgh_decompress_mask(p, n, C.byref(cfg), mp))
    del keep
    return mask.bool() if on_dev else mask.astype(bool)


def verify_masked(buf, original, config=None, coarsen=0):
    """mgh_verify_masked: (VerifyResult, n_masked) of a masked buffer against `original`, the user's own array with its
    NaN / +-Inf / fill values. Masked positions take part in nothing: stats.n counts the valid positions. s = inf:
    achieved = max_abs_err over them; s = 0: sqrt(sum_sq_err / N) with N ALL elements (the writer's guarantee is over
    the whole filled array). coarsen > 0 as in verify (within = -1)."""
    L = _hl()
    cfg = config if config is not None else Config()
    p, n, _, keep = _container_ptr(buf)
    optr, dt, shape, okeep = _as_ptr(original)
    nbytes = int(np.prod(shape)) * (4 if dt == FLOAT else 8)
    out = VerifyResult()
    n_masked = C.c_uint64(0)
    _check(L.mgh_verify_masked(p, n, optr, nbytes, dt, int(coarsen), C.byref(cfg), C.byref(out), C.byref(n_masked)))
    del keep, okeep
    return out, int(n_masked.value)


# ---- pointwise relative error bound ---------------------------------------------------------------------------
def compress_pwrel(data, eps, abs_floor=0.0, coords=None, config=None, out=None):
    """mgh_compress_pwrel: |x' - x| <= eps |x| at every element whose |x| >= max(abs_floor, smallest normal); +-0,
    denormals and smaller values decode to +0.0, NaN / +-Inf to NaN. Returns [masked buffer of y = log2|x|][flag
    record][56-byte footer]: buf[:pwrel_info(buf).masked_size] opens in decompress_masked, and its container part in
    every reader, as y. 0 < eps < 1; an eps the data type cannot carry at the field's dynamic range raises. Host array
    in, numpy buffer out; cuda tensor in, cuda buffer out. `out`: optional pre-allocated uint8 buffer of the same kind
    (its size is the capacity)."""
    L = _hl()
    cfg = config if config is not None else Config()
    ptr, dt, shape, keep = _as_ptr(data)
    _wait_for_current_stream(out)
    D = len(shape)
    shp = (C.c_uint64 * D)(*shape)
    cptr, ckeep = _coords_ptr(coords, dt, D)
    n = int(np.prod(shape))
    out, optr, size = _writer_out(data, out, n * (4 if dt == FLOAT else 8) + 1000000 + 16 * ((n + 63) // 64) + 48 + 56)
    _check(L.mgh_compress_pwrel(D, dt, shp, float(eps), float(abs_floor), ptr, C.byref(optr), C.byref(size), cptr,
                                C.byref(cfg), 1))
    del keep, ckeep
    return out[:size.value]


def pwrel_info(buf):
    """mgh_pwrel_info: the PwrelInfo of a pointwise-relative buffer, None for a buffer without its footer (a plain
    container, a masked buffer); MgardHipError for a footer that fails a check."""
    p, n, _, keep = _container_ptr(buf)
    info = PwrelInfo()
    rc = _check(_hl().mgh_pwrel_info(p, n, C.byref(info)))
    del keep
    return info if rc == 1 else None


def _pwrel_view(buf, cfg, level, coarsen, what):
    """(pointer, size, keepalive, container part, shape of the view) of a pointwise-relative buffer and one of the views
    level / coarsen (at most one of them; none: the full array). Any other buffer: the library's own refusal."""
    if level is not None and coarsen is not None:
        raise ValueError("%s: pass at most one of `level` and `coarsen`" % what)
    L = _hl()
    p, n, _, keep = _container_ptr(buf)
    info = pwrel_info(keep)
    if info is None:  # (raises: no footer)
        call = (L.mgh_decompress_pwrel_level if level is not None else
                L.mgh_decompress_pwrel_coarsened if coarsen is not None else L.mgh_decompress_pwrel_preview)
        _check(call(p, n, 0, C.byref(C.c_void_p()), C.byref(cfg), 0))
        raise MgardHipError("%s: a buffer without the pointwise-relative footer was not refused" % what)
    cont = keep[:info.container_size]
    if level is not None:
        shape, _ = infer_level(cont, int(level), cfg)
    elif coarsen is not None:
        if int(coarsen) < 0:
            raise ValueError("coarsen must be >= 0")
        shape, _ = infer_coarsened(cont, int(coarsen), cfg)
    else:
        shape = infer(cont)[0]
    return p, n, keep, cont, shape


def decompress_pwrel(buf, config=None, out=None, level=None, coarsen=None):
    """mgh_decompress_pwrel: the array of a pointwise-relative buffer. A numpy array (host buffer) or a cuda tensor;
    `out` as for decompress_layers. Any other buffer is refused.
    `level` / `coarsen`: mgh_decompress_pwrel_level / _coarsened -- every node takes its class and sign from the element
    of the FULL array it stands on (sampling): NaN, +0.0, or +-exp2 of what decompress(buf[:C], level=...) or
    (coarsen=...) gives for y. Such an array carries no error bound, and near zeroed or non-finite elements it carries
    the fill's influence. level = l_target and coarsen = 0 are the full array, bit for bit."""
    L = _hl()
    cfg = config if config is not None else Config()
    if level is None and coarsen is None:
        return _footed_full(L.mgh_decompress_pwrel, pwrel_info, buf, cfg, out)
    p, n, keep, cont, shape = _pwrel_view(buf, cfg, level, coarsen, "decompress_pwrel")
    out, optr = _masked_out(cont, shape, out)
    if level is not None:
        _check(L.mgh_decompress_pwrel_level(p, n, int(level), C.byref(optr), C.byref(cfg), 1))
    else:
        _check(L.mgh_decompress_pwrel_coarsened(p, n, int(coarsen), C.byref(optr), C.byref(cfg), 1))
    del keep
    return out


def decompress_pwrel_preview(buf, coarsen, config=None, out=None, window=None):
    """mgh_decompress_pwrel_preview(_window): NaN, +0.0 or +-exp2 of decompress_preview(buf[:C], coarsen, window=window),
    by the class and sign of every position of the array (of the window) in the full array. A preview carries no
    bound; coarsen = 0 is decompress_pwrel."""
    if coarsen is None:
        raise ValueError("decompress_pwrel_preview needs `coarsen`")
    if int(coarsen) < 0:
        raise ValueError("coarsen must be >= 0")
    L = _hl()
    cfg = config if config is not None else Config()
    p, n, keep, cont, shape = _pwrel_view(buf, cfg, None, None, "decompress_pwrel_preview")
    if window is None:
        out, optr = _masked_out(cont, shape, out)
        _check(L.mgh_decompress_pwrel_preview(p, n, int(coarsen), C.byref(optr), C.byref(cfg), 1))
    else:
        wlo, wext = _window_args(window, len(shape))
        out, optr = _masked_out(cont, tuple(int(e) for e in wext), out)
        _check(L.mgh_decompress_pwrel_preview_window(p, n, int(coarsen), wlo, wext, C.byref(optr), C.byref(cfg), 1))
    del keep
    return out


def verify_pwrel(buf, original, config=None):
    """mgh_verify_pwrel: (PwrelCompare, within) of a pointwise-relative buffer against `original`, the user's own array.
    within: max_rel_err <= eps, no class or sign mismatch, and nothing at or above the floor zeroed."""
    from . import PwrelCompare
    L = _hl()
    cfg = config if config is not None else Config()
    p, n, _, keep = _container_ptr(buf)
    optr, dt, shape, okeep = _as_ptr(original)
    nbytes = int(np.prod(shape)) * (4 if dt == FLOAT else 8)
    out = PwrelCompare()
    within = C.c_int(0)
    _check(L.mgh_verify_pwrel(p, n, optr, nbytes, dt, C.byref(cfg), C.byref(out), C.byref(within)))
    del keep, okeep
    return out, int(within.value)


# ---- region of interest: a tighter pointwise bound inside boxes ---------------------------------------------------
def compress_roi(data, tol, boxes, s=INF, mode=REL, coords=None, config=None, out=None):
    """mgh_compress_roi: `data` within `tol` (ABS, or REL: times the norm) everywhere and within tol_i inside every box
    of boxes = [(lo, ext, tol_i), ...] -- up to 16 disjoint boxes, every extent at least 3, 0 < tol_i < tol, s infinite.
    Returns [container][one record per box][box table][footer]: buf[:roi_info(buf).container_size] is, up to the order of
    the outlier pairs inside a record, byte for byte compress(data, tol) and opens in every plain reader as the unrefined base. A tol_i the data type cannot carry
    raises. Host array in, numpy buffer out; cuda tensor in, cuda buffer out. `out`: optional pre-allocated uint8
    buffer of the same kind (its size is the capacity)."""
    L = _hl()
    cfg = config if config is not None else Config()
    ptr, dt, shape, keep = _as_ptr(data)
    _wait_for_current_stream(out)
    D = len(shape)
    shp = (C.c_uint64 * D)(*shape)
    cptr, ckeep = _coords_ptr(coords, dt, D)
    boxes = list(boxes)
    cbox = (RoiBox * max(len(boxes), 1))()
    elem, room = (4 if dt == FLOAT else 8), 0
    for cb, (lo, ext, tol_i) in zip(cbox, boxes):
        if len(lo) != D or len(ext) != D:
            raise ValueError("compress_roi: `lo` and `ext` of a box must have the data's number of dimensions")
        cb.lo[:D] = [int(v) for v in lo]
        cb.ext[:D] = [int(v) for v in ext]
        cb.tol = float(tol_i)
        room += int(np.prod([int(v) for v in ext])) * elem + 1000000 + 120
    n = int(np.prod(shape))
    out, optr, size = _writer_out(data, out, n * elem + 1000000 + room + 40)
    _check(L.mgh_compress_roi(D, dt, shp, float(tol), float(s), int(mode), ptr, len(boxes), cbox, C.byref(optr), C.byref(size),
                              cptr, C.byref(cfg), 1))
    del keep, ckeep
    return out[:size.value]


def roi_info(buf):
    """mgh_roi_info: the RoiInfo of a buffer with boxes, None for a buffer without its footer (a plain container, a
    masked or pointwise-relative buffer); MgardHipError for a footer or table that fails a check."""
    p, n, _, keep = _container_ptr(buf)
    info = RoiInfo()
    rc = _check(_hl().mgh_roi_info(p, n, C.byref(info)))
    del keep
    return info if rc == 1 else None


def decompress_roi(buf, config=None, out=None):
    """mgh_decompress_roi: the array of a buffer with boxes -- decompress of its container part with every box's
    decoded residual added in place. A numpy array (host buffer) or a cuda tensor; `out`: optional pre-allocated
    array of the same kind. Any other buffer: the library's own refusal is raised."""
    L = _hl()
    cfg = config if config is not None else Config()
    p, n, _, keep = _container_ptr(buf)
    info = roi_info(keep)
    if info is None:
        _check(L.mgh_decompress_roi(p, n, C.byref(C.c_void_p()), C.byref(cfg), 0))  # (raises: no footer)
    out, optr = _layers_out(keep[:info.container_size], out)
    _check(L.mgh_decompress_roi(p, n, C.byref(optr), C.byref(cfg), 1))
    return out


def verify_roi(buf, original, config=None):
    """mgh_verify_roi: (whole, per_box) of a buffer with boxes against `original`, the user's own array: a VerifyResult
    over the entire array against the base bound, and one per box against that box's bound."""
    L = _hl()
    cfg = config if config is not None else Config()
    p, n, _, keep = _container_ptr(buf)
    info = roi_info(keep)
    nbox = info.nbox if info is not None else 1
    optr, dt, shape, okeep = _as_ptr(original)
    nbytes = int(np.prod(shape)) * (4 if dt == FLOAT else 8)
    whole, per_box = VerifyResult(), (VerifyResult * nbox)()
    _check(L.mgh_verify_roi(p, n, optr, nbytes, dt, C.byref(cfg), C.byref(whole), per_box))
    del keep, okeep
    return whole, list(per_box)


class Layers:
    """mgh_layers: the reader of precision layers -- the coefficients stay on the device, a layer is added when
    it arrives, an array is recomposed when it is wanted.

        with Layers(bufs[0], config) as r:
            coarse = r.data()
            fine = r.add(bufs[1]).add(bufs[2]).data()

    The containers are read during the call only. Their order is the caller's: a layer whose tolerance is not
    below the last one's, or that belongs to another array, raises and leaves the reader as it was."""

    def __init__(self, buf0, config=None):
        self._p = C.c_void_p()
        self._cfg = config if config is not None else Config()
        self._buf0 = buf0
        p, n, _, keep = _container_ptr(buf0)
        _check(_hl().mgh_layers_open(C.byref(self._p), p, n, C.byref(self._cfg)))

    def _open(self):
        if not self._p:
            raise MgardHipError("the reader is closed")
        return self._p

    @property
    def count(self):
        """Layers added so far, layer 0 included."""
        return int(_hl().mgh_layers_count(self._open()))

    @property
    def tolerance(self):
        """The tolerance of the last layer added (its header's)."""
        return float(_hl().mgh_layers_tolerance(self._open()))

    def add(self, buf):
        p, n, _, keep = _container_ptr(buf)
        _check(_hl().mgh_layers_add(self._open(), p, n))
        return self

    def data(self, out=None, level=None):
        """mgh_layers_data: the recomposition of the coefficients as they stand; the reader goes on. level = L:
        mgh_layers_data_level, the array of that level of the hierarchy only (what LevelLayers.data(L) answers)."""
        if level is not None:
            out, optr = _layers_out(self._buf0, out, int(level), self._cfg)
            _check(_hl().mgh_layers_data_level(self._open(), int(level), C.byref(optr), 1))
            return out
        out, optr = _layers_out(self._buf0, out)
        _check(_hl().mgh_layers_data(self._open(), C.byref(optr), 1))
        return out

    def close(self):
        if self._p:
            _hl().mgh_layers_close(self._p)
            self._p = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LevelLayers:
    """mgh_level_layers: the reader of precision layers in level order (compress_level_layers' containers) -- the
    coefficients stay on the device in level-linearised order, and every layer is read up to a level of its own:

        with LevelLayers(bufs[0], level=L - 2, config=cfg) as r:
            quick = r.data(L - 2)                       # coarse grid, loose tolerance
            r.add(bufs[1], L - 2)                       # ... a tighter tolerance on that grid
            full = r.extend(0, bufs[0], L).data(L)      # ... the full grid at layer 0's tolerance

    depth(k) never exceeds depth(k - 1); data(level) needs level <= depth(0). A call that breaks a rule raises and
    leaves the reader as it was. The containers are read during the call only."""

    def __init__(self, buf0, level, config=None):
        self._p = C.c_void_p()
        self._cfg = config if config is not None else Config()
        self._buf0 = buf0
        p, n, _, keep = _container_ptr(buf0)
        _check(_hl().mgh_level_layers_open(C.byref(self._p), p, n, C.byref(self._cfg), int(level)))

    def _open(self):
        if not self._p:
            raise MgardHipError("the reader is closed")
        return self._p

    @property
    def count(self):
        """Layers added so far, layer 0 included."""
        return int(_hl().mgh_level_layers_count(self._open()))

    def depth(self, k):
        """The level up to which layer k has been added."""
        return int(_hl().mgh_level_layers_depth(self._open(), int(k)))

    def tolerance(self, k):
        """The tolerance of layer k (its header's)."""
        return float(_hl().mgh_level_layers_tolerance(self._open(), int(k)))

    def add(self, buf, level):
        p, n, _, keep = _container_ptr(buf)
        _check(_hl().mgh_level_layers_add(self._open(), p, n, int(level)))
        return self

    def extend(self, k, buf, level):
        p, n, _, keep = _container_ptr(buf)
        _check(_hl().mgh_level_layers_extend(self._open(), int(k), p, n, int(level)))
        return self

    def data(self, level, out=None):
        """mgh_level_layers_data: level `level` (<= depth(0)) of the coefficients as they stand; the reader goes on."""
        out, optr = _layers_out(self._buf0, out, int(level), self._cfg)
        _check(_hl().mgh_level_layers_data(self._open(), int(level), C.byref(optr), 1))
        return out

    def close(self):
        if self._p:
            _hl().mgh_level_layers_close(self._p)
            self._p = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def last_compress_stats():
    """mgh_last_compress_stats as a dict: decompositions, quantize_passes, histogram_launches, records,
    raw_records, outlier_retries of the last writing call of this thread."""
    st = CompressStats()
    _check(_hl().mgh_last_compress_stats(C.byref(st)))
    return {k: int(getattr(st, k)) for k, _ in CompressStats._fields_}


def infer(buf):
    """(shape, dtype code) of a compressed stream (numpy uint8 array or cuda uint8 tensor)."""
    import torch
    L = _hl()
    if isinstance(buf, torch.Tensor):
        _wait_for_current_stream(buf)
        p, n = C.c_void_p(buf.data_ptr()), buf.numel()
    else:
        buf = np.ascontiguousarray(buf)
        p, n = C.c_void_p(buf.ctypes.data), buf.size
    D = C.c_int()
    shp = (C.c_uint64 * MAX_DIM)()
    _check(L.mgh_infer_shape(p, n, C.byref(D), shp))
    dt = C.c_int()
    _check(L.mgh_infer_data_type(p, n, C.byref(dt)))
    return tuple(int(shp[d]) for d in range(D.value)), dt.value


def infer_level(buf, level, config=None):
    """mgh_infer_level_shape: (shape of `level`, l_target) of the hierarchy of a compressed stream;
    level = None or < 0: (None, l_target). `config` carries max_larget_level as for decompress."""
    import torch
    L = _hl()
    cfg = config if config is not None else Config()
    if isinstance(buf, torch.Tensor):
        _wait_for_current_stream(buf)
        p, n = C.c_void_p(buf.data_ptr()), buf.numel()
    else:
        buf = np.ascontiguousarray(buf)
        p, n = C.c_void_p(buf.ctypes.data), buf.size
    level = -1 if level is None else int(level)
    D, lt = C.c_int(), C.c_int()
    shp = (C.c_uint64 * MAX_DIM)()
    _check(L.mgh_infer_level_shape(p, n, C.byref(cfg), level, C.byref(D), shp, C.byref(lt)))
    if level < 0:
        return None, lt.value
    return tuple(int(shp[d]) for d in range(D.value)), lt.value


def infer_level_nodes(buf, level, dim, config=None):
    """mgh_infer_level_nodes: index in the finest grid of every node of `level` along `dim`."""
    import torch
    L = _hl()
    if level < 0:
        raise ValueError("level must be >= 0 (infer_level(buf, None) gives l_target)")
    cfg = config if config is not None else Config()
    if isinstance(buf, torch.Tensor):
        _wait_for_current_stream(buf)
        p, n = C.c_void_p(buf.data_ptr()), buf.numel()
    else:
        buf = np.ascontiguousarray(buf)
        p, n = C.c_void_p(buf.ctypes.data), buf.size
    shape, _ = infer(buf)
    cap = shape[dim] if 0 <= dim < len(shape) else 1
    out = (C.c_uint64 * cap)()
    k = _check(L.mgh_infer_level_nodes(p, n, C.byref(cfg), int(level), int(dim), out, cap))
    return np.array(out[:k], dtype=np.int64)


def infer_coarsened(buf, halvings, config=None):
    """mgh_infer_coarsened_shape: (shape of the array after `halvings` coarsenings of every subdomain, K) with
    K the largest number of halvings the container allows; halvings = None or < 0: (None, K). Works on
    domain-decomposed containers; `config` carries max_larget_level and the sizes of a Variable decomposition."""
    import torch
    L = _hl()
    cfg = config if config is not None else Config()
    if isinstance(buf, torch.Tensor):
        _wait_for_current_stream(buf)
        p, n = C.c_void_p(buf.data_ptr()), buf.numel()
    else:
        buf = np.ascontiguousarray(buf)
        p, n = C.c_void_p(buf.ctypes.data), buf.size
    halvings = -1 if halvings is None else int(halvings)
    D, K = C.c_int(), C.c_int()
    shp = (C.c_uint64 * MAX_DIM)()
    _check(L.mgh_infer_coarsened_shape(p, n, C.byref(cfg), halvings, C.byref(D), shp, C.byref(K)))
    if halvings < 0:
        return None, K.value
    return tuple(int(shp[d]) for d in range(D.value)), K.value


def infer_coarsened_nodes(buf, halvings, dim, config=None):
    """mgh_infer_coarsened_nodes: index in the FULL array of every node along `dim` of the array that
    decompress(buf, coarsen=halvings) returns. The coordinates of that array are the full grid's at these
    indices (the stitched grid of a decomposed container is not uniform)."""
    import torch
    L = _hl()
    if halvings < 0:
        raise ValueError("halvings must be >= 0 (infer_coarsened(buf, None) gives the largest number)")
    cfg = config if config is not None else Config()
    if isinstance(buf, torch.Tensor):
        _wait_for_current_stream(buf)
        p, n = C.c_void_p(buf.data_ptr()), buf.numel()
    else:
        buf = np.ascontiguousarray(buf)
        p, n = C.c_void_p(buf.ctypes.data), buf.size
    shape, _ = infer(buf)
    cap = shape[dim] if 0 <= dim < len(shape) else 1
    out = (C.c_uint64 * cap)()
    k = _check(L.mgh_infer_coarsened_nodes(p, n, C.byref(cfg), int(halvings), int(dim), out, cap))
    return np.array(out[:k], dtype=np.int64)


def infer_level_range(buf, level, config=None):
    """mgh_infer_level_range: (first_elem, num_elems, first_chunk, num_chunks) of the coefficients of
    `level` in a level-linearised (reorder = 1) record; host only."""
    import torch
    L = _hl()
    cfg = config if config is not None else Config()
    if isinstance(buf, torch.Tensor):
        _wait_for_current_stream(buf)
        p, n = C.c_void_p(buf.data_ptr()), buf.numel()
    else:
        buf = np.ascontiguousarray(buf)
        p, n = C.c_void_p(buf.ctypes.data), buf.size
    v = [C.c_uint64() for _ in range(4)]
    _check(L.mgh_infer_level_range(p, n, C.byref(cfg), int(level), *[C.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


class Progressive:
    """mgh_progressive: a reduced-resolution reconstruction of a reorder = 1 container refined level by
    level -- every Huffman chunk decoded once, every level's solves run once.

        with Progressive(buf, config) as p:
            preview = p.refine(2)
            better = p.refine(3)

    `buf` (numpy uint8 array or cuda uint8 tensor) is borrowed until close()."""

    def __init__(self, buf, config=None):
        import torch
        self._p = C.c_void_p()
        self._cfg = config if config is not None else Config()
        self._on_dev = isinstance(buf, torch.Tensor) and buf.is_cuda
        if not self._on_dev:
            buf = np.ascontiguousarray(buf)
        _wait_for_current_stream(buf)
        self._buf = buf
        self._dt = infer(buf)[1]
        p, n = (C.c_void_p(buf.data_ptr()), buf.numel()) if self._on_dev else (C.c_void_p(buf.ctypes.data), buf.size)
        _check(_hl().mgh_progressive_open(C.byref(self._p), p, n, C.byref(self._cfg)))

    @property
    def level(self):
        """The level of the last refine; -1 before the first one."""
        return int(_hl().mgh_progressive_level(self._p)) if self._p else -1

    def refine(self, level, out=None):
        """The dense array of `level` (> self.level): a numpy array (host container) or a cuda tensor."""
        import torch
        if not self._p:
            raise MgardHipError("the reader is closed")
        _wait_for_current_stream(self._buf, out)
        shape, _ = infer_level(self._buf, int(level), self._cfg)
        if self._on_dev:
            want = torch.float32 if self._dt == FLOAT else torch.float64
            if out is None:
                out = torch.empty(shape, dtype=want, device=self._buf.device)
            if not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.dtype == want and
                    out.numel() == int(np.prod(shape))):
                raise ValueError("`out` must be a contiguous cuda tensor of the level's shape and the stream's type")
            optr = C.c_void_p(out.data_ptr())
        else:
            npdt = np.float32 if self._dt == FLOAT else np.float64
            if out is None:
                out = np.empty(shape, dtype=npdt)
            if not (isinstance(out, np.ndarray) and out.flags.c_contiguous and out.flags.writeable and
                    out.dtype == npdt and out.size == int(np.prod(shape))):
                raise ValueError("`out` must be a writeable C-contiguous numpy array of the level's shape and type")
            optr = C.c_void_p(out.ctypes.data)
        _check(_hl().mgh_progressive_refine(self._p, int(level), C.byref(optr), 1))
        return out

    def preview(self, out=None, window=None):
        """mgh_progressive_preview: the current level prolonged to the container's own grid -- an array
        of infer(buf)[0], equal to decompress_preview(buf, l_target - level). Needs one
        refine before it and leaves the reader's state as it is.
        window = (lo, ext): mgh_progressive_preview_window -- the box [lo, lo + ext) of that array alone."""
        import torch
        if not self._p:
            raise MgardHipError("the reader is closed")
        _wait_for_current_stream(self._buf, out)
        shape, _ = infer(self._buf)
        if window is not None:
            lo, ext = _window_args(window, len(shape))
            shape = tuple(int(e) for e in ext)
        if self._on_dev:
            want = torch.float32 if self._dt == FLOAT else torch.float64
            if out is None:
                out = torch.empty(shape, dtype=want, device=self._buf.device)
            if not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.dtype == want and
                    out.numel() == int(np.prod(shape))):
                raise ValueError("`out` must be a contiguous cuda tensor of the array's shape and the stream's type")
            optr = C.c_void_p(out.data_ptr())
        else:
            npdt = np.float32 if self._dt == FLOAT else np.float64
            if out is None:
                out = np.empty(shape, dtype=npdt)
            if not (isinstance(out, np.ndarray) and out.flags.c_contiguous and out.flags.writeable and
                    out.dtype == npdt and out.size == int(np.prod(shape))):
                raise ValueError("`out` must be a writeable C-contiguous numpy array of the array's shape and type")
            optr = C.c_void_p(out.ctypes.data)
        if window is not None:
            _check(_hl().mgh_progressive_preview_window(self._p, lo, ext, C.byref(optr), 1))
        else:
            _check(_hl().mgh_progressive_preview(self._p, C.byref(optr), 1))
        return out

    def close(self):
        if self._p:
            _hl().mgh_progressive_close(self._p)
            self._p = C.c_void_p()
        self._buf = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decompress(buf, config=None, out=None, level=None, coarsen=None):
    """mgard_x::decompress. Returns a numpy array (host stream) or a cuda tensor (device stream).
    `out`: optional pre-allocated buffer -- a contiguous cuda tensor (device streams) or a
    C-contiguous numpy array (host streams). Its size and type are checked by the library against the
    header it reads anyway (mgh_decompress_into: ValueError on a mismatch, nothing written).
    `level` (extension): mgh_decompress_level -- the array at that level of the hierarchy (0 =
    coarsest, infer_level(buf, None)[1] = full), of shape infer_level(buf, level)[0]. Containers with one
    subdomain only.
    `coarsen` (extension): mgh_decompress_coarsened -- every subdomain after that many halvings of its grid,
    stitched into one array of shape infer_coarsened(buf, coarsen)[0]; domain-decomposed containers included.
    infer_coarsened_nodes tells which nodes of the full grid the result holds.
    decompress_preview(buf, k) puts the coarsened subdomains back on the full grid."""
    return _decompress(buf, config, out, level, coarsen, False)


def _window_args(window, D):
    """(lo, ext) as two uint64 arrays of D entries (the library checks them against the array)."""
    lo, ext = window
    if len(lo) != D or len(ext) != D or min(lo) < 0 or min(ext) < 0:
        raise ValueError("window: (lo, ext) with one non-negative integer per dimension each")
    return (C.c_uint64 * D)(*[int(x) for x in lo]), (C.c_uint64 * D)(*[int(x) for x in ext])


def decompress_preview(buf, coarsen, config=None, out=None, window=None):
    """mgh_decompress_preview (extension): decompress(buf, coarsen=coarsen) with every coarsened subdomain
    prolonged back to its own grid -- an array of infer(buf)[0], placed like the full decompression; per
    subdomain the recomposition with every coefficient above its level zero. coarsen = 0 is decompress.
    window = (lo, ext): mgh_decompress_preview_window -- the box [lo, lo + ext) of that array alone, of shape
    ext; subdomains the box does not meet are not opened."""
    if coarsen is None:
        raise ValueError("decompress_preview needs `coarsen`")
    return _decompress(buf, config, out, None, coarsen, True, window)


def verify(buf, original, config=None, coarsen=0):
    """mgh_verify (extension): the error statistics of `original` (numpy array or cuda tensor, the data the
    container was made from) against decompress(buf) -- coarsen = 0 -- or decompress_preview(buf, coarsen),
    without that array being made: subdomain by subdomain, each compared on the device with its box of the
    original. Returns a VerifyResult; container and original may each live on the host or the device."""
    import torch
    L = _hl()
    cfg = config if config is not None else Config()
    if isinstance(buf, torch.Tensor) and buf.is_cuda:
        buf = buf.contiguous()
        _wait_for_current_stream(buf)
        p, n = C.c_void_p(buf.data_ptr()), buf.numel()
    else:
        buf = np.ascontiguousarray(buf)
        p, n = C.c_void_p(buf.ctypes.data), buf.size
    optr, dt, shape, keep = _as_ptr(original)
    nbytes = int(np.prod(shape)) * (4 if dt == FLOAT else 8)
    out = VerifyResult()
    _check(L.mgh_verify(p, n, optr, nbytes, dt, int(coarsen), C.byref(cfg), C.byref(out)))
    del keep
    return out


def _decompress(buf, config, out, level, coarsen, full_grid, window=None):
    """The body of decompress (full_grid = False) and decompress_preview (full_grid = True: mgh_decompress_preview
    instead of mgh_decompress_coarsened, the output of the full array's shape, or of the window's)."""
    import torch
    if level is not None and coarsen is not None:
        raise ValueError("pass either `level` or `coarsen`, not both")
    L = _hl()
    cfg = config if config is not None else Config()
    on_dev = isinstance(buf, torch.Tensor) and buf.is_cuda
    if not on_dev:
        buf = np.ascontiguousarray(buf)
    _wait_for_current_stream(buf, out)
    if level is not None or coarsen is not None:
        if level is not None:
            shape, _ = infer_level(buf, int(level), cfg)
        else:
            if int(coarsen) < 0:
                raise ValueError("coarsen must be >= 0")
            shape, _ = infer_coarsened(buf, int(coarsen), cfg)  # (also refuses more halvings than there are)
            if full_grid:
                shape = infer(buf)[0]
            if window is not None:
                wlo, wext = _window_args(window, len(shape))
                shape = tuple(int(e) for e in wext)
        _, dt = infer(buf)
        want = torch.float32 if dt == FLOAT else torch.float64
        if on_dev:
            if out is None:
                out = torch.empty(shape, dtype=want, device=buf.device)
            if not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.dtype == want and
                    out.device == buf.device and out.numel() == int(np.prod(shape))):
                raise ValueError("`out` must be a contiguous cuda tensor of the level's shape and the stream's type")
            p, n, optr = C.c_void_p(buf.data_ptr()), buf.numel(), C.c_void_p(out.data_ptr())
        else:
            npdt = np.float32 if dt == FLOAT else np.float64
            if out is None:
                out = np.empty(shape, dtype=npdt)
            if not (isinstance(out, np.ndarray) and out.flags.c_contiguous and out.flags.writeable and
                    out.dtype == npdt and out.size == int(np.prod(shape))):
                raise ValueError("`out` must be a writeable C-contiguous numpy array of the level's shape and type")
            p, n, optr = C.c_void_p(buf.ctypes.data), buf.size, C.c_void_p(out.ctypes.data)
        if level is not None:
            _check(L.mgh_decompress_level(p, n, int(level), C.byref(optr), C.byref(cfg), 1))
        elif window is not None:
            _check(L.mgh_decompress_preview_window(p, n, int(coarsen), wlo, wext, C.byref(optr), C.byref(cfg), 1))
        elif full_grid:
            _check(L.mgh_decompress_preview(p, n, int(coarsen), C.byref(optr), C.byref(cfg), 1))
        else:
            _check(L.mgh_decompress_coarsened(p, n, int(coarsen), C.byref(optr), C.byref(cfg), 1))
        return out
    if out is None:
        shape, dt = infer(buf)
        if on_dev:
            out = torch.empty(shape, dtype=torch.float32 if dt == FLOAT else torch.float64, device=buf.device)
        else:
            out = np.empty(shape, dtype=np.float32 if dt == FLOAT else np.float64)
    if on_dev:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and
                out.dtype in (torch.float32, torch.float64) and out.device == buf.device):
            raise ValueError("`out` must be a contiguous float32/float64 cuda tensor on the stream's device")
        p, n, optr = C.c_void_p(buf.data_ptr()), buf.numel(), C.c_void_p(out.data_ptr())
        nbytes, odt = out.numel() * out.element_size(), FLOAT if out.dtype == torch.float32 else DOUBLE
    else:
        if not (isinstance(out, np.ndarray) and out.flags.c_contiguous and out.flags.writeable and
                out.dtype in (np.float32, np.float64)):
            raise ValueError("`out` must be a writeable C-contiguous float32/float64 numpy array")
        p, n, optr = C.c_void_p(buf.ctypes.data), buf.size, C.c_void_p(out.ctypes.data)
        nbytes, odt = out.nbytes, FLOAT if out.dtype == np.float32 else DOUBLE
    rc = L.mgh_decompress_into(p, n, optr, nbytes, odt, C.byref(cfg))
    if rc == -1 and b"mgh_decompress_into" in L.mgh_last_error():
        raise ValueError(L.mgh_last_error().decode())
    _check(rc)
    return out


def pin(a):
    """mgard_x::pin_memory on a numpy array (hipHostRegister): transfers of it run asynchronously at
    the link's rate. Undo with unpin() before the array is freed."""
    _check(_hl().mgh_pin_memory(C.c_void_p(a.ctypes.data), a.nbytes))


def is_pinned(a):
    return bool(_hl().mgh_check_memory_pinned(C.c_void_p(a.ctypes.data)))


def unpin(a):
    _check(_hl().mgh_unpin_memory(C.c_void_p(a.ctypes.data)))


def compress_multi(data, tol, s=INF, mode=REL, devices=(0,), coords=None, config=None):
    """mgh_compress_multi: slab id of the slowest dimension runs on devices[id % len(devices)] (one
    host thread per device). `data`: host numpy array -> host stream (numpy uint8), or a cuda
    tensor resident on ONE device -> cuda uint8 tensor on that device (slabs of other devices travel
    device to device)."""
    import torch
    L = _hl()
    cfg = config if config is not None else Config()
    on_device = isinstance(data, torch.Tensor) and data.is_cuda
    if on_device:
        data = data.contiguous()
        _wait_for_current_stream(data)
        np_dt = np.dtype(np.float32) if data.dtype == torch.float32 else np.dtype(np.float64)
        shape, nbytes, dptr = tuple(data.shape), data.numel() * data.element_size(), data.data_ptr()
    else:
        data = np.ascontiguousarray(data)
        np_dt, shape, nbytes, dptr = data.dtype, data.shape, data.nbytes, data.ctypes.data
    dt = {np.dtype(np.float32): FLOAT, np.dtype(np.float64): DOUBLE}[np_dt]
    D = len(shape)
    shp = (C.c_uint64 * D)(*shape)
    cptr, ckeep = None, []
    if coords is not None:
        arr = (C.c_void_p * D)()
        for d in range(D):
            c = np.ascontiguousarray(coords[d], dtype=np_dt)
            ckeep.append(c)
            arr[d] = c.ctypes.data
        cptr = arr
    devs = (C.c_int * len(devices))(*devices)
    cap = nbytes + 1000000
    if on_device:
        out = torch.empty(cap, dtype=torch.uint8, device=data.device)
        optr = C.c_void_p(out.data_ptr())
    else:
        out = np.empty(cap, dtype=np.uint8)
        optr = C.c_void_p(out.ctypes.data)
    size = C.c_size_t(cap)
    _check(L.mgh_compress_multi(len(devices), devs, D, dt, shp, float(tol), float(s), int(mode),
                                C.c_void_p(dptr), C.byref(optr), C.byref(size), cptr,
                                C.byref(cfg), 1))
    return out[:size.value]


def last_decompress_stats():
    """mgh_last_decompress_stats as a dict: subdomains, chunks_total, chunks_decoded, symbols_decoded,
    record_bytes, record_bytes_moved of the last decompress* call of this thread."""
    st = DecompressStats()
    _check(_hl().mgh_last_decompress_stats(C.byref(st)))
    return {k: int(getattr(st, k)) for k, _ in DecompressStats._fields_}


def decompress_multi(buf, devices=(0,), config=None):
    """mgh_decompress_multi: host stream in, host numpy array out."""
    L = _hl()
    cfg = config if config is not None else Config()
    shape, dt = infer(buf)
    buf = np.ascontiguousarray(buf)
    out = np.empty(shape, dtype=np.float32 if dt == FLOAT else np.float64)
    optr = C.c_void_p(out.ctypes.data)
    devs = (C.c_int * len(devices))(*devices)
    _check(L.mgh_decompress_multi(len(devices), devs, C.c_void_p(buf.ctypes.data), buf.size,
                                  C.byref(optr), C.byref(cfg), 1))
    return out


def compress_dist(comm, rank, nranks, local, tol, s=INF, mode=REL, root=0, config=None, rccl_path=None):
    """mgh_compress_dist: `comm` = the ncclComm_t (int / c_void_p) of an RCCL communicator of `nranks`
    ranks, `local` = this rank's slab (cuda tensor). Returns the container (cuda uint8 tensor) on the
    root, None elsewhere. rccl_path: the librccl the communicator was created with (when it is not
    the one already in the process / librccl.so.1)."""
    import torch
    L = _hl()
    if rccl_path is not None:
        _check(L.mgh_dist_use_library(str(rccl_path).encode()))
    cfg = config if config is not None else Config()
    local = local.contiguous()
    _wait_for_current_stream(local)
    dt = FLOAT if local.dtype == torch.float32 else DOUBLE
    shp = (C.c_uint64 * local.dim())(*local.shape)
    optr, size = C.c_void_p(), C.c_size_t(0)
    _check(L.mgh_compress_dist(C.c_void_p(int(comm)), rank, nranks, root, local.dim(), dt, shp, float(tol), float(s),
                               int(mode), C.c_void_p(local.data_ptr()), C.byref(optr), C.byref(size), None,
                               C.byref(cfg), 0))
    if rank != root:
        return None
    out = torch.empty(size.value, dtype=torch.uint8, device=local.device)
    _check(L.mgh_memcpy(C.c_void_p(out.data_ptr()), optr, size.value))
    L.mgh_free_device(optr)
    return out


def decompress_dist(comm, rank, nranks, container, local_shape, dtype, root=0, config=None, device=None):
    """mgh_decompress_dist: the root passes the container (cuda uint8 tensor), the others None; every
    rank gets its slab (cuda tensor of local_shape)."""
    import torch
    L = _hl()
    cfg = config if config is not None else Config()
    dev = container.device if container is not None else device
    out = torch.empty(tuple(local_shape), dtype=dtype, device=dev)
    _wait_for_current_stream(container)
    p = C.c_void_p(container.data_ptr()) if container is not None else None
    n = int(container.numel()) if container is not None else 0
    _check(L.mgh_decompress_dist(C.c_void_p(int(comm)), rank, nranks, root, p, n, C.c_void_p(out.data_ptr()),
                                 C.byref(cfg)))
    return out


def release_cache():
    _hl().mgh_release_cache()


# ---- lossless stage on its own ----------------------------------------------------------------
def huffman_codebook(freq):
    """(code, first, entry, keys) for a histogram (host only, no device needed)."""
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    n = f.size
    code, keys = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    first, entry = np.zeros(64, np.uint64), np.zeros(64, np.uint64)
    _check(_hl().mgh_huffman_codebook(f.ctypes.data, n, code.ctypes.data, first.ctypes.data,
                                      entry.ctypes.data, keys.ctypes.data))
    return code, first, entry, keys


class Lossless:
    """mgh_lossless_ctx: Huffman [+ Zstd] on quantized symbols held in device memory."""

    def __init__(self, dev_id=0):
        self._c = C.c_void_p()
        _check(_hl().mgh_lossless_create(C.byref(self._c), dev_id))

    def close(self):
        if self._c:
            _hl().mgh_lossless_destroy(self._c)
            self._c = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _is16(q):
        """Whether q holds 16-bit symbols (torch.uint16 or int16: the same two bytes) rather than int64 values."""
        import torch
        if q.dtype in (torch.uint16, torch.int16):
            return True
        if q.dtype != torch.int64:
            raise ValueError("symbols: expected an int64, uint16 or int16 tensor, got %s" % q.dtype)
        return False

    def compress(self, q, dict_size=8192, chunk_size=20480, lossless=HUFFMAN, zstd_level=3,
                 outlier_idx=None, outlier_val=None):
        """q: cuda int64 tensor of symbols in [0, dict_size), or a cuda uint16 / int16 tensor of them
        (mgh_lossless_compress_sym16: the same record). Returns the payload bytes."""
        import torch
        n_out = 0 if outlier_idx is None else int(outlier_idx.numel())
        pay, size = C.c_void_p(), C.c_uint64()
        fn = _hl().mgh_lossless_compress_sym16 if self._is16(q) else _hl().mgh_lossless_compress
        _check(fn(
            self._c, C.c_void_p(q.data_ptr()), q.numel(), dict_size, chunk_size, lossless, zstd_level,
            C.c_void_p(outlier_idx.data_ptr()) if n_out else None,
            C.c_void_p(outlier_val.data_ptr()) if n_out else None, n_out, C.byref(pay), C.byref(size),
            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return C.string_at(pay, size.value)

    def compress_device(self, q, out, dict_size=8192, chunk_size=20480, outlier_idx=None, outlier_val=None):
        """The record written into `out` (cuda uint8 tensor or a view of one: any byte alignment).
        q as for compress. Returns the record as a view of `out`."""
        import torch
        n_out = 0 if outlier_idx is None else int(outlier_idx.numel())
        size = C.c_uint64()
        fn = _hl().mgh_lossless_compress_device_sym16 if self._is16(q) else _hl().mgh_lossless_compress_device
        _check(fn(
            self._c, C.c_void_p(q.data_ptr()), q.numel(), dict_size, chunk_size,
            C.c_void_p(outlier_idx.data_ptr()) if n_out else None,
            C.c_void_p(outlier_val.data_ptr()) if n_out else None, n_out, C.c_void_p(out.data_ptr()),
            out.numel(), C.byref(size), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out[:size.value]

    def decompress(self, payload, n, lossless=HUFFMAN, prefix=None, out=None, first=None, count=None, sym16=False):
        """payload: bytes, or a cuda uint8 tensor (decoded where it lies). Returns (q, outlier_idx,
        outlier_val) as cuda tensors.
        prefix: decode only the chunks that hold the first `prefix` integers
        (mgh_lossless_decompress_prefix): q[0 : min(n, ceil(prefix / chunk) * chunk)] is written and
        nothing behind it; the outlier lists come whole. out: a cuda int64 tensor to decode into (with
        a prefix it need only hold what is written); default: a new one of n elements.
        first, count: decode only the chunks that hold integers [first, first + count)
        (mgh_lossless_decompress_range): q[0:] receives the integers from (first // chunk) * chunk to
        the end of the last decoded chunk (or n), nothing behind them.
        sym16: decode to 16-bit symbols (mgh_lossless_decompress_sym16) -- q and `out` are uint16
        tensors (`out` may be int16); whole record or first / count, not prefix."""
        import torch
        if (first is None) != (count is None) or (first is not None and prefix is not None):
            raise ValueError("pass first and count together, and not with prefix")
        if sym16 and prefix is not None:
            raise ValueError("sym16: pass first and count, not prefix")
        kinds = (torch.uint16, torch.int16) if sym16 else (torch.int64,)
        if out is None:
            q = torch.empty(n, dtype=kinds[0], device="cuda")
        else:
            if not (out.is_cuda and out.dtype in kinds and out.is_contiguous()):
                raise ValueError("out: expected a contiguous cuda %s tensor" % ("uint16" if sym16 else "int64"))
            if prefix is None and first is None and out.numel() < n:
                raise ValueError("out: %d elements, the record holds %d" % (out.numel(), n))
            q = out
        if isinstance(payload, torch.Tensor):
            if not (payload.is_cuda and payload.dtype == torch.uint8 and payload.dim() == 1 and
                    payload.is_contiguous()):
                raise ValueError("payload tensor must be a contiguous 1-D uint8 cuda tensor")
            if payload.device != q.device:
                raise ValueError("payload tensor is on %s, the context decodes on %s" % (payload.device, q.device))
            raw, nbytes = C.c_void_p(payload.data_ptr()), int(payload.numel())
        else:
            raw, nbytes = (C.c_uint8 * len(payload)).from_buffer_copy(payload), len(payload)
        oi, ov, cnt = C.c_void_p(), C.c_void_p(), C.c_uint64()
        if sym16:
            lo, num = (0, n) if first is None else (int(first), int(count))
            _check(_hl().mgh_lossless_decompress_sym16(
                self._c, raw, nbytes, lossless, C.c_void_p(q.data_ptr()), n, lo, num, C.byref(oi),
                C.byref(ov), C.byref(cnt), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        elif first is not None:
            _check(_hl().mgh_lossless_decompress_range(
                self._c, raw, nbytes, lossless, C.c_void_p(q.data_ptr()), n, int(first), int(count), C.byref(oi),
                C.byref(ov), C.byref(cnt), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        elif prefix is None:
            _check(_hl().mgh_lossless_decompress(
                self._c, raw, nbytes, lossless, C.c_void_p(q.data_ptr()), n, C.byref(oi), C.byref(ov),
                C.byref(cnt), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        else:
            _check(_hl().mgh_lossless_decompress_prefix(
                self._c, raw, nbytes, lossless, C.c_void_p(q.data_ptr()), n, int(prefix), C.byref(oi), C.byref(ov),
                C.byref(cnt), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        k = cnt.value
        idx = torch.empty(k, dtype=torch.int64, device="cuda")
        val = torch.empty(k, dtype=torch.int64, device="cuda")
        if k:
            _check(_hl().mgh_memcpy(C.c_void_p(idx.data_ptr()), oi, k * 8))
            _check(_hl().mgh_memcpy(C.c_void_p(val.data_ptr()), ov, k * 8))
        return q, idx, val
