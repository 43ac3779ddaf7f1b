"""TEST INFRASTRUCTURE -- ctypes binding of oracle/_ref/libmgx_ref.so, the reference MGARD-X's own
SERIAL code path (oracle/ref_driver.cpp, built by oracle/build_ref.py).

``Hierarchy`` carries the method names of ``oracle.Hierarchy`` (l_target, level_shape, decompose,
recompose, quantize, dequantize) so a test can run one in place of the other; ``norm`` mirrors
``oracle.norm``. The library is loaded RTLD_LOCAL: it and the product library both define names at
namespace level (mgard_x::...), which must not bind to each other.
"""
import ctypes as C
import os

import numpy as np

from .build_ref import LIB_PATH

REL, ABS = 0, 1  # mgard_x::error_bound_type (Utilities/Types.h)
_lib = None
_declared = set()
_SFX = {np.dtype(np.float32): ("f32", C.c_float), np.dtype(np.float64): ("f64", C.c_double)}


def available():
    return os.path.exists(LIB_PATH)


def lib():
    global _lib
    if _lib is None:
        if not available():
            raise FileNotFoundError("%s is not built (oracle.build_ref())" % LIB_PATH)
        _lib = C.CDLL(LIB_PATH, mode=os.RTLD_LOCAL)
    return _lib


def _fn(name, D, dtype):
    """The (D, dtype) instance of one ABI function, declared on first use."""
    short, ct = _SFX[np.dtype(dtype)]
    full = "%s_%dd_%s" % (name, D, short)
    f = getattr(lib(), full)
    if full in _declared:
        return f
    rp, u64p, i64p = C.POINTER(ct), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
    sig = {
        "mgxr_hier_create": (C.c_void_p, [u64p, C.POINTER(rp), C.c_int, C.c_uint64]),
        "mgxr_hier_destroy": (None, [C.c_void_p]),
        "mgxr_l_target": (C.c_int, [C.c_void_p]),
        "mgxr_level_shape": (None, [C.c_void_p, C.c_int, u64p]),
        "mgxr_decompose": (None, [C.c_void_p, rp]),
        "mgxr_recompose": (None, [C.c_void_p, rp]),
        "mgxr_quantize": (C.c_uint64, [C.c_void_p, rp, C.c_int, ct, ct, ct, C.c_uint64, C.c_int,
                                       i64p, u64p, i64p, C.c_uint64]),
        "mgxr_dequantize": (None, [C.c_void_p, i64p, C.c_int, ct, ct, ct, C.c_uint64, C.c_int,
                                   u64p, i64p, C.c_uint64, rp]),
        "mgxr_norm": (ct, [u64p, rp, ct, C.c_int]),
    }[name]
    f.restype, f.argtypes = sig
    _declared.add(full)
    return f


class Hierarchy:
    """mgard_x::Hierarchy<D, T, SERIAL> with DataRefactor and LinearQuantizer of the reference."""

    def __init__(self, shape, dtype=np.float32, coords=None, normalize_coordinates=True,
                 max_level=2**64 - 1):
        self.dtype = np.dtype(dtype)
        self.ct = _SFX[self.dtype][1]
        self.shape = tuple(int(s) for s in shape)
        self.D = len(self.shape)
        shp = (C.c_uint64 * self.D)(*self.shape)
        cptr = None
        if coords is not None:
            self._coords = [np.ascontiguousarray(c, dtype=self.dtype) for c in coords]
            assert len(self._coords) == self.D
            for c, n in zip(self._coords, self.shape):
                assert c.shape == (n,)
            cptr = (C.POINTER(self.ct) * self.D)(*[self._rp(c) for c in self._coords])
        self._h = self._f("mgxr_hier_create")(shp, cptr, int(normalize_coordinates),
                                              int(max_level))
        if not self._h:
            raise ValueError("invalid shape for mgard_x hierarchy: %r" % (self.shape,))
        self.l_target = self._f("mgxr_l_target")(self._h)

    def _f(self, name):
        return _fn(name, self.D, self.dtype)

    def _rp(self, a):
        return a.ctypes.data_as(C.POINTER(self.ct))

    def __del__(self):
        if getattr(self, "_h", None):
            self._f("mgxr_hier_destroy")(self._h)
            self._h = None

    def level_shape(self, l):
        out = (C.c_uint64 * self.D)()
        self._f("mgxr_level_shape")(self._h, l, out)
        return tuple(int(x) for x in out)

    def decompose(self, data):
        v = np.array(data, dtype=self.dtype, order="C", copy=True).reshape(self.shape)
        self._f("mgxr_decompose")(self._h, self._rp(v))
        return v

    def recompose(self, coeffs):
        v = np.array(coeffs, dtype=self.dtype, order="C", copy=True).reshape(self.shape)
        self._f("mgxr_recompose")(self._h, self._rp(v))
        return v

    def quantize(self, coeffs, ebtype, tol, s, norm, dict_size=8192, prep_huffman=True,
                 outlier_cap=None):
        v = np.array(coeffs, dtype=self.dtype, order="C", copy=True).reshape(self.shape)
        cap = v.size if outlier_cap is None else int(outlier_cap)
        q = np.empty(self.shape, dtype=np.int64)
        oi = np.empty(max(cap, 1), dtype=np.uint64)
        ov = np.empty(max(cap, 1), dtype=np.int64)
        cnt = self._f("mgxr_quantize")(
            self._h, self._rp(v), ebtype, tol, s, norm, dict_size, int(prep_huffman),
            q.ctypes.data_as(C.POINTER(C.c_int64)), oi.ctypes.data_as(C.POINTER(C.c_uint64)),
            ov.ctypes.data_as(C.POINTER(C.c_int64)), cap)
        k = min(int(cnt), cap)
        return q, oi[:k].copy(), ov[:k].copy(), int(cnt)

    def dequantize(self, q, ebtype, tol, s, norm, dict_size=8192, prep_huffman=True,
                   outlier_idx=None, outlier_val=None):
        qq = np.ascontiguousarray(q, dtype=np.int64).reshape(self.shape)
        oi = np.ascontiguousarray(outlier_idx if outlier_idx is not None else [], dtype=np.uint64)
        ov = np.ascontiguousarray(outlier_val if outlier_val is not None else [], dtype=np.int64)
        out = np.empty(self.shape, dtype=self.dtype)
        self._f("mgxr_dequantize")(
            self._h, qq.ctypes.data_as(C.POINTER(C.c_int64)), ebtype, tol, s, norm, dict_size,
            int(prep_huffman), oi.ctypes.data_as(C.POINTER(C.c_uint64)),
            ov.ctypes.data_as(C.POINTER(C.c_int64)), len(oi), self._rp(out))
        return out


def norm(data, s, normalize_coordinates=True):
    """norm_calculator of the reference on `data` (its shape decides the instantiation)."""
    v = np.array(data, order="C", copy=True)
    D = max(v.ndim, 1)
    v = v.reshape(v.shape if v.ndim else (1,))
    ct = _SFX[v.dtype][1]
    shp = (C.c_uint64 * D)(*v.shape)
    return float(_fn("mgxr_norm", D, v.dtype)(shp, v.ctypes.data_as(C.POINTER(ct)), s,
                                              int(normalize_coordinates)))
