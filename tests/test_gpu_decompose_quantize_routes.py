"""GPU tests of the decomposition + quantization core behind mgh_decompose_quantize, _sym16 and _dn
(csrc/capi.hip, decompose_quantize): every route it can choose -- fused level kernels or staged on
dense arrays, host-built or device-made quantizer table -- gives what the stages run apart give
(mgh_norm, mgh_decompose, mgh_quantize on the same hierarchy); a streamed norm is gone after the call
that follows it, whichever route that call took; missing outlier buffers are refused before anything
is launched."""
import ctypes as C

import numpy as np
import pytest

from tests.util import smooth_field

pytestmark = pytest.mark.gpu

FUSED3 = (34, 33, 32)
SHAPES = [FUSED3,            # fused 3-D
          (6, 9, 8, 12),     # 4-D: fused where sym16_supported() says so
          (5000, 5, 7),      # thin: the one-thread-per-element kernels, staged
          (3, 4, 5, 6, 7),   # 5-D: the N-D kernels, staged
          (17, 20)]          # 2-D, staged
TOL = 1e-3
GIVEN = 1.25                 # a norm the caller gives (any value > 0 is taken as it is)
MGH_ERR_INVALID_ARGUMENT = -1


def _gpu():
    import torch
    import mgard_amd
    return torch, mgard_amd


_cache = {}


def _case(shape, dt):
    """Hierarchy, device input and (computed once, never modified) the stages' coefficients."""
    key = (shape, np.dtype(dt).name)
    if key not in _cache:
        torch, mg = _gpu()
        h = mg.Hierarchy(shape, dt)
        d = torch.from_numpy(smooth_field(shape, dt)).cuda()
        _cache[key] = (h, d, h.decompose(d), {})
    return _cache[key]


def _stages(shape, dt, eb, s, norm, dict_size=8192):
    """mgh_decompose (shared), mgh_quantize under `norm`: (q, outlier set, count)."""
    h, d, c, refs = _case(shape, dt)
    key = (eb, s, norm, dict_size)
    if key not in refs:
        q, oi, ov, n = h.quantize(c, eb, TOL, s, norm, dict_size=dict_size)
        refs[key] = (q, _outliers(oi, ov), n)
    return refs[key]


def _check_norm(h, d, dt, s, src, given, got):
    """The norm an entry returned against the stages': the given value, or mgh_norm's. Equal -- but for
    the float64 L2 norm, which mgh_norm itself does not reproduce from run to run (one MI355X, 30 runs
    of mgh_norm on the same array: 2 values on (34, 33, 32), 4 on (5000, 5, 7), one ulp apart): its
    blocks of 1024 elements add their float64 partial sums to the result with atomicAdd, in the order
    they finish. nb partial sums added in two orders differ by at most 2 (nb - 1) u relative
    (u = 2^-53), the square root halves that, and the division, the square root and the first half's
    own rounding add at most 3 u: (nb + 2) u. (The float32 partial sums add up exactly in float64, and
    max|x| is exact.) The integers are compared under the norm the entry returned either way."""
    if src != "rel0":
        assert got == given
        return
    ref = h.norm(d, s)
    if s == 0.0 and dt == np.float64:
        nb = min((h.total + 1023) // 1024, 2048)
        assert abs(got - ref) <= (nb + 2) * 2.0 ** -53 * ref, (got, ref)
    else:
        assert got == ref, (got, ref)


def _outliers(idx, val):
    return set(zip(idx.cpu().numpy().tolist(), val.cpu().numpy().tolist()))


def _same_bits(a, b):
    return np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))


def _bound(mg, src):
    """(error bound type, norm argument) of a norm source."""
    return {"rel0": (mg.REL, 0.0), "relgiven": (mg.REL, GIVEN), "abs": (mg.ABS, 1.0)}[src]


@pytest.mark.parametrize("src", ["rel0", "relgiven", "abs"])
@pytest.mark.parametrize("s", [np.inf, 0.0])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_route_equals_the_stages(shape, dt, s, src):
    torch, mg = _gpu()
    h, d, c, _ = _case(shape, dt)
    eb, norm = _bound(mg, src)
    for with_coeff in (False, True):
        co = torch.full_like(c, -777.0) if with_coeff else None
        q, oi, ov, n, nrm = h.decompose_quantize(d, eb, TOL, float(s), norm=norm, coeff_out=co)
        print(shape, np.dtype(dt).name, s, src, "coeff_out" if with_coeff else "no coeff_out", "norm", repr(nrm),
              "outliers", n)
        _check_norm(h, d, dt, float(s), src, norm, nrm)
        rq, rout, rn = _stages(shape, dt, eb, float(s), nrm)
        assert n == rn and _outliers(oi, ov) == rout
        assert torch.equal(q, rq)
        if with_coeff:
            assert _same_bits(co, c)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_a_large_dictionary_is_staged_on_a_fused_shape(dt):
    """dict_size = 2^31: the fused level kernels test the dictionary range in 32 bits."""
    torch, mg = _gpu()
    h, d, c, _ = _case(FUSED3, dt)
    q, oi, ov, n, nrm = h.decompose_quantize(d, mg.REL, TOL, float("inf"), dict_size=2 ** 31)
    _check_norm(h, d, dt, float("inf"), "rel0", 0.0, nrm)
    rq, rout, rn = _stages(FUSED3, dt, mg.REL, float("inf"), nrm, dict_size=2 ** 31)
    assert n == rn and _outliers(oi, ov) == rout and torch.equal(q, rq)


@pytest.mark.parametrize("nsub", [1, 4])
@pytest.mark.parametrize("s", [np.inf, 0.0])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_device_norm_entry_equals_the_stages(dt, s, nsub):
    """mgh_decompose_quantize_dn: the bound of one of nsub subdomains under the global norm
    (calc_local_abs_tol, ErrorToleranceCalculator.hpp:134-155) as an ABS bound through the stages."""
    torch, mg = _gpu()
    h, d, c, _ = _case(FUSED3, dt)
    g = dt(h.norm(d, float(s)))
    dn = torch.full((1,), float(g), dtype=h.torch_dtype, device="cuda")
    if np.isinf(s):
        atol = dt(TOL) * g
    else:
        atol = np.sqrt((dt(TOL) * g) * (dt(TOL) * g) / dt(nsub), dtype=dt)
    rq, roi, rov, rn = h.quantize(c, mg.ABS, float(atol), float(s), 1.0)
    bufs = (torch.empty(FUSED3, dtype=torch.int64, device="cuda"),) + h._outlier_bufs(h.total)
    q, oi, ov, cnt = h.decompose_quantize_dn(d, mg.REL, TOL, float(s), dn, nsub, bufs)
    n = int(cnt.item())
    assert n == rn and _outliers(oi[:n], ov[:n]) == _outliers(roi, rov)
    assert torch.equal(q, rq)


@pytest.mark.parametrize("src", ["rel0", "relgiven"])
@pytest.mark.parametrize("s", [np.inf, 0.0])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_sym16_entry_equals_the_stages(dt, s, src):
    """The 16-bit symbols are the stages' integers (dictionary shift in them) narrowed."""
    torch, mg = _gpu()
    h, d, c, _ = _case(FUSED3, dt)
    assert h.sym16_supported()
    eb, norm = _bound(mg, src)
    sym, oi, ov, n, nrm = h.decompose_quantize_sym16(d, eb, TOL, float(s), norm=norm)
    print(np.dtype(dt).name, s, src, "norm", repr(nrm))
    _check_norm(h, d, dt, float(s), src, norm, nrm)
    rq, rout, rn = _stages(FUSED3, dt, eb, float(s), nrm)
    assert n == rn and _outliers(oi, ov) == rout
    assert np.array_equal(sym.cpu().numpy().astype(np.int64), rq.cpu().numpy())


def test_the_shapes_cover_both_routes():
    """sym16_supported() is "the fused level kernels take this hierarchy". Which kernels run D = 4 is the
    library's choice (the cells above hold either way); the others are on the route their comment says."""
    for dt in (np.float32, np.float64):
        assert _case(FUSED3, dt)[0].sym16_supported()
        for shape in SHAPES[2:]:
            assert not _case(shape, dt)[0].sym16_supported()
        print("4-D fused:", _case(SHAPES[1], dt)[0].sym16_supported())


@pytest.mark.parametrize("other", ["coeff_out", "abs"])
@pytest.mark.parametrize("s", [np.inf, 0.0])
def test_a_streamed_norm_does_not_outlive_the_call_after_it(s, other):
    """mgh_norm_stream_* over A, then a call on A that does not take the streamed norm (staged because of
    the coefficient output, or fused with an ABS bound), then REL without a norm on B = 4 A: B is
    quantized under its own norm, as on a fresh hierarchy."""
    torch, mg = _gpu()
    dt = np.float32
    a = torch.from_numpy(smooth_field(FUSED3, dt)).cuda()
    b = 4 * a
    fresh = mg.Hierarchy(FUSED3, dt)
    rq, roi, rov, rn, rnorm = fresh.decompose_quantize(b, mg.REL, TOL, float(s))
    norm_b = fresh.norm(b, float(s))
    fresh.close()
    h = mg.Hierarchy(FUSED3, dt)
    h.norm_stream(a, float(s), [a.numel() // 2, a.numel() - a.numel() // 2])
    if other == "coeff_out":
        h.decompose_quantize(a, mg.REL, TOL, float(s), coeff_out=torch.empty_like(a))
    else:
        h.decompose_quantize(a, mg.ABS, TOL, float(s), norm=1.0)
    q, oi, ov, n, nrm = h.decompose_quantize(b, mg.REL, TOL, float(s))
    print(s, other, "norm", repr(nrm), "mgh_norm(B)", repr(norm_b), "fresh hierarchy", repr(rnorm))
    assert nrm == norm_b
    assert torch.equal(q, rq)
    assert n == rn and _outliers(oi, ov) == _outliers(roi, rov)
    h.close()


@pytest.mark.parametrize("shape", [FUSED3, (3, 4, 5, 6, 7), (17, 20)])
def test_missing_outlier_buffers_are_refused_before_any_launch(shape):
    """prep_huffman = 1 without an outlier counter, or a capacity without index / value arrays:
    MGH_ERR_INVALID_ARGUMENT from every entry, and (profile_read) not one launch."""
    torch, mg = _gpu()
    L = mg.load_library()
    dt = np.float32
    h = mg.Hierarchy(shape, dt)
    d = torch.from_numpy(smooth_field(shape, dt)).cuda()
    q = torch.empty(shape, dtype=torch.int64, device="cuda")
    sym = torch.empty(shape, dtype=torch.uint16, device="cuda")
    cnt, idx, val = h._outlier_bufs(h.total)
    dn = torch.ones(1, dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    inf = float("inf")
    missing = [(None, p(idx), p(val), h.total),   # no counter
               (p(cnt), None, None, h.total)]     # a capacity, nothing to hold it
    h.profile(True)
    for oc, oi, ov, cap in missing:
        nout = C.c_double()
        assert L.mgh_decompose_quantize(h._h, p(d), mg.REL, TOL, inf, 0.0, C.byref(nout), 8192, 1, p(q),
                                        oc, oi, ov, cap, None, mg._stream()) == MGH_ERR_INVALID_ARGUMENT
        if h.sym16_supported():
            assert L.mgh_decompose_quantize_dn(h._h, p(d), mg.REL, TOL, inf, p(dn), 1, 8192, 1, p(q),
                                               oc, oi, ov, cap, mg._stream()) == MGH_ERR_INVALID_ARGUMENT
            assert L.mgh_decompose_quantize_sym16(h._h, p(d), mg.REL, TOL, inf, 0.0, C.byref(nout), 8192, p(sym),
                                                  oc, oi, ov, cap, mg._stream()) == MGH_ERR_INVALID_ARGUMENT
    assert sum(launches for _, launches in h.profile_read().values()) == 0
    h.close()
