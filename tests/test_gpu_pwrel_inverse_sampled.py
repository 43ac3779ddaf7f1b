"""mgh_pwrel_inverse_sampled_ (k_pwrel_inverse_sampled) against the three launches it stands in for:

    pwrel_inverse(data.clone(), mask_sample(mask_words, ...)[0], mask_sample(flag_words, ...)[0])

bit for bit on integer views, float32 and float64. y is random in +-100 and the two bitmaps are random with all three
classes (valid of both signs, zeroed, non-finite). The cases are where the row walk can go wrong: every level's lists
of (34, 33, 32), a window, a 1-D output with a tail word, identity (NULL) lists, five dimensions, outputs of 64 and 65
elements, a row longer than a workgroup, rows at the group widths the host picks, and a list entry outside the array."""
import numpy as np
import pytest

from tests import mask_model as mm
from tests import mask_view_model as mv

pytestmark = pytest.mark.gpu

H = mv.halved_nodes
CASES = [("levels-34x33x32-%d-halvings" % k, (34, 33, 32), [H(34, k), H(33, k), H(32, k)]) for k in range(6)] + [
    ("window-17x130", (17, 130), [list(range(2, 11)), list(range(60, 130))]),
    ("1d-every-seventh", (1000,), [list(range(0, 1000, 7))]),               # 143 outputs: a tail word
    ("4d-identity-in-two", (5, 6, 7, 9), [None, [0, 2, 4, 5], None, [0, 2, 4, 6, 8]]),
    ("5d", (3, 2, 5, 4, 7), [[0, 2], None, [0, 2, 4], None, [0, 3, 6]]),
    ("5d-long-last", (3, 3, 4, 5, 70), [[0, 2], None, [0, 3], None, H(70, 1)]),
    ("64-outputs", (40, 40), [list(range(0, 40, 5)), list(range(0, 40, 5))]),   # 8 x 8
    ("65-outputs", (40, 70), [list(range(0, 40, 8)), list(range(0, 65, 5))]),   # 5 x 13
    ("one-row-longer-than-a-workgroup", (3, 700), [[1], list(range(0, 600, 2))]),   # 1 x 300
    ("rows-of-33", (9, 80), [None, list(range(0, 66, 2))]),                 # the first row length the whole wave walks
    ("rows-of-32", (9, 80), [None, list(range(0, 64, 2))]),
    ("rows-of-1", (300, 5), [None, [3]]),                                   # a lane is a row
    ("entry-outside", (17, 130), [[0, 5, 17, 16], [0, 200, 129, 3, 130, 2 ** 32 - 1]]),
]
DTYPES = [np.float32, np.float64]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _words(bits):
    return _dev(mm.packed_words(bits).view(np.int64))


def _inputs(shape, lists, dtype, seed):
    """(y of the view, mask and flag bits of the full array)"""
    rng = np.random.default_rng(seed)
    oshape = [e if l is None else len(l) for l, e in zip(lists, shape)]
    y = rng.uniform(-100.0, 100.0, size=oshape).astype(dtype)
    cls = rng.choice(4, size=shape, p=[0.4, 0.3, 0.15, 0.15])      # valid +, valid -, zeroed, non-finite
    return y, cls >= 2, (cls == 1) | (cls == 3)


def _both(y, mask, flag, lists):
    """(the fused pass, the three launches), as integer views on the host"""
    import torch
    import mgard_amd
    mw, fw = _words(mask), _words(flag)
    oshape = y.shape
    want = mgard_amd.pwrel_inverse(_dev(y), mgard_amd.mask_sample(mw, mask.shape, lists, out_shape=oshape)[0],
                                   mgard_amd.mask_sample(fw, mask.shape, lists, out_shape=oshape)[0])
    data = _dev(y)
    got = mgard_amd.pwrel_inverse_sampled(data, mw, fw, mask.shape, lists)
    torch.cuda.synchronize()   # (an error of the device would surface here)
    assert got is data
    return mm.int_view(got.cpu().numpy()), mm.int_view(want.cpu().numpy()), want.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name,shape,lists", CASES, ids=[c[0] for c in CASES])
def test_fused_pass_is_the_three_launches(name, shape, lists, dtype):
    y, mask, flag = _inputs(shape, lists, dtype, len(name))
    got, want, values = _both(y, mask, flag, lists)
    assert got.shape == want.shape == y.shape and np.array_equal(got, want), name
    # ... and the three launches are the model: the classes of the sampled bits
    smask, sflag = mv.sample_any(mask, lists), mv.sample_any(flag, lists)
    assert np.array_equal(np.isnan(values), smask & sflag)
    zero = smask & ~sflag
    assert np.all(values[zero] == 0) and not np.signbit(values[zero]).any()
    valid = ~smask
    assert np.all(np.abs(values[valid]) >= np.finfo(dtype).tiny) and np.isfinite(values[valid]).all()
    assert np.array_equal(np.signbit(values[valid]), sflag[valid])
    if y.size >= 64:
        assert (smask & sflag).any() and zero.any() and (valid & sflag).any() and (valid & ~sflag).any()
    if name == "entry-outside":
        # nothing is read for an entry >= shape[d]: both bits clear, a valid and positive element -- whatever the maps hold
        inside = mv.sample_any(np.ones(shape, dtype=bool), lists)
        assert not inside.all() and inside.any()
        got1, want1, values1 = _both(y, np.ones(shape, dtype=bool), np.ones(shape, dtype=bool), lists)
        assert np.array_equal(got1, want1)
        assert np.isnan(values1[inside]).all() and np.all(values1[~inside] > 0)
    if name == "1d-every-seventh":
        assert y.size == 143
    if name == "64-outputs":
        assert y.size == 64
    if name == "65-outputs":
        assert y.size == 65
    if name == "one-row-longer-than-a-workgroup":
        assert y.shape == (1, 300)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_index_tensors_and_the_identity_everywhere(dtype):
    import torch
    import mgard_amd
    shape = (17, 130)
    lists = [H(17, 1), H(130, 1)]
    y, mask, flag = _inputs(shape, lists, dtype, 3)
    got, want, _ = _both(y, mask, flag, lists)
    tensors = [torch.from_numpy(np.asarray(l, dtype=np.int32)).cuda() for l in lists]
    again = mgard_amd.pwrel_inverse_sampled(_dev(y), _words(mask), _words(flag), shape, tensors)
    assert np.array_equal(mm.int_view(again.cpu().numpy()), want)
    # every list the identity: the plain inverse pass over the whole array
    full, _, _ = _inputs(shape, [None, None], dtype, 4)
    got = mgard_amd.pwrel_inverse_sampled(_dev(full), _words(mask), _words(flag), shape, [None, None])
    want = mgard_amd.pwrel_inverse(_dev(full), _words(mask), _words(flag))
    assert np.array_equal(mm.int_view(got.cpu().numpy()), mm.int_view(want.cpu().numpy()))


def test_refusals():
    import torch
    import mgard_amd
    shape = (17, 130)
    mask = np.zeros(shape, dtype=bool)
    w = _words(mask)
    lists = [H(17, 1), H(130, 1)]
    data = torch.zeros((9, 66), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):                      # wrong dtype
        mgard_amd.pwrel_inverse_sampled(data.to(torch.float16), w, w, shape, lists)
    with pytest.raises(ValueError):
        mgard_amd.pwrel_inverse_sampled(data.to(torch.int32), w, w, shape, lists)
    with pytest.raises(ValueError):                      # a words tensor of the wrong length
        mgard_amd.pwrel_inverse_sampled(data, w[:-1], w, shape, lists)
    with pytest.raises(ValueError):
        mgard_amd.pwrel_inverse_sampled(data, w, torch.cat([w, w]), shape, lists)
    with pytest.raises(ValueError):                      # a list count that is not D
        mgard_amd.pwrel_inverse_sampled(data, w, w, shape, lists[:1])
    with pytest.raises(ValueError):
        mgard_amd.pwrel_inverse_sampled(data, w, w, shape, lists + [None])
    with pytest.raises(ValueError):                      # lists that are not the data's shape
        mgard_amd.pwrel_inverse_sampled(data, w, w, shape, [H(17, 1), H(130, 2)])
    # ... and the library's own, which the Python layer does not anticipate
    import ctypes as C
    L = mgard_amd.load_library()
    u64x2 = C.c_uint64 * 2
    args = lambda D, dt, out: (D, dt, u64x2(*shape), C.c_void_p(w.data_ptr()), C.c_void_p(w.data_ptr()), u64x2(*out), None,
                               C.c_void_p(data.data_ptr()), None)
    assert L.mgh_pwrel_inverse_sampled_(*args(2, 7, (9, 66))) == -1          # unknown dtype
    assert L.mgh_pwrel_inverse_sampled_(*args(6, mgard_amd.FLOAT, (9, 66))) == -1
    assert L.mgh_pwrel_inverse_sampled_(*args(2, mgard_amd.FLOAT, (18, 66))) == -1   # the identity list needs out_shape[d] <= shape[d]
    assert L.mgh_pwrel_inverse_sampled_(*args(2, mgard_amd.FLOAT, (0, 66))) == -1
    torch.cuda.synchronize()
    assert not data.cpu().numpy().any()                 # nothing was launched
    out = mgard_amd.pwrel_inverse_sampled(data, w, w, shape, lists)
    assert np.all(out.cpu().numpy() == 1.0)
