"""mgh_mask_sample_ (k_mask_sample) against tests/mask_view_model.py: the packed mask of a level grid, a coarsened
grid or a window, word for word, and the count of its set bits. The cases are tests/mask_view_model.sample_cases():
one output with 63 dead lanes in its word, rows longer and shorter than a wave, outputs that are no multiple of 64,
identity (NULL) lists mixed with strided ones in 4-D and 5-D, a window, and lists that lead outside the array."""
import numpy as np
import pytest

from tests import mask_model as mm
from tests import mask_view_model as mv

CASES = mv.sample_cases()


def _words(mask):
    import torch
    return torch.from_numpy(mm.packed_words(mask).view(np.int64)).cuda()


def _check(mask, lists, as_tensors=False):
    import torch
    import mgard_amd
    want = mv.sample_any(mask, lists)
    given = lists
    if as_tensors:
        given = [None if l is None else torch.from_numpy(np.asarray(l, dtype=np.int64).astype(np.uint32).view(np.int32)).cuda()
                 for l in lists]
    out_words, count = mgard_amd.mask_sample(_words(mask), mask.shape, given)
    torch.cuda.synchronize()   # (an error of the device would surface here)
    assert np.array_equal(out_words.cpu().numpy().view(np.uint64), mm.packed_words(want))
    assert count == int(want.sum())
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("name,shape,lists", CASES, ids=[c[0] for c in CASES])
def test_sampled_words_and_count(name, shape, lists):
    mask = np.random.default_rng(len(shape)).random(shape) < 0.35
    want = _check(mask, lists)
    if name == "1d-one-output":
        assert want.shape == (1,)
    if name == "2d-out-of-range":
        inside = mv.sample_any(np.ones(shape, dtype=bool), lists)
        assert not inside.all() and inside.any() and not want[~inside].any()
    _check(mask, lists, as_tensors=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name,shape,lists", CASES, ids=[c[0] for c in CASES])
def test_all_ones_and_all_zero_sources(name, shape, lists):
    ones = _check(np.ones(shape, dtype=bool), lists)
    if name != "2d-out-of-range":
        assert ones.all()        # the unused high bits of the last word stay zero: the words are compared whole
    assert not _check(np.zeros(shape, dtype=bool), lists).any()


@pytest.mark.gpu
def test_refusals():
    import mgard_amd
    mask = np.zeros((17, 130), dtype=bool)
    w = _words(mask)
    with pytest.raises(mgard_amd.MgardHipError, match="error -1"):   # the identity list needs out_shape[d] <= shape[d]
        mgard_amd.mask_sample(w, mask.shape, [None, [0, 1]], out_shape=(18, 2))
    with pytest.raises(ValueError):
        mgard_amd.mask_sample(w, mask.shape, [[0, 1]])
    with pytest.raises(ValueError):
        mgard_amd.mask_sample(w[:-1], mask.shape, [None, None])
    out_words, count = mgard_amd.mask_sample(w, mask.shape, [None, None])
    assert count == 0 and not out_words.cpu().numpy().any()
