"""Level-by-level refinement, the parts that need no device: the exported symbols and
mgh_infer_level_range on containers written by metadata_serialize, against oracle.Hierarchy."""
import numpy as np
import pytest

import oracle
from tests.test_multires_cpu import HEADERS, _container

NEW_SYMBOLS = ["mgh_refine_level", "mgh_lossless_decompress_range", "mgh_infer_level_range", "mgh_progressive_open",
               "mgh_progressive_level", "mgh_progressive_refine", "mgh_progressive_close"]


def test_new_symbols_are_exported():
    import mgard_amd
    from mgard_amd import highlevel
    L = mgard_amd.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in mgard_amd.SYMBOLS + highlevel.HL_SYMBOLS, name
    for attr in ("Progressive", "infer_level_range"):
        assert hasattr(highlevel, attr), attr
    assert hasattr(mgard_amd.Hierarchy, "refine_level")


@pytest.mark.parametrize("case", HEADERS + [((37, 50, 101), "f32", False, None)],
                         ids=lambda c: "x".join(map(str, c[0])) + "-" + c[1])
def test_infer_level_range(case):
    from mgard_amd import highlevel as hl
    shape, dt, nonuniform, ml = case
    buf = _container(shape, dt, nonuniform)
    block = hl.metadata_parse(bytes(buf))["block_size"]
    cfg = hl.Config()
    if ml is not None:
        cfg.max_larget_level = ml
    H = oracle.Hierarchy(shape, np.float64 if dt == "f64" else np.float32,
                         **({} if ml is None else dict(max_level=ml)))
    below = 0
    for level in range(H.l_target + 1):
        n_l = int(np.prod(H.level_shape(level)))
        first, num, c0, nc = hl.infer_level_range(buf, level, cfg)
        assert (first, num) == (below, n_l - below), level
        assert c0 == below // block and nc == (n_l - 1) // block - below // block + 1, level
        below = n_l
    assert below == int(np.prod(shape))
    for bad in (-1, H.l_target + 1):
        with pytest.raises(hl.MgardHipError, match=r"error -1\b"):
            hl.infer_level_range(buf, bad, cfg)


def test_infer_level_range_refuses_a_decomposed_container():
    from mgard_amd import highlevel as hl
    buf = _container((129, 40, 40), "f32", False, dd=(0, 0, 65))
    with pytest.raises(hl.MgardHipError, match=r"error -1\b.*domain-decomposed"):
        hl.infer_level_range(buf, 1)
    assert hl.infer_level_range(_container((20, 31), "f32", False), 0)[0] == 0
