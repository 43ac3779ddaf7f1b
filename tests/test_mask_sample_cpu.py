"""CPU test of the index arithmetic of mgh_mask_sample_ (mgard_amd/csrc/mask_plan.hpp: mask_unravel, mask_flat_index,
mask_sample_source), which the kernel k_mask_sample runs per lane.

tests/cpp/mask_sample_dump.cpp is compiled with g++ against the header alone (no HIP) and once more with
-fsanitize=address,undefined as a stand-alone binary. It prints the source bit of every output element of the cases
of tests/mask_view_model.py (those of tests/test_gpu_mask_sample.py); the expectation is np.ravel_multi_index."""
import os
import subprocess

import numpy as np
import pytest

from tests import mask_view_model as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgard_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "mask_sample_dump.cpp")


def _build(tmp_path_factory, name, extra=()):
    exe = str(tmp_path_factory.mktemp(name) / "mask_sample_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", CSRC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return _build(tmp_path_factory, "mask_sample")


def _line(shape, lists):
    out_shape = [shape[d] if l is None else len(l) for d, l in enumerate(lists)]
    parts = [str(len(shape))] + [str(e) for e in shape] + [str(e) for e in out_shape]
    for l in lists:
        parts += ["-1"] if l is None else [str(int(i)) for i in l]
    return " ".join(parts) + "\n"


def _expected(shape, lists):
    """Source bit of every output element, -1 where a list leads outside the array."""
    full = [np.arange(e, dtype=np.int64) if l is None else np.asarray(l, dtype=np.int64) for l, e in zip(lists, shape)]
    grid = np.meshgrid(*full, indexing="ij")
    inside = np.ones(grid[0].shape, dtype=bool)
    for g, e in zip(grid, shape):
        inside &= g < e
    flat = np.ravel_multi_index([np.minimum(g, e - 1) for g, e in zip(grid, shape)], shape)
    return np.where(inside, flat, -1).reshape(-1)


def _text():
    return "".join(_line(shape, lists) for _, shape, lists in mv.sample_cases())


def test_source_bits_are_ravel_multi_index(dump):
    out = subprocess.run([dump], input=_text(), capture_output=True, text=True, check=True, timeout=300).stdout.splitlines()
    cases = mv.sample_cases()
    assert len(out) == len(cases)
    for line, (name, shape, lists) in zip(out, cases):
        got = np.array(line.split(), dtype=np.int64)
        want = _expected(shape, lists)
        assert got.shape == want.shape and np.array_equal(got, want), name
    # the out-of-range case has outputs of both kinds
    want = _expected(*cases[-1][1:])
    assert (want < 0).any() and (want >= 0).any()


def test_model_sample_is_the_gather_of_those_bits():
    """mask_view_model.sample_any (what the GPU tests compare with) against the bits above."""
    rng = np.random.default_rng(11)
    for name, shape, lists in mv.sample_cases():
        mask = rng.random(shape) < 0.4
        src = _expected(shape, lists)
        want = np.where(src >= 0, mask.reshape(-1)[np.maximum(src, 0)], False)
        assert np.array_equal(mv.sample_any(mask, lists).reshape(-1), want), name


def test_program_is_clean_under_address_and_undefined_sanitizers(tmp_path_factory):
    exe = _build(tmp_path_factory, "mask_sample_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    p = subprocess.run([exe], input=_text(), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-4000:]
    assert len(p.stdout.splitlines()) == len(mv.sample_cases())
