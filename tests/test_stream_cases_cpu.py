"""Completeness of the stream-order cases, without a GPU: every function of the two public headers that takes a
`void *stream` has a row in CASE_TABLE of tests/test_gpu_stream_order.py, and the table names nothing the headers
do not declare. A new entry point with a stream parameter fails here until it has a stream case."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the only entry points with a stream parameter that have no stream case, each with its reason
EXCLUDED = {
    "mgh_stream_calibrate": "a measurement aid: it times launches of its own on the stream, and its output is a time",
}


def _stream_functions():
    """Names of the declared functions with a `void *stream` parameter (comments stripped, as
    tests/test_abi_and_format.py reads the headers)."""
    names = set()
    for h in ("mgard_hip.h", "mgard_hip_compress.h"):
        txt = open(os.path.join(ROOT, "include", h)).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        for name, params in re.findall(r"\b(mgh_[a-z_0-9]+)\s*\(([^;{}]*?)\)\s*;", txt, flags=re.S):
            if re.search(r"\bvoid\s*\*\s*stream\b", params):
                names.add(name)
    return names


def _table_entries():
    from tests.test_gpu_stream_order import CASE_TABLE
    return [e for _, entries, _ in CASE_TABLE for e in entries]


def test_the_parser_finds_the_stream_functions():
    found = _stream_functions()
    assert len(found) >= 40, sorted(found)
    for known in ("mgh_norm", "mgh_decompose_quantize", "mgh_prolong_window_strided", "mgh_mask_restore", "mgh_compare",
                  "mgh_histogram_sym16", "mgh_lossless_decompress_sym16", "mgh_stream_calibrate"):
        assert known in found, known
    # (functions without a stream, and the container calls, are not among them)
    for other in ("mgh_compress", "mgh_decompress", "mgh_set_ld", "mgh_level_nodes", "mgh_huffman_codebook"):
        assert other not in found, other


def test_every_stream_function_has_a_stream_case():
    entries = _table_entries()
    assert len(entries) == len(set(entries)), "an entry point is listed twice"
    missing = sorted(_stream_functions() - set(entries) - set(EXCLUDED))
    assert not missing, "no stream-order case (tests/test_gpu_stream_order.py: CASE_TABLE) for %s" % ", ".join(missing)


def test_the_table_names_only_declared_stream_functions():
    unknown = sorted(set(_table_entries()) - _stream_functions())
    assert not unknown, "CASE_TABLE names %s, which the headers do not declare with a stream" % ", ".join(unknown)
    assert not set(EXCLUDED) & set(_table_entries()), "an excluded entry point has a case: take it off the list"
    assert set(EXCLUDED) <= _stream_functions(), "the exclusion list names a function that is gone"


def test_every_case_has_its_function_and_known_routes():
    import tests.test_gpu_stream_order as m
    for name, entries, routes in m.CASE_TABLE:
        assert callable(getattr(m, "_case_" + name, None)), name
        assert entries and routes and set(routes) <= set(m.ROUTES), name
        assert "fused3" in routes, "%s: every entry point runs on the fused 3-D route" % name
