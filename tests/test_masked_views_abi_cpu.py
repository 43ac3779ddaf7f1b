"""CPU test of the C ABI the masked views add: the new entry points are exported by the built library and bound by
the Python side, and mgh_error_stats, which mgh_compare_masked_ and mgh_verify_masked fill, keeps its 72 bytes."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOW = ["mgh_mask_sample_", "mgh_compare_masked_"]
HIGH = ["mgh_decompress_masked_level", "mgh_decompress_masked_coarsened", "mgh_decompress_masked_preview",
        "mgh_decompress_masked_preview_window", "mgh_decompress_mask_level", "mgh_decompress_mask_coarsened",
        "mgh_decompress_mask_window", "mgh_verify_masked"]


def test_new_symbols_are_exported_and_bound():
    import mgard_amd
    from mgard_amd import highlevel
    L = mgard_amd.load_library()
    for name in LOW + HIGH:
        assert hasattr(L, name), name
    # (the two low-level entries are internal: exported and bound, declared in no public header)
    assert set(LOW) == set(mgard_amd.INTERNAL_SYMBOLS) and not set(LOW) & set(mgard_amd.SYMBOLS)
    assert set(HIGH) <= set(highlevel.HL_SYMBOLS)
    for fn in ("mask_sample", "compare_masked"):
        assert callable(getattr(mgard_amd, fn))
    for fn in ("decompress_masked_preview", "verify_masked"):
        assert callable(getattr(highlevel, fn))


def test_error_stats_stays_72_bytes(tmp_path):
    import mgard_amd
    from mgard_amd import highlevel
    assert ctypes.sizeof(mgard_amd.ErrorStats) == 72
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "mgard_hip_compress.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(mgh_error_stats), sizeof(mgh_verify_result)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    stats, result = (int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    assert stats == 72 and result == ctypes.sizeof(highlevel.VerifyResult)
