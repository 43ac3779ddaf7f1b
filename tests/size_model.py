"""NumPy / pure-Python restatement of what mgard_amd/csrc/size_plan.hpp computes, written from the
format description (tests/payload.py reads the same record) and from the issue's text of the search --
not from the header: the record's size as a function of its counts, the brackets, the rule for the
synchronisation points, and the log-quartile search in IEEE double precision."""
import numpy as np

HUFFMAN = 0
ENC_CHUNK_MAX = 40 * 512   # the single-pass encoder keeps 40 symbols per thread, 512 threads


def nchunks(n, chunk):
    return (n - 1) // chunk + 1


def record_total(nchunk, dict_size, units, noutlier, sync):
    """Bytes of a serialized Huffman record (Huffman.hpp:163-239; every member is 8-byte aligned)."""
    off = 8 + 4 + 4          # primary_count, dict_size, chunk_size
    off += 8                 # huffmeta_size
    off += 8 * 2 * nchunk    # bits per chunk, first unit per chunk
    off += 8                 # decodebook_size
    off += 8 * 128 + 8 * dict_size
    off += 8                 # ddata_size
    off += 8 * units
    off += 8 + 16 * noutlier
    if sync:
        off += 8 + 4 * 64 * nchunk
    return off


def sym16_ok(dict_size, chunk):
    return dict_size <= 65536 and dict_size * 8 + chunk * 2 <= 140 * 1024


def has_sync(lossless, dict_size, chunk, total_bits, n, sync_env=1):
    return (lossless == HUFFMAN and sym16_ok(dict_size, chunk) and 1024 <= chunk <= ENC_CHUNK_MAX
            and sync_env != 0 and total_bits >= 4 * n)


def record_bracket(n, dict_size, chunk, total_bits, noutlier, sync):
    nc = nchunks(n, chunk)
    return (record_total(nc, dict_size, (total_bits + 63) // 64, noutlier, sync),
            record_total(nc, dict_size, total_bits // 64 + nc, noutlier, sync))


def record_exact(n, dict_size, chunk, chunk_bits, noutlier, sync):
    """The size with the bits of every chunk known: each chunk is padded to whole 64-bit units."""
    nc = nchunks(n, chunk)
    assert len(chunk_bits) == nc
    return record_total(nc, dict_size, sum((int(b) + 63) // 64 for b in chunk_bits), noutlier, sync)


def container_bracket(metadata_bytes, n, elem, rec):
    dense = n * elem
    lo, hi = (metadata_bytes + 8 + min(r, dense) for r in rec)
    raw_lo, raw_hi = rec[0] >= dense, rec[1] >= dense
    return lo, hi, 1 if raw_lo and raw_hi else 0 if not raw_lo and not raw_hi else -1


def quartiles(a, b):
    a, b = np.float64(a), np.float64(b)
    m2 = np.sqrt(a) * np.sqrt(b)
    return np.sqrt(a) * np.sqrt(m2), m2, np.sqrt(m2) * np.sqrt(b)


def search(fits, tol_min, tol_max, rounds):
    """(tolerance or None when nothing fits, the next finer candidate of the last round)."""
    a, b = np.float64(tol_min), np.float64(tol_max)
    if fits(a):
        return a, None
    if not fits(b):
        return None, None
    for _ in range(rounds):
        cand = list(quartiles(a, b)) + [b]
        ok = [fits(m) for m in cand[:3]] + [True]
        k = ok.index(True)
        a, b = (cand[k - 1] if k else a), cand[k]
    return b, a
