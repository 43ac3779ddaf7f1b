"""CPU tests of mgard_amd/csrc/domain_plan.hpp -- the geometry of a domain decomposition, where the auto-split
lands, the slab sizes of the multi-device and the one-rank-per-GPU paths, the norm of the whole domain from the
subdomains' norms, the bound of one subdomain, the header of one slab and the `[u64 size][record]` frames --
through tests/cpp/domain_plan_dump.cpp (g++ against the header alone, no HIP).

Every expected value is restated here in Python, independent of the header: the geometry is tests.util.blocks(),
the footprint tests.util.reference_footprint(), the floating-point rules the same operations on Python floats
(IEEE double) and numpy.float32, compared bit for bit (the program prints and reads hexadecimal floats).
Damaged headers are one mutation of a valid one each; the verdict expected of every one is _header_model(): the
checks of highlevel.hip as they stood before they moved into the header, in the order they ran.
The same program is also built with -fsanitize=address,undefined and run once, as a stand-alone binary, over the
damaged set: every header it parses is a heap block of exactly its size."""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from tests.util import BLOCK, MAXDIM, VARIABLE, blocks, nonuniform_coords, reference_footprint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgard_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "domain_plan_dump.cpp")
INVALID, OOM, FORMAT = -1, -5, -8
INF = float("inf")
NO_MEMORY = (OOM, "domain decomposition: not enough device memory")
FEW_NODES = (FORMAT, "header: subdomain with fewer than 3 nodes")


def _build(tmp_path_factory, name, extra=()):
    exe = str(tmp_path_factory.mktemp(name) / "domain_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I", CSRC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return _build(tmp_path_factory, "domain_plan")


def _parse(out):
    """[(kind, rest)]; a refusal is ("err", (code, message))."""
    res = []
    for line in out.splitlines():
        kind, _, rest = line.partition(" ")
        if kind == "err":
            code, _, msg = rest.partition(" ")
            rest = (int(code), msg)
        res.append((kind, rest))
    return res


def _run(exe, text):
    return _parse(subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=300).stdout)


def _fields(rest):
    return {k: int(v) for k, v in (f.split("=") for f in rest.split())}


def _ints(*xs):
    return " ".join(str(int(x)) for x in xs)


def test_header_compiles_alone_without_hip(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "domain_plan.hpp"\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, str(src)])
    # what it includes, directly or not: the two host-only headers and the public C headers (the status codes)
    from mgard_amd import _build
    closure = _build._closure(os.path.join(CSRC, "domain_plan.hpp"))
    assert {os.path.basename(f) for f in closure} == {"domain_plan.hpp", "format.hpp", "hierarchy.hpp", "mgard_hip_compress.h",
                                                      "mgard_hip.h"}
    for f in closure:
        text = open(f).read()
        assert "#include <hip" not in text and "getenv" not in text, f


# ---- geometry ----------------------------------------------------------------------------------------------
# (shape, (method, dim, size), Variable sizes)
GEOMETRY = [
    ((40, 65, 70), (MAXDIM, 0, 17), None),         # a remainder slab (17 17 6)
    ((40, 65, 70), (MAXDIM, 1, 13), None),         # divides exactly, not the slowest dimension
    ((40, 65, 70), (MAXDIM, 2, 71), None),         # size > extent: one subdomain
    ((40, 65, 70), (MAXDIM, 0, 40), None),         # size == extent
    ((130,), (MAXDIM, 0, 33), None),               # 1-D, remainder 31
    ((129,), (BLOCK, 0, 43), None),                # 1-D blocks, exact
    ((7, 9, 11, 5, 13), (MAXDIM, 4, 5), None),     # 5-D, remainder 3
    ((7, 9, 11, 5, 13), (BLOCK, 0, 4), None),      # 5-D blocks: remainders 3, 1, 3, 1, 1 (the geometry only)
    ((70, 45, 37), (BLOCK, 0, 33), None),          # 3-D blocks with remainders in every dimension (4, 12, 4)
    ((66, 45, 40), (BLOCK, 0, 20), None),          # 3-D blocks with remainders in two dimensions (6, 5), one exact
    ((9, 8, 34), (VARIABLE, 2, 17), [17, 3, 14]),  # Variable on a dimension other than 0
    ((30, 8), (VARIABLE, 0, 10), [10, 4, 16]),     # Variable on dimension 0: contiguous slabs of unequal size
]


def _geometry_expected(shape, dd, sizes):
    """Per id (row-major over the decomposition grid, last dimension fastest): shape, offset, whether the
    subdomain is one contiguous run of the array, and where that run starts."""
    inner = int(np.prod(shape[1:], dtype=np.int64))
    out = []
    for cell in itertools.product(*blocks(shape, dd, sizes)):
        off, ext = [o for o, _ in cell], [e for _, e in cell]
        out.append((ext, off, int(ext[1:] == list(shape[1:])), off[0] * inner))
    return out


@pytest.mark.parametrize("case", GEOMETRY, ids=lambda c: "x".join(map(str, c[0])) + "-m%d-d%d-s%d" % c[1])
def test_geometry_equals_the_restated_rule(dump, case):
    shape, dd, sizes = case
    cmd = "geom %d %d %s %d %d %s\n" % (dd[0], len(shape), _ints(*shape), dd[1], dd[2], _ints(len(sizes or []), *(sizes or [])))
    (kind, rest), = _run(dump, cmd)
    assert kind == "geom", rest
    head, *groups = rest.split(" | ")
    want = _geometry_expected(shape, dd, sizes)
    assert _fields(head) == dict(num=len(want), max=max(int(np.prod(e)) for e, _, _, _ in want))
    got = []
    for g in groups:
        f = dict(x.split("=") for x in g.split())
        got.append(([int(x) for x in f["shape"].split(",")], [int(x) for x in f["off"].split(",")], int(f["contig"]), int(f["lin"])))
    assert got == want
    # the subdomains tile the array: every node exactly once
    seen = np.zeros(shape, np.int32)
    for ext, off, _, _ in got:
        seen[tuple(slice(o, o + e) for o, e in zip(off, ext))] += 1
    assert (seen == 1).all()


# ---- the split ---------------------------------------------------------------------------------------------
def _split_cmd(shape, elem, avail, method=MAXDIM, block_size=0, var_dim=0, sizes=(), ratio=1.0, dict_size=8192, block=20480):
    return "split %d %s %d %d %d %d %d %s %s %d %d\n" % (len(shape), _ints(*shape), elem, avail, method, block_size, var_dim,
                                                        _ints(len(sizes), *sizes), float(ratio).hex(), dict_size, block)


def test_footprint_equals_the_restated_estimate(dump):
    cases = [((66, 300, 80), 4, 1.0, 8192, 20480, 0), ((66, 150, 80), 4, 1.0, 8192, 20480, 1), ((24, 24, 24), 4, 1.0, 8192, 20480, 1),
             ((129,), 8, 0.25, 64, 4096, 0), ((7, 9, 11, 5, 13), 8, 0.5, 2048, 1024, 1), ((5, 6, 7, 8), 4, 1.0, 8192, 20480, 0)]
    res = _run(dump, "".join("footprint %d %s %d %s %d %d %d\n" % (len(s), _ints(*s), e, float(r).hex(), d, b, p) for s, e, r, d, b, p in cases))
    for (s, e, r, d, b, p), (kind, got) in zip(cases, res):
        assert kind == "footprint" and int(got) == reference_footprint(s, e, ratio=r, dict_size=d, block=b, prefetch=bool(p)), s


def test_maxdim_split_follows_the_reference_footprint(dump):
    """The three budgets of tests/test_gpu_highlevel.py::test_maxdim_split_follows_the_reference_footprint."""
    shape = (66, 300, 80)
    est = reference_footprint(shape, 4)
    half = reference_footprint((66, 150, 80), 4, prefetch=True)
    res = _run(dump, _split_cmd(shape, 4, est + 1) + _split_cmd(shape, 4, est) + _split_cmd(shape, 4, half))
    assert [k for k, _ in res] == ["split"] * 3
    none, halves, quarters = (_fields(r) for _, r in res)
    assert none == dict(decomposed=0, method=MAXDIM, dim=0, size=66, num=1)   # (need = estimate >= available)
    assert halves == dict(decomposed=1, method=MAXDIM, dim=1, size=150, num=2)
    assert quarters == dict(decomposed=1, method=MAXDIM, dim=1, size=75, num=4)


def test_block_split_halves_the_blocks(dump):
    """Blocks of block_size are planned with prefetch as soon as there are two of them, and halved (rounding up)
    until the estimate of one block is below the budget (DomainDecomposer.hpp:238-263)."""
    shape = (40, 54, 60)  # (remainders of at least 3 nodes at block sizes 24, 12 and 6)

    def fits(size, avail):
        count = int(np.prod([(n - 1) // size + 1 for n in shape]))
        return reference_footprint((size,) * 3, 4, prefetch=count > 1) < avail

    e24 = reference_footprint((24, 24, 24), 4, prefetch=True)
    e12 = reference_footprint((12, 12, 12), 4, prefetch=True)
    budgets = [e24 + 1, e24, e12 + 1, e12]
    res = _run(dump, "".join(_split_cmd(shape, 4, a, BLOCK, 24) for a in budgets) + _split_cmd(shape, 4, 2 ** 62, BLOCK, 64))
    sizes = []
    for a in budgets:
        size = 24
        while not fits(size, a):
            size = (size - 1) // 2 + 1
        sizes.append(size)
    assert sizes == [24, 12, 12, 6]
    for (kind, rest), size in zip(res, sizes + [64]):
        assert kind == "split", rest
        assert _fields(rest) == dict(decomposed=1, method=BLOCK, dim=0, size=size, num=int(np.prod([(n - 1) // size + 1 for n in shape])))
    assert _fields(res[-1][1])["num"] == 1  # (Block is recorded as a decomposition even of one block)


def test_split_refusals(dump):
    shape = (66, 300, 80)
    big = 2 ** 62
    cases = [
        (_split_cmd(shape, 4, 1), NO_MEMORY),                                    # MaxDim halved down to 3 planes
        (_split_cmd(shape, 4, 1, BLOCK, 24), NO_MEMORY),                         # blocks halved down to 3
        (_split_cmd(shape, 4, big, BLOCK, 2), (INVALID, "block_size")),
        (_split_cmd(shape, 4, big, VARIABLE, 0, 1, ()), (INVALID, "Variable domain decomposition needs dim and sizes")),
        (_split_cmd(shape, 4, big, VARIABLE, 0, 3, (100, 200)), (INVALID, "Variable domain decomposition needs dim and sizes")),
        (_split_cmd(shape, 4, big, VARIABLE, 0, -1, (100, 200)), (INVALID, "Variable domain decomposition needs dim and sizes")),
        (_split_cmd(shape, 4, big, VARIABLE, 0, 1, (100, 199)), (INVALID, "Variable sizes do not add up to the extent")),
        (_split_cmd(shape, 4, 1, 3), (INVALID, "domain_decomposition")),  # (an unknown method is looked at once a split is due)
        (_split_cmd(shape, 4, big, VARIABLE, 0, 1, (100, 198, 2)),
         (INVALID, "domain decomposition leaves a subdomain with fewer than 3 nodes in a dimension")),
        (_split_cmd(shape, 4, big, BLOCK, 32), (INVALID, "domain decomposition leaves a subdomain with fewer than 3 nodes in a dimension")),
    ]
    res = _run(dump, "".join(c for c, _ in cases))
    assert res == [("err", want) for _, want in cases]
    (kind, rest), = _run(dump, _split_cmd(shape, 4, big, VARIABLE, 0, 1, (100, 60, 140)))
    assert kind == "split" and _fields(rest) == dict(decomposed=1, method=VARIABLE, dim=1, size=100, num=3)


# ---- slab sizes --------------------------------------------------------------------------------------------
def _slabs(n0, size):
    return [size] * (n0 // size) + ([n0 % size] if n0 % size else [])


def test_multi_slab_size(dump):
    cases = [(n0, ndev) for n0 in range(3, 65) for ndev in range(1, 9)]
    res = _run(dump, "".join("multi %d %d\n" % c for c in cases))
    assert len(res) == len(cases)
    for (n0, ndev), (kind, got) in zip(cases, res):
        size = int(got)
        ok = lambda s: min(_slabs(n0, s)) >= 3
        assert kind == "multi" and ok(size) and sum(_slabs(n0, size)) == n0
        lowest = -(-n0 // ndev)
        assert size >= lowest and not any(ok(s) for s in range(lowest, size)), (n0, ndev, size)
        assert len(_slabs(n0, size)) <= ndev


def test_dist_slab_size(dump):
    same = (INVALID, "mgh_*_dist: every rank but the last must hold the same number of planes")
    last = (INVALID, "mgh_*_dist: the last rank holds more planes than the others, or fewer than 3")
    cases = [("20 20 20", ("dist", "20")), ("20 20 3", ("dist", "20")), ("20 7", ("dist", "20")), ("5 5 5 5", ("dist", "5")),
             ("20 19 20", ("err", same)), ("19 20 20", ("err", same)), ("20 20 21", ("err", last)), ("20 20 2", ("err", last)),
             ("2 2", ("err", last))]
    assert _run(dump, "".join("dist %s\n" % c for c, _ in cases)) == [w for _, w in cases]


# ---- the norm and the bound of one subdomain -----------------------------------------------------------------
def test_norm_of_the_whole_domain_bit_for_bit(dump):
    """max for s = inf; else sqrt(sum of ln^2 (* count)) (/ total), accumulated in id order from 0.0 in double."""
    rng = np.random.default_rng(11)
    cases = []
    for k in range(1, 6):
        counts = [int(c) for c in rng.integers(27, 5000, k)]
        lns = [float(x) for x in rng.uniform(0.01, 3.0, k)]
        lns[k // 2] = float(np.float32(lns[k // 2]))  # (a norm that came from a float32 reduction)
        for inf, normalize in itertools.product((1, 0), (1, 0)):
            cases.append((inf, normalize, counts, lns))
    text = ""
    for inf, normalize, counts, lns in cases:
        text += "norm %d %d %d %d %s\n" % (inf, normalize, sum(counts), len(counts), " ".join("%s %d" % (l.hex(), c) for l, c in zip(lns, counts)))
    res = _run(dump, text)
    assert len(res) == len(cases) == 20
    for (inf, normalize, counts, lns), (kind, got) in zip(cases, res):
        acc = 0.0
        for ln, c in zip(lns, counts):
            acc = max(acc, ln) if inf else acc + ln * ln * (float(c) if normalize else 1.0)
        want = acc if inf else math.sqrt(acc / float(sum(counts))) if normalize else math.sqrt(acc)
        assert kind == "norm" and float.fromhex(got) == want, (inf, normalize, counts)


def test_local_abs_tol_bit_for_bit(dump):
    """calc_local_abs_tol in the data type: REL tol * norm, ABS tol; s != inf: sqrt(that^2 / nsub)."""
    cases = [(eb, norm, tol, s, nsub) for eb in (0, 1) for norm in (1.0, 2.7182817459106445, 123.456) for tol in (1e-3, 0.37)
             for s in (INF, 0.0, 1.5) for nsub in (1, 2, 3, 7, 24)]
    text = "".join("%s %d %s %s %s %d\n" % (t, eb, float(norm).hex(), float(tol).hex(), "inf" if s == INF else float(s).hex(), nsub)
                   for eb, norm, tol, s, nsub in cases for t in ("tol32", "tol64"))
    res = _run(dump, text)
    assert len(res) == 2 * len(cases)
    for k, (eb, norm, tol, s, nsub) in enumerate(cases):
        for j, T in enumerate((np.float32, np.float64)):
            n, t = T(norm), T(tol)
            base = t * n if eb == 0 else t
            want = base if s == INF else np.sqrt((base * base) / T(nsub))
            assert type(want) is T
            kind, got = res[2 * k + j]
            assert kind == "tol" and float.fromhex(got) == float(want), (eb, norm, tol, s, nsub, T)


# ---- headers -----------------------------------------------------------------------------------------------
def _hl():
    from mgard_amd import highlevel as hl
    return hl


def _header(shape, dd=None, dt="f32", nonuniform=False, mode=None, tol=1e-3, s=INF, norm=1.0, dd_size0=None, **kw):
    """Bytes of a header. dd_size0: the size a header WITHOUT decomposition records (hl.metadata_serialize writes
    the extent of dimension 0 there; the slab headers of the library record 0)."""
    hl = _hl()
    npdt = np.float64 if dt == "f64" else np.float32
    coords = nonuniform if isinstance(nonuniform, list) else (
        [c.astype(np.float64).tolist() for c in nonuniform_coords(shape, npdt)] if nonuniform else None)
    mode = hl.REL if mode is None else mode
    b = hl.metadata_serialize(hl.DOUBLE if dt == "f64" else hl.FLOAT, list(shape), mode, tol, s, norm=norm, coords=coords, dd=dd, **kw)
    if dd is None and dd_size0 is not None:
        # the same C entry (mgh_metadata_serialize) with dd_size set: what metadata_serialize() leaves no way to say
        import ctypes as C
        import mgard_amd
        info, store = hl.HeaderInfo(), (C.c_double * (sum(shape) + 1))()
        raw = (C.c_uint8 * len(b)).from_buffer_copy(b)
        L = mgard_amd.load_library()
        assert L.mgh_metadata_parse(raw, len(b), C.byref(info), store, len(store), None) == 0
        info.dd_size = dd_size0
        n = L.mgh_metadata_serialize(C.byref(info), None, 0)
        out = (C.c_uint8 * n)()
        assert L.mgh_metadata_serialize(C.byref(info), out, n) == n
        b = bytes(out)
    return b


SLAB_CASES = [
    # (shape, dtype, non-uniform, size of the slabs of dimension 0, REL?, s, keywords of the header)
    ((40, 65, 70), "f32", False, 17, True, INF, {}),
    ((37, 33, 50), "f64", True, 13, True, 0.0, dict(reorder=1, dict_size=2048, block_size=4096)),
    ((64, 20, 33), "f32", True, 16, False, INF, {}),
    ((130,), "f64", False, 33, False, 1.5, {}),
]


@pytest.mark.parametrize("case", SLAB_CASES, ids=lambda c: "x".join(map(str, c[0])) + "-" + c[1])
def test_slab_header_is_the_header_of_the_slab_alone(dump, case):
    """slab_header() of every id against the header metadata_serialize writes for the slab itself: its shape, ABS,
    the local tolerance, norm 0, the coordinates of dimension 0 cut to the slab, no decomposition -- byte for byte.
    One field cannot be set through hl.metadata_serialize: without a decomposition it records dd_size = shape[0],
    where a slab header records 0. The expected bytes therefore come from the same C entry with that one field set
    (_header(dd_size0=0)); the fields are compared through hl.metadata_parse as well, dd_size among them."""
    hl = _hl()
    shape, dt, nonuniform, size, rel, s, kw = case
    npdt = np.float64 if dt == "f64" else np.float32
    coords = [c.astype(np.float64).tolist() for c in nonuniform_coords(shape, npdt)] if nonuniform else None
    whole = _header(shape, (MAXDIM, 0, size), dt, coords or False, hl.REL if rel else hl.ABS, 1e-3, s, norm=2.5 if rel else 0.0, **kw)
    local_tol = 0.00123 if dt == "f64" else float(np.float32(0.00123))
    cells = blocks(shape, (MAXDIM, 0, size))[0]
    res = _run(dump, "".join("slab %s %d %s\n" % (whole.hex(), i, local_tol.hex()) for i in range(len(cells))))
    assert len(res) == len(cells) > 1
    for (kind, got), (o0, e0) in zip(res, cells):
        sshape = (e0,) + tuple(shape[1:])
        scoords = [coords[0][o0:o0 + e0]] + coords[1:] if nonuniform else False
        want = _header(sshape, None, dt, scoords, hl.ABS, local_tol, s, norm=0.0, dd_size0=0, **kw)
        assert kind == "slab" and got == want.hex(), (o0, e0)
        m, w = hl.metadata_parse(bytes.fromhex(got)), hl.metadata_parse(_header(sshape, None, dt, scoords, hl.ABS, local_tol, s, **kw))
        assert (m["dd_size"], w.pop("dd_size")) == (0, e0) and not m["domain_decomposed"] and m["mode"] == hl.ABS
        assert m["shape"] == list(sshape) and m["tol"] == local_tol and m["norm"] == 0.0 and m["dd_dim"] == 0
        for key, value in w.items():
            if key == "coords":
                assert all(np.array_equal(a, b) for a, b in zip(m["coords"], value))
            elif key != "metadata_size":
                assert m[key] == value, key


UNKNOWN_DD = (FORMAT, "header: unknown domain decomposition")
BAD_DD = (FORMAT, "header: domain decomposition")
NO_SIZES = (INVALID, "Variable domain decomposition: pass the sizes in the config")
BAD_SUM = (INVALID, "Variable sizes do not add up to the extent")


def _header_model(shape, method, dim, size, sizes):
    """decomposer_from_header + the extents check as highlevel.hip made them, in order; None: accepted."""
    D = len(shape)
    if dim >= D or size == 0:
        return BAD_DD
    if method in (MAXDIM, BLOCK):
        ext = [[size] * (n // size) + ([n % size] if n % size else []) for n in (shape if method == BLOCK else [shape[dim]])]
    elif method == VARIABLE:
        if not sizes:
            return NO_SIZES
        if sum(sizes) != shape[dim]:
            return BAD_SUM
        ext = [sizes]
    else:
        return UNKNOWN_DD
    return FEW_NODES if min(min(e) for e in ext) < 3 else None


def _patch_dd_method(header, wire_value):
    """The header with the wire value of its decomposition method replaced (field 1 of message 7), CRC redone."""
    import struct
    import zlib
    body = bytearray(header[17:])
    # tag of field 7 (length-delimited), its length, tag of field 1 (varint), the method
    hits = [i for i in range(len(body) - 3) if body[i] == 0x3a and body[i + 2] == 0x08 and body[i + 3] in (1, 2, 3)]
    assert len(hits) == 1
    body[hits[0] + 3] = wire_value
    return header[:5] + struct.pack("<QI", len(body), zlib.crc32(bytes(body))) + bytes(body)


def _damaged():
    """[(name, header bytes, Variable sizes passed, verdict)]: one mutation of a valid header each."""
    shape = (40, 65, 70)
    out = []

    def add(name, method, dim, size, sizes=None, wire=None):
        hb = _header(shape, (min(method, VARIABLE), dim, size))
        if wire is not None:
            hb = _patch_dd_method(hb, wire)
        out.append((name, hb, sizes or [], _header_model(shape, method, dim, size, sizes)))

    add("valid MaxDim", MAXDIM, 0, 17)
    add("valid Block", BLOCK, 0, 33)
    add("valid Variable", VARIABLE, 1, 20, [20, 30, 15])
    add("dd_dim = D", MAXDIM, 3, 17)
    add("dd_dim huge", MAXDIM, 2 ** 40, 17)
    add("dd_size = 0", MAXDIM, 0, 0)
    add("dd_size = 0, Block", BLOCK, 0, 0)
    add("unknown method", 4, 0, 17, wire=4)
    add("unknown method, dd_dim = D", 4, 3, 17, wire=4)  # two defects: the dimension is looked at first
    add("remainder slab of 1", MAXDIM, 0, 13)
    add("remainder slab of 2", MAXDIM, 1, 21)
    add("remainder block of 1", BLOCK, 0, 23)
    add("slabs of 2", MAXDIM, 2, 2)
    add("Variable without sizes", VARIABLE, 1, 20)
    add("Variable, wrong sum", VARIABLE, 1, 20, [20, 30, 16])
    add("Variable, a size of 2", VARIABLE, 1, 20, [20, 43, 2])
    add("Variable, dd_dim = D", VARIABLE, 3, 20, [20, 30, 15])
    return out


def _damaged_text(cases):
    return "".join("fromheader %s %s\n" % (hb.hex(), _ints(len(sizes), *sizes)) for _, hb, sizes, _ in cases)


def _check_damaged(cases, res):
    assert len(res) == len(cases)
    for (name, hb, sizes, verdict), (kind, got) in zip(cases, res):
        if verdict is None:
            assert kind == "ok", (name, got)
        else:
            assert (kind, got) == ("err", verdict), name


def test_damaged_headers_are_refused_with_the_same_status_and_message(dump):
    cases = _damaged()
    _check_damaged(cases, _run(dump, _damaged_text(cases)))
    # the verdicts themselves, so that the model cannot drift along with the header
    v = {name: verdict for name, _, _, verdict in cases}
    assert v["valid MaxDim"] is v["valid Block"] is v["valid Variable"] is None
    assert v["dd_dim = D"] == v["dd_dim huge"] == v["dd_size = 0"] == v["dd_size = 0, Block"] == v["Variable, dd_dim = D"] == BAD_DD
    assert v["unknown method"] == UNKNOWN_DD and v["unknown method, dd_dim = D"] == BAD_DD
    assert v["remainder slab of 1"] == v["remainder slab of 2"] == v["remainder block of 1"] == v["slabs of 2"] == FEW_NODES
    assert (v["Variable without sizes"], v["Variable, wrong sum"], v["Variable, a size of 2"]) == (NO_SIZES, BAD_SUM, FEW_NODES)
    # the library gives the same verdicts today (mgh_infer_coarsened_shape runs both checks on a header alone)
    hl = _hl()
    for name, hb, sizes, verdict in cases:
        cfg = hl.Config(domain_decomposition_sizes=sizes) if sizes else hl.Config()
        buf = np.frombuffer(hb, np.uint8)
        if verdict is None:
            hl.infer_coarsened(buf, None, cfg)
        else:
            with pytest.raises(hl.MgardHipError, match=r"error %d\b.*%s" % (verdict[0], __import__("re").escape(verdict[1]))):
                hl.infer_coarsened(buf, None, cfg)


# ---- frames ------------------------------------------------------------------------------------------------
def test_frame_rule(dump):
    stream, record = (FORMAT, "truncated stream"), (FORMAT, "truncated record")
    cases = [((100, 60, 32), ("next", "100")),            # exact fit
             ((100, 60, 0), ("next", "68")), ((100, 92, 0), ("next", "100")),
             ((100, 93, 0), ("err", stream)),             # one byte short of the prefix
             ((100, 100, 0), ("err", stream)),
             ((100, 60, 33), ("err", record)),            # one byte more than is left
             ((100, 92, 1), ("err", record)),
             ((100, 60, 2 ** 64 - 1), ("err", record)), ((100, 60, 2 ** 64 - 68), ("err", record)),  # (at + 8 + cs wraps to 0)
             ((100, 60, 2 ** 63), ("err", record))]
    assert _run(dump, "".join("frame %d %d %d\n" % c for c, _ in cases)) == [w for _, w in cases]


# ---- sanitizers --------------------------------------------------------------------------------------------
def test_program_is_clean_under_address_and_undefined_sanitizers(tmp_path_factory):
    exe = _build(tmp_path_factory, "domain_plan_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    cases = _damaged()
    whole = _header((37, 33, 50), (MAXDIM, 0, 13), "f64", True)
    text = _damaged_text(cases) + "".join("slab %s %d 0x1p-10\n" % (whole.hex(), i) for i in range(3))
    text += "geom 1 3 70 45 37 0 33 0\n" + _split_cmd((66, 300, 80), 4, 1) + "frame 100 60 18446744073709551615\nmulti 64 7\n"
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-4000:]
    res = _parse(p.stdout)
    assert len(res) == len(cases) + 7
    _check_damaged(cases, res[:len(cases)])
    assert [k for k, _ in res[len(cases):]] == ["slab"] * 3 + ["geom", "err", "err", "multi"]
