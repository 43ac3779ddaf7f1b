"""Small arrays whose Thomas solves reach the six kernel families that tests/ipk_stream_cases.py does
not cover -- Dma, LdsContigChunked, LdsContig, LdsStrided, Spec and Thread of mgard_amd/csrc/ipk_plan.hpp
-- in the format of that table: ONE table for tests/test_ipk_family_cases_cpu.py (the planner picks
the family with these arguments: no GPU needed) and tests/test_gpu_ipk_families.py (the library's own
plan log shows exactly that, and the results are the oracle's bits).

A case: `shape`, `dtype`, `nonuniform`, the environment `env`, `chunk_need` (the warm-up length the
Thomas tables of the element type need: 24 for float, 40 for double on uniform grids, the values of
tests/golden/ipk_plans.json; the GPU test confirms it through the logged K of the LdsContigChunked
solves; 0 for a 4-D array, whose hierarchy derives no warm-up length from its tables, so that on the
fused 4-D route a contiguous solve is chunked only where MGH_IPK_CHUNK_K says how) and `solves`: the solves the case is there for as ipk_launch sees them -- element size, axis,
the compact coarse box m (a coarse extent is fine // 2 + 1), boxes per launch and their stride, every
`add` the log must show (0: plain, +1 / -1: the r-solve of decompose / recompose) -- with the family
expected and whichever of W (LdsStrided), P (LdsContig, LdsContigChunked), K (LdsContigChunked, Spec)
and KR (Dma) that family uses.

Which route brings a solve to the planner:
  * fused 3-D (the default): the r-solve only (axis 0, add +-1); the f- and c-solve (axes 2 and 1, add 0)
    too where a coarse plane does not fit LDS (ipk_plane_fits_lds: m1 * (m2 | 1) * elem > 150 KB, or an
    extent over 1024). Solves of a top level whose coarse box fits the tail kernel (about 12 K floats)
    leave no record: every fused 3-D box here is larger.
  * MGH_FORCE_V1=1, and every 1-D and 2-D array: the three solves of every level, add on the last.
  * fused 4-D (t, r, c, f): per level the f- and c-solve of the box (m_t * m_r, m_c, m_f), then the
    r-solve of m_t boxes (m_r, m_c, m_f) in one launch, m_r * m_c * m_f apart; add 0 throughout.

Arithmetic used below (ipk_plan.hpp), on 256 CUs where every box here is one round of tiles:
  * tile width of the LDS-staged families: the widest of 64, 48, 32, 16 with W * pencil bytes <= 160 KB,
    so 64 up to 640 floats / 320 doubles, 48 up to 853 / 426, 32 up to 1280 / 640, 16 up to 2560 / 1280
    (an even contiguous pencil is padded by one element); longer pencils fit no tile.
  * Dma: floats, axes 0 and 1, 160 <= n <= 784 (KR = 10 batches of 16 in registers, (n - 160) * 256 bytes
    of LDS <= 156 KB) and at least MGH_IPK_DMA_MIN tiles of 64 pencils (512 by default: never here).
  * LdsContigChunked: axis 2, n >= 64, W * pencil bytes + 8 KB <= 160 KB, warm-up K <= n / 2.
  * Spec: axis 2 with at most 64 pencils of 2048+; strided pencils of MGH_IPK_SPEC_LONG (1024)+; pencils
    of 2048+ that fit no tile. K = 64 floats / 128 doubles or MGH_IPK_SPEC_K.
  * Stream needs two rounds of tiles and is never planned here.

Thread with nbatch > 1 (`per_batch`: the boxes run one call each and leave one record each, nbatch 1)
is reached by the 4-D case "thread-4d-batches".

What the cases are chosen for is asserted over the whole table by test_ipk_family_cases_cpu.py
(`test_table_covers_every_class`)."""

V1 = {"MGH_FORCE_V1": "1"}
DMA0 = {"MGH_IPK_DMA_MIN": "0"}
NEED = {"f32": 24, "f64": 40}  # chunk_need of uniform grids (tests/golden/ipk_plans.json)
# every array at or below this many elements unless the row says why not
MAX_ELEMS = 1_500_000
LARGER = {}  # id -> reason

R = (+1, -1)  # an r-solve: decompose adds, recompose subtracts


def solve(elem, axis, m, add, family, W=0, P=0, K=0, KR=0, nbatch=1, batch_stride=0, per_batch=False):
    return dict(elem=elem, axis=axis, m=tuple(m), nbatch=nbatch, batch_stride=batch_stride, add=tuple(add),
                family=family, W=W, P=P, K=K, KR=KR, per_batch=per_batch)


def case(id, shape, dtype, env, solves, nonuniform=False):
    return dict(id=id, shape=tuple(shape), dtype=dtype, nonuniform=nonuniform, env=env, solves=solves,
                chunk_need=NEED[dtype] if len(shape) <= 3 else 0)


def dma(axis, m, add, **kw):
    return solve(4, axis, m, add, "Dma", KR=10, **kw)


def strided(elem, axis, m, add, W):
    return solve(elem, axis, m, add, "LdsStrided", W=W)


def contig(elem, m, P=64):
    return solve(elem, 2, m, (0,), "LdsContig", P=P)


def chunked(elem, m, K, P=64):
    return solve(elem, 2, m, (0,), "LdsContigChunked", P=P, K=K)


def spec(elem, axis, m, add, K, **kw):
    return solve(elem, axis, m, add, "Spec", K=K, **kw)


def thread(elem, axis, m, add, **kw):
    return solve(elem, axis, m, add, "Thread", **kw)


CASES = [
    # ---- Dma (float, MGH_IPK_DMA_MIN=0) ----
    # r-solve, n = 160 = KR batches exactly: no LDS part; 16 * 26 = 416 pencils = 6 tiles and one of 32
    case("dma-n160", (319, 30, 50), "f32", DMA0, [dma(0, (160, 16, 26), R)]),
    # n = 201 (fine extent 400: ghost node): an LDS part of 41 rows, 41 * 256 B
    case("dma-n201", (400, 30, 50), "f32", DMA0, [dma(0, (201, 16, 26), R)]),
    # n = 450: 290 rows in LDS (74 KB, two tiles per CU); 5 * 13 = 65 pencils: the last tile holds ONE
    case("dma-n450-1pencil", (899, 9, 25), "f32", DMA0, [dma(0, (450, 5, 13), R)], nonuniform=True),
    # fused 4-D: the r-solve of the three coarse t-slices in one launch, 161 * 6 * 18 = 17388 apart;
    # 3 * 108 = 324 pencils, tiles that straddle the slices
    case("dma-4d-batches", (5, 321, 11, 35), "f32", DMA0,
         [dma(0, (161, 6, 18), (0,), nbatch=3, batch_stride=161 * 6 * 18)]),
    # fused 3-D, planes of 200 x 201 floats = 160.8 KB > 150 KB: the f- and c-solve go through the planner.
    # c-solve: n = 200, rows of 200 pencils (200 % 64 = 8: tiles straddle planes), 600 pencils = 10 tiles;
    # f-solve: 64 * 201 * 4 + 8 KB fits, K = 24 <= 100: chunked, 600 rows = 9 tiles and one of 24
    case("dma-axis1-fused", (5, 399, 398), "f32", DMA0, [dma(1, (3, 200, 200), (0,)), chunked(4, (3, 200, 200), 24)]),
    # MGH_FORCE_V1: c-solve with n = 166 (6 rows in LDS) and rows of 36 pencils < 64: a tile covers two
    # planes; f-solve n = 36 < 64 even: LdsContig; r-solve n = 21 < 160: LdsStrided
    case("dma-axis1-v1", (40, 330, 70), "f32", dict(V1, **DMA0),
         [dma(1, (21, 166, 36), (0,)), contig(4, (21, 166, 36)), strided(4, 0, (21, 166, 36), R, 64)]),
    # ---- LdsContigChunked ----
    # the fused 3-D box above without the Dma switch: MGH_IPK_CHUNK_K=3 sends most tiles through the second
    # pass (n = 200 even: pad 1); its c-solve, 10 tiles < 512, is LdsStrided with tiles of 64 * 800 B
    case("chunk-f32-k3", (5, 399, 398), "f32", {"MGH_IPK_CHUNK_K": "3"},
         [chunked(4, (3, 200, 200), 3), strided(4, 1, (3, 200, 200), (0,), 64)]),
    # double, fused 3-D, planes of 140 x 141 doubles = 157.9 KB > 150 KB; n = 141 odd, K = 40 <= 70;
    # 420 rows = 6 tiles and one of 36; c-solve n = 140 <= 320 doubles: W = 64
    case("chunk-f64-fused", (5, 279, 281), "f64", {}, [chunked(8, (3, 140, 141), 40), strided(8, 1, (3, 140, 141), (0,), 64)]),
    # MGH_FORCE_V1, float, n = 199 odd, K = 24 <= 99; 416 rows = 6 tiles and one of 32
    case("chunk-f32-v1-odd", (30, 50, 397), "f32", V1, [chunked(4, (16, 26, 199), 24)]),
    # fused 4-D: f-solve of the box (3 * 16, 11, 100); n = 100 even; 528 rows = 8 tiles and one of 16. A 4-D
    # hierarchy has chunk_need 0 (above): chunked only with MGH_IPK_CHUNK_K, 3 <= 50
    case("chunk-f32-4d", (5, 30, 20, 199), "f32", {"MGH_IPK_CHUNK_K": "3"}, [chunked(4, (48, 11, 100), 3)]),
    # ... and without it the same solve is LdsContig: K = 0
    case("contig-f32-4d", (5, 30, 20, 199), "f32", {}, [contig(4, (48, 11, 100))]),
    # double, n = 140 even, second pass
    case("chunk-f64-v1-k3-even", (30, 50, 279), "f64", dict(V1, MGH_IPK_CHUNK_K="3"), [chunked(8, (16, 26, 140), 3)]),
    # ---- LdsContig ----
    # the chunked solve switched off: n = 199 odd, 6 tiles and one of 32
    case("contig-chunk-off", (30, 50, 397), "f32", dict(V1, MGH_IPK_CHUNK="0"), [contig(4, (16, 26, 199))]),
    # double, n = 75 >= 64 but K = 40 > 75 / 2 = 37: not chunked; c-solve n = 26 and r-solve n = 16 of doubles
    case("contig-f64-k-over-half", (30, 50, 149), "f64", V1,
         [contig(8, (16, 26, 75)), strided(8, 1, (16, 26, 75), (0,), 64), strided(8, 0, (16, 26, 75), R, 64)]),
    # ---- LdsStrided ----
    # r-solve, n = 200 floats <= 640: W = 64 (416 pencils = 7 tiles < 512: not Dma)
    case("strided-w64-f32", (399, 30, 50), "f32", {}, [strided(4, 0, (200, 16, 26), R, 64)]),
    # the same array with MGH_FORCE_V1: c-solve n = 16; f-solve n = 26 < 64 even: LdsContig
    case("strided-v1-f32", (399, 30, 50), "f32", V1,
         [strided(4, 1, (200, 16, 26), (0,), 64), contig(4, (200, 16, 26)), strided(4, 0, (200, 16, 26), R, 64)]),
    # n = 700 floats: 64 * 2800 = 179200 > 163840 >= 48 * 2800; 171 pencils = 3 tiles and one of 27
    case("strided-w48-f32", (1399, 17, 37), "f32", {}, [strided(4, 0, (700, 9, 19), R, 48)], nonuniform=True),
    # n = 901 floats: 48 * 3604 = 172992 > 163840 >= 32 * 3604; n < 1024: not yet Spec; (n - 160) * 256 > 156 KB: not Dma
    case("strided-w32-f32", (1801, 17, 21), "f32", {}, [strided(4, 0, (901, 9, 11), R, 32)]),
    # n = 1301 floats: 32 * 5204 = 166528 > 163840 >= 16 * 5204; 1301 >= 1024 needs MGH_IPK_SPEC_LONG=0
    case("strided-w16-f32", (2601, 9, 21), "f32", {"MGH_IPK_SPEC_LONG": "0"}, [strided(4, 0, (1301, 5, 11), R, 16)]),
    # doubles: n = 400: 64 * 3200 > 163840 >= 48 * 3200
    case("strided-w48-f64", (799, 17, 21), "f64", {}, [strided(8, 0, (400, 9, 11), R, 48)]),
    # n = 501: 48 * 4008 = 192384 > 163840 >= 32 * 4008
    case("strided-w32-f64", (1001, 9, 21), "f64", {}, [strided(8, 0, (501, 5, 11), R, 32)], nonuniform=True),
    # n = 700: 32 * 5600 = 179200 > 163840 >= 16 * 5600
    case("strided-w16-f64", (1399, 9, 21), "f64", {}, [strided(8, 0, (700, 5, 11), R, 16)]),
    # MGH_FORCE_V1, c-solve with tiles of 48: n = 700, rows of 19 pencils, 171 pencils; f-solve n = 19 odd
    case("strided-axis1-w48-v1", (17, 1399, 37), "f32", V1,
         [strided(4, 1, (9, 700, 19), (0,), 48), contig(4, (9, 700, 19)), strided(4, 0, (9, 700, 19), R, 64)]),
    # ---- Spec ----
    # a 1-D array: ONE contiguous pencil of 35001 per level, add on the only solve: k_ipk_spec_apply
    case("spec-1d", (70001,), "f32", {}, [spec(4, 2, (1, 1, 35001), R, 64)], nonuniform=True),
    # warm-up of 2: nearly every chunk fails the comparison and is repaired
    case("spec-1d-k2", (70001,), "f32", {"MGH_IPK_SPEC_K": "2"}, [spec(4, 2, (1, 1, 35001), R, 2)], nonuniform=True),
    # strided pencils of 1301 >= MGH_IPK_SPEC_LONG = 1024 that would fit tiles of 16; 55 pencils <= 64 * 256
    case("spec-long-f32", (2601, 9, 21), "f32", {}, [spec(4, 0, (1301, 5, 11), R, 64)]),
    case("spec-long-f32-k2", (2601, 9, 21), "f32", {"MGH_IPK_SPEC_K": "2"}, [spec(4, 0, (1301, 5, 11), R, 2)]),
    # strided pencils too long for LDS: 2101 doubles > 1280, >= 2048; the SPEC_LONG rule switched off
    case("spec-toolong-f64", (4201, 9, 13), "f64", {"MGH_IPK_SPEC_LONG": "0"}, [spec(8, 0, (2101, 5, 7), R, 128)]),
    # contiguous pencils too long for LDS, 72 > 64 of them; m2 = 2101 > 1024: the plane kernel does not take the box
    case("spec-axis2-f64", (14, 16, 4201), "f64", {}, [spec(8, 2, (8, 9, 2101), (0,), 128)]),
    # c-solve of 2101 doubles (m1 > 1024: no plane kernel), 72 pencils
    case("spec-axis1-f64", (14, 4201, 16), "f64", {}, [spec(8, 1, (8, 2101, 9), (0,), 128)]),
    # fused 4-D: three boxes back to back (stride = m0 * m1 * m2 = 19515) are one Spec solve of 45 pencils
    case("spec-4d-batches", (5, 2601, 5, 9), "f64", {}, [spec(8, 0, (1301, 3, 5), (0,), 128, nbatch=3, batch_stride=1301 * 15)]),
    # ---- Thread (MGH_IPK_SPEC=0 on pencils too long for LDS) ----
    case("thread-axis0", (4201, 9, 13), "f64", {"MGH_IPK_SPEC": "0"}, [thread(8, 0, (2101, 5, 7), R)]),
    case("thread-axis1", (14, 4201, 16), "f64", {"MGH_IPK_SPEC": "0"}, [thread(8, 1, (8, 2101, 9), (0,))]),
    case("thread-axis2", (14, 16, 4201), "f64", {"MGH_IPK_SPEC": "0"}, [thread(8, 2, (8, 9, 2101), (0,))]),
    # 1301 doubles > 1280 fit no tile: the three boxes of the 4-D r-solve run one call each
    case("thread-4d-batches", (5, 2601, 5, 9), "f64", {"MGH_IPK_SPEC": "0"},
         [thread(8, 0, (1301, 3, 5), (0,), nbatch=3, batch_stride=1301 * 15, per_batch=True)]),
]
