"""Small arrays whose Thomas solves run k_ipk_stream (mgard_amd/csrc/kernels_ipk_stream.hpp), the
solver of the production sizes: ONE table for tests/test_ipk_stream_cases_cpu.py (the planner picks
the kernel with these attributes: no GPU needed) and tests/test_gpu_ipk_stream.py (the library
planned exactly that, and the results are the oracle's bits).

The planner takes the streaming kernel only where the LDS-staged tiles need two or more rounds of
resident workgroups -- arrays of tens of megabytes on 256 CUs. MGH_IPK_PLAN_CU tells it the device
has 1 or 2, and then boxes of a few hundred thousand elements get there: pencils of 128+ floats or
64+ doubles (n / U >= KR = 8 batches of U = 16 floats / 8 doubles), 512+ floats for KR = 16.

A case: `shape` of the array, `dtype`, `nonuniform` coordinates or not, the environment `env`, and
`solves`, the solves the case is there for as ipk_launch sees them -- element size, axis and extents
m of the compact coarse box (a coarse extent n comes from a fine extent 2n - 1 or, with a ghost node,
2n - 2), boxes per launch and their stride, and `add`: every value the log must show for that solve
(0: plain, +1: the r-solve of decompose adds to the coarse nodes, -1: that of recompose subtracts)
-- with the plan expected for it: tile width W, leading elements n_glob parked in global memory and
register-resident batches KR. MGH_FORCE_V1=1 sends the f-, c- and r-solve of every level through
ipk_launch; without it the f- and c-solves of boxes whose planes fit in LDS run in another kernel and
only the r-solves get there.

What the cases are chosen for is asserted over the whole table by test_ipk_stream_cases_cpu.py
(`test_table_covers_every_class`). One class cannot be reached and is not in it: n_glob == parked
with parked > 0. The planner raises n_glob only while that lowers the rounds of resident workgroups;
with one batch left in LDS a tile needs W * U * elem <= 4 KB (+ 4.25 KB of staging for contiguous
pencils), 18 or more tiles fit the 156 KB of a CU, the cap is MGH_IPK_WPC <= 16 tiles either way, and
so parking the last batch as well never wins. The table has n_glob == parked == 0 instead (n / U ==
KR: no LDS at all for strided pencils, the staging area alone for contiguous ones) and n_glob up to
parked - U."""

V1 = {"MGH_FORCE_V1": "1"}
CU1 = {"MGH_IPK_PLAN_CU": "1"}
STRIDED = dict(CU1, MGH_IPK_DMA="0")                      # (float strided pencils: not the LDS-DMA kernel)
CONTIG = dict(CU1, MGH_IPK_CHUNK="0", MGH_IPK_CONTIG="2")  # (not the chunked LDS-staged kernel; stream from 2 rounds)

# environment -> members of IpkTuning (capi.hip: ipk_tuning_from_env), as tests/cpp/ipk_plan_dump.cpp names them
SWITCH_MEMBER = {"MGH_IPK_PLAN_CU": "num_cu", "MGH_IPK_DMA": "dma", "MGH_IPK_DMA_MIN": "dma_min", "MGH_IPK_WPC": "wpc",
                 "MGH_IPK_W": "w", "MGH_IPK_KR16": "kr16", "MGH_IPK_CONTIG": "contig_rounds", "MGH_IPK_CHUNK": "chunk",
                 "MGH_IPK_STREAM": "stream", "MGH_IPK_SPEC": "spec", "MGH_IPK_SPEC_K": "spec_k",
                 "MGH_IPK_SPEC_LONG": "spec_long", "MGH_IPK_SPEC_MAX": "spec_max", "MGH_IPK_CHUNK_K": "chunk_k",
                 "MGH_IPK_DMA_ROUNDS": "dma_rounds"}
NOT_THE_PLANNERS = ("MGH_FORCE_V1", "MGH_IPK_RANGE_MB")


def tuning(env, num_cu=256):
    """The planner's switches for an environment on a device of num_cu CUs."""
    t = {SWITCH_MEMBER[k]: int(v) for k, v in env.items() if k not in NOT_THE_PLANNERS}
    t.setdefault("num_cu", num_cu)
    t.setdefault("dma_min", 2 * t["num_cu"])
    return t


def solve(elem, axis, m, add, W, n_glob, KR, nbatch=1, batch_stride=0):
    return dict(elem=elem, axis=axis, m=tuple(m), nbatch=nbatch, batch_stride=batch_stride, add=tuple(add), W=W,
                n_glob=n_glob, KR=KR)


def case(id, shape, dtype, env, solves, nonuniform=False):
    return dict(id=id, shape=tuple(shape), dtype=dtype, nonuniform=nonuniform, env=env, solves=solves)


R = (+1, -1)  # an r-solve: decompose adds, recompose subtracts

CASES = [
    # ---- float, strided along axis 0
    # 520 = 32 batches + 8: KR = 16, 16 batches in LDS; 90 pencils = a tile of 64 and one of 26, six empty tiles
    case("f32-kr16", (1038, 17, 18), "f32", dict(V1, **STRIDED), [solve(4, 0, (520, 9, 10), R, 64, 0, 16)]),
    # the same box with KR = 8: 24 batches in LDS, which leaves room for tiles of 48
    case("f32-kr16-off", (1038, 17, 18), "f32", dict(V1, MGH_IPK_KR16="0", **STRIDED),
         [solve(4, 0, (520, 9, 10), R, 48, 0, 8)]),
    # 513 = 32 batches + 1; three batches of every pencil parked in global memory
    case("f32-kr16-glob", (1025, 41, 51), "f32", dict(V1, **STRIDED), [solve(4, 0, (513, 21, 26), R, 64, 48, 16)],
         nonuniform=True),
    # without MGH_FORCE_V1: the r-solves alone; two of the four parked batches in global memory
    case("f32-r-glob", (399, 79, 99), "f32", dict(STRIDED, MGH_IPK_WPC="16"), [solve(4, 0, (200, 40, 50), R, 64, 32, 8)]),
    case("f32-w32", (399, 79, 99), "f32", dict(V1, MGH_IPK_W="32", **STRIDED), [solve(4, 0, (200, 40, 50), R, 32, 0, 8)]),
    # 2310 pencils over two CUs: 39 tiles of 60 are one round less than 37 of 64
    case("f32-w60", (398, 65, 139), "f32", dict(V1, MGH_IPK_PLAN_CU="2", MGH_IPK_DMA="0", MGH_IPK_WPC="16"),
         [solve(4, 0, (200, 33, 70), R, 60, 0, 8)]),
    # 128 = KR batches exactly: nothing parked, no LDS
    case("f32-lds0", (255, 39, 59), "f32", dict(V1, MGH_IPK_WPC="16", **STRIDED), [solve(4, 0, (128, 20, 30), R, 64, 0, 8)]),
    # ---- float, strided along axis 1: rows of 45 pencils, so every tile of 64 straddles planes; 159 = 9 batches + 15
    case("f32-axis1", (39, 317, 89), "f32", dict(V1, **STRIDED), [solve(4, 1, (20, 159, 45), (0,), 64, 0, 8)]),
    # ---- float, contiguous along axis 2 (TileIO)
    case("f32-contig-glob", (79, 99, 399), "f32", dict(V1, **CONTIG), [solve(4, 2, (40, 50, 200), (0,), 64, 16, 8)]),
    # 143 = KR batches + 15: LDS is the staging area alone; 513 rows: the last tile holds ONE
    case("f32-contig-1row", (37, 53, 285), "f32", dict(V1, **CONTIG), [solve(4, 2, (19, 27, 143), (0,), 64, 0, 8)]),
    # 520 rows: the last tile holds 8
    case("f32-contig-8rows", (38, 50, 284), "f32", dict(V1, **CONTIG), [solve(4, 2, (20, 26, 143), (0,), 64, 0, 8)],
         nonuniform=True),
    # 2800 rows in tiles of 60: lanes 60..63 shadow the last row of their tile and write ITS LDS column, so
    # they must carry its values (a change to what the lanes beyond the rows of a tile read shows up here)
    case("f32-contig-w60", (27, 399, 398), "f32", dict(V1, **CONTIG), [solve(4, 2, (14, 200, 200), (0,), 60, 0, 8)]),
    # ---- double
    case("f64-r-glob", (199, 79, 99), "f64", dict(CU1, MGH_IPK_WPC="16"), [solve(8, 0, (100, 40, 50), R, 64, 16, 8)],
         nonuniform=True),
    case("f64-lds0", (127, 59, 79), "f64", dict(V1, **CU1), [solve(8, 0, (64, 30, 40), R, 64, 0, 8)]),
    case("f64-axis1", (39, 145, 89), "f64", dict(V1, **CU1), [solve(8, 1, (20, 73, 45), (0,), 64, 0, 8)]),
    case("f64-contig-glob", (79, 99, 199), "f64", dict(V1, **CONTIG), [solve(8, 2, (40, 50, 100), (0,), 64, 8, 8)]),
    case("f64-contig-rem3", (41, 51, 149), "f64", dict(V1, **CONTIG), [solve(8, 2, (21, 26, 75), (0,), 64, 0, 8)]),
    case("f64-contig-1row", (37, 53, 157), "f64", dict(V1, **CONTIG), [solve(8, 2, (19, 27, 79), (0,), 64, 0, 8)],
         nonuniform=True),
    case("f64-contig-stage-only", (65, 64, 141), "f64", dict(V1, **CONTIG), [solve(8, 2, (33, 33, 71), (0,), 64, 0, 8)]),
    # ---- 4-D, slice by slice: the r-solve of the three coarse t-slices in one launch
    case("f32-4d-batches", (5, 259, 41, 51), "f32", STRIDED,
         [solve(4, 0, (130, 21, 26), (0,), 64, 0, 8, nbatch=3, batch_stride=130 * 21 * 26)]),
]

# The f- and c-solve of a level in ranges of r-planes (capi.hip, the level loop of decompose_fused:
# boxes of more than 2 * MGH_IPK_RANGE_MB). `coarse`: the box; `ranges`: the planes of each range;
# `plane_in_lds`: the two solves of a range are ONE launch of the plane kernel ("ipk_fc" in the
# profile) and leave no record, else `solves` lists them per sub-box (family Stream where the
# environment plans it, with the plan attributes as above; else None for the three).
RANGE_MB1 = {"MGH_IPK_RANGE_MB": "1"}
RANGE_CASES = [
    dict(id="range-f32", shape=(259, 131, 131), dtype="f32", nonuniform=False, env=RANGE_MB1, coarse=(130, 66, 66),
         ranges=(43, 43, 44), plane_in_lds=True, solves=[]),
    dict(id="range-f64", shape=(258, 130, 67), dtype="f64", nonuniform=True, env=RANGE_MB1, coarse=(130, 66, 34),
         ranges=(43, 43, 44), plane_in_lds=True, solves=[]),
    # planes of 200 x 200 floats do not fit in LDS: every range is an f- and a c-solve of its own,
    # streaming ones with MGH_IPK_PLAN_CU=1; 14 planes in ranges of 4, 5 and 5
    dict(id="range-f32-plan-cu", shape=(27, 399, 398), dtype="f32", nonuniform=False,
         env=dict(RANGE_MB1, MGH_IPK_DMA="0", **CONTIG), coarse=(14, 200, 200), ranges=(4, 5, 5), plane_in_lds=False,
         solves=[solve(4, 2, (4, 200, 200), (0,), 64, 0, 8), solve(4, 2, (5, 200, 200), (0,), 64, 16, 8),
                 solve(4, 1, (4, 200, 200), (0,), 64, 0, 8), solve(4, 1, (5, 200, 200), (0,), 64, 0, 8)]),
    # three planes in five ranges: two of them are empty and must be skipped
    dict(id="range-empty", shape=(5, 1199, 1198), dtype="f32", nonuniform=False, env=RANGE_MB1, coarse=(3, 600, 600),
         ranges=(0, 1, 0, 1, 1), plane_in_lds=False,
         solves=[solve(4, 2, (1, 600, 600), (0,), None, None, None), solve(4, 1, (1, 600, 600), (0,), None, None, None)]),
]
