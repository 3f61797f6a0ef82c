"""Exact-arithmetic checks of every factorisation and GEMM path: inputs (oracle/exact.py) for which every intermediate of every
correct algorithm is representable in fp64, so the device result must equal the known answer TO THE BIT whatever the summation
order, tile shape, fusion, look-ahead or batch geometry.  A dropped, doubled or stale term is an integer-sized error at a known
(row, column), which names the tile and the step.

What a case list reaches is not taken on trust: tests/test_exact_cases.py (no GPU) runs the schedule printer over POTRF_CASES and the
restatement `gemm_paths` below over GEMM_CASES and asserts the forms and paths named in the ids.  Rounding behaviour and conditioning
are NOT checked here - the tolerance suites (test_hip_primitives.py, test_augmented_tail_gpu.py, ...) keep that job.
"""
import collections
import functools

import numpy as np
import pytest

from oracle import exact

UNFUSED = 2   # GPAR_POTRF_UNFUSED
NO_LOOKAHEAD = 1   # GPAR_POTRF_NO_LOOKAHEAD
SEED0 = 100   # member b of a batch is drawn from seed SEED0 + b; a lone matrix is member 0
DIAG = (1.0, 2.0, 4.0)
IN_BLOCK = 0.125

PotrfCase = collections.namedtuple("PotrfCase", "id N nf odd_lda batch flags env diag in_block")


def _pc(id, N, nf, batch=1, odd_lda=False, flags=0, env=(), diag=DIAG, in_block=IN_BLOCK):
    return PotrfCase(id, N, nf, odd_lda, batch, flags, tuple(sorted(dict(env).items())), diag, in_block)


_GROUP2 = {"GPAR_POTRF_PAIR_ROWS": "512", "GPAR_POTRF_GROUP": "2"}
# (the ids name the form each case is there for; tests/test_exact_cases.py::test_factorisation_cases_reach_the_forms_they_name)
POTRF_CASES = [
    _pc("2113-lone-fused-group4-small-slice", 2113, 2112),
    _pc("2113-lone-grouped", 2113, 2112, env={**_GROUP2, "GPAR_POTRF_FUSE2_ROWS": "0"}),
    _pc("2113-batch3-grouped-lockstep", 2113, 2112, batch=3, env={**_GROUP2, "GPAR_POTRF_FUSE2_BATCH_ROWS": "0"}),
    _pc("2064-batch3-grouped-tail16-on-slice-and-rest", 2064, 2048, batch=3, env={**_GROUP2, "GPAR_POTRF_FUSE2_BATCH_ROWS": "0"}),
    _pc("1601-batch3-fused-group-lockstep", 1601, 1600, batch=3),
    _pc("1601-batch3-single-fused-panels", 1601, 1600, batch=3, env={"GPAR_POTRF_FUSE2_BATCH_ROWS": "0"}),
    _pc("1552-batch3-tail16-on-rest", 1552, 1536, batch=3, env={"GPAR_POTRF_FUSE2_BATCH_ROWS": "0"}),
    _pc("1553-batch3-tail17-stays-in-the-tiles", 1553, 1536, batch=3, env={"GPAR_POTRF_FUSE2_BATCH_ROWS": "0"}),
    _pc("1537-batch3-tail1-on-gemm-slice", 1537, 1536, batch=3, env={"GPAR_POTRF_FUSE2_BATCH_ROWS": "0", "GPAR_POTRF_LA_SMALL_TILES": "0"}),
    _pc("1100-batch3-leaf-batch-ragged", 1100, 1038, batch=3),
    _pc("1100-lone-odd-lda-leaf", 1100, 1038, odd_lda=True),
    _pc("1100-lone-unfused", 1100, 1038, flags=UNFUSED),
    _pc("2661-lone-gemm-slices-ragged-tail-panels", 2661, 2660, env={"GPAR_POTRF_FUSE2_ROWS": "0", "GPAR_POTRF_LA_SMALL_TILES": "0"}),
    _pc("5121-lone-mixed-last-round", 5121, 5120, env={"GPAR_POTRF_FUSE2_ROWS": "0"}),
    _pc("1024-lone-no-update", 1024, 1024),
    # (pivots 1 and 64 inside one 16 x 16 block: above P2_REFINE_RATIO = 32, the strips' refinement branch runs.  The explicit inverse of a
    # 64 x 64 block with such pivots is exact only while the chains of couplings inside the block are short: a thinner block)
    _pc("1601-lone-refinement-pivots-1-and-64", 1601, 1600, diag=(1.0, 64.0), in_block=0.03125),
]
# Lock-step batches at the COUNTS where the batch code branches (the count is the number of layers of a GPAR, or of samples): the
# smallest matrices at which the named predicate is live, every member with data of its own (seed SEED0 + b), so that a wrong matrix
# index is an integer-sized error.  BATCH_CROSSES holds the value of each predicate; tests/test_exact_cases.py checks it against the
# schedule printer and the restatements below.
# (up to 257 seeds reach further into the tail of the block inverses' sizes than three do - one 64 x 64 block of seed 100 + b at 129 rows has an
# inverse entry of 19.2 at in_block = 0.125, above the premise's bound of 16: thinner blocks, largest entry 3.7 over all members)
def _bc(id, N, nf, batch, env=()):
    return _pc(id, N, nf, batch=batch, env=env, in_block=0.0625)


# 128-column steps: a slice that ends on a tile row - the tail split - at 257 rows; with the default 512 columns it takes 641
_NBO128 = {"GPAR_POTRF_NBO": "128"}
BATCH_CASES = [
    _bc("1089-batch5-fused-group-split-team-on-waiting-475", 1089, 1088, batch=5),
    _bc("1105-batch5-tail17-fused-group-split-team-on", 1105, 1088, batch=5),
    _bc("1089-batch6-fused-group-split-team-off-waiting-570", 1089, 1088, batch=6),
    _bc("1105-batch6-tail17-fused-group-split-team-off", 1105, 1088, batch=6),
    _bc("1105-batch7-fused-group-split-team-off-tail17", 1105, 1088, batch=7),
    _bc("1089-batch17-fuse2-rows-970-below-N-single-panels", 1089, 1088, batch=17),
    _bc("1105-batch17-tail17-single-panels", 1105, 1088, batch=17),
    _bc("577-batch65-two-panels-small-slice", 577, 576, batch=65),
    _bc("593-batch65-tail17-half-tile-update", 593, 576, batch=65),
    _bc("257-batch65-small-slice-325-tiles-no-tail", 257, 256, batch=65, env=_NBO128),
    _bc("321-batch130-one-panel", 321, 320, batch=130),
    _bc("337-batch130-tail17-half-tile-update", 337, 320, batch=130),
    _bc("272-batch130-gemm-slice-650-tiles-tail16-gmax1", 272, 256, batch=130, env=_NBO128),
    _bc("129-batch257-one-panel", 129, 128, batch=257),
    _bc("257-batch257-gemm-slice-tail1-gmax1-from-256-on", 257, 256, batch=257, env=_NBO128),
    _bc("145-batch257-tail17-whole-tile-update", 145, 128, batch=257),
]
POTRF_CASES += BATCH_CASES
POTRF_BY_ID = {c.id: c for c in POTRF_CASES}
LONE_TWIN = _pc("1601-lone", 1601, 1600)   # member 0 of "1601-batch3-fused-group-lockstep" on its own

# (b) an exactly zero pivot at column j of member `member`: (case id, member, j, what the column is)
ZERO_PIVOT_CASES = [
    ("1601-batch3-single-fused-panels", 0, 512, "first column of a fused panel"),
    ("1601-batch3-single-fused-panels", 2, 1023, "last column of a fused panel"),
    ("2113-lone-fused-group4-small-slice", 0, 612, "second panel of a fused-group launch"),
    ("1100-lone-odd-lda-leaf", 0, 1030, "ragged leaf panel"),
    ("1601-batch3-fused-group-lockstep", 1, 700, "one member of a lock-step batch"),
    # one indefinite member of a wide batch: the first, the ones on either side of index 64, the last
    ("577-batch65-two-panels-small-slice", 0, 0, "batch 65 member 0 first column"),
    ("577-batch65-two-panels-small-slice", 63, 511, "batch 65 member 63 last column of the first panel"),
    ("577-batch65-two-panels-small-slice", 64, 575, "batch 65 last member last column"),
    ("321-batch130-one-panel", 0, 319, "batch 130 member 0 last column"),
    ("321-batch130-one-panel", 63, 64, "batch 130 member 63 second row block"),
    ("321-batch130-one-panel", 64, 200, "batch 130 member 64"),
    ("321-batch130-one-panel", 129, 0, "batch 130 last member first column"),
]


# (group_waiting and tail_grid RESTATE host code of panel2.h / potrf.h - the schedule printer shows neither the split team nor the
# tail companion's grid -, slice_tiles restates what decides the printer's "small" / "gemm": a change of those rules has to be made here too)
def group_waiting(case, k0=0, S=8):
    """potrf_group_fused (gpar_amd/csrc/panel2.h): the workgroups of a fused launch that mostly wait, over the whole batch; above 512
    the split team (and with it the next team's rows by tile) is switched off."""
    R0 = (case.N - k0 + 63) // 64
    return case.batch * (S + (S - 1) * (S - 2) // 2 + S * S + max(R0 - 2 * S, 0))


def tail_grid(batch, ncols):
    """potrf_tail_update (gpar_amd/csrc/potrf.h): (workgroups per matrix the panel's columns ask for, the clamp gmax)."""
    return -(-ncols // 64), 1 if batch >= 256 else 256 // batch


def slice_tiles(case, kend, next_end):
    """potrf_slice_small (gpar_amd/csrc/potrf_schedule.h): the 64 x 64 tiles of the slice [kend, next_end), counted over the batch."""
    nc, tr = (next_end - kend) // 64, (case.N - kend + 63) // 64
    return (nc * (nc + 1) // 2 + (tr - nc) * nc) * case.batch


# the value of every batch-dependent predicate a case of BATCH_CASES is there for
BATCH_CROSSES = {
    "1089-batch5-fused-group-split-team-on-waiting-475": dict(fuse2_rows=3300, waiting=475),
    "1105-batch5-tail17-fused-group-split-team-on": dict(fuse2_rows=3300, waiting=475, tail_split=0, update_kernel="half-NT"),
    "1089-batch6-fused-group-split-team-off-waiting-570": dict(fuse2_rows=2750, waiting=570),
    "1105-batch6-tail17-fused-group-split-team-off": dict(fuse2_rows=2750, waiting=570, tail_split=0, update_kernel="half-NT"),
    "1105-batch7-fused-group-split-team-off-tail17": dict(fuse2_rows=2357, waiting=665, tail_split=0, update_kernel="half-NT"),
    "1089-batch17-fuse2-rows-970-below-N-single-panels": dict(fuse2_rows=970, tail_split=1),
    "1105-batch17-tail17-single-panels": dict(fuse2_rows=970, tail_split=0, slice=(1024, 1088, 34), update_kernel="half-NT"),
    "577-batch65-two-panels-small-slice": dict(fuse2_rows=253, slice=(512, 576, 130)),
    "593-batch65-tail17-half-tile-update": dict(tail_split=0, slice=(512, 576, 130), update_kernel="half-NT"),
    "257-batch65-small-slice-325-tiles-no-tail": dict(slice=(128, 256, 325)),
    "321-batch130-one-panel": dict(fuse2_rows=126),
    "337-batch130-tail17-half-tile-update": dict(fuse2_rows=126, tail_split=0, update_kernel="half-NT"),
    "272-batch130-gemm-slice-650-tiles-tail16-gmax1": dict(slice=(128, 256, 650), tail_grid=(2, 1), tail_split=1),
    "129-batch257-one-panel": dict(fuse2_rows=64),
    "257-batch257-gemm-slice-tail1-gmax1-from-256-on": dict(slice=(128, 256, 1285), tail_grid=(2, 1), tail_split=1),
    "145-batch257-tail17-whole-tile-update": dict(tail_split=0, update_kernel="whole-NT"),
}


def padded_ld(cols):
    return max(16, (cols + 15) // 16 * 16)   # hip.alloc_matrix


def potrf_lda(case):
    return case.N + (1 - case.N % 2) if case.odd_lda else padded_ld(case.N)


def potrf_problems():
    """Every (n, seed, diag, in_block, nf) the factorisation tests generate."""
    return sorted({(c.N, SEED0 + b, c.diag, c.in_block, c.nf) for c in POTRF_CASES + [LONE_TWIN] if c not in BATCH_CASES for b in range(c.batch)})


def batch_case_problems(case):
    """The same for a case of BATCH_CASES (tests/test_exact_cases.py checks their members case by case, not one test per member)."""
    return [(case.N, SEED0 + b, case.diag, case.in_block, case.nf) for b in range(case.batch)]


@functools.lru_cache(maxsize=4)
def factor_problem(n, seed, diag=DIAG, in_block=IN_BLOCK):
    L = exact.exact_factor(n, seed, diag, in_block)
    return L, exact.exact_spd(L)


# ---- GEMM ----------------------------------------------------------------------------------------------------------
ALPHA_BETA = [(1.0, 0.0), (-1.0, 1.0), (1.0, 1.0), (0.5, -2.0)]
GemmCase = collections.namedtuple("GemmCase", "id ta tb m n k pad_a pad_b pad_c c_lower a_lower k_from_row k_to_col batch")


def _gc(id, tr, m, n, k, pad=(True, True, True), c_lower=False, a_lower=False, k_from_row=False, k_to_col=False, batch=1):
    return GemmCase(id, tr[0] == "T", tr[1] == "T", m, n, k, pad[0], pad[1], pad[2], c_lower, a_lower, k_from_row, k_to_col, batch)


_UNPADDED = (False, False, False)
GEMM_CASES = [
    _gc("whole-nn-289-tiles-k64", "NN", 2176, 2176, 64),
    _gc("whole-nt-289-tiles-k64", "NT", 2176, 2176, 64),
    _gc("whole-nn-batch65-k80-odd-stage-count", "NN", 256, 256, 80, batch=65),
    _gc("whole-nt-batch65-k80-odd-stage-count", "NT", 256, 256, 80, batch=65),
    _gc("half-nt-384-preload", "NT", 384, 384, 64),
    _gc("half-nn-384-preload", "NN", 384, 384, 64),
    _gc("whole-nt-lower-2944-preload-off-diagonal-only", "NT", 2944, 2944, 64, c_lower=True),
    _gc("half-nt-129-fast-clamped", "NT", 129, 129, 64),
    _gc("whole-nt-333x257-k32-fast-clamped", "NT", 333, 257, 32),
    _gc("general-nn-k33", "NN", 130, 257, 33),
    _gc("general-nt-k33", "NT", 130, 257, 33),
    _gc("general-tn-k33", "TN", 130, 257, 33),
    _gc("general-tt-k33", "TT", 130, 257, 33),
    _gc("general-nn-odd-ld", "NN", 130, 257, 33, pad=_UNPADDED),
    _gc("general-nt-odd-ld", "NT", 130, 257, 33, pad=_UNPADDED),
    _gc("general-tn-odd-ld", "TN", 131, 257, 33, pad=_UNPADDED),
    _gc("general-tt-odd-ld", "TT", 131, 257, 33, pad=_UNPADDED),
    _gc("half-nn-interior-plain-epilogue-odd-ldc", "NN", 256, 257, 64, pad=(True, True, False)),
    _gc("whole-nn-k-to-col-column-grouping", "NN", 4224, 1024, 1024, k_to_col=True),
    _gc("whole-nn-k-to-col-round-robin", "NN", 4224, 1152, 1152, k_to_col=True),
    _gc("half-nn-k-to-col", "NN", 384, 384, 384, k_to_col=True),
    _gc("half-nt-k-from-row-lower", "NT", 384, 384, 384, k_from_row=True, c_lower=True),
    _gc("whole-nt-k-from-row-lower", "NT", 2944, 2944, 2944, k_from_row=True, c_lower=True),
    _gc("half-nt-k-from-row", "NT", 384, 384, 384, k_from_row=True),
    _gc("whole-nt-k-from-row", "NT", 2944, 1536, 2944, k_from_row=True),
    _gc("half-nn-a-lower", "NN", 384, 384, 384, a_lower=True),
    _gc("whole-nn-a-lower", "NN", 2944, 1536, 2944, a_lower=True),
    _gc("splitk-nn-257x130", "NN", 257, 130, 20000),
    _gc("splitk-tn-257x130", "TN", 257, 130, 20000),
    _gc("splitk-nt-1025", "NT", 1025, 1025, 16411),
    _gc("splitk-nt-1025-lower", "NT", 1025, 1025, 16411, c_lower=True),
]
GEMM_BY_ID = {c.id: c for c in GEMM_CASES}


def _ld(rows, cols, pad):
    return padded_ld(cols) if pad else cols


def splitk_splits(c):
    """gpar_amd/hip.py: gemm - the split-K rule (0: the plain launch)."""
    tm, tn = -(-c.m // 128), -(-c.n // 128)
    t = min(tm, tn)
    tiles = t * (t + 1) // 2 + (tm - t) * t if c.c_lower else tm * tn
    if c.batch == 1 and not (c.a_lower or c.k_from_row or c.k_to_col) and c.k >= 8192 and tiles <= 128:
        return max(2, min(64, 512 // max(tiles, 1), c.k // 1024))
    return 0


def gemm_paths(c, alpha, beta, role=0, splits=None, fast=None):
    """The paths one launch takes, tile by tile: a restatement of the predicates of gemm_launch / gemm_splitk_launch
    (gpar_amd/csrc/gemm_f64.h:549-614, 631-669) and gemm_tile_body (:355-507) with the default switches (half tiles up to 256 tiles,
    triangular-aware launches included, MIXED last round on, PRELOAD on).  Returns the set of (kernel, tile map, main loop, epilogue):

        kernel     whole-XY / half-XY / mixed-tail-XY (XY: NN, NT, TN, TT), with a `splitk-` prefix for a slab launch     (:591-611)
        tile map   xcd-contiguous / round-robin / k-to-col-columns, `+lower` for the lower-trapezoid enumeration           (:367-405)
        main loop  preload+ / preload- (the sign of alpha) / fast-inner / fast-clamped / general / empty                   (:431-440)
        epilogue   lds-beta / lds-nobeta / interior-plain / edge                                                           (:450-507)

    `fast`: (fastA, fastB, fastC) - 16-byte aligned with an even leading dimension (:566-568); by default from the case's padding."""
    BMW, BN, BK = 128, 128, 16
    flagged = c.a_lower or c.k_from_row or c.k_to_col
    tiles_m, tiles_n = -(-c.m // BMW), -(-c.n // BN)
    if c.c_lower and tiles_n > tiles_m:
        tiles_n = tiles_m                                                                        # :562-565
    if fast is None:
        am, ak = (c.k, c.m) if c.ta else (c.m, c.k)
        bm, bk = (c.n, c.k) if c.tb else (c.k, c.n)
        fast = tuple(_ld(r, cc, p) % 2 == 0 for r, cc, p in ((am, ak, c.pad_a), (bm, bk, c.pad_b), (c.m, c.n, c.pad_c)))
    fastA, fastB, fastC = fast
    if c.c_lower:                                                                                # gemm_num_tiles :540-546
        order = [(tm, tn) for tm in range(tiles_m) for tn in range(min(tm + 1, tiles_n))]
    else:
        order = [(tm, tn) for tm in range(tiles_m) for tn in range(tiles_n)]
    ntiles = len(order)
    splits = splitk_splits(c) if splits is None else splits
    ksplit, nslabs = 0, 1
    if splits > 1:                                                                               # gemm_splitk_launch :636-660
        ksplit = -(-(-(-c.k // splits)) // BK) * BK
        nslabs = -(-c.k // ksplit)
        alpha, beta = 1.0, 0.0
        fastC = c.n % 2 == 0 and (c.m * c.n) % 2 == 0
        half, nfull = False, ntiles
    else:
        half = (not c.ta) and ntiles * c.batch <= 256 and c.k >= 64                              # :591-592
        nfull = ntiles
        if (not half and role == 1 and not c.ta and c.tb and c.batch == 1 and c.k >= 64 and ntiles > 512 and ntiles % 512 != 0
                and ntiles % 512 <= 256 and not flagged):                                        # :598-602
            nfull = ntiles - ntiles % 512
    tr = ("T" if c.ta else "N") + ("T" if c.tb else "N")
    out = set()
    for idx, (tm, tn) in enumerate(order):
        mixed = idx >= nfull
        BM = 64 if (half or mixed) else 128
        kernel = ("splitk-" if ksplit else "") + ("half-" if half else "mixed-tail-" if mixed else "whole-") + tr
        tri_rect = not c.c_lower and BM == BMW                                                   # :368
        if tri_rect and c.k_to_col and not (c.k_from_row or c.a_lower) and tiles_n % 8 == 0:     # :369
            tmap = "k-to-col-columns"
        elif flagged:                                                                            # :376
            tmap = "round-robin"
        else:
            tmap = "xcd-contiguous"
        if c.c_lower:
            tmap += "+lower"                                                                     # :389
        for hblk in range(BMW // BM):
            m0, n0 = tm * BMW + hblk * BM, tn * BN                                               # :406
            for slab in range(nslabs):
                kend = min(c.k, m0 + BM) if c.a_lower else c.k                                   # :412
                if c.k_to_col:
                    kend = min(kend, n0 + BN)                                                    # :413
                kbeg = min(m0, kend) if c.k_from_row else 0                                      # :416
                if ksplit:                                                                       # :417-422
                    kbeg, kend = max(kbeg, slab * ksplit), min(kend, (slab + 1) * ksplit)
                    kend = max(kend, kbeg)
                nk = -(-(kend - kbeg) // BK)
                fastk = fastA and fastB and not c.a_lower and (kend - kbeg) % BK == 0             # :431
                inner = m0 + BM <= c.m and n0 + BN <= c.n                                        # :432
                below = not c.c_lower or n0 + BN - 1 <= m0
                preload = fastk and inner and nk > 0 and not ksplit and beta == 1.0 and alpha in (1.0, -1.0) and below   # :435-436
                if nk <= 0:
                    loop = "empty"
                elif preload:
                    loop = "preload+" if alpha > 0 else "preload-"
                elif fastk and inner:
                    loop = "fast-inner"
                elif fastk and not c.ta and c.tb:
                    loop = "fast-clamped"                                                        # :439
                else:
                    loop = "general"
                beta_eff = 0.0 if preload else beta                                              # :450
                interior = inner and below                                                       # :454
                if interior and fastC:
                    epi = "lds-beta" if beta_eff != 0.0 else "lds-nobeta"
                elif interior:
                    epi = "interior-plain"
                else:
                    epi = "edge"
                out.add((kernel, tmap, loop, epi))
    return out


def gemm_case_paths(c):
    """Union over the (alpha, beta) pairs the product test runs."""
    out = set()
    for alpha, beta in ALPHA_BETA:
        out |= gemm_paths(c, alpha, beta)
    return out


@functools.lru_cache(maxsize=2)
def gemm_problem(case_id):
    """(A, B, C, op(A) op(B)) of a case as stored, integer-valued; triangular operands hold stored zeros where K_FROM_ROW /
    K_TO_COL skip, NaN where A_LOWER promises not to read."""
    c = GEMM_BY_ID[case_id]
    seed = 7000 + GEMM_CASES.index(c)
    As, Bs, Cs, Ps = [], [], [], []
    for b in range(c.batch):
        A = exact.exact_operands((c.k, c.m) if c.ta else (c.m, c.k), seed * 1000 + 3 * b)
        B = exact.exact_operands((c.n, c.k) if c.tb else (c.k, c.n), seed * 1000 + 3 * b + 1)
        C = exact.exact_operands((c.m, c.n), seed * 1000 + 3 * b + 2)
        if c.k_from_row:
            A = np.triu(A)                  # op(A) upper triangular, stored zeros
            if c.c_lower:
                B = np.triu(B)              # (tb: B is stored n x k; op(B)^T upper triangular as well - U1 U2^T, lower part)
        if c.k_to_col:
            B = np.triu(B)                  # op(B) = B upper triangular, stored zeros below
        opA, opB = (A.T if c.ta else A), (B.T if c.tb else B)
        if c.a_lower:
            opA = np.tril(A)
            A = opA + np.triu(np.full(A.shape, np.nan), 1)
        As.append(A), Bs.append(B), Cs.append(C), Ps.append(exact.exact_product(opA, opB))
    return np.concatenate(As), np.concatenate(Bs), np.concatenate(Cs), np.concatenate(Ps)


# ---- triangular solves: (n, rows) of test_trsm / test_trsm_forward_with_paired_blocks that cross the path boundaries ----------------
TRSM_CASES = [(50, 3), (64, 64), (333, 130), (513, 1), (1024, 300), (1100, 64), (2100, 700), (5000, 130)]
TRSM_SEED = 300


@functools.lru_cache(maxsize=2)
def trsm_problem(n, rows):
    L = exact.exact_factor(n, TRSM_SEED + n)
    X = exact.exact_operands((rows, n), TRSM_SEED + n + rows)
    return L, X, exact.exact_product(X, L.T), exact.exact_product(X, L)


# =====================================================================================================================
@pytest.fixture(scope="module")
def env():
    import torch

    from gpar_amd import hip

    assert torch.cuda.is_available()
    return torch, hip, torch.device("cuda:0")


def _device_matrix(torch, hip, dev, host, pad=True, odd=False):
    rows, cols = host.shape
    if odd:
        buf = torch.empty((rows, cols + (1 - cols % 2)), dtype=torch.float64, device=dev)
        out = buf[:, :cols]
    elif pad:
        out = hip.alloc_matrix(rows, cols, dev)
    else:
        out = torch.empty((rows, cols), dtype=torch.float64, device=dev)
    out.copy_(torch.from_numpy(np.ascontiguousarray(host)))
    return out


def _first_difference(got, want):
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if len(bad) == 0:
        return None
    r, c = bad[0]
    return "%d entries differ, the first at (row %d, column %d): got %r, want %r, largest |difference| %g" % (
        len(bad), r, c, got[r, c], want[r, c], np.nanmax(np.abs(got - want)[tuple(bad.T)]))


def _run_potrf(env, monkeypatch, case, lookahead, zero=None):
    """Factor the case's batch; returns (per-member matrices after the call, logdet list, info list)."""
    torch, hip, dev = env
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    if case.batch > 1:
        monkeypatch.setenv("GPAR_POTRF_BATCH_LOOKAHEAD", "1" if lookahead else "0")
    N = case.N
    host = []
    for b in range(case.batch):
        L, A = factor_problem(N, SEED0 + b, case.diag, case.in_block)
        A = np.tril(A) + np.triu(np.full((N, N), np.nan), 1)
        if zero is not None and zero[0] == b:
            A[zero[1], zero[1]] -= L[zero[1], zero[1]] ** 2
        host.append(A)
    dA = _device_matrix(torch, hip, dev, np.concatenate(host), odd=case.odd_lda)
    assert int(dA.stride(0)) == potrf_lda(case)
    if case.batch == 1:
        logdet, info = hip.potrf_(dA, case.nf, lookahead=lookahead, fused=not (case.flags & UNFUSED))
    else:
        logdet, info = hip.potrf_batch_(dA, case.batch, case.nf, fused=not (case.flags & UNFUSED))
    torch.cuda.synchronize()
    return dA.cpu().numpy().reshape(case.batch, N, N), logdet.cpu().tolist(), info.cpu().tolist()


def _check_member(case, b, got):
    """Factor, solved rows and Schur complement of member b, to the bit; the strict upper triangle untouched outside the panel
    kernels' scratch words (the mask of tests/test_augmented_tail_gpu.py)."""
    N, nf = case.N, case.nf
    L, _ = factor_problem(N, SEED0 + b, case.diag, case.in_block)
    iu = np.triu_indices(N, 1)
    scratch = (iu[0] // 64 == iu[1] // 64) & (iu[1] // 64 < N // 64) & (iu[0] < nf)
    assert np.all(np.isnan(got[iu[0][~scratch], iu[1][~scratch]])), "the strict upper triangle was written (or read: NaN below)"
    want = np.tril(L[:, :nf].copy())
    have = got[:, :nf].copy()
    have[:nf] = np.tril(have[:nf])
    diff = _first_difference(have, want)
    assert diff is None, "factor / solved rows of member %d: %s" % (b, diff)
    if N > nf:
        S = exact.exact_product(L[nf:, nf:], L[nf:, nf:].T)
        diff = _first_difference(np.tril(got[nf:, nf:]), np.tril(S))
        assert diff is None, "Schur complement of member %d: %s" % (b, diff)


@pytest.mark.gpu
@pytest.mark.parametrize("lookahead", [True, False], ids=["la-on", "la-off"])
@pytest.mark.parametrize("case", POTRF_CASES, ids=[c.id for c in POTRF_CASES])
def test_factorisation_is_exact_on_exact_inputs(env, monkeypatch, case, lookahead):
    """tril(got[:nf, :nf]) == L, got[nf:, :nf] == L[nf:, :nf], the lower triangle of got[nf:, nf:] == L22 L22^T, info == 0, the
    NaN-filled strict upper triangle still NaN; logdet == 2 sum log diag L at rtol 1e-12 (its atomicAdd order is not fixed).
    The cases of BATCH_CASES - batches of 5 .. 257 - each cross one batch-dependent predicate, named in the id and held in
    BATCH_CROSSES: fuse2_rows = 16500 / batch against N, the fused launch's waiting workgroups against 512 (split team on / off), the
    slice's tiles over the batch against 512 (small tile kernel / GEMM), potrf_tail_update's grid clamp 256 / batch (1 from batch 129
    on, a branch of its own from 256 on), tail_split, the GEMM's half-tile rule ntiles * batch <= 256.  Every batch count has a case with
    17 rows below the factored part (tail_split off; those rows through the GEMM: a half tile per matrix up to batch 256, whole at 257),
    batch 130 one with 16 (the tail companion in launches of 4 rows)."""
    got, logdet, info = _run_potrf(env, monkeypatch, case, lookahead)
    assert info == [0] * case.batch
    for b in range(case.batch):
        _check_member(case, b, got[b])
        L, _ = factor_problem(case.N, SEED0 + b, case.diag, case.in_block)
        assert np.isclose(logdet[b], 2 * np.sum(np.log(np.diag(L)[:case.nf])), rtol=1e-12, atol=0.0)


@pytest.mark.gpu
def test_a_batch_member_and_the_same_matrix_alone_agree_to_the_bit(env, monkeypatch):
    """Both are exact, so - unlike on rounded inputs, where the two schedules sum in different orders - they must be equal."""
    lone, batch = LONE_TWIN, POTRF_BY_ID["1601-batch3-fused-group-lockstep"]
    assert (lone.N, lone.nf) == (batch.N, batch.nf)
    a, _, ia = _run_potrf(env, monkeypatch, lone, True)
    b, _, ib = _run_potrf(env, monkeypatch, batch, True)
    assert ia == [0] and ib == [0, 0, 0]
    assert np.array_equal(np.tril(a[0]), np.tril(b[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("case_id,member,j,what", ZERO_PIVOT_CASES, ids=[z[3].replace(" ", "-") for z in ZERO_PIVOT_CASES])
def test_an_exactly_zero_pivot_is_reported_at_its_column(env, monkeypatch, case_id, member, j, what):
    """A[j, j] -= L[j, j]^2 makes pivot j exactly 0.0: info == j + 1 for that matrix; the other members of a batch still exact."""
    case = POTRF_BY_ID[case_id]
    got, _, info = _run_potrf(env, monkeypatch, case, True, zero=(member, j))
    assert info[member] == j + 1
    for b in range(case.batch):
        if b != member:
            assert info[b] == 0
            _check_member(case, b, got[b])


@pytest.mark.gpu
@pytest.mark.parametrize("case", GEMM_CASES, ids=[c.id for c in GEMM_CASES])
def test_products_of_integer_operands_are_exact(env, case):
    """C <- alpha op(A) op(B) + beta C for every (alpha, beta) of ALPHA_BETA, to the bit.  beta == 0: C is NaN-filled (never read);
    c_lower: the strict upper triangle of C is NaN and keeps its bits."""
    torch, hip, dev = env
    c = case
    A, B, C, P = gemm_problem(c.id)
    dA, dB = _device_matrix(torch, hip, dev, A, c.pad_a), _device_matrix(torch, hip, dev, B, c.pad_b)
    upper = np.triu(np.ones((c.m, c.n), dtype=bool), 1)
    upper = np.concatenate([upper] * c.batch)
    flags = dict(c_lower=c.c_lower, a_lower=c.a_lower, k_from_row=c.k_from_row, k_to_col=c.k_to_col)
    for alpha, beta in ALPHA_BETA:
        start = np.full(C.shape, np.nan) if beta == 0.0 else C.copy()
        if c.c_lower:
            start[upper] = np.nan
        want = alpha * P + (beta * C if beta != 0.0 else 0.0)
        if c.c_lower:
            want[upper] = np.nan
        dC = _device_matrix(torch, hip, dev, start, c.pad_c)
        if c.batch > 1:
            hip.gemm_batch_(dA, dB, dC, c.batch, ta=c.ta, tb=c.tb, alpha=alpha, beta=beta, c_lower=c.c_lower)
        else:
            hip.gemm(dA, dB, ta=c.ta, tb=c.tb, alpha=alpha, beta=beta, out=dC, **flags)
        got = dC.cpu().numpy()
        diff = _first_difference(got, want)
        assert diff is None, "alpha %g beta %g: %s" % (alpha, beta, diff)
        if c.c_lower:   # the NaNs above the diagonal bit for bit
            assert np.array_equal(got.view(np.uint64)[upper], start.view(np.uint64)[upper])


@pytest.mark.gpu
@pytest.mark.parametrize("n,rows", TRSM_CASES)
def test_triangular_solves_return_the_integer_solution(env, n, rows):
    """B = X L^T (X L) for an integer X: gpar_trsm_rlt (gpar_trsm_rln) returns X bit for bit; the strict upper triangle of L is NaN."""
    torch, hip, dev = env
    L, X, Bf, Bb = trsm_problem(n, rows)
    dL = _device_matrix(torch, hip, dev, L + np.triu(np.full((n, n), np.nan), 1))
    got = hip.trsm_rlt_(dL, _device_matrix(torch, hip, dev, Bf)).cpu().numpy()
    diff = _first_difference(got, X)
    assert diff is None, "forward: " + diff
    got = hip.trsm_rln_(dL, _device_matrix(torch, hip, dev, Bb)).cpu().numpy()
    diff = _first_difference(got, X)
    assert diff is None, "backward: " + diff
