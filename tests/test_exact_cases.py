"""Before any GPU is involved: the premises of the exact-arithmetic tests (tests/test_exact_arithmetic_gpu.py) hold on the CPU, and
their case lists reach what their ids claim - the factorisation cases through the schedule printer (tools/potrf_schedule.cpp), the
product cases through the restatement of the GEMM launch predicates (gemm_paths).  Removing a case from either list fails a test here."""
import numpy as np
import pytest

from oracle import exact
from tests import test_exact_arithmetic_gpu as gpu
from tests.test_potrf_schedule import _parse, _run, printer  # noqa: F401 - the printer, built as that module builds it


# ---- premises ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed,diag,in_block,nf", gpu.potrf_problems())
def test_cholesky_of_an_exact_matrix_is_exact_on_the_cpu(n, seed, diag, in_block, nf):
    """numpy's factor equals L bit for bit; so does a blocked right-looking restatement that multiplies by explicit inverses of the
    64 x 64 diagonal blocks, composed [Wa 0; -Wb Lba Wa, Wb] from 8 x 8 substitutions as p2_inverse_sub / p2_inverse_couple compose
    theirs; Dinv D == I exactly for every block; the partial factorisation (nf columns) leaves L[nf:, :nf] and L22 L22^T."""
    L, A = gpu.factor_problem(n, seed, diag, in_block)
    assert np.array_equal(A, np.rint(A)) and np.abs(A).max() < 2.0 ** 53
    assert np.array_equal(np.linalg.cholesky(A), L)
    R, pairs = exact.blocked_cholesky(A, nf)
    for D, Dinv in pairs:
        assert np.array_equal(Dinv @ D, np.eye(len(D)))
        assert np.abs(Dinv).max() <= 16.0
    assert np.array_equal(R[:, :nf], L[:, :nf])
    assert np.array_equal(R[nf:, nf:], np.tril(L[nf:, nf:] @ L[nf:, nf:].T))


@pytest.mark.parametrize("case", gpu.BATCH_CASES, ids=[c.id for c in gpu.BATCH_CASES])
def test_every_member_of_a_wide_batch_is_exact_on_the_cpu(case):
    """The premises above for ALL members of the batch-count cases (up to 257 seeds of small matrices: one test per case, not per
    member), and no two members of a batch hold the same matrix."""
    seen = set()
    for n, seed, diag, in_block, nf in gpu.batch_case_problems(case):
        L, A = gpu.factor_problem(n, seed, diag, in_block)
        assert np.array_equal(A, np.rint(A)) and np.abs(A).max() < 2.0 ** 53
        assert np.array_equal(np.linalg.cholesky(A), L)
        R, pairs = exact.blocked_cholesky(A, nf)
        for D, Dinv in pairs:
            assert np.array_equal(Dinv @ D, np.eye(len(D))) and np.abs(Dinv).max() <= 16.0
        assert np.array_equal(R[:, :nf], L[:, :nf])
        assert np.array_equal(R[nf:, nf:], np.tril(L[nf:, nf:] @ L[nf:, nf:].T))
        seen.add(A.tobytes())
    assert len(seen) == case.batch


def test_the_refinement_case_has_blocks_above_the_refinement_ratio():
    case = gpu.POTRF_BY_ID["1601-lone-refinement-pivots-1-and-64"]
    d = np.diag(gpu.factor_problem(case.N, gpu.SEED0, case.diag, case.in_block)[0])[:case.nf].reshape(-1, 16)
    assert np.all(d.max(axis=1) > 32.0 * d.min(axis=1))   # P2_REFINE_RATIO (csrc/panel2.h), in every 16 x 16 diagonal block
    others = np.diag(gpu.factor_problem(1601, gpu.SEED0)[0])
    assert others.max() <= 32.0 * others.min()            # and in no block of the other cases


@pytest.mark.parametrize("n,rows", gpu.TRSM_CASES)
@pytest.mark.parametrize("block", [16, 64])
def test_triangular_solves_of_exact_systems_are_exact_on_the_cpu(n, rows, block):
    """The only blocks the solves invert are the 16 x 16 diagonal blocks of a 64 x 64 tile (p2_inverse_blocks / p2_strip in
    csrc/panel2.h: trsm_block2_kernel and its backward twin; the leaf strips of csrc/potrf.h substitute with reciprocal pivots);
    everything wider - the 512-column blocks, their groups of four from n = 5120 on (trsm_rlt_run2) - is products.  A restatement
    through the explicit inverse of every 16-wide block, and of every 64-wide one (coarser than anything the kernels form), is exact."""
    L, X, Bf, Bb = gpu.trsm_problem(n, rows)
    assert np.array_equal(exact.blocked_solve(L, Bf, forward=True, block=block), X)
    assert np.array_equal(exact.blocked_solve(L, Bb, forward=False, block=block), X)


# ---- the factorisation cases reach the schedule forms they name ---------------------------------------------------------
def _schedule(exe, case, lookahead):
    flags = case.flags | (0 if lookahead or case.batch > 1 else gpu.NO_LOOKAHEAD)
    env = dict(case.env)
    if case.batch > 1:
        env["GPAR_POTRF_BATCH_LOOKAHEAD"] = "1" if lookahead else "0"
    (shape, policy, steps), = _parse(_run(exe, [(case.N, case.nf, gpu.potrf_lda(case), case.batch, flags)], **env))
    return shape, policy, steps


def _features(shape, policy, steps):
    """What a schedule consists of, as tokens: lock-step or not, the panel forms, update forms, slice kinds, tail-split pieces."""
    mode = "lockstep" if policy["lockstep"] else "lone"
    out = {(mode, "lookahead=%d" % policy["lookahead"]), (mode, "tail_split=%d" % policy["tail_split"]), (mode, "fused=%d" % policy["fused"])}
    for k0, kend, form, G, update, s0, s1, kind, stail, r0, r1, rtail in steps:
        out.add((mode, "panel", form))
        out.add((mode, "update", update))
        if kind:
            out.add((mode, "slice", kind + (stail or "")))
        if r0 is not None:
            out.add((mode, "rest", "rest" + (rtail or "")))
        if form == "fused-group":
            out.add((mode, "fused-group G=%s" % G))
        if form in ("fused", "leaf") and (int(kend) - int(k0)) % 64 != 0:
            out.add((mode, "ragged", form))
    return out


# what each case is there for (a case that is removed from POTRF_CASES, or no longer reaches its form, fails the test below)
POTRF_REACHES = {
    "2113-lone-fused-group4-small-slice": {("lone", "fused-group G=4"), ("lone", "slice", "small")},
    "2113-lone-grouped": {("lone", "panel", "grouped")},
    "2113-batch3-grouped-lockstep": {("lockstep", "panel", "grouped"), ("lockstep", "tail_split=1")},
    "2064-batch3-grouped-tail16-on-slice-and-rest": {("lockstep", "panel", "grouped"), ("lockstep", "slice", "gemm+tail"), ("lockstep", "rest", "rest+tail")},
    "1601-batch3-fused-group-lockstep": {("lockstep", "panel", "fused-group")},
    "1601-batch3-single-fused-panels": {("lockstep", "panel", "fused"), ("lockstep", "slice", "small")},
    "1552-batch3-tail16-on-rest": {("lockstep", "rest", "rest+tail"), ("lockstep", "slice", "small")},
    "1553-batch3-tail17-stays-in-the-tiles": {("lockstep", "tail_split=0"), ("lockstep", "rest", "rest")},
    "1537-batch3-tail1-on-gemm-slice": {("lockstep", "slice", "gemm+tail")},
    "1100-batch3-leaf-batch-ragged": {("lockstep", "panel", "leaf-batch")},
    "1100-lone-odd-lda-leaf": {("lone", "panel", "leaf"), ("lone", "ragged", "leaf"), ("lone", "fused=1")},
    "1100-lone-unfused": {("lone", "fused=0"), ("lone", "panel", "leaf")},
    "2661-lone-gemm-slices-ragged-tail-panels": {("lone", "lookahead=1"), ("lone", "slice", "gemm"), ("lone", "panel", "fused"), ("lone", "ragged", "leaf")},
    "5121-lone-mixed-last-round": {("lone", "lookahead=1"), ("lone", "update", "slice+rest")},
    "1024-lone-no-update": {("lone", "update", "none")},
    "1601-lone-refinement-pivots-1-and-64": {("lone", "panel", "fused-group")},
    # the batch-count cases (their predicates: test_batch_count_cases_cross_the_predicates_they_name)
    "1089-batch5-fused-group-split-team-on-waiting-475": {("lockstep", "fused-group G=2"), ("lockstep", "slice", "small")},
    "1105-batch5-tail17-fused-group-split-team-on": {("lockstep", "fused-group G=2"), ("lockstep", "tail_split=0"), ("lockstep", "update", "one")},
    "1089-batch6-fused-group-split-team-off-waiting-570": {("lockstep", "fused-group G=2")},
    "1105-batch6-tail17-fused-group-split-team-off": {("lockstep", "fused-group G=2"), ("lockstep", "tail_split=0")},
    "1105-batch7-fused-group-split-team-off-tail17": {("lockstep", "fused-group G=2"), ("lockstep", "tail_split=0")},
    "1089-batch17-fuse2-rows-970-below-N-single-panels": {("lockstep", "panel", "fused"), ("lockstep", "slice", "gemm"), ("lockstep", "slice", "small")},
    "1105-batch17-tail17-single-panels": {("lockstep", "panel", "fused"), ("lockstep", "slice", "gemm"), ("lockstep", "slice", "small"), ("lockstep", "tail_split=0")},
    "577-batch65-two-panels-small-slice": {("lockstep", "panel", "fused"), ("lockstep", "slice", "small")},
    "593-batch65-tail17-half-tile-update": {("lockstep", "panel", "fused"), ("lockstep", "slice", "small"), ("lockstep", "tail_split=0")},
    "257-batch65-small-slice-325-tiles-no-tail": {("lockstep", "slice", "small"), ("lockstep", "tail_split=1")},
    "321-batch130-one-panel": {("lockstep", "panel", "fused"), ("lockstep", "update", "one")},
    "337-batch130-tail17-half-tile-update": {("lockstep", "panel", "fused"), ("lockstep", "update", "one"), ("lockstep", "tail_split=0")},
    "272-batch130-gemm-slice-650-tiles-tail16-gmax1": {("lockstep", "slice", "gemm+tail")},
    "129-batch257-one-panel": {("lockstep", "panel", "fused"), ("lockstep", "update", "one")},
    "257-batch257-gemm-slice-tail1-gmax1-from-256-on": {("lockstep", "slice", "gemm+tail")},
    "145-batch257-tail17-whole-tile-update": {("lockstep", "tail_split=0"), ("lockstep", "update", "one")},
}


def test_factorisation_cases_reach_the_forms_they_name(printer):  # noqa: F811
    assert [c.id for c in gpu.POTRF_CASES] == list(POTRF_REACHES)
    union, lookaheads = set(), set()
    for case in gpu.POTRF_CASES:
        on, off = _schedule(printer, case, True), _schedule(printer, case, False)
        assert on[2] == off[2]   # the steps do not depend on the look-ahead setting
        assert (on[0]["N"], on[0]["nf"], on[0]["lda"], on[0]["batch"]) == (case.N, case.nf, gpu.potrf_lda(case), case.batch)   # (lock-step where a batch)
        lookaheads |= {on[1]["lookahead"], off[1]["lookahead"]}
        feats = _features(*on)
        assert POTRF_REACHES[case.id] <= feats, (case.id, POTRF_REACHES[case.id] - feats)
        union |= {f[1:] for f in feats}
    assert lookaheads == {0, 1}
    for form in ("grouped", "fused-group", "fused", "leaf-batch", "leaf"):
        assert ("panel", form) in union
    for update in ("none", "one", "slice+rest"):
        assert ("update", update) in union
    for piece in (("slice", "gemm"), ("slice", "small"), ("slice", "gemm+tail"), ("rest", "rest+tail")):
        assert piece in union
    # the tails of the lock-step cases: 1, 16 and 17 rows (and the 62 appended rows of the ragged case)
    assert {c.N - c.nf for c in gpu.POTRF_CASES if c.batch > 1} == {1, 16, 17, 62}


def test_batch_count_cases_cross_the_predicates_they_name(printer):  # noqa: F811
    """Every case of BATCH_CASES sits on the side of the batch-dependent predicate its id names - fuse2_rows = 16500 / batch against N
    (potrf_policy), the waiting workgroups of a fused launch against 512 (potrf_group_fused), the tiles of a slice over the whole batch
    against GPAR_POTRF_LA_SMALL_TILES = 512 (potrf_slice_small), the grid clamp 256 / batch of potrf_tail_update (1 from batch 129 on,
    and by the branch of its own from 256 on), tail_split (batches only, 1 .. 16 rows), the half-tile rule ntiles * batch <= 256 of the
    update's GEMM - and a neighbour in the list sits on the other side.  The schedules are printed (pytest -s).
    The forms, fuse2_rows, tail_split and small / gemm are READ from the printer; the waiting count and the tail companion's grid are
    restatements (gpu.group_waiting, gpu.tail_grid) of host code the printer does not show, checked against the figures in BATCH_CROSSES."""
    assert [c.id for c in gpu.BATCH_CASES] == list(gpu.BATCH_CROSSES)
    assert {c.batch for c in gpu.BATCH_CASES} == {5, 6, 7, 17, 65, 130, 257}
    seen = {}
    for case in gpu.BATCH_CASES:
        shape, policy, steps = _schedule(printer, case, True)
        print(case.id, policy, *[" ".join(str(f) for f in s if f is not None) for s in steps], sep="\n    ")
        want = gpu.BATCH_CROSSES[case.id]
        assert shape["batch"] == case.batch and policy["lockstep"] == 1
        nbo = int(dict(case.env).get("GPAR_POTRF_NBO", 512))
        assert policy["nbo"] == nbo and policy["fuse2_rows"] == 16500 // case.batch
        forms = {s[2] for s in steps}
        # fuse2_rows against N: a fused launch of several panels exactly where the matrix has at most fuse2_rows rows
        assert ("fused-group" in forms) == (nbo == 512 and case.nf >= 1024 and case.N <= policy["fuse2_rows"]), case.id
        if "fuse2_rows" in want:
            assert policy["fuse2_rows"] == want["fuse2_rows"]
        if "waiting" in want:
            assert steps[0][2] == "fused-group" and int(steps[0][0]) == 0 and gpu.group_waiting(case) == want["waiting"]
            seen.setdefault("split", set()).add(want["waiting"] > 512)
        if "tail_split" in want:
            assert policy["tail_split"] == want["tail_split"] == int(0 < case.N - case.nf <= 16)
        if "slice" in want:
            kend, next_end, tiles = want["slice"]
            (step,) = [s for s in steps if s[5] is not None and (int(s[5]), int(s[6])) == (kend, next_end)]
            assert gpu.slice_tiles(case, kend, next_end) == tiles and step[7] == ("small" if tiles <= 512 else "gemm"), case.id
            seen.setdefault("slice", set()).add(step[7])
            if "tail_grid" in want:
                assert step[8] == "+tail" and gpu.tail_grid(case.batch, next_end - kend) == want["tail_grid"]
                seen.setdefault("gmax", set()).add("branch" if case.batch >= 256 else "quotient")
        if "update_kernel" in want:   # the 17 rows below the last step: one tile of the GEMM per matrix, a half tile while batch <= 256
            step = steps[-1]
            rows, K = case.N - int(step[1]), int(step[1]) - int(step[0])
            assert step[4] == "one" and rows == 17 and K >= 64   # (not the one-wave kernel, which takes up to 16 rows)
            kernels = {p[0] for p in gpu.gemm_paths(gpu._gc("rest", "NT", rows, rows, K, c_lower=True, batch=case.batch), -1.0, 1.0, role=1,
                                                    fast=(True, True, True))}
            assert kernels == {want["update_kernel"]} == {"half-NT" if case.batch <= 256 else "whole-NT"}, case.id
            seen.setdefault("tail17", {})[case.batch] = want["update_kernel"]
    # every batch count has a case with a 17-row tail (tail_split off, the rows below the last step through the GEMM), one has 16 rows
    assert seen.pop("tail17") == {5: "half-NT", 6: "half-NT", 7: "half-NT", 17: "half-NT", 65: "half-NT", 130: "half-NT", 257: "whole-NT"}
    assert sorted(c.batch for c in gpu.BATCH_CASES if c.N - c.nf == 17) == [5, 6, 7, 17, 65, 130, 257]
    assert [c.batch for c in gpu.BATCH_CASES if c.N - c.nf == 16] == [130]
    assert seen == {"split": {False, True}, "slice": {"small", "gemm"}, "gmax": {"branch", "quotient"}}
    # 257 / 256 rows with 128-column steps: the same shape is a small slice without a companion at batch 65 and a GEMM slice with one at 257
    assert {(c.N, c.nf, c.env) for c in gpu.BATCH_CASES if c.id.startswith("257-")} == {(257, 256, (("GPAR_POTRF_NBO", "128"),))}


def test_the_5121_case_ends_its_first_trailing_update_on_a_mixed_round(printer):  # noqa: F811
    """The rest updates of the factorisation are role-1 launches of the GEMM (potrf.h: potrf_rest_update); the first of the 5121-row
    case has 561 lower tiles, 49 of them in a last round that the MIXED rule computes as half tiles."""
    case = gpu.POTRF_BY_ID["5121-lone-mixed-last-round"]
    _, _, steps = _schedule(printer, case, True)
    kernels = set()
    for k0, kend, form, G, update, s0, s1, kind, stail, r0, r1, rtail in steps:
        if r0 is None:
            continue
        rows = (case.nf if rtail else case.N) - int(r0)
        if rows <= 16:
            continue   # (the one-wave kernel)
        launch = gpu._gc("rest", "NT", rows, rows, int(kend) - int(k0), c_lower=True)
        paths = gpu.gemm_paths(launch, -1.0, 1.0, role=1, fast=(True, True, True))
        kernels |= {p[0] for p in paths}
        if int(r0) == 1024:
            assert ("mixed-tail-NT", "xcd-contiguous+lower", "preload-", "lds-nobeta") in paths
            assert ("mixed-tail-NT", "xcd-contiguous+lower", "general", "edge") not in paths
            assert any(p[0] == "mixed-tail-NT" and p[3] == "edge" for p in paths)   # the overhanging last tile row is in the tail
    assert kernels == {"whole-NT", "mixed-tail-NT", "half-NT"}


def test_zero_pivot_columns_sit_where_their_names_say(printer):  # noqa: F811
    where = {}
    for case_id, member, j, what in gpu.ZERO_PIVOT_CASES:
        case = gpu.POTRF_BY_ID[case_id]
        assert member < case.batch and j < case.nf
        _, _, steps = _schedule(printer, case, True)
        (k0, kend, form, G), = [(int(s[0]), int(s[1]), s[2], int(s[3])) for s in steps if int(s[0]) <= j < int(s[1])]
        where[what] = (form, j - k0, kend - k0, G, case.batch)
    assert where["first column of a fused panel"][:2] == ("fused", 0)
    form, off, width, _, _ = where["last column of a fused panel"]
    assert form == "fused" and off == width - 1
    form, off, width, G, _ = where["second panel of a fused-group launch"]
    assert form == "fused-group" and G >= 2 and 512 <= off < 1024
    form, off, width, _, _ = where["ragged leaf panel"]
    assert form == "leaf" and width % 64 != 0
    assert where["one member of a lock-step batch"][4] > 1
    wide = [(case_id, member, j) for case_id, member, j, what in gpu.ZERO_PIVOT_CASES if what.startswith("batch ")]
    for batch in (65, 130):
        members = {member for case_id, member, j in wide if gpu.POTRF_BY_ID[case_id].batch == batch}
        assert {0, 63, 64, batch - 1} <= members
    assert len({j for _, _, j in wide}) >= 5   # (first, last and interior columns)


# ---- the product cases reach the GEMM paths they name -------------------------------------------------------------------
GEMM_REACHES = {
    "whole-nn-289-tiles-k64": {("whole-NN", "xcd-contiguous", "fast-inner", "lds-beta"), ("whole-NN", "xcd-contiguous", "preload-", "lds-nobeta")},
    "whole-nt-289-tiles-k64": {("whole-NT", "xcd-contiguous", "fast-inner", "lds-nobeta"), ("whole-NT", "xcd-contiguous", "preload+", "lds-nobeta")},
    "whole-nn-batch65-k80-odd-stage-count": {("whole-NN", "xcd-contiguous", "fast-inner", "lds-beta")},
    "whole-nt-batch65-k80-odd-stage-count": {("whole-NT", "xcd-contiguous", "fast-inner", "lds-beta")},
    "half-nt-384-preload": {("half-NT", "xcd-contiguous", "preload-", "lds-nobeta"), ("half-NT", "xcd-contiguous", "preload+", "lds-nobeta")},
    "half-nn-384-preload": {("half-NN", "xcd-contiguous", "preload-", "lds-nobeta")},
    "whole-nt-lower-2944-preload-off-diagonal-only": {("whole-NT", "xcd-contiguous+lower", "preload-", "lds-nobeta"),   # off-diagonal tiles preload,
                                                      ("whole-NT", "xcd-contiguous+lower", "fast-inner", "edge")},     # diagonal tiles do not
    "half-nt-129-fast-clamped": {("half-NT", "xcd-contiguous", "fast-clamped", "edge")},
    "whole-nt-333x257-k32-fast-clamped": {("whole-NT", "xcd-contiguous", "fast-clamped", "edge")},
    "general-nn-k33": {("whole-NN", "xcd-contiguous", "general", "lds-beta")},
    "general-nt-k33": {("whole-NT", "xcd-contiguous", "general", "lds-beta")},
    "general-tn-k33": {("whole-TN", "xcd-contiguous", "general", "lds-beta")},
    "general-tt-k33": {("whole-TT", "xcd-contiguous", "general", "lds-beta")},
    "general-nn-odd-ld": {("whole-NN", "xcd-contiguous", "general", "interior-plain")},
    "general-nt-odd-ld": {("whole-NT", "xcd-contiguous", "general", "interior-plain")},
    "general-tn-odd-ld": {("whole-TN", "xcd-contiguous", "general", "interior-plain")},
    "general-tt-odd-ld": {("whole-TT", "xcd-contiguous", "general", "interior-plain")},
    "half-nn-interior-plain-epilogue-odd-ldc": {("half-NN", "xcd-contiguous", "fast-inner", "interior-plain"), ("half-NN", "xcd-contiguous", "preload-", "interior-plain")},
    "whole-nn-k-to-col-column-grouping": {("whole-NN", "k-to-col-columns", "fast-inner", "lds-beta"), ("whole-NN", "k-to-col-columns", "preload-", "lds-nobeta")},
    "whole-nn-k-to-col-round-robin": {("whole-NN", "round-robin", "fast-inner", "lds-nobeta")},
    "half-nn-k-to-col": {("half-NN", "round-robin", "fast-inner", "lds-nobeta")},
    "half-nt-k-from-row-lower": {("half-NT", "round-robin+lower", "fast-inner", "lds-beta")},
    "whole-nt-k-from-row-lower": {("whole-NT", "round-robin+lower", "fast-inner", "lds-beta")},
    "half-nt-k-from-row": {("half-NT", "round-robin", "fast-inner", "lds-beta")},
    "whole-nt-k-from-row": {("whole-NT", "round-robin", "fast-inner", "lds-beta")},
    "half-nn-a-lower": {("half-NN", "round-robin", "general", "lds-beta")},
    "whole-nn-a-lower": {("whole-NN", "round-robin", "general", "lds-beta")},
    "splitk-nn-257x130": {("splitk-whole-NN", "xcd-contiguous", "fast-inner", "lds-nobeta")},
    "splitk-tn-257x130": {("splitk-whole-TN", "xcd-contiguous", "fast-inner", "lds-nobeta")},
    "splitk-nt-1025": {("splitk-whole-NT", "xcd-contiguous", "fast-clamped", "edge"), ("splitk-whole-NT", "xcd-contiguous", "general", "interior-plain")},
    "splitk-nt-1025-lower": {("splitk-whole-NT", "xcd-contiguous+lower", "fast-inner", "interior-plain")},
}


# every (kernel, tile map, main loop, epilogue) the product cases reach together, written down: a case that is removed, or a launch rule
# that changes, shows up as a difference here
REACHED = {
    ('half-NN', 'round-robin', 'fast-inner', 'lds-beta'),
    ('half-NN', 'round-robin', 'fast-inner', 'lds-nobeta'),
    ('half-NN', 'round-robin', 'general', 'lds-beta'),
    ('half-NN', 'round-robin', 'general', 'lds-nobeta'),
    ('half-NN', 'round-robin', 'preload+', 'lds-nobeta'),
    ('half-NN', 'round-robin', 'preload-', 'lds-nobeta'),
    ('half-NN', 'xcd-contiguous', 'fast-inner', 'interior-plain'),
    ('half-NN', 'xcd-contiguous', 'fast-inner', 'lds-beta'),
    ('half-NN', 'xcd-contiguous', 'fast-inner', 'lds-nobeta'),
    ('half-NN', 'xcd-contiguous', 'general', 'edge'),
    ('half-NN', 'xcd-contiguous', 'preload+', 'interior-plain'),
    ('half-NN', 'xcd-contiguous', 'preload+', 'lds-nobeta'),
    ('half-NN', 'xcd-contiguous', 'preload-', 'interior-plain'),
    ('half-NN', 'xcd-contiguous', 'preload-', 'lds-nobeta'),
    ('half-NT', 'round-robin', 'fast-inner', 'lds-beta'),
    ('half-NT', 'round-robin', 'fast-inner', 'lds-nobeta'),
    ('half-NT', 'round-robin', 'preload+', 'lds-nobeta'),
    ('half-NT', 'round-robin', 'preload-', 'lds-nobeta'),
    ('half-NT', 'round-robin+lower', 'fast-inner', 'edge'),
    ('half-NT', 'round-robin+lower', 'fast-inner', 'lds-beta'),
    ('half-NT', 'round-robin+lower', 'fast-inner', 'lds-nobeta'),
    ('half-NT', 'round-robin+lower', 'preload+', 'lds-nobeta'),
    ('half-NT', 'round-robin+lower', 'preload-', 'lds-nobeta'),
    ('half-NT', 'xcd-contiguous', 'fast-clamped', 'edge'),
    ('half-NT', 'xcd-contiguous', 'fast-inner', 'lds-beta'),
    ('half-NT', 'xcd-contiguous', 'fast-inner', 'lds-nobeta'),
    ('half-NT', 'xcd-contiguous', 'preload+', 'lds-nobeta'),
    ('half-NT', 'xcd-contiguous', 'preload-', 'lds-nobeta'),
    ('splitk-whole-NN', 'xcd-contiguous', 'fast-inner', 'lds-nobeta'),
    ('splitk-whole-NN', 'xcd-contiguous', 'general', 'edge'),
    ('splitk-whole-NT', 'xcd-contiguous', 'fast-clamped', 'edge'),
    ('splitk-whole-NT', 'xcd-contiguous', 'fast-inner', 'interior-plain'),
    ('splitk-whole-NT', 'xcd-contiguous', 'general', 'edge'),
    ('splitk-whole-NT', 'xcd-contiguous', 'general', 'interior-plain'),
    ('splitk-whole-NT', 'xcd-contiguous+lower', 'fast-clamped', 'edge'),
    ('splitk-whole-NT', 'xcd-contiguous+lower', 'fast-inner', 'edge'),
    ('splitk-whole-NT', 'xcd-contiguous+lower', 'fast-inner', 'interior-plain'),
    ('splitk-whole-NT', 'xcd-contiguous+lower', 'general', 'edge'),
    ('splitk-whole-NT', 'xcd-contiguous+lower', 'general', 'interior-plain'),
    ('splitk-whole-TN', 'xcd-contiguous', 'fast-inner', 'lds-nobeta'),
    ('splitk-whole-TN', 'xcd-contiguous', 'general', 'edge'),
    ('whole-NN', 'k-to-col-columns', 'fast-inner', 'lds-beta'),
    ('whole-NN', 'k-to-col-columns', 'fast-inner', 'lds-nobeta'),
    ('whole-NN', 'k-to-col-columns', 'preload+', 'lds-nobeta'),
    ('whole-NN', 'k-to-col-columns', 'preload-', 'lds-nobeta'),
    ('whole-NN', 'round-robin', 'fast-inner', 'lds-beta'),
    ('whole-NN', 'round-robin', 'fast-inner', 'lds-nobeta'),
    ('whole-NN', 'round-robin', 'general', 'lds-beta'),
    ('whole-NN', 'round-robin', 'general', 'lds-nobeta'),
    ('whole-NN', 'round-robin', 'preload+', 'lds-nobeta'),
    ('whole-NN', 'round-robin', 'preload-', 'lds-nobeta'),
    ('whole-NN', 'xcd-contiguous', 'fast-inner', 'lds-beta'),
    ('whole-NN', 'xcd-contiguous', 'fast-inner', 'lds-nobeta'),
    ('whole-NN', 'xcd-contiguous', 'general', 'edge'),
    ('whole-NN', 'xcd-contiguous', 'general', 'interior-plain'),
    ('whole-NN', 'xcd-contiguous', 'general', 'lds-beta'),
    ('whole-NN', 'xcd-contiguous', 'general', 'lds-nobeta'),
    ('whole-NN', 'xcd-contiguous', 'preload+', 'lds-nobeta'),
    ('whole-NN', 'xcd-contiguous', 'preload-', 'lds-nobeta'),
    ('whole-NT', 'round-robin', 'fast-inner', 'lds-beta'),
    ('whole-NT', 'round-robin', 'fast-inner', 'lds-nobeta'),
    ('whole-NT', 'round-robin', 'preload+', 'lds-nobeta'),
    ('whole-NT', 'round-robin', 'preload-', 'lds-nobeta'),
    ('whole-NT', 'round-robin+lower', 'fast-inner', 'edge'),
    ('whole-NT', 'round-robin+lower', 'fast-inner', 'lds-beta'),
    ('whole-NT', 'round-robin+lower', 'fast-inner', 'lds-nobeta'),
    ('whole-NT', 'round-robin+lower', 'preload+', 'lds-nobeta'),
    ('whole-NT', 'round-robin+lower', 'preload-', 'lds-nobeta'),
    ('whole-NT', 'xcd-contiguous', 'fast-clamped', 'edge'),
    ('whole-NT', 'xcd-contiguous', 'fast-inner', 'lds-beta'),
    ('whole-NT', 'xcd-contiguous', 'fast-inner', 'lds-nobeta'),
    ('whole-NT', 'xcd-contiguous', 'general', 'edge'),
    ('whole-NT', 'xcd-contiguous', 'general', 'interior-plain'),
    ('whole-NT', 'xcd-contiguous', 'general', 'lds-beta'),
    ('whole-NT', 'xcd-contiguous', 'general', 'lds-nobeta'),
    ('whole-NT', 'xcd-contiguous', 'preload+', 'lds-nobeta'),
    ('whole-NT', 'xcd-contiguous', 'preload-', 'lds-nobeta'),
    ('whole-NT', 'xcd-contiguous+lower', 'fast-inner', 'edge'),
    ('whole-NT', 'xcd-contiguous+lower', 'fast-inner', 'lds-beta'),
    ('whole-NT', 'xcd-contiguous+lower', 'fast-inner', 'lds-nobeta'),
    ('whole-NT', 'xcd-contiguous+lower', 'preload+', 'lds-nobeta'),
    ('whole-NT', 'xcd-contiguous+lower', 'preload-', 'lds-nobeta'),
    ('whole-TN', 'xcd-contiguous', 'general', 'edge'),
    ('whole-TN', 'xcd-contiguous', 'general', 'interior-plain'),
    ('whole-TN', 'xcd-contiguous', 'general', 'lds-beta'),
    ('whole-TN', 'xcd-contiguous', 'general', 'lds-nobeta'),
    ('whole-TT', 'xcd-contiguous', 'general', 'edge'),
    ('whole-TT', 'xcd-contiguous', 'general', 'interior-plain'),
    ('whole-TT', 'xcd-contiguous', 'general', 'lds-beta'),
    ('whole-TT', 'xcd-contiguous', 'general', 'lds-nobeta'),
}


def test_product_cases_reach_the_paths_they_name():
    assert [c.id for c in gpu.GEMM_CASES] == list(GEMM_REACHES)
    union = set()
    for case in gpu.GEMM_CASES:
        paths = gpu.gemm_case_paths(case)
        assert GEMM_REACHES[case.id] <= paths, (case.id, GEMM_REACHES[case.id] - paths)
        assert (gpu.splitk_splits(case) > 1) == case.id.startswith("splitk-")
        assert not any(p[2] == "empty" for p in paths)
        union |= paths
    assert union == REACHED, (sorted(union - REACHED), sorted(REACHED - union))
    # every value of every axis that a launch through the C ABI can take (MIXED: the factorisation's own launches, above)
    assert {p[0].replace("splitk-", "") for p in union} == {"whole-NN", "whole-NT", "whole-TN", "whole-TT", "half-NN", "half-NT"}
    assert {p[1] for p in union} == {"xcd-contiguous", "xcd-contiguous+lower", "round-robin", "round-robin+lower", "k-to-col-columns"}
    assert {p[2] for p in union} == {"preload+", "preload-", "fast-inner", "fast-clamped", "general"}
    assert {p[3] for p in union} == {"lds-beta", "lds-nobeta", "interior-plain", "edge"}


def test_the_restatement_knows_the_thresholds_of_the_launch_rule():
    """Half tiles up to 256 tiles and from k = 64 on, never for a transposed A; MIXED only for role 1 beyond 512 tiles."""
    sq = lambda n, k, tr="NT", **kw: gpu._gc("x", tr, n, n, k, **kw)   # noqa: E731
    kernel = lambda c, **kw: {p[0] for p in gpu.gemm_paths(c, 1.0, 0.0, **kw)}   # noqa: E731
    assert kernel(sq(2048, 64)) == {"half-NT"} and kernel(sq(2049, 64)) == {"whole-NT"}       # 256 / 289 tiles
    assert kernel(sq(384, 63)) == {"whole-NT"} and kernel(sq(384, 64, "TN")) == {"whole-TN"}
    assert kernel(sq(4096, 512, c_lower=True), role=1) == {"whole-NT", "mixed-tail-NT"}        # 528 tiles: 16 in the last round
    assert kernel(sq(4096, 512, c_lower=True), role=0) == {"whole-NT"}
    assert kernel(sq(5120, 512, c_lower=True), role=1) == {"whole-NT"}                         # 820 tiles: 308 in the last round
