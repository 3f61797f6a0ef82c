"""Purged blocked cross-validation on the GPU: gpar_cv_gap_dense / gpar_cv_gap_dense_grad / gpar_cv_gap_dense_grad_finish through the
C ABI against the numpy references of tests/test_cv_gap.py (brute-force deletion for the value, the means and the marginal variances;
the closed form's W, which that file checks against the complex step, for W itself and for 1/2 sum W o dK/dtheta with dK by the
complex-step derivative of the numpy kernel), then `GPARRegressor.cv(gap=)` and `fit(objective="cv", gap=)` end to end.

Cases (n, fold size, gap): (7, 1, 1); (64, 5, 3) and (65, 5, 3) - ragged last folds, both sides of a 64-row tile; (130, 16, 24) - blocks of
64 rows, the fold kernel's largest tile, across the 128-wide GEMM tile; (513, 7, 10) - one past the first panel boundary of the
factorisation, 74 folds.  Both kernels of tests/test_loo_gpu.py, weighted and unweighted, at 65 rows; the weighted EQ + linear kernel
elsewhere.  Tolerances: the parity rules - values rtol 1e-10, means / variances rtol 1e-8 / atol 1e-10, W and kernel gradients
rtol 1e-6 / atol 1e-7, trained objectives of the two training routes rtol 1e-6.
"""
import ctypes

import numpy as np
import pytest
import torch

from .conftest import make_engine
from .test_cv_gap import layer_case
from .test_loo import _KW, _data
from .test_loo_gpu import KERNELS, _library_grads, _library_kernel

pytestmark = pytest.mark.gpu


@pytest.fixture
def hip():
    from gpar_amd.engine import set_engine

    eng = make_engine("hip")
    previous = set_engine(eng)
    yield eng
    set_engine(previous)


def _kernel_grads(case):
    """1/2 sum W o dK/dtheta of the case's reference weights, dK by the complex step; once per case."""
    if "w_grads" not in case:
        kfun, theta = KERNELS[case["name"]]
        grads = np.zeros(theta.size)
        for j in range(theta.size):
            moved = theta.astype(complex)
            moved[j] += 1e-30j
            grads[j] = 0.5 * np.sum(case["W"] * (kfun(case["x"], moved).imag / 1e-30))
        case["w_grads"] = grads
    return case["w_grads"]


def _device(case):
    dev = torch.device("cuda:0")
    return (torch.tensor(case["x"], device=dev), torch.tensor(case["y"], device=dev), torch.tensor(case["noise"], device=dev))


def _hold(case):
    return case["lo"], case["hi"]


ABI_CASES = [(7, 1, 1, "eq_linear", True), (64, 5, 3, "eq_linear", True), (130, 16, 24, "eq_linear", True), (513, 7, 10, "eq_linear", True)]
ABI_CASES += [(65, 5, 3, name, weighted) for name in sorted(KERNELS) for weighted in (False, True)]


@pytest.mark.parametrize("n,fold,gap,name,weighted", ABI_CASES, ids=lambda v: str(v))
def test_cv_gap_dense_and_cv_gap_dense_grad_against_the_numpy_references(hip, n, fold, gap, name, weighted):
    from gpar_amd import hip as lib

    case = layer_case(n, fold, gap, weighted, name)
    if n == 130:
        assert int((case["hi"] - case["lo"]).max()) == 64
    ck = hip.compile(_library_kernel(name, KERNELS[name][1]), 3)
    x, y, noise = _device(case)
    out, mean, var, info = lib.cv_gap_dense(ck, x, y, noise, 1e-12, case["starts"], _hold(case))
    assert int(info.cpu()) == 0
    got = out.cpu().numpy()
    print(f"{name} n={n} fold={fold} gap={gap}: value {got[0]:.12e} (ref {case['value']:.12e})")
    np.testing.assert_allclose(got[0], case["value"], rtol=1e-10)
    np.testing.assert_allclose(got[1], case["logdet"], rtol=1e-10)
    np.testing.assert_allclose(mean.cpu().numpy(), case["mean"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var.cpu().numpy(), case["var"], rtol=1e-8, atol=1e-10)
    out, half, mean, var, info, _, W = lib.cv_gap_dense_grad(ck, x, y, noise, 1e-12, hip._periodic(ck), case["starts"], _hold(case))
    assert int(info.cpu()) == 0
    got = out.cpu().numpy()
    np.testing.assert_allclose(got[0], case["value"], rtol=1e-10)
    np.testing.assert_allclose(got[1], case["logdet"], rtol=1e-10)
    np.testing.assert_allclose(mean.cpu().numpy(), case["mean"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var.cpu().numpy(), case["var"], rtol=1e-8, atol=1e-10)
    il = np.tril_indices(n)
    print(f"  largest |W - ref| {np.max(np.abs(W.cpu().numpy()[il] - case['W'][il])):.3e} of {np.max(np.abs(case['W'])):.3e}")
    np.testing.assert_allclose(W.cpu().numpy()[il], case["W"][il], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(half.cpu().numpy(), 0.5 * np.diag(case["W"]), rtol=1e-6, atol=1e-7)
    grads = _library_grads(name, hip._grads_from_moments(ck, got[2:], 0.5))
    print(f"  gradients {grads} (ref {_kernel_grads(case)})")
    np.testing.assert_allclose(grads, _kernel_grads(case), rtol=1e-6, atol=1e-7)


def test_two_runs_of_the_same_call_return_identical_bits(hip):
    """b and the band image of C are summed in a fixed order (ascending folds, no atomics)."""
    from gpar_amd import hip as lib

    case = layer_case(130, 16, 24, True)
    ck = hip.compile(_library_kernel("eq_linear", KERNELS["eq_linear"][1]), 3)
    x, y, noise = _device(case)
    runs = [lib.cv_gap_dense_grad(ck, x, y, noise, 1e-12, False, case["starts"], _hold(case)) for _ in range(2)]
    il = torch.tril_indices(130, 130)
    for a, b in zip(runs[0][:4], runs[1][:4]):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][6][il[0], il[1]], runs[1][6][il[0], il[1]])


def test_finish_form_after_build_and_batched_factorisation_gives_the_bits_of_the_one_call_form(hip):
    from gpar_amd import _lib
    from gpar_amd import hip as lib

    n, name = 130, "rq_periodic"
    case = layer_case(n, 16, 24, True, name)
    ck = hip.compile(_library_kernel(name, KERNELS[name][1]), 3)
    x, y, noise = _device(case)
    out1, half1, mean1, var1, _, _, W1 = lib.cv_gap_dense_grad(ck, x, y, noise, 1e-12, True, case["starts"], _hold(case))
    cdll, dev, nacc = _lib.load(), x.device, _lib.GRAD_NACC
    starts, lo, hi, nfolds, max_hold = lib.upload_hold(case["starts"], _hold(case), n, dev)
    assert (nfolds, max_hold) == (9, 64)
    z, zd = lib.alloc_matrix(n, 3, dev), lib.alloc_matrix(n, 3, dev, zero=True)
    A, X, W = lib.alloc_matrix(n + 1, n + 1, dev), lib.alloc_matrix(n, n, dev), lib.alloc_matrix(n, n, dev)
    logdet, info = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    nblocks = 6   # (as hip.cv_gap_dense_grad sizes it: three 64-row tiles, their lower triangle)
    nvec = int(cdll.gpar_workspace_doubles(_lib.WS_CV_GAP, n, 1, max_hold))
    assert nvec == 5 * n + 3 * n * max_hold + n * (2 * max_hold - 1) + n * n   # (n even: no padding)
    assert cdll.gpar_workspace_doubles(_lib.WS_CV_GAP, n, 0, max_hold) == n and cdll.gpar_workspace_doubles(_lib.WS_CV_GAP, n, 1, 65) == -1
    work = torch.empty(nblocks * nacc + n + nvec, dtype=torch.float64, device=dev)
    out, vectors = torch.empty(2 + nacc, dtype=torch.float64, device=dev), torch.empty(3, n, dtype=torch.float64, device=dev)
    stream = lib.stream_ptr(dev)
    fs, ks = ctypes.byref(ck.fspec), ctypes.byref(ck.kspec)
    _lib.check(cdll.gpar_logpdf_dense_build(fs, ks, x.data_ptr(), n, lib._ld(x), y.data_ptr(), 1, noise.data_ptr(), 1e-12, z.data_ptr(), lib._ld(z),
                                            A.data_ptr(), lib._ld(A), logdet.data_ptr(), info.data_ptr(), stream), "build")
    _lib.check(cdll.gpar_potrf_batch(A.data_ptr(), 1, 0, n + 1, n, lib._ld(A), logdet.data_ptr(), info.data_ptr(), 0, stream), "potrf_batch")
    _lib.check(cdll.gpar_cv_gap_dense_grad_finish(fs, ks, x.data_ptr(), n, lib._ld(x), y.data_ptr(), 1, z.data_ptr(), zd.data_ptr(), lib._ld(z),
                                                  A.data_ptr(), lib._ld(A), logdet.data_ptr(), info.data_ptr(), X.data_ptr(), lib._ld(X), W.data_ptr(),
                                                  lib._ld(W), work[nblocks * nacc:].data_ptr(), work[nblocks * nacc + n:].data_ptr(), work.data_ptr(),
                                                  nblocks, out.data_ptr(), vectors[0].data_ptr(), vectors[1].data_ptr(), vectors[2].data_ptr(),
                                                  starts.data_ptr(), lo.data_ptr(), hi.data_ptr(), nfolds, max_hold, info[1:].data_ptr(), stream),
               "finish")
    assert info.cpu().tolist() == [0, 0]
    assert torch.equal(out, out1) and torch.equal(vectors[0], half1) and torch.equal(vectors[1], mean1) and torch.equal(vectors[2], var1)
    il = torch.tril_indices(n, n)
    assert torch.equal(W[il[0], il[1]], W1[il[0], il[1]])


def test_blocks_equal_to_the_folds_agree_with_the_blocked_entry(hip):
    """Gap 0 through the new entry: the numbers of gpar_cv_dense_grad (another chain, so not its bits)."""
    from gpar_amd import hip as lib

    n, name = 130, "eq_linear"
    case = layer_case(n, 16, 24, True)
    starts = case["starts"]
    ck = hip.compile(_library_kernel(name, KERNELS[name][1]), 3)
    x, y, noise = _device(case)
    want_out, want_half, want_mean, want_var, _, _, want_W = lib.cv_dense_grad(ck, x, y, noise, 1e-12, False, starts)
    out, half, mean, var, info, _, W = lib.cv_gap_dense_grad(ck, x, y, noise, 1e-12, False, starts, (starts[:-1], starts[1:]))
    assert int(info.cpu()) == 0
    got, want = out.cpu().numpy(), want_out.cpu().numpy()
    np.testing.assert_allclose(got[:2], want[:2], rtol=1e-10)
    np.testing.assert_allclose(mean.cpu().numpy(), want_mean.cpu().numpy(), rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var.cpu().numpy(), want_var.cpu().numpy(), rtol=1e-8, atol=1e-10)
    il = np.tril_indices(n)
    np.testing.assert_allclose(W.cpu().numpy()[il], want_W.cpu().numpy()[il], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(half.cpu().numpy(), want_half.cpu().numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(got[2:], want[2:], rtol=1e-6, atol=1e-7)


def test_malformed_extents_are_reported_in_the_info_word(hip):
    """Argument checks of the device side: extents that pass the host's eye only because they are handed over already uploaded.  A block
    of 65 rows, a block that does not contain its fold, a decreasing hold_lo, a block beyond the last row: n + 1 + the fold.  Nothing
    behind the info word is read.  The host's own check (`hip.hold_extents`) refuses the same extents before anything is uploaded."""
    from gpar_amd import _lib
    from gpar_amd import hip as lib

    n = 130
    case = layer_case(n, 16, 24, True)
    ck = hip.compile(_library_kernel("eq_linear", KERNELS["eq_linear"][1]), 3)
    x, y, noise = _device(case)
    dev = x.device
    up = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=dev)   # noqa: E731
    starts = up([0, 40, 90, 130])
    for lo, hi, fold in (([0, 30, 80], [50, 95, 130], 1),      # fold 1: rows 30 ... 94, 65 of them
                         ([0, 45, 80], [50, 100, 130], 1),     # fold 1 begins at row 40, its block at row 45
                         ([0, 30, 20], [50, 94, 130], 2),      # hold_lo decreases at fold 2
                         ([0, 30, 80], [50, 94, 131], 2)):     # a block beyond the last row
        for call in ("value", "grad"):
            folds = (starts, up(lo), up(hi), 3, 64)
            if call == "value":
                info = lib.cv_gap_dense(ck, x, y, noise, 1e-12, folds, None)[3]
            else:
                info = lib.cv_gap_dense_grad(ck, x, y, noise, 1e-12, False, folds, None)[4]
            assert int(info.cpu()) == n + 1 + fold, (lo, hi, call)
    assert _lib.load().gpar_workspace_doubles(_lib.WS_CV_GAP, n, 1, 65) == -1 and _lib.load().gpar_workspace_doubles(_lib.WS_CV_GAP, n, 0, 0) == -1
    for hold in (([0, 30, 80], [50, 95, 130]), ([0, 45, 80], [50, 100, 130]), ([0, 30, 20], [50, 94, 130])):
        with pytest.raises(ValueError):
            lib.cv_gap_dense(ck, x, y, noise, 1e-12, [0, 40, 90, 130], hold)


def test_malformed_extents_at_257_rows_are_reported_by_the_fold_behind_column_256(hip):
    """The malformed extents of the test above at n = 257, in the last of six folds - rows 250 ... 256, so the fold that reports holds the
    one column of the second 256-column block of loo_rank2_kernel: info = n + 1 + 5 from the value-only, the one-call and the finish
    form.  The fold that reports is skipped whole: its rows of the means and the variances come back as the sentinel they went in
    with, as do the padding of every buffer and every word behind n.  (The other folds have written theirs, and include/gpar_hip.h
    promises nothing for W, 1/2 diag W and the value behind a set info word: "Results are garbage then" - so those are not held.)"""
    from .test_cv_large_gpu import SENTINEL, case, padding_untouched, raw_call

    n, fold = 257, 5
    c = dict(case("loo", None, n), family="cv_gap")   # (the inputs of the large cases at 257 rows)
    starts = [0, 50, 100, 150, 200, 250, 257]
    for lo, hi in (([0, 45, 95, 145, 192, 192], [55, 105, 155, 205, 250, 257]),     # fold 5: rows 192 ... 256, 65 of them
                   ([0, 45, 95, 145, 192, 252], [55, 105, 155, 205, 250, 257]),     # fold 5 begins at row 250, its block at row 252
                   ([0, 45, 95, 145, 200, 199], [55, 105, 155, 205, 250, 257]),     # hold_lo decreases at fold 5
                   ([0, 45, 95, 145, 192, 240], [55, 105, 155, 205, 250, 258])):    # a block beyond the last row
        for mode in ("value", "grad", "finish"):
            got = raw_call(hip, c, mode, pad=3, extents=(starts, lo, hi, 64))
            assert got["rc"] == 0 and got["info"][1 if mode == "finish" else 0] == n + 1 + fold, (lo, hi, mode, got["info"])
            assert bool((got["mean"][250:] == SENTINEL).all()) and bool((got["var"][250:] == SENTINEL).all()), (lo, hi, mode)
            assert padding_untouched(got), (lo, hi, mode)


def test_regressor_cv_and_fit_with_a_gap_against_the_composed_route_on_the_same_engine(hip, monkeypatch):
    from gpar_amd.engine import HipEngine
    from gpar_amd.regression import GPARRegressor

    x, y = _data(130, 2, seed=51, missing=0.1)
    got = GPARRegressor(**_KW).cv(x, y, folds=10, gap=4)
    finals = {}
    for fast in (True, False):
        reg = GPARRegressor(**_KW)
        reg.fast_fit = fast
        reg.condition(x, y)
        finals[fast] = reg._train(range(2), objective="cv", folds=10, gap=4, iters=5)
    # the composed route: the same engine without its fused purged calls
    monkeypatch.delattr(HipEngine, "cv_gap_dense")
    monkeypatch.delattr(HipEngine, "cv_gap_dense_grad")
    want = GPARRegressor(**_KW).cv(x, y, folds=10, gap=4)
    np.testing.assert_allclose(got[0], want[0], rtol=1e-10)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(got[2], want[2], rtol=1e-8, atol=1e-10)
    reg = GPARRegressor(**_KW)
    reg.fast_fit = False
    reg.condition(x, y)
    finals["composed"] = reg._train(range(2), objective="cv", folds=10, gap=4, iters=5)
    print("trained purged cross-validation objectives, prepared / general / composed:", finals[True], finals[False], finals["composed"])
    for pi in range(2):
        np.testing.assert_allclose(finals[True][pi], finals[False][pi], rtol=1e-6)
        np.testing.assert_allclose(finals[False][pi], finals["composed"][pi], rtol=1e-6)
