"""Blocked cross-validation on the GPU: gpar_cv_dense / gpar_cv_dense_grad / gpar_cv_dense_grad_finish through the C ABI against the numpy
closed form of tests/test_cv.py (value, log-determinant, means, marginal variances, the weights W themselves and 1/2 sum W o dK/dtheta with
dK by the complex-step derivative of the numpy kernel), then `fit(objective="cv")` and `GPARRegressor.cv` end to end.

Sizes and fold patterns (sizes taken in a cycle until the rows are used up, the last fold cut short), the smallest that reach every edge:
7 rows in 3 + 4; 64 rows in one fold (the fold kernel's largest tile; the value is the log marginal likelihood); 65 rows in 1 + 2 + 31 + 31
(a fold across the 32-row tiles of the S build, a ragged tail); 130 rows in 33 + 63 + 34 (folds across rows 64 and 128); 513 rows in
64 + 1 + 17 + 32 + 33 + ... (full folds at offsets that are no multiple of anything, the first panel boundary of the factorisation); one
case per kernel at 1024 rows in folds of 16, where the inverse takes its recursive path.  Data as tests/test_loo_gpu.py (noise 0.05,
cond(K) <= 1.4e4 at 513 rows), where the numpy closed form agrees with deletion to 2e-12 on values and 3e-12 on means.  Tolerances: the
parity rules for well-conditioned problems - values rtol 1e-10, means / variances rtol 1e-8 / atol 1e-10, W and kernel gradients
rtol 1e-6 / atol 1e-7, trained objectives of the two training routes rtol 1e-6.
"""
import ctypes

import numpy as np
import pytest
import torch

from .conftest import make_engine
from .test_cv import _closed_form, _cv_weights, _fold_starts
from .test_loo import _KW, _data
from .test_loo_gpu import KERNELS, _library_grads, _library_kernel

pytestmark = pytest.mark.gpu

PATTERNS = {7: [3, 4], 64: [64], 65: [1, 2, 31, 32], 130: [33, 63, 64], 513: [64, 1, 17, 32, 33], 1024: [16]}


@pytest.fixture
def hip():
    from gpar_amd.engine import set_engine

    eng = make_engine("hip")
    previous = set_engine(eng)
    yield eng
    set_engine(previous)


_CASES = {}


def _case(name, n, weighted, pattern=None):
    """Inputs and the numpy reference of one case, computed once and shared by the tests (never modified)."""
    pattern = PATTERNS[n] if pattern is None else pattern
    key = (name, n, weighted, tuple(pattern))
    if key not in _CASES:
        kfun, theta = KERNELS[name]
        rng = np.random.default_rng(1000 * n + weighted)
        x = rng.uniform(0.0, 1.0, (n, 3))
        y = np.sin(5.0 * x[:, 0]) + np.cos(3.0 * x[:, 1]) + 0.5 * x[:, 2] + 0.2 * rng.standard_normal(n)
        noise = 0.05 / rng.uniform(0.5, 2.0, n) if weighted else np.full(n, 0.05)
        starts = _fold_starts(n, pattern)
        K = kfun(x, theta) + np.diag(noise) + 1e-12 * np.eye(n)
        value, mean, var = _closed_form(K, y, starts)[:3]
        W = _cv_weights(K, y, starts)
        grads = np.zeros(theta.size)
        for j in range(theta.size):   # dK/dtheta_j by the complex-step derivative: exact to rounding, no cancellation
            moved = theta.astype(complex)
            moved[j] += 1e-30j
            grads[j] = 0.5 * np.sum(W * (kfun(x, moved).imag / 1e-30))
        logdet = np.linalg.slogdet(K)[1]
        mll = -0.5 * (logdet + y @ np.linalg.solve(K, y) + n * np.log(2.0 * np.pi))
        _CASES[key] = dict(x=x, y=y, noise=noise, starts=starts, value=value, mean=mean, var=var, W=W, grads=grads, logdet=logdet, mll=mll)
    return _CASES[key]


def _device(case):
    dev = torch.device("cuda:0")
    return (torch.tensor(case["x"], device=dev), torch.tensor(case["y"], device=dev), torch.tensor(case["noise"], device=dev))


ABI_CASES = [(n, name, weighted) for n in (7, 64, 65, 130, 513) for name in sorted(KERNELS) for weighted in (False, True)]
ABI_CASES += [(1024, "eq_linear", True), (1024, "rq_periodic", False)]


@pytest.mark.parametrize("n,name,weighted", ABI_CASES, ids=lambda v: str(v))
def test_cv_dense_and_cv_dense_grad_against_the_numpy_closed_form(hip, n, name, weighted):
    from gpar_amd import hip as lib

    case = _case(name, n, weighted)
    ck = hip.compile(_library_kernel(name, KERNELS[name][1]), 3)
    assert ck.dz == 3
    x, y, noise = _device(case)
    if n == 64:   # one fold of every row: the log marginal likelihood
        np.testing.assert_allclose(case["value"], case["mll"], rtol=1e-11)
    # value only
    out, mean, var, info = lib.cv_dense(ck, x, y, noise, 1e-12, case["starts"])
    assert int(info.cpu()) == 0
    got = out.cpu().numpy()
    print(f"{name} n={n}: value {got[0]:.12e} (ref {case['value']:.12e})")
    np.testing.assert_allclose(got[0], case["value"], rtol=1e-10)
    np.testing.assert_allclose(got[1], case["logdet"], rtol=1e-10)
    np.testing.assert_allclose(mean.cpu().numpy(), case["mean"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var.cpu().numpy(), case["var"], rtol=1e-8, atol=1e-10)
    # value, weights and gradient
    out, half, mean, var, info, _, W = lib.cv_dense_grad(ck, x, y, noise, 1e-12, hip._periodic(ck), case["starts"])
    assert int(info.cpu()) == 0
    got = out.cpu().numpy()
    np.testing.assert_allclose(got[0], case["value"], rtol=1e-10)
    np.testing.assert_allclose(got[1], case["logdet"], rtol=1e-10)
    if n == 64:
        np.testing.assert_allclose(got[0], case["mll"], rtol=1e-10)
    np.testing.assert_allclose(mean.cpu().numpy(), case["mean"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var.cpu().numpy(), case["var"], rtol=1e-8, atol=1e-10)
    il = np.tril_indices(n)
    np.testing.assert_allclose(W.cpu().numpy()[il], case["W"][il], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(half.cpu().numpy(), 0.5 * np.diag(case["W"]), rtol=1e-6, atol=1e-7)
    grads = _library_grads(name, hip._grads_from_moments(ck, got[2:], 0.5))
    print(f"  gradients {grads} (ref {case['grads']})")
    np.testing.assert_allclose(grads, case["grads"], rtol=1e-6, atol=1e-7)


def test_folds_of_one_row_against_the_leave_one_out_entry(hip):
    from gpar_amd import hip as lib

    n, name = 130, "eq_linear"
    case = _case(name, n, True, pattern=[1])
    ck = hip.compile(_library_kernel(name, KERNELS[name][1]), 3)
    x, y, noise = _device(case)
    want_out, want_half, want_mean, want_var, _, _, want_W = lib.loo_dense_grad(ck, x, y, noise, 1e-12, hip._periodic(ck))
    out, half, mean, var, info, _, W = lib.cv_dense_grad(ck, x, y, noise, 1e-12, hip._periodic(ck), np.arange(n + 1))
    assert int(info.cpu()) == 0
    got, want = out.cpu().numpy(), want_out.cpu().numpy()
    np.testing.assert_allclose(got[:2], want[:2], rtol=1e-10)
    np.testing.assert_allclose(mean.cpu().numpy(), want_mean.cpu().numpy(), rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var.cpu().numpy(), want_var.cpu().numpy(), rtol=1e-8, atol=1e-10)
    il = np.tril_indices(n)
    np.testing.assert_allclose(W.cpu().numpy()[il], want_W.cpu().numpy()[il], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(half.cpu().numpy(), want_half.cpu().numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(got[2:], want[2:], rtol=1e-6, atol=1e-7)


def test_finish_form_after_build_and_batched_factorisation_gives_the_bits_of_the_one_call_form(hip):
    from gpar_amd import _lib
    from gpar_amd import hip as lib

    n, name = 130, "rq_periodic"
    case = _case(name, n, True)
    ck = hip.compile(_library_kernel(name, KERNELS[name][1]), 3)
    x, y, noise = _device(case)
    out1, half1, mean1, var1, _, _, W1 = lib.cv_dense_grad(ck, x, y, noise, 1e-12, True, case["starts"])
    cdll, dev, nacc = _lib.load(), x.device, _lib.GRAD_NACC
    starts, nfolds, max_fold = lib.upload_folds(case["starts"], n, dev)
    assert (nfolds, max_fold) == (3, 63)
    z, zd = lib.alloc_matrix(n, 3, dev), lib.alloc_matrix(n, 3, dev, zero=True)
    A, X, W = lib.alloc_matrix(n + 1, n + 1, dev), lib.alloc_matrix(n, n, dev), lib.alloc_matrix(n, n, dev)
    logdet, info = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    nblocks = 6   # (as hip.cv_dense_grad sizes it: three 64-row tiles, their lower triangle)
    nvec = int(cdll.gpar_workspace_doubles(_lib.WS_CV, n, 1, max_fold))
    assert nvec == n * (3 + max_fold)
    work = torch.empty(nblocks * nacc + n + nvec, dtype=torch.float64, device=dev)
    out, vectors = torch.empty(2 + nacc, dtype=torch.float64, device=dev), torch.empty(3, n, dtype=torch.float64, device=dev)
    stream = lib.stream_ptr(dev)
    fs, ks = ctypes.byref(ck.fspec), ctypes.byref(ck.kspec)
    _lib.check(cdll.gpar_logpdf_dense_build(fs, ks, x.data_ptr(), n, lib._ld(x), y.data_ptr(), 1, noise.data_ptr(), 1e-12, z.data_ptr(), lib._ld(z),
                                            A.data_ptr(), lib._ld(A), logdet.data_ptr(), info.data_ptr(), stream), "build")
    _lib.check(cdll.gpar_potrf_batch(A.data_ptr(), 1, 0, n + 1, n, lib._ld(A), logdet.data_ptr(), info.data_ptr(), 0, stream), "potrf_batch")
    _lib.check(cdll.gpar_cv_dense_grad_finish(fs, ks, x.data_ptr(), n, lib._ld(x), y.data_ptr(), 1, z.data_ptr(), zd.data_ptr(), lib._ld(z), A.data_ptr(),
                                              lib._ld(A), logdet.data_ptr(), info.data_ptr(), X.data_ptr(), lib._ld(X), W.data_ptr(), lib._ld(W),
                                              work[nblocks * nacc:].data_ptr(), work[nblocks * nacc + n:].data_ptr(), work.data_ptr(), nblocks,
                                              out.data_ptr(), vectors[0].data_ptr(), vectors[1].data_ptr(), vectors[2].data_ptr(),
                                              starts.data_ptr(), nfolds, max_fold, info[1:].data_ptr(), stream), "finish")
    assert info.cpu().tolist() == [0, 0]
    assert torch.equal(out, out1) and torch.equal(vectors[0], half1) and torch.equal(vectors[1], mean1) and torch.equal(vectors[2], var1)
    il = torch.tril_indices(n, n)
    assert torch.equal(W[il[0], il[1]], W1[il[0], il[1]])


def test_a_fold_bound_beyond_the_limit_is_an_argument_error(hip):
    """max_fold = 65: the entry returns its argument error before the first launch (the outputs keep their contents)."""
    from gpar_amd import _lib
    from gpar_amd import hip as lib

    n, name = 70, "eq_linear"
    ck = hip.compile(_library_kernel(name, KERNELS[name][1]), 3)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(70)
    x, y = torch.tensor(rng.uniform(0.0, 1.0, (n, 3)), device=dev), torch.tensor(rng.standard_normal(n), device=dev)
    cdll = _lib.load()
    assert _lib.CV_MAX_FOLD == 64
    assert cdll.gpar_workspace_doubles(_lib.WS_CV, n, 1, 65) == -1 and cdll.gpar_workspace_doubles(_lib.WS_CV, n, 0, 0) == -1
    starts = torch.tensor([0, 65, 70], dtype=torch.int32, device=dev)
    z, A, X, T = lib.alloc_matrix(n, 3, dev), lib.alloc_matrix(n + 1, n + 1, dev), lib.alloc_matrix(n, n, dev), lib.alloc_matrix(n, n, dev)
    vec = torch.empty(n * 70, dtype=torch.float64, device=dev)
    out = torch.full((2,), -7.0, dtype=torch.float64, device=dev)
    moments = torch.full((2, n), -7.0, dtype=torch.float64, device=dev)
    info = torch.full((1,), -7, dtype=torch.int32, device=dev)
    fs, ks = ctypes.byref(ck.fspec), ctypes.byref(ck.kspec)
    for max_fold in (65, 0):
        rc = cdll.gpar_cv_dense(fs, ks, x.data_ptr(), n, lib._ld(x), y.data_ptr(), 1, None, 1e-12, z.data_ptr(), lib._ld(z), A.data_ptr(), lib._ld(A),
                                X.data_ptr(), lib._ld(X), T.data_ptr(), lib._ld(T), vec.data_ptr(), out.data_ptr(), moments[0].data_ptr(),
                                moments[1].data_ptr(), starts.data_ptr(), 2, max_fold, info.data_ptr(), 0, lib.stream_ptr(dev))
        assert rc == -1003
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [-7.0, -7.0] and int(info.cpu()) == -7 and bool((moments == -7.0).all())
    with pytest.raises(ValueError):
        lib.cv_dense(ck, x, y, None, 1e-12, [0, 65, 70])


def test_fit_with_the_cv_objective_by_the_prepared_and_the_general_route(hip):
    from gpar_amd.regression import GPARRegressor

    x, y = _data(100, 4, seed=21)
    finals = {}
    for fast in (True, False):
        reg = GPARRegressor(**_KW)
        reg.fast_fit = fast
        reg.condition(x, y)
        finals[fast] = reg._train(range(4), objective="cv", folds=10, iters=10)
    print("trained cross-validation objectives, prepared / general:", finals[True], finals[False])
    for pi in range(4):
        np.testing.assert_allclose(finals[True][pi], finals[False][pi], rtol=1e-6)


def test_regressor_cv_on_the_gpu_against_the_oracle_engine(hip):
    from gpar_amd.engine import set_engine
    from gpar_amd.regression import GPARRegressor

    x, y = _data(65, 3, seed=22, missing=0.1)
    labels = np.random.default_rng(22).integers(0, 7, 65)
    got = GPARRegressor(**_KW).cv(x, y, folds=labels)
    previous = set_engine(make_engine("oracle"))
    try:
        want = GPARRegressor(**_KW).cv(x, y, folds=labels)
    finally:
        set_engine(previous)
    np.testing.assert_allclose(got[0], want[0], rtol=1e-10)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(got[2], want[2], rtol=1e-8, atol=1e-10)
