"""Leave-one-out cross-validation on the GPU: gpar_loo_dense / gpar_loo_dense_grad / gpar_loo_dense_grad_finish through the C ABI against
the numpy closed form of this file (value, means, variances, the weights W themselves and 1/2 sum W o dK/dtheta with dK by the complex-step
derivative of the numpy kernel), then `fit(objective="loo")` and `GPARRegressor.loo` end to end.

Sizes 7 / 64 / 65 / 130 / 512 / 513: below one tile, exactly one and just over one 64 x 64 Gram / gradient tile, across a 128-wide GEMM
tile, the first panel boundary of the factorisation and one past it (32-wide tiles of the S build: 7 / 64 / 65 cover ragged, exact and
one-over); one case per kernel at 1024 rows, where the inverse switches to its recursive path.  Tolerances: the parity rules of
tests/test_parity_gpu.py for well-conditioned problems (noise >= 1e-2 of the signal) - values rtol 1e-10, means / variances
rtol 1e-8 / atol 1e-10, W and kernel gradients rtol 1e-6 / atol 1e-7, trained objectives of the two training routes rtol 1e-6.
"""
import ctypes

import numpy as np
import pytest
import torch

from .conftest import make_engine
from .test_loo import _KW, _closed_form, _data, _loo_weights

pytestmark = pytest.mark.gpu

SIZES = [7, 64, 65, 130, 512, 513]


@pytest.fixture
def hip():
    from gpar_amd.engine import set_engine

    eng = make_engine("hip")
    previous = set_engine(eng)
    yield eng
    set_engine(previous)


# ---- two kernels over three feature dims, in numpy and as library kernels --------------------------------------------------------
def _k_eq_linear(x, theta):
    s0, s1, coef, sl = theta
    d2 = (x[:, None, 0] - x[None, :, 0]) ** 2 / s0**2 + (x[:, None, 1] - x[None, :, 1]) ** 2 / s1**2
    return np.exp(-0.5 * d2) + coef * np.outer(x[:, 2], x[:, 2]) / sl**2


def _k_rq_periodic(x, theta):
    s, alpha, sp, period = theta
    r2 = (x[:, None, 0] - x[None, :, 0]) ** 2 / s**2
    u = 2.0 * np.pi * x[:, 1] / period
    e2 = ((np.sin(u)[:, None] - np.sin(u)[None, :]) ** 2 + (np.cos(u)[:, None] - np.cos(u)[None, :]) ** 2) / sp**2
    return (1.0 + r2 / (2.0 * alpha)) ** (-alpha) * np.exp(-0.5 * e2)


def _library_kernel(name, theta):
    from gpar_amd.kernels import EQ, RQ, Linear

    if name == "eq_linear":
        s0, s1, coef, sl = theta
        return EQ().stretch(np.array([s0, s1])).select([0, 1]) + coef * Linear().stretch(sl).select([2])
    s, alpha, sp, period = theta
    return RQ(alpha).stretch(s).select([0]) * EQ().stretch(sp).periodic(period).select([1])


def _library_grads(name, grads):
    """The engine's gradient dictionary in the order of theta."""
    if name == "eq_linear":
        f0, f1 = grads["factors"][0][0], grads["factors"][1][0]
        return np.concatenate([np.ravel(f0["scales"]), [grads["coef"][1]], [np.sum(f1["scales"])]])
    f0, f1 = grads["factors"][0]
    return np.array([np.sum(f0["scales"]), float(f0["alpha"]), np.sum(f1["scales"]), np.sum(f1["periods"])])


KERNELS = {"eq_linear": (_k_eq_linear, np.array([0.5, 0.7, 0.3, 2.0])), "rq_periodic": (_k_rq_periodic, np.array([0.6, 1.5, 0.8, 1.3]))}
_CASES = {}


def _case(name, n, weighted):
    """Inputs and the numpy reference of one case, computed once and shared by the tests (never modified)."""
    key = (name, n, weighted)
    if key not in _CASES:
        kfun, theta = KERNELS[name]
        rng = np.random.default_rng(1000 * n + weighted)
        x = rng.uniform(0.0, 1.0, (n, 3))
        y = np.sin(5.0 * x[:, 0]) + np.cos(3.0 * x[:, 1]) + 0.5 * x[:, 2] + 0.2 * rng.standard_normal(n)
        noise = 0.05 / rng.uniform(0.5, 2.0, n) if weighted else np.full(n, 0.05)

        def K(t):
            return kfun(x, t) + np.diag(noise) + 1e-12 * np.eye(n)

        value, mean, var, _, _ = _closed_form(K(theta), y)
        W = _loo_weights(K(theta), y)
        grads = np.zeros(theta.size)
        for j in range(theta.size):   # dK/dtheta_j by the complex-step derivative: exact to rounding, no cancellation
            moved = theta.astype(complex)
            moved[j] += 1e-30j
            grads[j] = 0.5 * np.sum(W * (kfun(x, moved).imag / 1e-30))
        _CASES[key] = dict(x=x, y=y, noise=noise, value=value, mean=mean, var=var, W=W, grads=grads, logdet=np.linalg.slogdet(K(theta))[1])
    return _CASES[key]


def _device(case):
    dev = torch.device("cuda:0")
    return (torch.tensor(case["x"], device=dev), torch.tensor(case["y"], device=dev), torch.tensor(case["noise"], device=dev))


# (1024: the smallest size at which the inverse takes its recursive path - a multiple of 512 from 1024 rows on)
ABI_CASES = [(n, name, weighted) for n in SIZES for name in sorted(KERNELS) for weighted in (False, True)] + [(1024, "eq_linear", True), (1024, "rq_periodic", False)]


@pytest.mark.parametrize("n,name,weighted", ABI_CASES, ids=lambda v: str(v))
def test_loo_dense_and_loo_dense_grad_against_the_numpy_closed_form(hip, n, name, weighted):
    from gpar_amd import hip as lib

    case = _case(name, n, weighted)
    ck = hip.compile(_library_kernel(name, KERNELS[name][1]), 3)
    assert ck.dz == 3
    x, y, noise = _device(case)
    # value only
    out, mean, var, info = lib.loo_dense(ck, x, y, noise, 1e-12)
    assert int(info.cpu()) == 0
    got = out.cpu().numpy()
    print(f"{name} n={n}: value {got[0]:.12e} (ref {case['value']:.12e})")
    np.testing.assert_allclose(got[0], case["value"], rtol=1e-10)
    np.testing.assert_allclose(got[1], case["logdet"], rtol=1e-10)
    np.testing.assert_allclose(mean.cpu().numpy(), case["mean"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var.cpu().numpy(), case["var"], rtol=1e-8, atol=1e-10)
    # value, weights and gradient
    out, half, mean, var, info, _, W = lib.loo_dense_grad(ck, x, y, noise, 1e-12, hip._periodic(ck))
    assert int(info.cpu()) == 0
    got = out.cpu().numpy()
    np.testing.assert_allclose(got[0], case["value"], rtol=1e-10)
    np.testing.assert_allclose(got[1], case["logdet"], rtol=1e-10)
    np.testing.assert_allclose(mean.cpu().numpy(), case["mean"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var.cpu().numpy(), case["var"], rtol=1e-8, atol=1e-10)
    il = np.tril_indices(n)
    np.testing.assert_allclose(W.cpu().numpy()[il], case["W"][il], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(half.cpu().numpy(), 0.5 * np.diag(case["W"]), rtol=1e-6, atol=1e-7)
    grads = _library_grads(name, hip._grads_from_moments(ck, got[2:], 0.5))
    print(f"  gradients {grads} (ref {case['grads']})")
    np.testing.assert_allclose(grads, case["grads"], rtol=1e-6, atol=1e-7)


def test_finish_form_after_build_and_batched_factorisation_gives_the_bits_of_the_one_call_form(hip):
    from gpar_amd import _lib
    from gpar_amd import hip as lib

    n, name = 130, "rq_periodic"
    case = _case(name, n, True)
    ck = hip.compile(_library_kernel(name, KERNELS[name][1]), 3)
    x, y, noise = _device(case)
    out1, half1, mean1, var1, _, _, W1 = lib.loo_dense_grad(ck, x, y, noise, 1e-12, True)
    cdll, dev, nacc = _lib.load(), x.device, _lib.GRAD_NACC
    z, zd = lib.alloc_matrix(n, 3, dev), lib.alloc_matrix(n, 3, dev, zero=True)
    A, X, W = lib.alloc_matrix(n + 1, n + 1, dev), lib.alloc_matrix(n, n, dev), lib.alloc_matrix(n, n, dev)
    logdet, info = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    nblocks = 6   # (as hip.loo_dense_grad sizes it: three 64-row tiles, their lower triangle)
    work = torch.empty(nblocks * nacc + n + 4 * n, dtype=torch.float64, device=dev)
    out, vectors = torch.empty(2 + nacc, dtype=torch.float64, device=dev), torch.empty(3, n, dtype=torch.float64, device=dev)
    stream = lib.stream_ptr(dev)
    fs, ks = ctypes.byref(ck.fspec), ctypes.byref(ck.kspec)
    _lib.check(cdll.gpar_logpdf_dense_build(fs, ks, x.data_ptr(), n, lib._ld(x), y.data_ptr(), 1, noise.data_ptr(), 1e-12, z.data_ptr(), lib._ld(z),
                                            A.data_ptr(), lib._ld(A), logdet.data_ptr(), info.data_ptr(), stream), "build")
    _lib.check(cdll.gpar_potrf_batch(A.data_ptr(), 1, 0, n + 1, n, lib._ld(A), logdet.data_ptr(), info.data_ptr(), 0, stream), "potrf_batch")
    _lib.check(cdll.gpar_loo_dense_grad_finish(fs, ks, x.data_ptr(), n, lib._ld(x), y.data_ptr(), 1, z.data_ptr(), zd.data_ptr(), lib._ld(z), A.data_ptr(),
                                               lib._ld(A), logdet.data_ptr(), info.data_ptr(), X.data_ptr(), lib._ld(X), W.data_ptr(), lib._ld(W),
                                               work[nblocks * nacc:].data_ptr(), work[nblocks * nacc + n:].data_ptr(), work.data_ptr(), nblocks,
                                               out.data_ptr(), vectors[0].data_ptr(), vectors[1].data_ptr(), vectors[2].data_ptr(),
                                               info[1:].data_ptr(), stream), "finish")
    assert info.cpu().tolist() == [0, 0]
    assert torch.equal(out, out1) and torch.equal(vectors[0], half1) and torch.equal(vectors[1], mean1) and torch.equal(vectors[2], var1)
    il = torch.tril_indices(n, n)
    assert torch.equal(W[il[0], il[1]], W1[il[0], il[1]])


def test_fit_with_the_loo_objective_by_the_prepared_and_the_general_route(hip):
    from gpar_amd.regression import GPARRegressor

    x, y = _data(100, 4, seed=21)
    finals = {}
    for fast in (True, False):
        reg = GPARRegressor(**_KW)
        reg.fast_fit = fast
        reg.condition(x, y)
        finals[fast] = reg._train(range(4), objective="loo", iters=10)
    print("trained leave-one-out objectives, prepared / general:", finals[True], finals[False])
    for pi in range(4):
        np.testing.assert_allclose(finals[True][pi], finals[False][pi], rtol=1e-6)


def test_regressor_loo_on_the_gpu_against_the_oracle_engine(hip):
    from gpar_amd.engine import set_engine
    from gpar_amd.regression import GPARRegressor

    x, y = _data(65, 3, seed=22, missing=0.1)
    got = GPARRegressor(**_KW).loo(x, y)
    previous = set_engine(make_engine("oracle"))
    try:
        want = GPARRegressor(**_KW).loo(x, y)
    finally:
        set_engine(previous)
    np.testing.assert_allclose(got[0], want[0], rtol=1e-10)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(got[2], want[2], rtol=1e-8, atol=1e-10)
