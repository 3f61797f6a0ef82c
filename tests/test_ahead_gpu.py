"""Rolling-origin forecast scoring on the GPU: gpar_ahead_dense / gpar_ahead_dense_grad / gpar_ahead_dense_grad_finish through the C ABI
against the brute-force numpy yardstick of tests/test_ahead.py (one fresh conditioning per scored row; gradients by the complex step of that
same value), then `Obs.ahead`, `GPARRegressor.ahead` and `fit(objective="ahead")` end to end.

Sizes 1 / 2 / 31 / 32 / 33 / 63 / 64 / 65 / 130: the smallest, one below / at / one above the 32-row tile of the abar and banded kernels
(and the chunk of origins they skip by), the same around two tiles, and several tiles across a 128-wide GEMM tile.  Horizons 1 / 2 / 7 / 64 /
65 / n (those above n predict every row from the prior, as n does: they are kept for the sizes they differ at).  What is compared: value,
log-determinant, means, variances; the kernel-parameter gradients (every entry of W enters them); 1/2 diag W against the complex step on
single noise entries - all of them up to 33 rows, eight spread over the rows above; and W whole where a closed form exists (horizon 1 from
row 0: alpha alpha^T - K^-1).  The brute-force value costs n solves, its W n^2 / 2 values: the whole W by the complex step is taken at 7
rows only.  Tolerances: the parity rules (tests/test_cv_gpu.py) - values rtol 1e-10, means / variances rtol 1e-8 / atol 1e-10, W and
gradients rtol 1e-6 / atol 1e-7, trained objectives of the two training routes rtol 1e-6.
"""
import ctypes

import numpy as np
import pytest
import torch

from .conftest import make_engine
from .test_ahead import _KW, brute_force, complex_step, origins_for, ragged_origin, regressor_brute_force, regressor_data
from .test_loo_gpu import KERNELS, _library_grads, _library_kernel

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 130]
HORIZONS = [1, 2, 7, 64, 65, None]   # None: n


@pytest.fixture
def hip():
    from gpar_amd.engine import set_engine

    eng = make_engine("hip")
    previous = set_engine(eng)
    yield eng
    set_engine(previous)


_CASES = {}


def _case(name, n, origin_key, weighted=True):
    """Inputs and the brute-force reference of one case, computed once and shared by the tests (never modified)."""
    key = (name, n, origin_key, weighted)
    if key not in _CASES:
        kfun, theta = KERNELS[name]
        rng = np.random.default_rng(1000 * n + weighted)
        t = (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / max(n, 8)
        x = np.stack([t, rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)], axis=1)
        y = np.sin(5.0 * x[:, 0]) + np.cos(3.0 * x[:, 1]) + 0.5 * x[:, 2] + 0.2 * rng.standard_normal(n)
        noise = 0.05 / rng.uniform(0.5, 2.0, n) if weighted else np.full(n, 0.05)
        origin = ragged_origin(n) if origin_key == "ragged" else origins_for(n, n if origin_key is None else origin_key)

        def value(th, d):
            return brute_force(kfun(x, th) + np.diag(d) + 1e-12 * np.eye(n), y, origin)[0]

        K = kfun(x, theta) + np.diag(noise) + 1e-12 * np.eye(n)
        val, mean, var = brute_force(K, y, origin)
        grads = complex_step(lambda th: value(th, noise), theta)
        rows = np.arange(n) if n <= 33 else np.unique(np.linspace(0, n - 1, 8).astype(int))
        half = np.zeros(rows.size)
        for k, a in enumerate(rows):   # d value / d noise_a = 1/2 W_aa
            moved = noise.astype(complex)
            moved[a] += 1e-30j
            half[k] = np.imag(value(theta.astype(complex), moved)) / 1e-30
        _CASES[key] = dict(x=x, y=y, noise=noise, origin=origin, K=K, value=val, mean=mean, var=var, grads=grads, rows=rows, half=half,
                           logdet=np.linalg.slogdet(K)[1], name=name)
    return _CASES[key]


def _padded(rows, cols, pad, dev, fill=None):
    buf = torch.empty(rows, cols + pad, dtype=torch.float64, device=dev)
    if fill is not None:
        buf.fill_(fill)
    return buf[:, :cols]


def _call(hip, case, mode, pad=0, origin=None, noise=None, prefill=None):
    """One C ABI call with every buffer allocated here (leading dimensions widened by `pad`): "value", "grad", or "finish" (build + batched
    factorisation + gpar_ahead_dense_grad_finish).  Returns a dict of the outputs."""
    from gpar_amd import _lib
    from gpar_amd import hip as lib

    name = case["name"]
    ck = hip.compile(_library_kernel(name, KERNELS[name][1]), 3)
    dev = torch.device("cuda:0")
    n = len(case["y"])
    x = _padded(n, 3, pad, dev)
    x.copy_(torch.tensor(case["x"]))
    y = torch.tensor(case["y"], device=dev)
    nz = torch.tensor(case["noise"] if noise is None else noise, device=dev)
    og = torch.tensor(case["origin"] if origin is None else origin, dtype=torch.int32, device=dev)
    cdll, nacc = _lib.load(), _lib.GRAD_NACC
    z, zd = _padded(n, 3, pad, dev), _padded(n, 3, pad, dev, fill=0.0)
    A = _padded(n + 1, n + 1, pad + (n + 1) % 2, dev)
    X, W = _padded(n, n, pad + n % 2, dev), _padded(n, n, pad + n % 2, dev)
    nblocks = max(1, min(((n + 63) // 64) * ((n + 63) // 64 + 1) // 2, 1024))
    grad = mode != "value"
    nvec = int(cdll.gpar_workspace_doubles(_lib.WS_AHEAD, n, int(grad), 0))
    assert nvec == (5 * n + n % 2 + n * (n + n % 2) if grad else n)
    vec = torch.empty(nvec, dtype=torch.float64, device=dev)
    work, alpha = torch.empty(nblocks * nacc, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    out = torch.full((2 + nacc,), -7.0 if prefill else 0.0, dtype=torch.float64, device=dev)
    vectors = torch.full((3, n), -7.0 if prefill else 0.0, dtype=torch.float64, device=dev)
    info = torch.zeros(2, dtype=torch.int32, device=dev)
    stream = lib.stream_ptr(dev)
    fs, ks = ctypes.byref(ck.fspec), ctypes.byref(ck.kspec)
    ld = lib._ld
    if mode == "value":
        _lib.check(cdll.gpar_ahead_dense(fs, ks, x.data_ptr(), n, ld(x), y.data_ptr(), 1, nz.data_ptr(), 1e-12, z.data_ptr(), ld(z), A.data_ptr(), ld(A),
                                         vec.data_ptr(), out.data_ptr(), vectors[1].data_ptr(), vectors[2].data_ptr(), og.data_ptr(),
                                         info.data_ptr(), 0, stream), "gpar_ahead_dense")
    elif mode == "grad":
        _lib.check(cdll.gpar_ahead_dense_grad(fs, ks, x.data_ptr(), n, ld(x), y.data_ptr(), 1, nz.data_ptr(), 1e-12, z.data_ptr(), zd.data_ptr(), ld(z),
                                              A.data_ptr(), ld(A), X.data_ptr(), ld(X), W.data_ptr(), ld(W), alpha.data_ptr(), vec.data_ptr(),
                                              work.data_ptr(), nblocks, out.data_ptr(), vectors[0].data_ptr(), vectors[1].data_ptr(),
                                              vectors[2].data_ptr(), og.data_ptr(), info.data_ptr(), 0, stream), "gpar_ahead_dense_grad")
    else:
        logdet = torch.zeros(1, dtype=torch.float64, device=dev)
        _lib.check(cdll.gpar_logpdf_dense_build(fs, ks, x.data_ptr(), n, ld(x), y.data_ptr(), 1, nz.data_ptr(), 1e-12, z.data_ptr(), ld(z), A.data_ptr(),
                                                ld(A), logdet.data_ptr(), info.data_ptr(), stream), "build")
        _lib.check(cdll.gpar_potrf_batch(A.data_ptr(), 1, 0, n + 1, n, ld(A), logdet.data_ptr(), info.data_ptr(), 0, stream), "potrf_batch")
        _lib.check(cdll.gpar_ahead_dense_grad_finish(fs, ks, x.data_ptr(), n, ld(x), y.data_ptr(), 1, z.data_ptr(), zd.data_ptr(), ld(z), A.data_ptr(),
                                                     ld(A), logdet.data_ptr(), info.data_ptr(), X.data_ptr(), ld(X), W.data_ptr(), ld(W),
                                                     alpha.data_ptr(), vec.data_ptr(), work.data_ptr(), nblocks, out.data_ptr(),
                                                     vectors[0].data_ptr(), vectors[1].data_ptr(), vectors[2].data_ptr(), og.data_ptr(),
                                                     info[1:].data_ptr(), stream), "finish")
    torch.cuda.synchronize()
    return dict(out=out, half=vectors[0], mean=vectors[1], var=vectors[2], info=info.cpu().tolist(), W=W, ck=ck)


def _check(hip, case, got, grad):
    n = len(case["y"])
    out = got["out"].cpu().numpy()
    np.testing.assert_allclose(out[0], case["value"], rtol=1e-10)
    np.testing.assert_allclose(out[1], case["logdet"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(got["mean"].cpu().numpy(), case["mean"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(got["var"].cpu().numpy(), case["var"], rtol=1e-8, atol=1e-10)
    if not grad:
        return
    grads = _library_grads(case["name"], hip._grads_from_moments(got["ck"], out[2:], 0.5))
    print(f"  n={n}: value {out[0]:.12e} (ref {case['value']:.12e}), gradients {grads} (ref {case['grads']})")
    np.testing.assert_allclose(grads, case["grads"], rtol=1e-6, atol=1e-7)
    half = got["half"].cpu().numpy()
    np.testing.assert_allclose(half[case["rows"]], case["half"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(half, 0.5 * np.diag(got["W"].cpu().numpy()), rtol=0, atol=0)


ABI_CASES = [(n, h) for n in SIZES for h in HORIZONS if h is None or h < n or (h, n) in ((64, 64), (65, 65), (2, 2), (2, 1), (7, 2))]


@pytest.mark.parametrize("n,horizon", ABI_CASES, ids=lambda v: str(v))
def test_the_three_entries_against_the_brute_force(hip, n, horizon):
    name = "eq_linear" if (n + (horizon or 0)) % 2 == 0 else "rq_periodic"
    case = _case(name, n, horizon, weighted=n % 2 == 1)
    value_only = _call(hip, case, "value")
    assert value_only["info"] == [0, 0]
    _check(hip, case, value_only, grad=False)
    one_call = _call(hip, case, "grad")
    assert one_call["info"] == [0, 0]
    _check(hip, case, one_call, grad=True)
    if horizon == 1:   # the marginal likelihood: its value and its weights, whole
        K, y = case["K"], case["y"]
        Kinv = np.linalg.inv(K)
        alpha = Kinv @ y
        mll = -0.5 * (case["logdet"] + y @ alpha + n * np.log(2.0 * np.pi))
        np.testing.assert_allclose(one_call["out"].cpu().numpy()[0], mll, rtol=1e-10)
        il = np.tril_indices(n)
        np.testing.assert_allclose(one_call["W"].cpu().numpy()[il], (np.outer(alpha, alpha) - Kinv)[il], rtol=1e-6, atol=1e-7)
    if horizon is None:   # from the prior: mean 0, var = diag K
        np.testing.assert_allclose(one_call["mean"].cpu().numpy(), 0.0, atol=1e-10)
        np.testing.assert_allclose(one_call["var"].cpu().numpy(), np.diag(case["K"]), rtol=1e-8)


@pytest.mark.parametrize("n", [33, 130])
def test_ragged_origins_with_unscored_rows(hip, n):
    case = _case("rq_periodic", n, "ragged")
    got = _call(hip, case, "grad")
    assert got["info"] == [0, 0]
    _check(hip, case, got, grad=True)
    unscored = case["origin"] < 0
    assert unscored.any() and np.array_equal(np.isnan(got["mean"].cpu().numpy()), unscored)
    _check(hip, case, _call(hip, case, "value"), grad=False)


def test_the_whole_of_w_against_the_complex_step_on_the_entries_of_k(hip):
    """7 rows, ragged: W_ab = d value / d K_ab with K_ab and K_ba moved together (a != b), 2 d value / d K_aa on the diagonal."""
    n = 7
    case = _case("eq_linear", n, "ragged")
    W = np.zeros((n, n))
    for a in range(n):
        for b in range(a + 1):
            moved = case["K"].astype(complex)
            moved[a, b] += 1e-30j
            if a != b:
                moved[b, a] += 1e-30j
            W[a, b] = np.imag(brute_force(moved, case["y"], case["origin"])[0]) / 1e-30 * (2.0 if a == b else 1.0)
    got = _call(hip, case, "grad")["W"].cpu().numpy()
    il = np.tril_indices(n)
    np.testing.assert_allclose(got[il], W[il], rtol=1e-6, atol=1e-7)


def test_padded_leading_dimensions(hip):
    case = _case("eq_linear", 65, 7)
    got = _call(hip, case, "grad", pad=5)
    assert got["info"] == [0, 0]
    _check(hip, case, got, grad=True)
    _check(hip, case, _call(hip, case, "value", pad=3), grad=False)


def test_finish_form_gives_the_bits_of_the_one_call_form_and_two_calls_give_the_same_bits(hip):
    for n, key in ((130, 7), (65, "ragged")):
        case = _case("rq_periodic", n, key)
        first, second, finish = _call(hip, case, "grad"), _call(hip, case, "grad"), _call(hip, case, "finish")
        assert first["info"] == [0, 0] and finish["info"] == [0, 0]
        il = torch.tril_indices(n, n)
        for other in (second, finish):
            assert torch.equal(other["out"], first["out"]) and torch.equal(other["half"], first["half"])
            assert torch.equal(other["var"].nan_to_num(-1.0), first["var"].nan_to_num(-1.0))
            assert torch.equal(other["mean"].nan_to_num(-1.0), first["mean"].nan_to_num(-1.0))
            assert torch.equal(other["W"][il[0], il[1]], first["W"][il[0], il[1]])


def test_a_bad_origin_and_a_matrix_that_is_not_positive_definite_report_and_leave_the_outputs(hip):
    n = 33
    case = _case("eq_linear", n, 2)
    nacc_tail = slice(2, None)
    for mode in ("value", "grad", "finish"):
        bad = case["origin"].copy()
        bad[20], bad[25] = 21, -2   # (the first bad row is the one reported)
        got = _call(hip, case, mode, origin=bad, prefill=True)
        assert got["info"][1 if mode == "finish" else 0] == n + 1 + 20
        assert float(got["out"][0]) == -7.0 and bool((got["out"][nacc_tail] == -7.0).all())
        assert bool((got["mean"] == -7.0).all()) and bool((got["var"] == -7.0).all()) and bool((got["half"] == -7.0).all())
        noise = case["noise"].copy()
        noise[10] = -50.0   # K + D loses its positive definiteness at row 11
        got = _call(hip, case, mode, noise=noise, prefill=True)
        assert got["info"][0] == 11
        assert float(got["out"][0]) == -7.0 and bool((got["out"][nacc_tail] == -7.0).all())
        assert bool((got["mean"] == -7.0).all()) and bool((got["var"] == -7.0).all()) and bool((got["half"] == -7.0).all())


def test_fused_and_composed_routes_agree_through_obs_ahead(hip):
    from gpar_amd.gp import GP, Obs
    from gpar_amd.kernels import EQ, RQ

    n = 130
    case = _case("rq_periodic", n, 7)
    theta = KERNELS["rq_periodic"][1]
    results = {}
    for fused in (True, False):
        params = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in theta]
        kernel = RQ(params[1]).stretch(params[0]).select([0]) * EQ().stretch(params[2]).periodic(params[3]).select([1])
        noise = torch.tensor(case["noise"], device="cuda:0", requires_grad=True)
        obs = Obs(GP(kernel)(hip.tensor(case["x"]), noise), hip.tensor(case["y"]))
        with hip.defer_checks():
            if not fused:
                obs.factor()   # (a factor that exists already: the one-call entry does not apply, the composed route runs)
            value, mean, var = obs.ahead(case["origin"])
            value.backward()
        results[fused] = (float(value.detach()), mean.cpu().numpy(), var.cpu().numpy(), np.array([float(p.grad) for p in params]), noise.grad.cpu().numpy())
    a, b = results[True], results[False]
    np.testing.assert_allclose(a[0], case["value"], rtol=1e-10)
    np.testing.assert_allclose(a[0], b[0], rtol=1e-10)
    np.testing.assert_allclose(a[1], b[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(a[2], b[2], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(a[3], b[3], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(a[4], b[4], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(a[3], case["grads"], rtol=1e-6, atol=1e-7)


def test_regressor_ahead_on_the_gpu_against_the_brute_force(hip):
    from gpar_amd.regression import GPARRegressor

    n, p, horizon, start = 60, 3, 3, 5
    x, y = regressor_data(n, p, seed=11, missing=0.1)
    value, mean, var = GPARRegressor(impute=False, **_KW).ahead(x, y, horizon=horizon, start=start)
    want = regressor_brute_force(x, y, horizon, start)
    np.testing.assert_allclose(float(value), want[0], rtol=1e-10)
    np.testing.assert_allclose(mean, want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var, want[2], rtol=1e-8, atol=1e-10)


def test_fit_with_the_ahead_objective_by_the_prepared_and_the_general_route(hip):
    from gpar_amd.regression import GPARRegressor

    x, y = regressor_data(200, 2, seed=21, missing=0.0)
    finals = {}
    for fast in (True, False):
        reg = GPARRegressor(**_KW)
        reg.fast_fit = fast
        reg.condition(x, y)
        finals[fast] = reg._train(range(2), objective="ahead", horizon=2, iters=5)
    print("trained rolling-origin objectives, prepared / general:", finals[True], finals[False])
    for pi in range(2):
        np.testing.assert_allclose(finals[True][pi], finals[False][pi], rtol=1e-6)
