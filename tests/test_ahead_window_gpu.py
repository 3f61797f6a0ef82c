"""Sliding-window forecast scoring on the GPU: gpar_ahead_window_dense / gpar_ahead_window_dense_grad through the C ABI against the numpy
yardstick of tests/test_ahead_window.py (one fresh conditioning per scored row on its window alone; gradients by the complex step of that
same value), then `Obs.ahead(lo=)`, `GPARRegressor.ahead(window=)` and `fit(objective="ahead", window=)` end to end.

Sizes 1 / 2 / 31 / 32 / 33 / 64 / 65 / 66 / 130: the smallest, one below / at / one above the 32-row tile of the gather kernel, the same
around the 64-row limit of a window plus the scored row, and several tiles.  Windows 1 / 2 / 7 / 63 / 64 go through the library calls;
65 and n go through `Obs` and must take the composed route.  Horizons 1 / 7 / 65.  What is compared: value, means, variances; the
kernel-parameter gradients (every entry of W enters them); 1/2 diag W against the complex step on single noise entries - all of them up to
33 rows, eight spread over the rows above; W whole where a closed form exists or at 7 rows.  Tolerances: the parity rules
(tests/test_cv_gpu.py) - values rtol 1e-10, means / variances rtol 1e-8 / atol 1e-10, W and gradients rtol 1e-6 / atol 1e-7, trained
objectives of the two training routes rtol 1e-6.
"""
import ctypes

import numpy as np
import pytest
import torch

from .conftest import make_engine
from .test_ahead import _KW, complex_step, origins_for, regressor_data
from .test_ahead_window import regressor_window_brute_force, window_brute_force, window_starts
from .test_loo_gpu import KERNELS, _library_grads, _library_kernel

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 31, 32, 33, 64, 65, 66, 130]
WINDOWS = [1, 2, 7, 63, 64]
HORIZONS = [1, 7, 65]


@pytest.fixture
def hip():
    from gpar_amd.engine import set_engine

    eng = make_engine("hip")
    previous = set_engine(eng)
    yield eng
    set_engine(previous)


def ragged_window(n, seed=5):
    """Windows of every length up to 64 with unscored rows: origins that advance by 0 - 2 rows a row, every fourth row unscored."""
    rng = np.random.default_rng(seed)
    origin = np.minimum(np.arange(n), np.cumsum(rng.integers(0, 3, n)))
    lo = np.maximum.accumulate(np.maximum(0, origin - rng.integers(0, 65, n)))
    origin[::4] = -1
    return lo, origin


_CASES = {}


def _case(name, n, window, horizon, score="log", weighted=True):
    """Inputs and the yardstick of one case, computed once and shared by the tests (never modified).  `window` "ragged": `ragged_window`."""
    key = (name, n, window, horizon, score, weighted)
    if key not in _CASES:
        kfun, theta = KERNELS[name]
        rng = np.random.default_rng(1000 * n + weighted)
        t = (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / max(n, 8)
        x = np.stack([t, rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)], axis=1)
        y = np.sin(5.0 * x[:, 0]) + np.cos(3.0 * x[:, 1]) + 0.5 * x[:, 2] + 0.2 * rng.standard_normal(n)
        noise = 0.05 / rng.uniform(0.5, 2.0, n) if weighted else np.full(n, 0.05)
        if window == "ragged":
            lo, origin = ragged_window(n)
        else:
            lo, origin = window_starts(n, horizon, window), origins_for(n, horizon)

        def value(th, d):
            return window_brute_force(kfun(x, th) + np.diag(d) + 1e-12 * np.eye(n), y, lo, origin, score)[0]

        K = kfun(x, theta) + np.diag(noise) + 1e-12 * np.eye(n)
        val, mean, var = window_brute_force(K, y, lo, origin, score)
        grads = complex_step(lambda th: value(th, noise), theta)
        rows = np.arange(n) if n <= 33 else np.unique(np.linspace(0, n - 1, 8).astype(int))
        half = np.zeros(rows.size)
        for k, a in enumerate(rows):   # d value / d noise_a = 1/2 W_aa
            moved = noise.astype(complex)
            moved[a] += 1e-30j
            half[k] = np.imag(value(theta.astype(complex), moved)) / 1e-30
        _CASES[key] = dict(x=x, y=y, noise=noise, lo=lo, origin=origin, K=K, value=val, mean=mean, var=var, grads=grads, rows=rows, half=half,
                           name=name, score=score)
    return _CASES[key]


def _padded(rows, cols, pad, dev, fill=None):
    buf = torch.empty(rows, cols + pad, dtype=torch.float64, device=dev)
    if fill is not None:
        buf.fill_(fill)
    return buf[:, :cols]


def _call(hip, case, mode, pad=0, lo=None, origin=None, noise=None, prefill=False):
    """One C ABI call with every buffer allocated here (leading dimensions widened by `pad`): "value" or "grad".  A dict of the outputs."""
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
    lo_dev = torch.tensor(case["lo"] if lo is None else lo, dtype=torch.int32, device=dev)
    og = torch.tensor(case["origin"] if origin is None else origin, dtype=torch.int32, device=dev)
    cdll, nacc = _lib.load(), _lib.GRAD_NACC
    z, zd = _padded(n, 3, pad, dev), _padded(n, 3, pad, dev, fill=0.0)
    A = _padded(n + 1, n + 1, pad + (n + 1) % 2, dev)
    W = _padded(n, n, pad + n % 2, dev, fill=float("nan"))   # (whatever the gather kernel leaves unwritten on the lower triangle shows)
    nblocks = max(1, min(((n + 63) // 64) * ((n + 63) // 64 + 1) // 2, 1024))
    grad = mode == "grad"
    nvec = int(cdll.gpar_workspace_doubles(_lib.WS_AHEAD_WINDOW, n, int(grad), 0))
    assert nvec == ((3 + 2 * (_lib.AHEAD_WINDOW_MAX + 1)) * n if grad else n)
    vec = torch.empty(nvec, dtype=torch.float64, device=dev)
    work = torch.empty(nblocks * nacc, dtype=torch.float64, device=dev)
    out = torch.full((2 + nacc,), -7.0 if prefill else 0.0, dtype=torch.float64, device=dev)
    vectors = torch.full((3, n), -7.0 if prefill else 0.0, dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = lib.stream_ptr(dev)
    fs, ks = ctypes.byref(ck.fspec), ctypes.byref(ck.kspec)
    ld, rule = lib._ld, _lib.SCORES[case["score"]]
    if grad:
        _lib.check(cdll.gpar_ahead_window_dense_grad(fs, ks, x.data_ptr(), n, ld(x), y.data_ptr(), 1, nz.data_ptr(), 1e-12, z.data_ptr(), zd.data_ptr(),
                                                     ld(z), A.data_ptr(), ld(A), W.data_ptr(), ld(W), vec.data_ptr(), work.data_ptr(), nblocks,
                                                     out.data_ptr(), vectors[0].data_ptr(), vectors[1].data_ptr(), vectors[2].data_ptr(),
                                                     lo_dev.data_ptr(), og.data_ptr(), rule, info.data_ptr(), stream), "gpar_ahead_window_dense_grad")
    else:
        _lib.check(cdll.gpar_ahead_window_dense(fs, ks, x.data_ptr(), n, ld(x), y.data_ptr(), 1, nz.data_ptr(), 1e-12, z.data_ptr(), ld(z), A.data_ptr(),
                                                ld(A), vec.data_ptr(), out.data_ptr(), vectors[1].data_ptr(), vectors[2].data_ptr(), lo_dev.data_ptr(),
                                                og.data_ptr(), rule, info.data_ptr(), stream), "gpar_ahead_window_dense")
    torch.cuda.synchronize()
    return dict(out=out, half=vectors[0], mean=vectors[1], var=vectors[2], info=info.cpu().tolist(), W=W, ck=ck)


def _check(hip, case, got, grad):
    n = len(case["y"])
    out = got["out"].cpu().numpy()
    if grad:
        grads = _library_grads(case["name"], hip._grads_from_moments(got["ck"], out[2:], 0.5))
        print(f"  n={n}: value {out[0]:.12e} (ref {case['value']:.12e}), gradients {grads} (ref {case['grads']})")
    else:
        print(f"  n={n}: value {out[0]:.12e} (ref {case['value']:.12e})")
    np.testing.assert_allclose(out[0], case["value"], rtol=1e-10)
    assert out[1] == 0.0   # (no factor of the whole matrix: no log-determinant)
    np.testing.assert_allclose(got["mean"].cpu().numpy(), case["mean"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(got["var"].cpu().numpy(), case["var"], rtol=1e-8, atol=1e-10)
    if not grad:
        return
    np.testing.assert_allclose(grads, case["grads"], rtol=1e-6, atol=1e-7)
    half = got["half"].cpu().numpy()
    np.testing.assert_allclose(half[case["rows"]], case["half"], rtol=1e-6, atol=1e-7)
    W = got["W"].cpu().numpy()
    assert not np.isnan(W[np.tril_indices(n)]).any()   # (W is written whole, zeros outside the band)
    np.testing.assert_allclose(half, 0.5 * np.diag(W), rtol=0, atol=0)


def _abi_cases():
    cases = []
    for i, n in enumerate(SIZES):
        for j, w in enumerate(WINDOWS):
            if w > n and not (n, w) == (1, 1):
                continue
            if n >= 66:
                cases += [(n, w, h) for h in HORIZONS]
            else:
                cases.append((n, w, (1, 7)[(i + j) % 2]))
    return cases + [(2, 1, 7), (65, 64, 65)]   # (horizons that leave every window empty: the prior)


@pytest.mark.parametrize("n,window,horizon", _abi_cases(), ids=lambda v: str(v))
def test_the_two_entries_against_one_conditioning_per_row(hip, n, window, horizon):
    name = "eq_linear" if (n + window + horizon) % 2 == 0 else "rq_periodic"
    case = _case(name, n, window, horizon, weighted=n % 2 == 1)
    value_only = _call(hip, case, "value")
    assert value_only["info"] == [0]
    _check(hip, case, value_only, grad=False)
    one_call = _call(hip, case, "grad")
    assert one_call["info"] == [0]
    _check(hip, case, one_call, grad=True)
    if horizon >= n:
        np.testing.assert_allclose(one_call["mean"].cpu().numpy(), 0.0, atol=1e-10)
        np.testing.assert_allclose(one_call["var"].cpu().numpy(), np.diag(case["K"]), rtol=1e-8)


@pytest.mark.parametrize("n", [33, 66])
@pytest.mark.parametrize("score", ["log", "crps", "se"])
def test_the_three_rules(hip, n, score):
    case = _case("rq_periodic" if n == 33 else "eq_linear", n, 7, 1, score=score)
    _check(hip, case, _call(hip, case, "value"), grad=False)
    _check(hip, case, _call(hip, case, "grad"), grad=True)


@pytest.mark.parametrize("n", [33, 130])
def test_ragged_windows_with_unscored_rows(hip, n):
    case = _case("rq_periodic", n, "ragged", None)
    got = _call(hip, case, "grad")
    assert got["info"] == [0]
    _check(hip, case, got, grad=True)
    unscored = case["origin"] < 0
    assert unscored.any() and np.array_equal(np.isnan(got["mean"].cpu().numpy()), unscored)
    _check(hip, case, _call(hip, case, "value"), grad=False)


def test_lo_zero_horizon_one_gives_the_marginal_likelihood_and_its_weights(hip):
    n = 65   # (the longest window the call takes, from row 0 on: lo = 0 everywhere)
    case = _case("eq_linear", n, 64, 1)
    assert not case["lo"].any()
    got = _call(hip, case, "grad")
    K, y = case["K"], case["y"]
    Kinv = np.linalg.inv(K)
    alpha = Kinv @ y
    np.testing.assert_allclose(got["out"].cpu().numpy()[0], -0.5 * (np.linalg.slogdet(K)[1] + y @ alpha + n * np.log(2.0 * np.pi)), rtol=1e-10)
    il = np.tril_indices(n)
    np.testing.assert_allclose(got["W"].cpu().numpy()[il], (np.outer(alpha, alpha) - Kinv)[il], rtol=1e-6, atol=1e-7)


def test_the_whole_of_w_against_the_complex_step_on_the_entries_of_k(hip):
    """7 rows, ragged: W_ab = d value / d K_ab with K_ab and K_ba moved together (a != b), 2 d value / d K_aa on the diagonal."""
    n = 7
    case = _case("eq_linear", n, "ragged", None)
    W = np.zeros((n, n))
    for a in range(n):
        for b in range(a + 1):
            moved = case["K"].astype(complex)
            moved[a, b] += 1e-30j
            if a != b:
                moved[b, a] += 1e-30j
            W[a, b] = np.imag(window_brute_force(moved, case["y"], case["lo"], case["origin"])[0]) / 1e-30 * (2.0 if a == b else 1.0)
    got = _call(hip, case, "grad")["W"].cpu().numpy()
    il = np.tril_indices(n)
    np.testing.assert_allclose(got[il], W[il], rtol=1e-6, atol=1e-7)


def test_padded_leading_dimensions(hip):
    case = _case("eq_linear", 66, 7, 1)
    got = _call(hip, case, "grad", pad=5)
    assert got["info"] == [0]
    _check(hip, case, got, grad=True)
    _check(hip, case, _call(hip, case, "value", pad=3), grad=False)


def test_two_calls_give_the_same_bits(hip):
    for n, window, horizon in ((130, 63, 7), (66, "ragged", None)):
        case = _case("rq_periodic", n, window, horizon)
        first, second = _call(hip, case, "grad"), _call(hip, case, "grad")
        assert first["info"] == [0] and second["info"] == [0]
        il = torch.tril_indices(n, n)
        assert torch.equal(second["out"], first["out"]) and torch.equal(second["half"], first["half"])
        assert torch.equal(second["var"].nan_to_num(-1.0), first["var"].nan_to_num(-1.0))
        assert torch.equal(second["mean"].nan_to_num(-1.0), first["mean"].nan_to_num(-1.0))
        assert torch.equal(second["W"][il[0], il[1]], first["W"][il[0], il[1]])


def _untouched(got):
    return (float(got["out"][0]) == -7.0 and bool((got["out"][2:] == -7.0).all()) and bool((got["mean"] == -7.0).all())
            and bool((got["var"] == -7.0).all()) and bool((got["half"] == -7.0).all()))


def test_malformed_windows_report_the_first_offending_row_and_leave_the_outputs(hip):
    n = 130
    case = _case("eq_linear", n, 7, 1)
    lo, origin = case["lo"], case["origin"]   # lo = max(0, r - 7), origin = r

    def moved(array, row, to):
        out = array.copy()
        out[row] = to
        return out

    wide_lo, wide_origin = np.zeros(n, dtype=np.int64), np.minimum(np.arange(n), 65)   # (rows from 65 on: a window of 65 rows, nothing else wrong)
    kinds = {"lo > origin": (moved(moved(lo, 20, 21), 90, 95), origin, 20),
             "origin - lo = 65": (wide_lo, wide_origin, 65),
             "lo decreasing": (moved(lo, 20, 11), moved(origin, 100, 101), 20),
             "origin > r": (lo, moved(moved(origin, 20, 21), 50, -2), 20)}
    for mode in ("value", "grad"):
        for kind, (bad_lo, bad_origin, row) in kinds.items():
            got = _call(hip, case, mode, lo=bad_lo, origin=bad_origin, prefill=True)
            assert got["info"] == [n + 1 + row], (mode, kind, got["info"])
            assert _untouched(got), (mode, kind)


def test_a_block_that_is_not_positive_definite_reports_its_row(hip):
    n = 33
    case = _case("eq_linear", n, 7, 1)
    noise = case["noise"].copy()
    noise[10] = -50.0   # every block that holds row 11 of K loses its positive definiteness there
    for mode in ("value", "grad"):
        got = _call(hip, case, mode, noise=noise, prefill=True)
        assert got["info"] == [11]
        # the value, the moment sums and 1/2 diag W keep what they held (rows whose blocks are sound have written their means and variances)
        assert float(got["out"][0]) == -7.0 and bool((got["out"][2:] == -7.0).all()) and bool((got["half"] == -7.0).all())


def _through_obs(hip, case, forbid_fused):
    from gpar_amd.gp import GP, Obs
    from gpar_amd.kernels import EQ, RQ

    theta = KERNELS["rq_periodic"][1]
    params = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in theta]
    kernel = RQ(params[1]).stretch(params[0]).select([0]) * EQ().stretch(params[2]).periodic(params[3]).select([1])
    noise = torch.tensor(case["noise"], device="cuda:0", requires_grad=True)
    obs = Obs(GP(kernel)(hip.tensor(case["x"]), noise), hip.tensor(case["y"]))
    calls = []
    real = hip.ahead_window_dense_grad

    def spy(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)

    hip.ahead_window_dense_grad = spy
    try:
        with hip.defer_checks():
            value, mean, var = obs.ahead(case["origin"], lo=case["lo"])
            value.backward()
    finally:
        del hip.ahead_window_dense_grad
    assert bool(calls) != forbid_fused
    return float(value.detach()), mean.cpu().numpy(), var.cpu().numpy(), np.array([float(p.grad) for p in params]), noise.grad.cpu().numpy()


@pytest.mark.parametrize("n,window", [(130, 65), (130, 130), (66, 65), (66, 66)])
def test_longer_windows_take_the_composed_route_through_obs(hip, n, window):
    case = _case("rq_periodic", n, window, 1)
    got = _through_obs(hip, case, forbid_fused=True)
    np.testing.assert_allclose(got[0], case["value"], rtol=1e-10)
    np.testing.assert_allclose(got[1], case["mean"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(got[2], case["var"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(got[3], case["grads"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(got[4][case["rows"]], case["half"], rtol=1e-6, atol=1e-7)


def test_fused_and_composed_routes_agree_through_obs(hip):
    from gpar_amd.gp import GP, Obs

    case = _case("rq_periodic", 130, 64, 7)
    fused = _through_obs(hip, case, forbid_fused=False)
    np.testing.assert_allclose(fused[0], case["value"], rtol=1e-10)
    np.testing.assert_allclose(fused[3], case["grads"], rtol=1e-6, atol=1e-7)
    obs = Obs(GP(_library_kernel("rq_periodic", KERNELS["rq_periodic"][1]))(hip.tensor(case["x"]), hip.tensor(case["noise"])), hip.tensor(case["y"]))
    with torch.no_grad():   # (outside defer_checks no one-call form applies: the composed route)
        value, mean, var = obs.ahead(case["origin"], lo=case["lo"])
    np.testing.assert_allclose(float(value), fused[0], rtol=1e-10)
    np.testing.assert_allclose(mean.cpu().numpy(), fused[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var.cpu().numpy(), fused[2], rtol=1e-8, atol=1e-10)


def test_regressor_ahead_with_a_window_on_the_gpu(hip):
    from gpar_amd.regression import GPARRegressor

    n, p, horizon, start, window = 66, 3, 3, 5, 8
    x, y = regressor_data(n, p, seed=11, missing=0.1)
    value, mean, var = GPARRegressor(impute=False, **_KW).ahead(x, y, horizon=horizon, start=start, window=window)
    want = regressor_window_brute_force(x, y, horizon, start, window)
    np.testing.assert_allclose(float(value), want[0], rtol=1e-10)
    np.testing.assert_allclose(mean, want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var, want[2], rtol=1e-8, atol=1e-10)


def test_fit_with_a_window_by_the_prepared_and_the_general_route(hip):
    from gpar_amd.regression import GPARRegressor

    x, y = regressor_data(66, 3, seed=21, missing=0.1)
    finals = {}
    for fast in (True, False):
        reg = GPARRegressor(impute=False, **_KW)
        reg.fast_fit = fast
        reg.condition(x, y)
        finals[fast] = reg._train(range(3), objective="ahead", horizon=1, window=8, iters=5)
    print("trained sliding-window objectives, prepared / general:", finals[True], finals[False])
    for pi in range(3):
        np.testing.assert_allclose(finals[True][pi], finals[False][pi], rtol=1e-6)
    before = float(GPARRegressor(impute=False, **_KW).ahead(x, y, horizon=1, window=8)[0])
    reg = GPARRegressor(impute=False, **_KW)
    reg.fit(x, y, objective="ahead", horizon=1, window=8, iters=5)
    assert float(reg.ahead(x, y, horizon=1, window=8)[0]) > before
