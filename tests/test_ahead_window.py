"""Sliding-window forecast scoring: `Obs.ahead(origin, lo=...)`, `GPAR.ahead(window=)`, `GPARRegressor.ahead(window=)` and
`fit(objective="ahead", window=...)` on the CPU oracle engine, where the composed route (`gp._ahead_window_algebra`) runs.

The yardstick lives in this file, in numpy, and follows the definition literally: for every scored row r one fresh `np.linalg.solve`
conditioning on rows lo[r] ... origin[r] - 1 ALONE gives the predictive mean and variance of the noisy observation (an empty window: the
prior), and the value is the sum of the rule's terms.  Gradients come from that same value by the complex step (the solves, erf and exp are
analytic).  Nothing here is computed from the code under test.  Inputs, kernels and helpers are those of tests/test_ahead.py.  Tolerances
are the project's parity rules (tests/test_cv_gpu.py): values rtol 1e-10, means / variances rtol 1e-8 / atol 1e-10, W and gradients rtol
1e-6 / atol 1e-7, trained objectives of the two training routes rtol 1e-6.
"""
import numpy as np
import pytest
import scipy.special
import torch

from gpar_amd.gp import GP, Obs
from gpar_amd.kernels import EQ, Linear
from gpar_amd.regression import GPARRegressor

from .conftest import to_np
from .test_ahead import (_KW, SPECTRAL, THETA, _obs, brute_force, complex_step, k_eq_cos, k_eq_linear, layer_data, library_kernel, origins_for,
                         regressor_data, spectral_terms)

N = 40


# ---- the numpy yardstick -------------------------------------------------------------------------------------------------------
def score_term(score, e, v):
    """What one scored entry adds to the value (to be maximised); works on complex arguments."""
    if score == "se":
        return -(e * e)
    if score == "crps":
        sd = np.sqrt(v)
        z = e / sd
        return -sd * (z * scipy.special.erf(z / np.sqrt(2.0)) + 2.0 * np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi) - 1.0 / np.sqrt(np.pi))
    return -0.5 * (np.log(2.0 * np.pi) + np.log(v) + e * e / v)


def window_brute_force(K, y, lo, origin, score="log"):
    """(value, mean, var) by one fresh conditioning per scored row on rows lo[r] ... origin[r] - 1; complex K allowed (no conjugates)."""
    n = len(y)
    mean, var = np.full(n, np.nan, dtype=K.dtype), np.full(n, np.nan, dtype=K.dtype)
    value = 0.0
    for r in range(n):
        o, l = int(origin[r]), int(lo[r])
        if o < 0:
            continue
        if o == l:
            mean[r], var[r] = 0.0, K[r, r]
        else:
            sol = np.linalg.solve(K[l:o, l:o], np.stack([y[l:o].astype(K.dtype), K[l:o, r]], axis=1))
            mean[r], var[r] = K[r, l:o] @ sol[:, 0], K[r, r] - K[r, l:o] @ sol[:, 1]
        value = value + score_term(score, y[r] - mean[r], var[r])
    return value, mean, var


def window_starts(n, horizon, window):
    """lo of complete data, from the definition: the number of rows with index <= r - horizon - window."""
    return np.clip(np.arange(n) - horizon - window + 1, 0, None)


def regressor_window_brute_force(x, y, horizon, start, window, scale=0.5, noise=0.1, spectral=None):
    """Every layer built here, as tests/test_ahead.py's `regressor_brute_force` builds it, with the window: the row with index r is
    predicted from the layer's rows with index in r - horizon - window + 1 ... r - horizon."""
    n, p = y.shape
    value, mean, var = 0.0, np.full((n, p), np.nan), np.full((n, p), np.nan)
    alive = np.ones(n, dtype=bool)
    for i in range(p):
        alive = alive & ~np.isnan(y[:, i])
        rows = np.flatnonzero(alive)
        xs, ys = x[rows], y[rows][:, :i]
        K = np.exp(-0.5 * ((xs[:, None, :] - xs[None, :, :]) ** 2).sum(-1) / scale**2)
        if spectral is not None:   # (periods, scale): tests/test_ahead.py's `spectral_terms` over x in every layer
            K = K + spectral_terms(xs, *spectral)
        if i:
            K = K + (ys / 100.0) @ (ys / 100.0).T + np.exp(-0.5 * ((ys[:, None, :] - ys[None, :, :]) ** 2).sum(-1))
        origin = np.array([-1 if r < start else int(np.sum(rows <= r - horizon)) for r in rows])
        lo = np.array([int(np.sum(rows <= r - horizon - window)) for r in rows])
        v, m, s = window_brute_force(K + (noise + 1e-12) * np.eye(len(rows)), y[rows, i], lo, origin)
        value += v
        mean[rows, i], var[rows, i] = m, s
    return value, mean, var


def _kernel_with_grads(theta):
    params = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in theta]
    return EQ().stretch(torch.stack(params[:2])).select([0, 1]) + params[2] * Linear().select([0, 1]), params


_CASES = [(h, w, "log") for h in (1, 3, N) for w in (1, 2, 5, N)] + [(3, 5, "crps"), (1, 2, "crps"), (3, 5, "se"), (1, 2, "se")]


@pytest.mark.parametrize("horizon,window,score", _CASES)
def test_composed_route_against_one_conditioning_per_row(oracle_engine, horizon, window, score):
    """Value, means, variances, kernel-parameter and noise gradients; start = 2."""
    x, y, noise = layer_data(N, seed=6)
    theta = THETA["eq_linear"]
    origin, lo = origins_for(N, horizon, start=2), window_starts(N, horizon, window)
    K = k_eq_linear(x, theta) + np.diag(noise) + 1e-12 * np.eye(N)
    want = window_brute_force(K, y, lo, origin, score)
    want_theta = complex_step(lambda t: window_brute_force(k_eq_linear(x, t) + np.diag(noise) + 1e-12 * np.eye(N), y, lo, origin, score)[0], theta)
    want_noise = complex_step(lambda d: window_brute_force(k_eq_linear(x, theta.astype(complex)) + np.diag(d) + 1e-12 * np.eye(N), y, lo, origin,
                                                          score)[0], noise)
    kernel, params = _kernel_with_grads(theta)
    noise_t = oracle_engine.tensor(noise).clone().requires_grad_(True)
    value, mean, var = Obs(GP(kernel)(oracle_engine.tensor(x), noise_t), oracle_engine.tensor(y)).ahead(origin, score, lo=lo)
    value.backward()
    got = np.array([float(p.grad) for p in params])
    print(f"H={horizon} W={window} {score}: value {float(value.detach()):.12e} (ref {want[0]:.12e}), gradients {got} (ref {want_theta})")
    np.testing.assert_allclose(float(value.detach()), want[0], rtol=1e-10)
    np.testing.assert_allclose(to_np(mean), want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(to_np(var), want[2], rtol=1e-8, atol=1e-10)
    assert np.array_equal(np.isnan(to_np(mean)), origin < 0) and np.array_equal(np.isnan(to_np(var)), origin < 0)
    np.testing.assert_allclose(got, want_theta, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(to_np(noise_t.grad), want_noise, rtol=1e-6, atol=1e-7)
    if horizon == N:   # every window is empty: the prior
        np.testing.assert_allclose(to_np(mean)[origin >= 0], 0.0, atol=1e-10)
        np.testing.assert_allclose(to_np(var)[origin >= 0], np.diag(K)[origin >= 0], rtol=1e-8)


@pytest.mark.parametrize("horizon,window,score", [(1, 2, "log"), (3, 5, "log"), (3, 5, "crps"), (1, N, "se")])
def test_composed_route_with_an_eq_x_cosine_kernel_against_one_conditioning_per_row(oracle_engine, horizon, window, score):
    """As above with one spectral-mixture component, EQ x cosine of the sum over both columns: value, means, variances, the gradients of
    the envelope's scales and the cosine's periods, and the noise gradient; start = 2."""
    x, y, noise = layer_data(N, seed=6)
    theta = THETA["eq_cos"]
    origin, lo = origins_for(N, horizon, start=2), window_starts(N, horizon, window)

    def ref(t, d):
        return window_brute_force(k_eq_cos(x, t) + np.diag(d) + 1e-12 * np.eye(N), y, lo, origin, score)

    want = ref(theta, noise)
    want_theta = complex_step(lambda t: ref(t, noise)[0], theta)
    want_noise = complex_step(lambda d: ref(theta.astype(complex), d)[0], noise)
    params = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in theta]
    noise_t = oracle_engine.tensor(noise).clone().requires_grad_(True)
    value, mean, var = Obs(GP(library_kernel("eq_cos", params))(oracle_engine.tensor(x), noise_t), oracle_engine.tensor(y)).ahead(origin, score, lo=lo)
    value.backward()
    got = np.array([float(p.grad) for p in params])
    np.testing.assert_allclose(float(value.detach()), want[0], rtol=1e-10)
    np.testing.assert_allclose(to_np(mean), want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(to_np(var), want[2], rtol=1e-8, atol=1e-10)
    assert np.max(np.abs(want_theta[2:])) > 1e-2   # (the periods matter)
    np.testing.assert_allclose(got, want_theta, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(to_np(noise_t.grad), want_noise, rtol=1e-6, atol=1e-7)


def test_ragged_windows_of_a_spectral_model_with_missing_values(oracle_engine):
    """tests below: `test_ragged_windows_with_missing_values_in_two_outputs`, with spectral=2 in every layer."""
    n, p, horizon, start, window = 60, 3, 3, 5, 5
    x, y = regressor_data(n, p, seed=11, missing=0.1)
    value, mean, var = GPARRegressor(impute=False, **_KW, **SPECTRAL).ahead(x, y, horizon=horizon, start=start, window=window)
    want = regressor_window_brute_force(x, y, horizon, start, window, spectral=(SPECTRAL["spectral_period"], SPECTRAL["spectral_scale"]))
    assert abs(want[0] - regressor_window_brute_force(x, y, horizon, start, window)[0]) > 1e-3 * abs(want[0])
    np.testing.assert_allclose(float(value), want[0], rtol=1e-10)
    np.testing.assert_allclose(mean, want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var, want[2], rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("horizon", [1, 3])
def test_a_window_of_every_row_is_the_expanding_score(oracle_engine, horizon):
    x, y, noise = layer_data(N)
    theta = THETA["eq_linear"]
    origin = origins_for(N, horizon)
    K = k_eq_linear(x, theta) + np.diag(noise) + 1e-12 * np.eye(N)
    with torch.no_grad():
        whole = _obs(oracle_engine, "eq_linear", theta, x, y, oracle_engine.tensor(noise)).ahead(origin)
        for window in (N, N + 7):
            got = _obs(oracle_engine, "eq_linear", theta, x, y, oracle_engine.tensor(noise)).ahead(origin, lo=window_starts(N, horizon, window))
            np.testing.assert_allclose(float(got[0]), float(whole[0]), rtol=1e-10)
            np.testing.assert_allclose(float(got[0]), brute_force(K, y, origin)[0], rtol=1e-10)
            np.testing.assert_allclose(to_np(got[1]), to_np(whole[1]), rtol=1e-8, atol=1e-10)
            np.testing.assert_allclose(to_np(got[2]), to_np(whole[2]), rtol=1e-8, atol=1e-10)
    reg = GPARRegressor(**_KW)
    xr, yr = regressor_data(30, 2, seed=3, missing=0.0)
    np.testing.assert_allclose(float(reg.ahead(xr, yr, horizon=horizon, window=30)[0]), float(reg.ahead(xr, yr, horizon=horizon)[0]), rtol=1e-10)


def test_every_entry_of_w_against_the_complex_step_on_the_entries_of_k(oracle_engine):
    """7 rows, horizon 1, window 3, the first row unscored: W_ab = d value / d K_ab with K_ab and K_ba moved together (a != b), twice
    d value / d K_aa on the diagonal."""
    from gpar_amd.gp import _ahead_window_algebra

    n = 7
    x, y, noise = layer_data(n, seed=2)
    K = k_eq_linear(x, THETA["eq_linear"]) + np.diag(noise) + 1e-12 * np.eye(n)
    origin, lo = origins_for(n, 1, start=1), window_starts(n, 1, 3)
    for score in ("log", "crps", "se"):
        W = np.zeros((n, n))
        for a in range(n):
            for b in range(a + 1):
                moved = K.astype(complex)
                moved[a, b] += 1e-30j
                if a != b:
                    moved[b, a] += 1e-30j
                W[a, b] = np.imag(window_brute_force(moved, y, lo, origin, score)[0]) / 1e-30 * (2.0 if a == b else 1.0)
        got = to_np(_ahead_window_algebra(oracle_engine, oracle_engine.tensor(K), oracle_engine.tensor(y), lo, origin, score)[4]())
        il = np.tril_indices(n)
        np.testing.assert_allclose(got[il], W[il], rtol=1e-6, atol=1e-7)
        assert np.count_nonzero(W[il]) < il[0].size   # (banded: entries further apart than the window are zero)


def test_lo_zero_horizon_one_gives_the_weights_of_the_marginal_likelihood(oracle_engine):
    from gpar_amd.gp import _ahead_window_algebra

    x, y, noise = layer_data(N)
    K = k_eq_linear(x, THETA["eq_linear"]) + np.diag(noise) + 1e-12 * np.eye(N)
    value, _, _, _, weights = _ahead_window_algebra(oracle_engine, oracle_engine.tensor(K), oracle_engine.tensor(y), np.zeros(N, dtype=np.int64),
                                                    origins_for(N, 1))
    Kinv = np.linalg.inv(K)
    alpha = Kinv @ y
    np.testing.assert_allclose(float(value), -0.5 * (np.linalg.slogdet(K)[1] + y @ alpha + N * np.log(2.0 * np.pi)), rtol=1e-10)
    il = np.tril_indices(N)
    np.testing.assert_allclose(to_np(weights())[il], (np.outer(alpha, alpha) - Kinv)[il], rtol=1e-6, atol=1e-7)


def test_ragged_windows_with_missing_values_in_two_outputs(oracle_engine):
    """p = 3, n = 60, 10 % missing in every output, horizon 3, window 5, start 5: every layer rebuilt here."""
    n, p, horizon, start, window = 60, 3, 3, 5, 5
    x, y = regressor_data(n, p, seed=11, missing=0.1)
    assert np.isnan(y[:, 0]).any() and np.isnan(y[:, 1]).any()
    value, mean, var = GPARRegressor(impute=False, **_KW).ahead(x, y, horizon=horizon, start=start, window=window)
    want = regressor_window_brute_force(x, y, horizon, start, window)
    np.testing.assert_allclose(float(value), want[0], rtol=1e-10)
    np.testing.assert_allclose(mean, want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var, want[2], rtol=1e-8, atol=1e-10)
    reach = np.cumprod(~np.isnan(y), axis=1).astype(bool)
    scored = reach & (np.arange(n)[:, None] >= start)   # (`start` is respected: NaN exactly where a row is unscored or does not reach)
    assert (~scored).any() and np.array_equal(np.isnan(mean), ~scored) and np.array_equal(np.isnan(var), ~scored)
    # the windowed score is not the expanding one
    assert abs(float(GPARRegressor(impute=False, **_KW).ahead(x, y, horizon=horizon, start=start)[0]) - float(value)) > 1e-3


def test_a_window_that_holds_only_missing_rows_gives_the_prior(oracle_engine):
    n = 12
    x, y = regressor_data(n, 1, seed=5, missing=0.0)
    y[[4, 5], 0] = np.nan
    value, mean, var = GPARRegressor(impute=False, **_KW).ahead(x, y, horizon=1, window=2)
    want = regressor_window_brute_force(x, y, 1, 0, 2)
    np.testing.assert_allclose(float(value), want[0], rtol=1e-10)
    # rows 0 and 6 look at nothing observed: mean 0, the prior variance 1 + noise + jitter
    np.testing.assert_allclose(mean[[0, 6], 0], 0.0, atol=1e-10)
    np.testing.assert_allclose(var[[0, 6], 0], 1.0 + 0.1 + 1e-12, rtol=1e-8)
    assert abs(mean[7, 0]) > 1e-3 and var[7, 0] < 1.0


def test_rolling_window_starts_against_a_literal_table_with_gaps():
    from gpar_amd.model import rolling_origins, rolling_window_starts

    observed = np.array([0, 1, 2, 5, 6, 9])   # rows 3, 4, 7, 8 are missing
    assert rolling_origins(observed, 1).tolist() == [0, 1, 2, 3, 4, 5]
    assert rolling_window_starts(observed, 1, 2).tolist() == [0, 0, 0, 3, 3, 5]   # (rows 5 and 9: empty windows; row 6: row 5 alone)
    assert rolling_window_starts(observed, 1, 4).tolist() == [0, 0, 0, 1, 2, 3]
    assert rolling_origins(observed, 3).tolist() == [0, 0, 0, 3, 3, 5]
    assert rolling_window_starts(observed, 3, 3).tolist() == [0, 0, 0, 0, 1, 3]
    assert rolling_window_starts(observed, 1, 100).tolist() == [0] * 6
    full = np.arange(8)
    assert rolling_window_starts(full, 2, 3).tolist() == [0, 0, 0, 0, 0, 1, 2, 3]


def test_window_none_is_the_expanding_evaluation_bit_for_bit(oracle_engine):
    x, y = regressor_data(30, 2, seed=9, missing=0.1)
    reg = GPARRegressor(impute=False, **_KW)
    for score in ("log", "crps"):
        a, b = reg.ahead(x, y, horizon=2, start=3, score=score), reg.ahead(x, y, horizon=2, start=3, score=score, window=None)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True) and np.array_equal(a[2], b[2], equal_nan=True)
    finals = []
    for kw in ({}, {"window": None}):
        reg = GPARRegressor(**_KW)
        reg.fit(x[:20], np.nan_to_num(y[:20]), objective="ahead", horizon=2, iters=3, **kw)
        finals.append(reg.vs.get_vector(reg.vs.names).copy())
    assert np.array_equal(finals[0], finals[1])


def test_error_surface(oracle_engine):
    x, y = regressor_data(20, 2, seed=2, missing=0.0)
    reg = GPARRegressor(**_KW)
    for bad in (0, -1, 1.5, True, "3"):
        with pytest.raises(ValueError, match="window"):
            reg.ahead(x, y, window=bad)
        with pytest.raises(ValueError, match="window"):
            reg.fit(x, y, objective="ahead", window=bad, iters=1)
    for objective, extra in (("mll", {}), ("loo", {}), ("cv", {"folds": 4})):
        with pytest.raises(ValueError, match="window belongs"):
            reg.fit(x, y, objective=objective, window=3, iters=1, **extra)
    with pytest.raises(ValueError, match="sequence of horizons"):
        reg.ahead(x, y, horizon=(1, 2), window=3)
    with pytest.raises(ValueError, match="sequence of horizons"):
        reg.fit(x, y, objective="ahead", horizon=[1, 2], window=3, iters=1)
    with pytest.raises(ValueError, match="sequence of horizons"):
        reg.greedy_order(x, y, objective="ahead", horizon=(1, 2), window=3, iters=1)
    with pytest.raises(NotImplementedError):
        reg.fit(x, y, objective="ahead", window=3, fix=False, iters=1)
    sparse = GPARRegressor(x_ind=np.linspace(0, 1, 5), **_KW)
    with pytest.raises(ValueError, match="inducing points"):
        sparse.ahead(x, y, window=3)
    with pytest.raises(ValueError, match="inducing points"):
        sparse.fit(x, y, objective="ahead", window=3, iters=1)
    obs = Obs(GP(EQ())(oracle_engine.tensor(x), 0.1), oracle_engine.tensor(y[:, 0]))
    origin = origins_for(20, 1)
    for bad in (origin + 1, np.full(20, -1), np.zeros(19, dtype=int), np.zeros(20), np.arange(20)[::-1].copy() // 4):
        with pytest.raises(ValueError):
            obs.ahead(origin, lo=bad)
    with pytest.raises(ValueError, match="one horizon"):
        obs.ahead(np.stack([origin, origin]), lo=np.zeros(20, dtype=int))


def test_fit_with_a_window_by_the_prepared_and_the_general_route(oracle_engine):
    x, y = regressor_data(40, 2, seed=4, missing=0.0)
    finals = {}
    for fast in (True, False):
        reg = GPARRegressor(**_KW)
        reg.fast_fit = fast
        reg.condition(x, y)
        finals[fast] = reg._train(range(2), objective="ahead", horizon=1, window=4, iters=5)
    print("trained sliding-window objectives, prepared / general:", finals[True], finals[False])
    for pi in range(2):
        np.testing.assert_allclose(finals[True][pi], finals[False][pi], rtol=1e-6)
    before = float(GPARRegressor(**_KW).ahead(x, y, horizon=1, window=4)[0])
    reg = GPARRegressor(**_KW)
    reg.fit(x, y, objective="ahead", horizon=1, window=4, iters=5)
    assert float(reg.ahead(x, y, horizon=1, window=4)[0]) > before
    order, values = GPARRegressor(**_KW).greedy_order(x, y, objective="ahead", horizon=1, window=4, iters=2)
    assert sorted(order) == [0, 1] and np.all(np.isfinite(values))
