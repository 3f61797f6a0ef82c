"""Multi-horizon rolling-origin forecast scoring: `ahead(horizon=(1, 4, 16))`, `Obs.ahead` with K x n origins and
`fit(objective="ahead", horizon=(...), horizon_weights=(...))`, on the CPU oracle engine (the composed route: `_ahead_algebra`'s terms and
weights summed over the horizons).

The yardstick is the brute force of tests/test_ahead.py and tests/test_scores.py - one fresh `np.linalg.solve` conditioning per scored row
and horizon, the scoring rule applied to the resulting moments in numpy, gradients by the complex step of that same value - and the
regressor's layers (rows, inputs, covariance, origins) are built here as `regressor_brute_force` builds them.  Nothing is computed from the
code under test.  n <= 40 rows, p = 3 outputs, 10 % missing values.  Tolerances: the parity rules (tests/test_ahead.py) - values rtol 1e-10,
means / variances rtol 1e-8 / atol 1e-10, W and gradients rtol 1e-6 / atol 1e-7, trained objectives of two training routes rtol 1e-6.
"""
import numpy as np
import pytest
import torch

from gpar_amd.gp import GP, Obs
from gpar_amd.kernels import EQ, Linear
from gpar_amd.regression import GPARRegressor

from .conftest import to_np
from .test_ahead import (_KW, KFUN, SPECTRAL, THETA, complex_step, layer_data, library_kernel, origins_for, ragged_origin, regressor_data,
                         spectral_terms)
from .test_scores import brute_force

N, P, START = 36, 3, 2
HORIZONS = (1, 4, 16)


def multi_brute_force(K, y, origins, weights, rule="log"):
    """(weighted value, the K values, K x n means, K x n variances): the single-horizon brute force, once per origin array."""
    parts = [brute_force(K, y, rule, o) for o in origins]
    values = np.array([p[0] for p in parts])
    return np.sum(np.asarray(weights) * values), values, np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts])


def regressor_multi_brute_force(x, y, horizons, start, rule="log", weights=None, scale=0.5, noise=0.1, spectral=None):
    """`regressor_brute_force` of tests/test_ahead.py for several horizons and any rule: every layer's rows, inputs [x, y_<i], covariance
    and origins are built here (`impute=False`: rows missing at an earlier output never reach a later layer)."""
    n, p = y.shape
    k = len(horizons)
    weights = np.ones(k) if weights is None else np.asarray(weights, dtype=float)
    values, mean, var = np.zeros(k), np.full((k, n, p), np.nan), np.full((k, n, p), np.nan)
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
        origins = [np.array([-1 if r < start else int(np.sum(rows <= r - h)) for r in rows]) for h in horizons]
        _, v, m, s = multi_brute_force(K + (noise + 1e-12) * np.eye(len(rows)), y[rows, i], origins, weights, rule)
        values += v
        mean[:, rows, i], var[:, rows, i] = m, s
    return np.sum(weights * values), values, mean, var


@pytest.fixture(scope="module")
def data():
    return regressor_data(N, P, seed=13, missing=0.1)


@pytest.mark.parametrize("rule", ["log", "crps", "se"])
def test_three_horizons_against_the_brute_force(oracle_engine, data, rule):
    x, y = data
    assert np.isnan(y).any()
    reg = GPARRegressor(impute=False, **_KW)
    value, mean, var = reg.ahead(x, y, horizon=HORIZONS, start=START, score=rule)
    want = regressor_multi_brute_force(x, y, HORIZONS, START, rule)
    assert mean.shape == var.shape == (3, N, P) and reg.ahead_values_.shape == (3,)
    np.testing.assert_allclose(float(value), want[0], rtol=1e-10)
    np.testing.assert_allclose(reg.ahead_values_, want[1], rtol=1e-10)
    for k in range(3):
        np.testing.assert_allclose(mean[k], want[2][k], rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(var[k], want[3][k], rtol=1e-8, atol=1e-10)
        assert np.array_equal(np.isnan(mean[k]), np.isnan(want[2][k]))
    # weights: the same per-horizon values, another sum
    weights = (0.5, 2.0, 1.25)
    value_w = reg.ahead(x, y, horizon=HORIZONS, start=START, score=rule, horizon_weights=weights)[0]
    np.testing.assert_allclose(float(value_w), np.sum(np.array(weights) * want[1]), rtol=1e-10)
    np.testing.assert_allclose(reg.ahead_values_, want[1], rtol=1e-10)


@pytest.mark.parametrize("rule", ["log", "crps"])
def test_three_horizons_of_a_spectral_model_against_the_brute_force(oracle_engine, data, rule):
    x, y = data
    reg = GPARRegressor(impute=False, **_KW, **SPECTRAL)
    value, mean, var = reg.ahead(x, y, horizon=HORIZONS, start=START, score=rule)
    want = regressor_multi_brute_force(x, y, HORIZONS, START, rule, spectral=(SPECTRAL["spectral_period"], SPECTRAL["spectral_scale"]))
    plain = regressor_multi_brute_force(x, y, HORIZONS, START, rule)
    assert abs(want[0] - plain[0]) > 1e-3 * abs(plain[0])
    np.testing.assert_allclose(float(value), want[0], rtol=1e-10)
    np.testing.assert_allclose(reg.ahead_values_, want[1], rtol=1e-10)
    for k in range(3):
        np.testing.assert_allclose(mean[k], want[2][k], rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(var[k], want[3][k], rtol=1e-8, atol=1e-10)


def test_the_value_is_the_weighted_sum_of_the_single_horizon_calls_and_the_order_permutes_the_outputs(oracle_engine, data):
    x, y = data
    reg = GPARRegressor(impute=False, **_KW)
    weights = np.array([1.0, 3.0, 0.25])
    single = [reg.ahead(x, y, horizon=h, start=START) for h in HORIZONS]
    assert reg.ahead_values_.shape == (1,) and float(reg.ahead_values_[0]) == float(single[-1][0])
    value, mean, var = reg.ahead(x, y, horizon=HORIZONS, start=START, horizon_weights=weights)
    np.testing.assert_allclose(float(value), sum(w * float(s[0]) for w, s in zip(weights, single)), rtol=1e-10)
    for k in range(3):
        np.testing.assert_allclose(reg.ahead_values_[k], float(single[k][0]), rtol=1e-10)
        np.testing.assert_allclose(mean[k], single[k][1], rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(var[k], single[k][2], rtol=1e-8, atol=1e-10)
    order = [2, 0, 1]   # horizons (16, 1, 4)
    value_p, mean_p, var_p = reg.ahead(x, y, horizon=[HORIZONS[j] for j in order], start=START, horizon_weights=weights[order])
    np.testing.assert_allclose(float(value_p), float(value), rtol=1e-10)
    np.testing.assert_allclose(reg.ahead_values_, [float(single[j][0]) for j in order], rtol=1e-10)
    np.testing.assert_allclose(mean_p, mean[order], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var_p, var[order], rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("horizon", [(3,), [3], np.array([3])], ids=["tuple", "list", "array"])
def test_one_horizon_as_a_sequence_is_the_scalar_call_with_an_extra_axis(oracle_engine, data, horizon):
    x, y = data
    reg = GPARRegressor(impute=False, **_KW)
    want = reg.ahead(x, y, horizon=3, start=START)
    value, mean, var = reg.ahead(x, y, horizon=horizon, start=START)
    assert mean.shape == var.shape == (1, N, P) and reg.ahead_values_.shape == (1,)
    np.testing.assert_allclose(float(value), float(want[0]), rtol=1e-10)
    np.testing.assert_allclose(reg.ahead_values_[0], float(want[0]), rtol=1e-10)
    np.testing.assert_allclose(mean[0], want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var[0], want[2], rtol=1e-8, atol=1e-10)


def test_horizons_of_at_least_n_rows_give_the_prior_for_every_horizon(oracle_engine, data):
    x, y = data
    reg = GPARRegressor(impute=False, **_KW)
    horizons = (N, N + 5, 3 * N)
    value, mean, var = reg.ahead(x, y, horizon=horizons)
    want = regressor_multi_brute_force(x, y, horizons, 0)
    np.testing.assert_allclose(float(value), want[0], rtol=1e-10)
    seen = ~np.isnan(want[2][0])
    for k in range(3):
        assert np.array_equal(np.isnan(mean[k]), ~seen)
        np.testing.assert_allclose(mean[k][seen], 0.0, atol=1e-10)
        np.testing.assert_allclose(var[k], want[3][k], rtol=1e-8, atol=1e-10)   # (the brute force's prior rows: diag K)
        np.testing.assert_allclose(reg.ahead_values_[k], want[1][0], rtol=1e-10)
    np.testing.assert_allclose(var[0][seen[:, 0], 0], 1.0 + 0.1 + 1e-12, rtol=1e-8)   # the first layer: a unit EQ and the noise


def _layer_origins(n):
    """Three origin arrays of one layer: two horizons from a start, and ragged origins with unscored rows (in that array alone)."""
    return np.stack([origins_for(n, 1, start=2), origins_for(n, 5, start=2), ragged_origin(n)])


WEIGHTS = np.array([0.5, 2.0, 1.25])


@pytest.mark.parametrize("name", ["eq_linear", "periodic", "eq_cos"])
@pytest.mark.parametrize("rule", ["log", "crps"])
def test_kernel_parameter_and_noise_gradients_against_the_complex_step(oracle_engine, name, rule):
    engine, n = oracle_engine, 40
    x, y, noise = layer_data(n, seed=8)
    origins = _layer_origins(n)
    theta, kfun = THETA[name], KFUN[name]

    def value(t, d):
        return multi_brute_force(kfun(x, t) + np.diag(d) + 1e-12 * np.eye(n), y, origins, WEIGHTS, rule)[0]

    want_theta = complex_step(lambda t: value(t, noise), theta)
    want_noise = complex_step(lambda d: value(theta.astype(complex), d), noise)
    params = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in theta]
    if name == "eq_linear":
        kernel = EQ().stretch(torch.stack(params[:2])).select([0, 1]) + params[2] * Linear().select([0, 1])
    elif name == "eq_cos":
        kernel = library_kernel(name, params)
    else:
        kernel = EQ().stretch(params[0]).select([0]) * EQ().stretch(params[1]).periodic(params[2]).select([1])
    noise_t = engine.tensor(noise).clone().requires_grad_(True)
    obs = Obs(GP(kernel)(engine.tensor(x), noise_t), engine.tensor(y))
    got_value, mean, var = obs.ahead(origins, score=rule, weights=WEIGHTS)
    want = multi_brute_force(kfun(x, theta) + np.diag(noise) + 1e-12 * np.eye(n), y, origins, WEIGHTS, rule)
    np.testing.assert_allclose(float(got_value.detach()), want[0], rtol=1e-10)
    np.testing.assert_allclose(to_np(obs._held_out_values), want[1], rtol=1e-10)
    np.testing.assert_allclose(to_np(mean), want[2], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(to_np(var), want[3], rtol=1e-8, atol=1e-10)
    got_value.backward()
    got = np.array([float(p.grad) for p in params])
    print(f"{name} {rule}: gradients {got} (complex step {want_theta})")
    np.testing.assert_allclose(got, want_theta, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(to_np(noise_t.grad), want_noise, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("rule", ["log", "crps", "se"])
def test_the_whole_of_w_against_the_complex_step_on_the_entries_of_k(oracle_engine, rule):
    """7 rows: W_ab = d value / d K_ab with K_ab and K_ba moved together (a != b), 2 d value / d K_aa on the diagonal."""
    engine, n = oracle_engine, 7
    x, y, noise = layer_data(n)
    origins = _layer_origins(n)
    K = KFUN["eq_linear"](x, THETA["eq_linear"]) + np.diag(noise) + 1e-12 * np.eye(n)
    want = np.zeros((n, n))
    for a in range(n):
        for b in range(a + 1):
            moved = K.astype(complex)
            moved[a, b] += 1e-30j
            if a != b:
                moved[b, a] += 1e-30j
            want[a, b] = np.imag(multi_brute_force(moved, y, origins, WEIGHTS, rule)[0]) / 1e-30 * (2.0 if a == b else 1.0)
    seen = []
    pass_of_the_engine = engine.kernel_grads
    engine.kernel_grads = lambda ck, xx, W, *args, **kw: (seen.append(to_np(W).copy()), pass_of_the_engine(ck, xx, W, *args, **kw))[1]
    try:
        noise_t = engine.tensor(noise).clone().requires_grad_(True)
        theta = THETA["eq_linear"]
        kernel = EQ().stretch(theta[:2]).select([0, 1]) + theta[2] * Linear().select([0, 1])
        obs = Obs(GP(kernel)(engine.tensor(x), noise_t), engine.tensor(y))
        obs.ahead(origins, score=rule, weights=WEIGHTS)[0].backward()
    finally:
        del engine.kernel_grads
    assert len(seen) == 1
    il = np.tril_indices(n)
    np.testing.assert_allclose(seen[0][il], want[il], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(to_np(noise_t.grad), 0.5 * np.diag(want), rtol=1e-6, atol=1e-7)


def test_more_horizons_than_the_fused_call_takes_go_through_the_composed_route(oracle_engine):
    """The composed route has no limit on K: ten horizons."""
    n = 24
    x, y, noise = layer_data(n)
    origins = np.stack([origins_for(n, h) for h in range(1, 11)])
    K = KFUN["eq_linear"](x, THETA["eq_linear"]) + np.diag(noise) + 1e-12 * np.eye(n)
    theta = THETA["eq_linear"]
    kernel = EQ().stretch(theta[:2]).select([0, 1]) + theta[2] * Linear().select([0, 1])
    with torch.no_grad():
        value, mean, var = Obs(GP(kernel)(oracle_engine.tensor(x), oracle_engine.tensor(noise)), oracle_engine.tensor(y)).ahead(origins)
    want = multi_brute_force(K, y, origins, np.ones(10))
    np.testing.assert_allclose(float(value), want[0], rtol=1e-10)
    np.testing.assert_allclose(to_np(mean), want[2], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(to_np(var), want[3], rtol=1e-8, atol=1e-10)


def test_fit_on_a_weighted_mix_of_horizons_by_the_prepared_and_the_general_route(oracle_engine):
    x, y = regressor_data(40, 2, seed=4, missing=0.0)
    kw = dict(objective="ahead", horizon=(1, 4), horizon_weights=(1, 2), iters=5)
    finals = {}
    for fast in (True, False):
        reg = GPARRegressor(**_KW)
        reg.fast_fit = fast
        reg.condition(x, y)
        finals[fast] = reg._train(range(2), **kw)
    print("trained two-horizon objectives, prepared / general:", finals[True], finals[False])
    for pi in range(2):
        np.testing.assert_allclose(finals[True][pi], finals[False][pi], rtol=1e-6)
    before = float(GPARRegressor(**_KW).ahead(x, y, horizon=(1, 4), horizon_weights=(1, 2))[0])
    reg = GPARRegressor(**_KW)
    reg.fit(x, y, **kw)
    after = float(reg.ahead(x, y, horizon=(1, 4), horizon_weights=(1, 2))[0])
    assert after >= before
    np.testing.assert_allclose(after, -sum(finals[True].values()), rtol=1e-6)   # (fit minimises minus the weighted value, layer by layer)


def test_greedy_order_accepts_the_keywords(oracle_engine):
    x, y = regressor_data(30, 2, seed=6, missing=0.0)
    order, values = GPARRegressor(**_KW).greedy_order(x, y, objective="ahead", horizon=(1, 4), horizon_weights=(1.0, 0.5), iters=2)
    assert sorted(order) == [0, 1] and len(values) == 2 and all(np.isfinite(values))


def test_error_surface(oracle_engine):
    x, y = regressor_data(20, 2, seed=2, missing=0.0)
    reg = GPARRegressor(**_KW)
    bad_horizons = [(), [], (1, 1), (2, 4, 2), (1, 2.0), (1, True), (0, 3), (3, -1), np.array([1.0, 2.0]), np.array([[1, 2]]), ("1", 2)]
    for bad in bad_horizons:
        with pytest.raises(ValueError):
            reg.ahead(x, y, horizon=bad)
        with pytest.raises(ValueError):
            reg.fit(x, y, objective="ahead", horizon=bad, iters=1)
    bad_weights = [(1.0,), (1.0, 2.0, 3.0), (1.0, 0.0), (1.0, -2.0), (1.0, np.inf), (1.0, np.nan), (1.0, "x"), 2.0, ((1.0, 2.0),)]
    for bad in bad_weights:
        with pytest.raises(ValueError):
            reg.ahead(x, y, horizon=(1, 4), horizon_weights=bad)
        with pytest.raises(ValueError):
            reg.fit(x, y, objective="ahead", horizon=(1, 4), horizon_weights=bad, iters=1)
    with pytest.raises(ValueError, match="sequence of horizons"):   # a scalar horizon has nothing to weigh
        reg.ahead(x, y, horizon=2, horizon_weights=(1.0,))
    with pytest.raises(ValueError, match="sequence of horizons"):
        reg.fit(x, y, objective="ahead", horizon=2, horizon_weights=(1.0,), iters=1)
    with pytest.raises(ValueError, match="sequence of horizons"):
        reg.greedy_order(x, y, objective="ahead", horizon_weights=(1.0,), iters=1)
    for objective, extra in (("mll", {}), ("loo", {}), ("cv", {"folds": 3})):
        with pytest.raises(ValueError, match="horizon_weights belong"):
            reg.fit(x, y, objective=objective, horizon_weights=(1.0, 2.0), iters=1, **extra)
    obs = Obs(GP(EQ())(oracle_engine.tensor(x), 0.1), oracle_engine.tensor(y[:, 0]))
    good = np.stack([origins_for(20, 1), origins_for(20, 3)])
    for bad in (np.zeros((2, 19), dtype=int), np.zeros((0, 20), dtype=int), np.zeros((2, 20)), np.stack([np.arange(20) + 1, np.zeros(20, dtype=int)])):
        with pytest.raises(ValueError):
            obs.ahead(bad)
    for bad in ((1.0,), (1.0, 0.0), (1.0, np.inf)):
        with pytest.raises(ValueError):
            obs.ahead(good, weights=bad)
    with pytest.raises(ValueError, match="weights belong"):
        obs.ahead(good[0], weights=(1.0,))
