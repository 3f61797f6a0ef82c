"""Rolling-origin forecast scoring: `Obs.ahead`, `GPAR.ahead`, `GPARRegressor.ahead` and `fit(objective="ahead", horizon=...)`.

The yardstick lives in this file, in numpy, and follows the definition literally: for every scored row r a fresh `np.linalg.solve`
conditioning on rows 0 ... origin[r] - 1 gives the predictive mean and variance of the noisy observation, and the value is the sum of
the Gaussian log-densities.  Gradients come from that same brute-force value by the complex step (theta_j + 1e-30 i: the solves are
analytic, so the imaginary part is the derivative to rounding).  Nothing here is computed from the code under test.  Inputs sit on a
jittered grid with unit signal and noise variance >= 1e-2, where the brute force is good to ~1e-12.  Tolerances are the project's parity
rules (tests/test_cv_gpu.py): values rtol 1e-10, means / variances rtol 1e-8 / atol 1e-10, W and gradients rtol 1e-6 / atol 1e-7, trained
objectives of two training routes rtol 1e-6.  Tests that take the `engine` fixture run the composed route on the CPU oracle here and the
fused library calls on the GPU.
"""
import numpy as np
import pytest
import torch

from gpar_amd.gp import GP, Obs
from gpar_amd.kernels import EQ, Cosine, Linear
from gpar_amd.model import rolling_origins
from gpar_amd.regression import GPARRegressor

from .conftest import to_np

_KW = dict(scale=0.5, linear=True, nonlinear=True, noise=0.1, normalise_y=False)


# ---- the numpy yardstick -------------------------------------------------------------------------------------------------------
def brute_force(K, y, origin):
    """(value, mean, var) by one fresh conditioning per scored row; works on complex K (the complex step): no conjugates anywhere."""
    n = len(y)
    mean, var = np.full(n, np.nan, dtype=K.dtype), np.full(n, np.nan, dtype=K.dtype)
    value = 0.0
    for r in range(n):
        o = int(origin[r])
        if o < 0:
            continue
        if o == 0:
            mean[r], var[r] = 0.0, K[r, r]
        else:
            sol = np.linalg.solve(K[:o, :o], np.stack([y[:o].astype(K.dtype), K[:o, r]], axis=1))
            mean[r], var[r] = K[r, :o] @ sol[:, 0], K[r, r] - K[r, :o] @ sol[:, 1]
        value = value - 0.5 * (np.log(2.0 * np.pi) + np.log(var[r]) + (y[r] - mean[r]) ** 2 / var[r])
    return value, mean, var


def complex_step(f, theta):
    """d f / d theta_j for every j by the complex step."""
    grads = np.zeros(theta.size)
    for j in range(theta.size):
        moved = theta.astype(complex)
        moved[j] += 1e-30j
        grads[j] = np.imag(f(moved)) / 1e-30
    return grads


def origins_for(n, horizon, start=0):
    return rolling_origins(np.arange(n), horizon, start)


def ragged_origin(n, seed=5):
    """Non-monotone origins with unscored rows: every third row unscored, the others anywhere in 0 ... r."""
    rng = np.random.default_rng(seed)
    o = np.array([rng.integers(0, r + 1) for r in range(n)])
    o[::3] = -1
    o[1] = 1   # (a row predicted from everything before it, as the marginal likelihood does)
    return o


def k_eq_linear(x, theta):
    s0, s1, coef = theta
    d2 = (x[:, None, 0] - x[None, :, 0]) ** 2 / s0**2 + (x[:, None, 1] - x[None, :, 1]) ** 2 / s1**2
    return np.exp(-0.5 * d2) + coef * (x @ x.T)


def k_periodic(x, theta):
    s, sp, period = theta
    r2 = (x[:, None, 0] - x[None, :, 0]) ** 2 / s**2
    u = 2.0 * np.pi * x[:, 1] / period
    e2 = ((np.sin(u)[:, None] - np.sin(u)[None, :]) ** 2 + (np.cos(u)[:, None] - np.cos(u)[None, :]) ** 2) / sp**2
    return np.exp(-0.5 * r2) * np.exp(-0.5 * e2)


def k_eq_cos(x, theta):
    """One component of a spectral mixture over both columns: EQ with scales s0, s1 times the cosine of the SUM of the differences over
    the periods T0, T1 (include/gpar_hip.h: GPAR_K_COS)."""
    s0, s1, t0, t1 = theta
    d0, d1 = x[:, None, 0] - x[None, :, 0], x[:, None, 1] - x[None, :, 1]
    return np.exp(-0.5 * (d0**2 / s0**2 + d1**2 / s1**2)) * np.cos(2.0 * np.pi * (d0 / t0 + d1 / t1))


def spectral_terms(xs, periods, scale):
    """What GPARRegressor(spectral=len(periods), spectral_period=periods, spectral_scale=scale) adds to every layer's kernel over the
    inputs xs at its initial values: sum_q (1 / Q) EQ(scale) cos(2 pi sum_d (x_d - x'_d) / periods[q])."""
    d = xs[:, None, :] - xs[None, :, :]
    envelope = np.exp(-0.5 * (d**2).sum(-1) / scale**2)
    return sum(envelope * np.cos(2.0 * np.pi * d.sum(-1) / t) for t in periods) / len(periods)


THETA = {"eq_linear": np.array([0.5, 0.7, 0.3]), "periodic": np.array([0.6, 0.8, 1.3]), "eq_cos": np.array([0.5, 0.7, 0.45, 1.3])}
KFUN = {"eq_linear": k_eq_linear, "periodic": k_periodic, "eq_cos": k_eq_cos}
SPECTRAL = dict(spectral=2, spectral_period=(0.7, 0.31), spectral_scale=0.8)


def library_kernel(name, params):
    if name == "eq_linear":
        return EQ().stretch(params[:2]).select([0, 1]) + params[2] * Linear().select([0, 1])
    if name == "eq_cos":   # (params: floats, or tensors that carry gradients)
        stack = torch.stack if torch.is_tensor(params[0]) else np.array
        return EQ().stretch(stack(list(params[:2]))).select([0, 1]) * Cosine().stretch(stack(list(params[2:4]))).select([0, 1])
    return EQ().stretch(params[0]).select([0]) * EQ().stretch(params[1]).periodic(params[2]).select([1])


def layer_data(n, seed=3):
    """Time on a jittered grid in the first column, a second input; unit signal, noise variance 0.02 - 0.08."""
    rng = np.random.default_rng(seed)
    t = (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / n
    x = np.stack([t, rng.uniform(0.0, 1.0, n)], axis=1)
    y = np.sin(6.0 * t) + 0.5 * x[:, 1] + 0.2 * rng.standard_normal(n)
    noise = 0.04 / rng.uniform(0.5, 2.0, n)
    return x, y, noise


def _obs(engine, name, params, x, y, noise):
    return Obs(GP(library_kernel(name, params))(engine.tensor(x), noise), engine.tensor(y))


N = 40


@pytest.mark.parametrize("which", ["h1", "h3", "hn", "hn5", "ragged"])
def test_value_means_and_variances_against_the_brute_force(engine, which):
    x, y, noise = layer_data(N)
    origin = ragged_origin(N) if which == "ragged" else origins_for(N, {"h1": 1, "h3": 3, "hn": N, "hn5": N + 5}[which])
    K = k_eq_linear(x, THETA["eq_linear"]) + np.diag(noise) + 1e-12 * np.eye(N)
    want = brute_force(K, y, origin)
    with torch.no_grad():
        value, mean, var = _obs(engine, "eq_linear", THETA["eq_linear"], x, y, engine.tensor(noise)).ahead(origin)
    np.testing.assert_allclose(float(value), want[0], rtol=1e-10)
    np.testing.assert_allclose(to_np(mean), want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(to_np(var), want[2], rtol=1e-8, atol=1e-10)
    assert np.array_equal(np.isnan(to_np(mean)), origin < 0) and np.array_equal(np.isnan(to_np(var)), origin < 0)
    if which in ("hn", "hn5"):   # every row from the prior: mean 0, var = diag K
        np.testing.assert_allclose(to_np(mean), 0.0, atol=1e-10)
        np.testing.assert_allclose(to_np(var), np.diag(K), rtol=1e-8)


def test_horizon_one_from_the_first_row_is_logpdf_and_its_weights_are_those_of_the_marginal_likelihood(engine):
    x, y, noise = layer_data(N)
    theta = THETA["eq_linear"]
    K = k_eq_linear(x, theta) + np.diag(noise) + 1e-12 * np.eye(N)
    obs = _obs(engine, "eq_linear", theta, x, y, engine.tensor(noise))
    with torch.no_grad():
        value = obs.ahead(origins_for(N, 1))[0]
        logpdf = _obs(engine, "eq_linear", theta, x, y, engine.tensor(noise)).logpdf()
    np.testing.assert_allclose(float(value), float(logpdf), rtol=1e-11)
    # W = alpha alpha^T - K^-1: on the diagonal through the noise gradient 1/2 W_aa, as a whole through the composed weights
    noise_t = engine.tensor(noise).clone().requires_grad_(True)
    value = _obs(engine, "eq_linear", theta, x, y, noise_t).ahead(origins_for(N, 1))[0]
    value.backward()
    Kinv = np.linalg.inv(K)
    alpha = Kinv @ y
    W = np.outer(alpha, alpha) - Kinv
    np.testing.assert_allclose(to_np(noise_t.grad), 0.5 * np.diag(W), rtol=1e-6, atol=1e-7)
    from gpar_amd.gp import _ahead_algebra

    fac = _obs(engine, "eq_linear", theta, x, y, engine.tensor(noise)).factor()
    weights = _ahead_algebra(engine, fac.L, fac.zrow.reshape(-1), origins_for(N, 1))[4]
    got = to_np(weights(engine.tensor(Kinv)))
    il = np.tril_indices(N)
    np.testing.assert_allclose(got[il], W[il], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("name", ["eq_linear", "periodic", "eq_cos"])
@pytest.mark.parametrize("which", ["h3", "ragged"])
def test_kernel_parameter_and_noise_gradients_against_the_complex_step(engine, name, which):
    x, y, noise = layer_data(N, seed=8)
    origin = ragged_origin(N) if which == "ragged" else origins_for(N, 3, start=4)
    theta, kfun = THETA[name], KFUN[name]
    want_theta = complex_step(lambda t: brute_force(kfun(x, t) + np.diag(noise) + 1e-12 * np.eye(N), y, origin)[0], theta)
    want_noise = complex_step(lambda d: brute_force(kfun(x, theta.astype(complex)) + np.diag(d) + 1e-12 * np.eye(N), y, origin)[0], noise)
    params = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in theta]
    if name == "eq_linear":
        kernel = EQ().stretch(torch.stack(params[:2])).select([0, 1]) + params[2] * Linear().select([0, 1])
    elif name == "eq_cos":
        kernel = library_kernel(name, params)
    else:
        kernel = EQ().stretch(params[0]).select([0]) * EQ().stretch(params[1]).periodic(params[2]).select([1])
    noise_t = engine.tensor(noise).clone().requires_grad_(True)
    value = Obs(GP(kernel)(engine.tensor(x), noise_t), engine.tensor(y)).ahead(origin)[0]
    value.backward()
    got = np.array([float(p.grad) for p in params])
    print(f"{name} {which}: gradients {got} (complex step {want_theta})")
    np.testing.assert_allclose(got, want_theta, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(to_np(noise_t.grad), want_noise, rtol=1e-6, atol=1e-7)


def regressor_data(n, p, seed, missing):
    rng = np.random.default_rng(seed)
    t = (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / n
    x = t[:, None]
    cols = []
    for i in range(p):
        base = np.sin(5.0 * t + i) + (0.5 * cols[-1] if cols else 0.0)
        cols.append(base + 0.1 * rng.standard_normal(n))
    y = np.stack(cols, axis=1)
    y = (y - y.mean(0)) / y.std(0)
    if missing:
        y[rng.uniform(size=y.shape) < missing] = np.nan
    return x, y


def regressor_brute_force(x, y, horizon, start, scale=0.5, noise=0.1, spectral=None):
    """Every layer's rows, inputs [x, y_<i], covariance and origins built here, independently of the model code: rows missing at an earlier
    output never reach a later layer (`impute=False`); the origin of the row with index r is the number of the layer's rows with index
    <= r - horizon.  The kernel is the regressor's at its initial values: EQ(scale) over x, plus, behind the first layer, a linear kernel
    (scales 100) and a unit EQ over the previous outputs; `spectral` = (periods, scale): and `spectral_terms` over x in every layer."""
    n, p = y.shape
    value, mean, var = 0.0, np.full((n, p), np.nan), np.full((n, p), np.nan)
    alive = np.ones(n, dtype=bool)
    for i in range(p):
        alive = alive & ~np.isnan(y[:, i])
        rows = np.flatnonzero(alive)
        xs, ys = x[rows], y[rows][:, :i]
        K = np.exp(-0.5 * ((xs[:, None, :] - xs[None, :, :]) ** 2).sum(-1) / scale**2)
        if spectral is not None:
            K = K + spectral_terms(xs, *spectral)
        if i:
            K = K + (ys / 100.0) @ (ys / 100.0).T + np.exp(-0.5 * ((ys[:, None, :] - ys[None, :, :]) ** 2).sum(-1))
        origin = np.array([-1 if r < start else int(np.sum(rows <= r - horizon)) for r in rows])
        v, m, s = brute_force(K + (noise + 1e-12) * np.eye(len(rows)), y[rows, i], origin)
        value += v
        mean[rows, i], var[rows, i] = m, s
    return value, mean, var


def test_regressor_ahead_against_a_brute_force_that_builds_every_layer_itself(engine):
    """p = 3, n = 60, 10 % missing, horizon 3, start 5."""
    n, p, horizon, start = 60, 3, 3, 5
    x, y = regressor_data(n, p, seed=11, missing=0.1)
    reg = GPARRegressor(impute=False, **_KW)
    value, mean, var = reg.ahead(x, y, horizon=horizon, start=start)
    assert isinstance(value, np.ndarray) and mean.shape == var.shape == (n, p)
    want = regressor_brute_force(x, y, horizon, start)
    np.testing.assert_allclose(float(value), want[0], rtol=1e-10)
    np.testing.assert_allclose(mean, want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var, want[2], rtol=1e-8, atol=1e-10)
    # NaN exactly where the row does not reach the layer or is not scored
    reach = np.cumprod(~np.isnan(y), axis=1).astype(bool)
    scored = reach & (np.arange(n)[:, None] >= start)
    assert (~scored).any() and np.array_equal(np.isnan(mean), ~scored) and np.array_equal(np.isnan(var), ~scored)
    # torch inputs give a tensor value
    assert isinstance(reg.ahead(torch.tensor(x), y, horizon=horizon, start=start)[0], torch.Tensor)


def test_spectral_regressor_ahead_against_a_brute_force_that_builds_every_layer_itself(engine):
    """The same with spectral=2 (periods 0.7 and 0.31, envelopes of 0.8): value, means and variances of a spectral model."""
    n, p, horizon, start = 60, 3, 3, 5
    x, y = regressor_data(n, p, seed=11, missing=0.1)
    reg = GPARRegressor(impute=False, **_KW, **SPECTRAL)
    value, mean, var = reg.ahead(x, y, horizon=horizon, start=start)
    want = regressor_brute_force(x, y, horizon, start, spectral=(SPECTRAL["spectral_period"], SPECTRAL["spectral_scale"]))
    plain = regressor_brute_force(x, y, horizon, start)
    assert abs(want[0] - plain[0]) > 1e-3 * abs(plain[0])   # (the spectral terms are not lost in the tolerance)
    np.testing.assert_allclose(float(value), want[0], rtol=1e-10)
    np.testing.assert_allclose(mean, want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var, want[2], rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("which", ["h3", "ragged"])
def test_eq_x_cosine_value_means_and_variances_against_the_brute_force(engine, which):
    x, y, noise = layer_data(N)
    origin = ragged_origin(N) if which == "ragged" else origins_for(N, 3)
    K = k_eq_cos(x, THETA["eq_cos"]) + np.diag(noise) + 1e-12 * np.eye(N)
    want = brute_force(K, y, origin)
    with torch.no_grad():
        value, mean, var = _obs(engine, "eq_cos", THETA["eq_cos"], x, y, engine.tensor(noise)).ahead(origin)
    np.testing.assert_allclose(float(value), want[0], rtol=1e-10)
    np.testing.assert_allclose(to_np(mean), want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(to_np(var), want[2], rtol=1e-8, atol=1e-10)


def test_error_surface(oracle_engine):
    x, y = regressor_data(20, 2, seed=2, missing=0.0)
    reg = GPARRegressor(**_KW)
    for bad in (dict(horizon=0), dict(horizon=1.5), dict(start=-1), dict(start=20), dict(horizon=True)):
        with pytest.raises(ValueError):
            reg.ahead(x, y, **bad)
    with pytest.raises(ValueError, match="horizon and start belong"):
        reg.fit(x, y, objective="mll", horizon=2, iters=1)
    with pytest.raises(ValueError, match="horizon and start belong"):
        reg.fit(x, y, objective="loo", start=2, iters=1)
    with pytest.raises(ValueError, match="folds belong"):
        reg.fit(x, y, objective="ahead", folds=3, iters=1)
    with pytest.raises(NotImplementedError):
        reg.fit(x, y, objective="ahead", fix=False, iters=1)
    sparse = GPARRegressor(x_ind=np.linspace(0, 1, 5), **_KW)
    with pytest.raises(ValueError, match="inducing points"):
        sparse.ahead(x, y)
    with pytest.raises(ValueError, match="inducing points"):
        sparse.fit(x, y, objective="ahead", iters=1)
    prior = GP(EQ())
    obs = Obs(prior(oracle_engine.tensor(x), 0.1), oracle_engine.tensor(y[:, 0]))
    for bad in ([0] * 19, np.arange(20) + 1, np.full(20, -2), np.zeros(20)):
        with pytest.raises(ValueError):
            obs.ahead(bad)
    post = prior | obs
    with pytest.raises(NotImplementedError):
        Obs(post(oracle_engine.tensor(x), 0.1), oracle_engine.tensor(y[:, 0])).ahead(np.zeros(20, dtype=int))
    # a covariance that is not positive definite: the factorisation's error, as logpdf raises it
    xx = np.zeros((6, 1))
    from gpar_amd.engine import NotPositiveDefiniteError

    with pytest.raises(NotPositiveDefiniteError):
        Obs(GP(-1.0 * EQ())(oracle_engine.tensor(xx), 0.0), oracle_engine.tensor(np.ones(6))).ahead(np.zeros(6, dtype=int))


def test_fit_with_the_ahead_objective_by_the_prepared_and_the_general_route(engine):
    x, y = regressor_data(50, 2, seed=4, missing=0.0)
    finals = {}
    for fast in (True, False):
        reg = GPARRegressor(**_KW)
        reg.fast_fit = fast
        reg.condition(x, y)
        finals[fast] = reg._train(range(2), objective="ahead", horizon=2, iters=5)
    print("trained rolling-origin objectives, prepared / general:", finals[True], finals[False])
    for pi in range(2):
        np.testing.assert_allclose(finals[True][pi], finals[False][pi], rtol=1e-6)
    before = float(GPARRegressor(**_KW).ahead(x, y, horizon=2)[0])
    reg = GPARRegressor(**_KW)
    reg.fit(x, y, objective="ahead", horizon=2, iters=5)
    assert float(reg.ahead(x, y, horizon=2)[0]) > before
