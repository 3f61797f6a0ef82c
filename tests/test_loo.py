"""Leave-one-out cross-validation (Rasmussen & Williams 5.4.2; Sundararajan & Keerthi 2001): `Obs.loo`, `GPAR.loo`, `GPARRegressor.loo`
and `fit(objective="loo")`.

The references live in this file, in numpy: the closed form  mean_-i = y_i - alpha_i / d_i,  var_-i = 1 / d_i,
L = sum_i [1/2 log d_i - alpha_i^2 / (2 d_i)] - n/2 log 2 pi  (alpha = K^-1 y, d = diag K^-1) and brute-force deletion of each point.  At
the conditionings used here (noise 0.05 - 0.1 of a unit signal) the two agree to ~2e-14, well inside the tolerances, which are the
project's parity rules (tests/test_parity_gpu.py): values rtol 1e-10, posterior moments rtol 1e-8 / atol 1e-10, finite differences as
tests/test_matern_gpu.py.  Tests that take the `engine` fixture run on the CPU oracle here and through the library on the GPU.
"""
import numpy as np
import pytest
import torch

from gpar_amd import fastfit
from gpar_amd.gp import GP, Obs
from gpar_amd.kernels import EQ, Linear
from gpar_amd.optimise import objective_and_gradient
from gpar_amd.regression import GPARRegressor, _construct_gpar

from .conftest import to_np
from .test_fastfit import _layer_objectives

_LOG_2PI = np.log(2.0 * np.pi)


# ---- numpy references --------------------------------------------------------------------------------------------------------
def _closed_form(K, y):
    """(value, means, variances, alpha, K^-1) of leave-one-out under N(0, K)."""
    Kinv = np.linalg.inv(K)
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha, d = Kinv @ y, np.diag(Kinv)
    value = np.sum(0.5 * np.log(d) - alpha**2 / (2.0 * d)) - 0.5 * len(y) * _LOG_2PI
    return value, y - alpha / d, 1.0 / d, alpha, Kinv


def _brute_force(K, y):
    """The same by deleting one point at a time and conditioning on the rest."""
    n = len(y)
    mean, var = np.zeros(n), np.zeros(n)
    for i in range(n):
        rest = np.delete(np.arange(n), i)
        sol = np.linalg.solve(K[np.ix_(rest, rest)], np.stack([y[rest], K[rest, i]], axis=1))
        mean[i] = K[i, rest] @ sol[:, 0]
        var[i] = K[i, i] - K[i, rest] @ sol[:, 1]
    return np.sum(-0.5 * (np.log(2.0 * np.pi * var) + (y - mean) ** 2 / var)), mean, var


def _loo_weights(K, y):
    """W of dL/dtheta = 1/2 sum_ab W_ab dK_ab/dtheta."""
    _, _, _, alpha, Kinv = _closed_form(K, y)
    d = np.diag(Kinv)
    b = alpha / d
    c = 0.5 * (1.0 / d + b**2)
    u = Kinv @ b
    return np.outer(alpha, u) + np.outer(u, alpha) - 2.0 * (Kinv * c[None, :]) @ Kinv


def _eq_linear(x, scale=0.5, coef=0.3):
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1) / scale**2
    return np.exp(-0.5 * d2) + coef * (x @ x.T)


def _one_layer(n, weights, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (n, 2))
    y = np.sin(4.0 * x[:, 0]) + x[:, 1] + 0.2 * rng.standard_normal(n)
    w = rng.uniform(0.5, 2.0, n) if weights else np.ones(n)
    return x, y, w


def _data(n, p, seed, missing=0.0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (n, 2))
    cols = []
    for i in range(p):
        base = np.sin(3.0 * x[:, 0] + i) + x[:, 1] * (i + 1) / p
        if cols:
            base = base + 0.5 * cols[-1]
        cols.append(base + 0.1 * rng.standard_normal(n))
    y = np.stack(cols, axis=1)
    y = (y - y.mean(0)) / y.std(0)
    if missing:
        y[rng.uniform(size=y.shape) < missing] = np.nan
    return x, y


_KW = dict(scale=0.5, linear=True, nonlinear=True, noise=0.1, normalise_y=False)


# ---- one layer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [False, True], ids=["unit", "weighted"])
@pytest.mark.parametrize("noise", [0.05, 0.1])
@pytest.mark.parametrize("n", [7, 65])
def test_closed_form_equals_brute_force_deletion_for_one_layer(engine, n, noise, weights):
    x, y, w = _one_layer(n, weights, seed=n)
    K = _eq_linear(x) + np.diag(noise / w) + engine.epsilon * np.eye(n)
    v_brute, m_brute, s_brute = _brute_force(K, y)
    v_closed, m_closed, s_closed, _, _ = _closed_form(K, y)
    assert abs(v_closed - v_brute) <= 1e-12 * abs(v_brute)
    np.testing.assert_allclose(m_closed, m_brute, rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(s_closed, s_brute, rtol=1e-11)
    f = GP(EQ().stretch(0.5) + 0.3 * Linear())
    with torch.no_grad():
        value, mean, var = Obs(f(x, noise / w), y).loo()
    assert abs(float(value) - v_brute) <= 1e-10 * abs(v_brute)
    np.testing.assert_allclose(to_np(mean), m_brute, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(to_np(var), s_brute, rtol=1e-8, atol=1e-10)


def test_observations_of_a_posterior_process_leave_one_out_of_the_residual(engine):
    """`Obs.loo` on observations of f | (x1, y1): alpha = S^-1 (y2 - m) with m, S the posterior mean and covariance at x2."""
    x, y, _ = _one_layer(30, False, seed=13)
    (x1, y1), (x2, y2) = (x[:12], y[:12]), (x[12:], y[12:])
    K = _eq_linear(x)
    A = K[:12, :12] + (0.1 + engine.epsilon) * np.eye(12)
    m = K[12:, :12] @ np.linalg.solve(A, y1)
    S = K[12:, 12:] - K[12:, :12] @ np.linalg.solve(A, K[:12, 12:]) + (0.05 + engine.epsilon) * np.eye(18)
    v_ref, m_ref, s_ref, _, _ = _closed_form(S, y2 - m)
    f = GP(EQ().stretch(0.5) + 0.3 * Linear())
    with torch.no_grad():
        post = f | Obs(f(x1, 0.1), y1)
        value, mean, var = Obs(post(x2, 0.05), y2).loo()
    assert abs(float(value) - v_ref) <= 1e-10 * abs(v_ref)
    np.testing.assert_allclose(to_np(mean), m + m_ref, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(to_np(var), s_ref, rtol=1e-8, atol=1e-10)


# ---- the public API ----------------------------------------------------------------------------------------------------------
def test_value_is_the_sum_of_deletion_differences_of_logpdf_for_one_output(engine):
    x, y = _data(24, 1, seed=1)
    reg = GPARRegressor(**_KW)
    value, mean, var = reg.loo(x, y)
    full = float(reg.logpdf(x, y))
    want = sum(full - float(reg.logpdf(np.delete(x, i, 0), np.delete(y, i, 0))) for i in range(len(x)))
    assert isinstance(value, np.ndarray) and mean.shape == var.shape == y.shape
    assert abs(float(value) - want) <= 1e-10 * abs(want)
    assert torch.is_tensor(reg.loo(torch.tensor(x), y)[0])


def test_leaving_out_an_entry_of_the_last_output_changes_the_last_layer_only(engine):
    x, y = _data(20, 3, seed=2)
    reg = GPARRegressor(impute=False, **_KW)
    value, mean, var = reg.loo(x, y)
    last = np.sum(-0.5 * (np.log(2.0 * np.pi * var[:, 2]) + (y[:, 2] - mean[:, 2]) ** 2 / var[:, 2]))
    full = float(reg.logpdf(x, y))
    want = 0.0
    for i in range(len(x)):
        y_i = y.copy()
        y_i[i, 2] = np.nan
        want += full - float(reg.logpdf(x, y_i))
        _, mean_i, var_i = reg.loo(x, y_i) if i < 2 else (None, None, None)
        if mean_i is not None:   # the first two layers do not see the change
            np.testing.assert_array_equal(mean_i[:, :2], mean[:, :2])
            np.testing.assert_array_equal(var_i[:, :2], var[:, :2])
    assert abs(last - want) <= 1e-10 * abs(want)
    others = np.sum(-0.5 * (np.log(2.0 * np.pi * var[:, :2]) + (y[:, :2] - mean[:, :2]) ** 2 / var[:, :2]))
    assert abs(float(value) - (last + others)) <= 1e-10 * abs(float(value))


@pytest.mark.parametrize("replace", [False, True])
def test_missing_entries_are_nan_and_contribute_nothing(engine, replace):
    x, y = _data(40, 3, seed=3, missing=0.1)
    assert np.isnan(y).any()
    reg = GPARRegressor(impute=True, replace=replace, **_KW)
    value, mean, var = reg.loo(x, y)
    np.testing.assert_array_equal(np.isnan(mean), np.isnan(y))
    np.testing.assert_array_equal(np.isnan(var), np.isnan(y))
    logpdf = -0.5 * (np.log(2.0 * np.pi * var) + (y - mean) ** 2 / var)
    want = np.sum(logpdf[np.isfinite(logpdf)])
    assert abs(float(value) - want) <= 1e-10 * abs(want)


def test_first_layer_of_the_model_equals_the_numpy_closed_form_with_weights(engine):
    """Through GPAR.loo, with the noise diagonal noise / w: the default layer kernel over two inputs is EQ over both."""
    x, y = _data(30, 1, seed=4)
    w = np.random.default_rng(4).uniform(0.5, 2.0, y.shape)
    reg = GPARRegressor(scale=0.5, linear=False, nonlinear=False, noise=0.05, normalise_y=False)
    value, mean, var = reg.loo(x, y, w)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1) / 0.5**2
    K = np.exp(-0.5 * d2) + np.diag(0.05 / w[:, 0]) + engine.epsilon * np.eye(len(x))
    v_ref, m_ref, s_ref, _, _ = _closed_form(K, y[:, 0])
    assert abs(float(value) - v_ref) <= 1e-10 * abs(v_ref)
    np.testing.assert_allclose(mean[:, 0], m_ref, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var[:, 0], s_ref, rtol=1e-8, atol=1e-10)


def _spectral_first_layer(x):
    """The first layer's kernel of GPARRegressor(scale=0.5, linear=False, nonlinear=False, spectral=2, spectral_period=(0.7, 0.31),
    spectral_scale=0.8) at its initial values, in numpy: EQ(0.5) + sum_q 1/2 EQ(0.8) cos(2 pi sum_d (x_d - x'_d) / T_q)."""
    d = x[:, None, :] - x[None, :, :]
    K = np.exp(-0.5 * (d**2).sum(-1) / 0.5**2)
    return K + sum(0.5 * np.exp(-0.5 * (d**2).sum(-1) / 0.8**2) * np.cos(2.0 * np.pi * d.sum(-1) / t) for t in (0.7, 0.31))


_SPECTRAL_KW = dict(scale=0.5, linear=False, nonlinear=False, noise=0.05, normalise_y=False, spectral=2, spectral_period=(0.7, 0.31), spectral_scale=0.8)


def test_first_layer_of_a_spectral_model_equals_the_closed_form_and_the_brute_force_with_weights(engine):
    """`test_first_layer_of_the_model_equals_the_numpy_closed_form_with_weights` for a spectral model: the VALUE of loo, its means and
    variances against the dense restatement (closed form and one deletion per row)."""
    x, y = _data(30, 1, seed=4)
    w = np.random.default_rng(4).uniform(0.5, 2.0, y.shape)
    value, mean, var = GPARRegressor(**_SPECTRAL_KW).loo(x, y, w)
    K = _spectral_first_layer(x) + np.diag(0.05 / w[:, 0]) + engine.epsilon * np.eye(len(x))
    v_ref, m_ref, s_ref, _, _ = _closed_form(K, y[:, 0])
    v_brute, m_brute, s_brute = _brute_force(K, y[:, 0])
    assert abs(v_ref - v_brute) <= 1e-12 * abs(v_brute)
    assert abs(float(value) - v_brute) <= 1e-10 * abs(v_brute)
    np.testing.assert_allclose(mean[:, 0], m_brute, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var[:, 0], s_brute, rtol=1e-8, atol=1e-10)
    plain = GPARRegressor(scale=0.5, linear=False, nonlinear=False, noise=0.05, normalise_y=False).loo(x, y, w)[0]
    assert abs(float(plain) - v_brute) > 1e-3 * abs(v_brute)


# ---- gradient ----------------------------------------------------------------------------------------------------------------
def _fd(f, vector, rel_step=1e-3):
    """Fourth-order central differences, entry by entry (the helper of tests/test_matern_gpu.py)."""
    grad = np.zeros_like(vector)
    for j in range(vector.size):
        h = rel_step * max(abs(vector[j]), 1e-3)
        vals = {}
        for k in (-2, -1, 1, 2):
            moved = vector.copy()
            moved[j] += k * h
            vals[k] = f(moved)
        grad[j] = (-vals[2] + 8.0 * vals[1] - 8.0 * vals[-1] + vals[-2]) / (12.0 * h)
    return grad


@pytest.mark.parametrize("matern,spectral", [(None, None), (1.5, None), (None, 2)], ids=["eq", "matern32", "spectral2"])
def test_autograd_gradient_of_the_loo_value_against_central_differences(engine, matern, spectral):
    x, y = _data(40, 2, seed=5)
    w = np.random.default_rng(5).uniform(0.5, 2.0, y.shape)
    # (spectral: two components at periods 0.7 and 0.31 with short envelopes - periods, envelope scales and variances are differentiated)
    reg = GPARRegressor(matern=matern, **_KW, **({} if spectral is None else dict(spectral=spectral, spectral_period=(0.7, 0.31), spectral_scale=0.8)))

    def value():
        return _construct_gpar(reg, reg.vs, 2, 2).loo(x, y, w)[0]

    with torch.no_grad():
        value()
    names = reg.vs.names
    reg.vs.requires_grad(True)
    value().backward()
    got = np.concatenate([(v.grad if v.grad is not None else torch.zeros_like(v)).numpy().reshape(-1) for v in reg.vs.get_vars(*names)])
    reg.vs.requires_grad(False)
    x0 = reg.vs.get_vector(names)

    def f(vector):
        reg.vs.set_vector(vector, names)
        with torch.no_grad():
            return float(value())

    # The stencil's step is relative to the optimiser's variable, ~ -10 for a value of 0.3 between the bounds 1e-4 and 1e4, where
    # d log(value) / d variable ~ 1: the default 1e-3 moves a period by 1 % and the phase 2 pi |x - x'| / T ~ 20 by h k = 0.2, a truncation
    # error (h k)^4 / 30 ~ 5e-5 of that component - above the tolerance below.  A tenth of the step: 5e-9; rounding 1e-16 |L| / h ~ 1e-11.
    want = _fd(f, x0, rel_step=1e-3 if spectral is None else 1e-4)
    reg.vs.set_vector(x0, names)
    print(f"matern={matern} spectral={spectral}: {got.size} variables, largest |fd| {np.max(np.abs(want)):.3e}, max error {np.max(np.abs(got - want)):.2e}")
    assert np.max(np.abs(want)) > 1e-2
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6 * np.max(np.abs(want)))


def test_numpy_weights_reproduce_central_differences_of_the_numpy_value():
    """The reference of the GPU tests checks itself: 1/2 sum W o dK/dtheta against differences of L, for the EQ length scale."""
    x, y, w = _one_layer(30, True, seed=6)

    def K(scale):
        return _eq_linear(x, scale=scale) + np.diag(0.1 / w)

    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    dK = np.exp(-0.5 * d2 / 0.5**2) * d2 / 0.5**3
    got = 0.5 * np.sum(_loo_weights(K(0.5), y) * dK)
    h = 1e-5
    want = (_closed_form(K(0.5 + h), y)[0] - _closed_form(K(0.5 - h), y)[0]) / (2.0 * h)
    assert abs(got - want) <= 1e-7 * abs(want)


# ---- training ----------------------------------------------------------------------------------------------------------------
def test_fit_with_the_loo_objective_raises_the_loo_value(engine):
    x, y = _data(40, 2, seed=7)
    reg = GPARRegressor(**_KW)
    before = float(reg.loo(x, y)[0])
    reg.fit(x, y, objective="loo", iters=15)
    assert float(reg.loo(x, y)[0]) > before


def test_fit_with_the_mll_objective_is_fit_without_the_keyword(engine):
    x, y = _data(30, 2, seed=8)
    a, b = GPARRegressor(**_KW), GPARRegressor(**_KW)
    a.fit(x, y, iters=8)
    b.fit(x, y, objective="mll", iters=8)
    va, vb = a.get_variables(), b.get_variables()
    assert sorted(va) == sorted(vb)
    for name in va:
        np.testing.assert_array_equal(va[name], vb[name], err_msg=name)


def test_greedy_order_ranks_by_the_trained_loo_value(engine):
    x, y = _data(25, 2, seed=9)
    reg = GPARRegressor(**_KW)
    order, values = reg.greedy_order(x, y, objective="loo", iters=4)
    assert sorted(order) == [0, 1] and all(np.isfinite(values))
    # the first position's value is the trained leave-one-out value of that output as a single layer
    single = GPARRegressor(**_KW)
    single.fit(x, y[:, order[:1]], objective="loo", iters=4)
    assert abs(values[0] - float(single.loo(x, y[:, order[:1]])[0])) <= 1e-8 * abs(values[0])


# ---- host logic of the fast route ---------------------------------------------------------------------------------------------
class NumpyLooObjective(fastfit.DenseLayerObjective):
    """DenseLayerObjective with the device side in numpy: what the library call returns, from the closed form above."""

    def _allocate(self, ck):
        pass

    def _device_eval(self, ck, noise):
        from oracle import kernels as ok

        assert self.objective == "loo"
        spec = ok.spec_to_dict(self.kernel.resolve(self.width))
        X, y, w = self.X.numpy(), self.y.numpy(), self.w.numpy()
        K = ok.gram(spec, X, None, noise_diag=noise / w, jitter=self.eng.epsilon)
        try:
            np.linalg.cholesky(K)
        except np.linalg.LinAlgError:
            return None
        W = _loo_weights(K, y)
        return _closed_form(K, y)[0], ok.kernel_grads(spec, X, W), 0.5 * np.diag(W).copy()


@pytest.mark.parametrize("variant", ["plain", "weights", "missing"])
def test_fast_and_general_routes_agree_on_the_host_side(oracle_engine, variant, monkeypatch):
    rng = np.random.default_rng(10)
    x, y = _data(28, 3, seed=10, missing=0.15 if variant == "missing" else 0.0)
    w = rng.uniform(0.5, 2.0, y.shape) if variant == "weights" else None
    reg = GPARRegressor(scale=0.5, linear=True, nonlinear=True, rq=True, noise=0.1)
    reg.condition(x, y, w)
    real_build = fastfit.build
    monkeypatch.setattr(fastfit, "build", lambda *a, **k: real_build(*a, objective="loo", **k))
    for pi in range(reg.p):
        fast, _, x0 = _layer_objectives(reg, oracle_engine, pi, NumpyLooObjective)
        assert fast.objective == "loo" and fast.group is None
        def objective(vs, pi=pi, fast=fast):
            f, noise = _construct_gpar(reg, vs, reg.m, pi + 1).layers[pi]()
            return -Obs(f(fast.X, noise / fast.w), fast.y).loo()[0]

        general, _, _ = objective_and_gradient(objective, reg.vs, [f"{pi}/*"])
        for trial in range(2):
            xv = x0 + (0.0 if trial == 0 else 0.3 * rng.standard_normal(x0.shape))
            v_fast, g_fast = fast.fg(xv)
            v_ref, g_ref = general(xv)
            assert abs(v_fast - v_ref) <= 1e-9 * max(1.0, abs(v_ref)), (variant, pi, v_fast, v_ref)
            np.testing.assert_allclose(g_fast, g_ref, rtol=1e-6, atol=1e-7 * max(1.0, np.abs(g_ref).max()))
        reg.vs.set_vector(x0, fast.names)


def test_fit_hands_the_objective_to_the_prepared_route_and_trains_the_same_model(oracle_engine, monkeypatch):
    x, y = _data(30, 3, seed=12, missing=0.1)
    built = []
    real_build = fastfit.build

    def build(*args, **kwargs):
        built.append(real_build(*args, cls=NumpyLooObjective, **kwargs))
        return built[-1]

    monkeypatch.setattr(fastfit, "build", build)
    fast, slow = GPARRegressor(**_KW), GPARRegressor(**_KW)
    fast.fit(x, y, objective="loo", iters=6)
    assert len(built) == 3 and all(b is not None and b.objective == "loo" and b.evaluations > 0 and b.fallbacks == 0 for b in built)
    slow.fast_fit = False
    slow.fit(x, y, objective="loo", iters=6)
    assert len(built) == 3
    a, b = fast.get_variables(), slow.get_variables()
    assert sorted(a) == sorted(b)
    for name in a:
        np.testing.assert_allclose(a[name], b[name], rtol=1e-6, atol=1e-9, err_msg=name)


# ---- errors ------------------------------------------------------------------------------------------------------------------
def test_error_cases(oracle_engine):
    x, y = _data(12, 2, seed=11)
    with pytest.raises(ValueError):
        GPARRegressor(**_KW).fit(x, y, objective="elbo", iters=1)
    sparse = GPARRegressor(x_ind=x[:4], **_KW)
    with pytest.raises(ValueError):
        sparse.fit(x, y, objective="loo", iters=1)
    with pytest.raises(ValueError):
        sparse.loo(x, y)
    with pytest.raises(NotImplementedError):
        GPARRegressor(**_KW).fit(x, y, objective="loo", fix=False, iters=1)
    with pytest.raises(ValueError):
        fastfit.DenseLayerObjective(None, None, [], None, None, {}, None, None, None, objective="elbo")
