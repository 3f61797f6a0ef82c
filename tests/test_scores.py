"""Scoring rules of the held-out objectives: `score="log" | "crps" | "se"` on `Obs.loo` / `Obs.ahead`, `GPAR`, `GPARRegressor.loo` / `ahead`,
`fit(objective="loo" | "ahead", score=...)` and `greedy_order`.

The yardstick lives in this file, in numpy + `scipy.special.erf`, and follows the definitions literally: every scored row is conditioned on
afresh with `np.linalg.solve` (leave-one-out: on all other rows; rolling origins: on rows 0 ... origin[r] - 1), which gives the predictive
mean and variance of the noisy observation, and the value is the sum of the rule's terms - minus the CRPS of the Gaussian predictive
(Gneiting & Raftery 2007, eq. 21), minus the squared error.  The CRPS formula itself is checked against a quadrature of its definition.
Gradients come from that same brute-force value by the complex step (theta_j + 1e-30 i: solves, sqrt, exp and scipy's erf are analytic, so
the imaginary part is the derivative to rounding).  Nothing here is computed from the code under test.  Data and kernels are those of
tests/test_ahead.py (unit signal, noise variance >= 2e-2: the brute force is good to ~1e-12).  Tolerances are the project's parity rules
(tests/test_cv_gpu.py), which tests/test_loo.py and tests/test_ahead.py use for the log score: values rtol 1e-10, means / variances rtol
1e-8 / atol 1e-10, W and gradients rtol 1e-6 / atol 1e-7, trained objectives of two training routes rtol 1e-6.  Tests that take the
`engine` fixture run the composed route on the CPU oracle here and, under `defer_checks`, the fused library calls on the GPU.
"""
import numpy as np
import pytest
import scipy.integrate
import scipy.special
import torch

from gpar_amd.gp import GP, Obs
from gpar_amd.kernels import EQ, Linear
from gpar_amd.regression import GPARRegressor

from .conftest import to_np
from .test_ahead import _KW, KFUN, THETA, complex_step, layer_data, library_kernel, origins_for, ragged_origin, regressor_data

RULES = ("crps", "se")


# ---- the numpy yardstick -------------------------------------------------------------------------------------------------------
def rule_terms(rule, e, v):
    """What scored entries with errors e = y - mean and variances v add to the value (works on complex arguments)."""
    if rule == "se":
        return -(e * e)
    if rule == "log":
        return -0.5 * (np.log(2.0 * np.pi) + np.log(v) + e * e / v)
    sd = np.sqrt(v)
    z = e / sd
    return -sd * (z * scipy.special.erf(z / np.sqrt(2.0)) + 2.0 * np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi) - 1.0 / np.sqrt(np.pi))


def held_out_moments(K, y, origin=None):
    """(mean, var) by one fresh conditioning per scored row: on every other row (`origin` None: leave-one-out) or on rows
    0 ... origin[r] - 1 (-1: not scored, NaN).  Works on complex K: no conjugates anywhere."""
    n = len(y)
    mean, var = np.full(n, np.nan, dtype=K.dtype), np.full(n, np.nan, dtype=K.dtype)
    for r in range(n):
        if origin is None:
            given = np.delete(np.arange(n), r)
        elif origin[r] < 0:
            continue
        else:
            given = np.arange(int(origin[r]))
        if given.size == 0:
            mean[r], var[r] = 0.0, K[r, r]
            continue
        sol = np.linalg.solve(K[np.ix_(given, given)], np.stack([y[given].astype(K.dtype), K[given, r]], axis=1))
        mean[r], var[r] = K[r, given] @ sol[:, 0], K[r, r] - K[r, given] @ sol[:, 1]
    return mean, var


def brute_force(K, y, rule, origin=None):
    mean, var = held_out_moments(K, y, origin)
    scored = np.ones(len(y), dtype=bool) if origin is None else np.asarray(origin) >= 0
    return np.sum(rule_terms(rule, y[scored] - mean[scored], var[scored])), mean, var


ORIGINS = {
    "h1": lambda n: origins_for(n, 1),
    "h5": lambda n: origins_for(n, 5),
    "hn": lambda n: origins_for(n, n + 2),      # a horizon >= n: every row from the prior
    "start": lambda n: origins_for(n, 2, start=3),
    "ragged": lambda n: ragged_origin(n),        # non-monotone, every third row unscored
}


def _gram(name, x, theta, noise):
    return KFUN[name](x, theta) + np.diag(noise) + 1e-12 * np.eye(len(x))


def _obs(engine, name, params, x, y, noise):
    return Obs(GP(library_kernel(name, params))(engine.tensor(x), noise), engine.tensor(y))


def _evaluate(engine, obs, origin, **kw):
    """`loo` (`origin` None) or `ahead` without a gradient; `transient` and `defer_checks` let the GPU engine take its one-call forms."""
    obs.transient = True
    with torch.no_grad(), engine.defer_checks():
        return obs.loo(**kw) if origin is None else obs.ahead(origin, **kw)


@pytest.mark.parametrize("n,which", [(n, None) for n in (7, 33)] + [(n, w) for n in (7, 33, 65) for w in sorted(ORIGINS)], ids=lambda v: str(v))
def test_value_means_and_variances_against_the_brute_force(engine, n, which):
    x, y, noise = layer_data(n)
    origin = None if which is None else ORIGINS[which](n)
    K = _gram("eq_linear", x, THETA["eq_linear"], noise)
    mean_ref, var_ref = held_out_moments(K, y, origin)
    for rule in RULES:
        want = brute_force(K, y, rule, origin)[0]
        value, mean, var = _evaluate(engine, _obs(engine, "eq_linear", THETA["eq_linear"], x, y, engine.tensor(noise)), origin, score=rule)
        print(f"n={n} {which} {rule}: value {float(value):.12e} (brute force {want:.12e})")
        np.testing.assert_allclose(float(value), want, rtol=1e-10)
        np.testing.assert_allclose(to_np(mean), mean_ref, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(to_np(var), var_ref, rtol=1e-8, atol=1e-10)
        assert np.array_equal(np.isnan(to_np(mean)), np.isnan(mean_ref)) and np.array_equal(np.isnan(to_np(var)), np.isnan(var_ref))


@pytest.mark.parametrize("e,v", [(0.0, 0.7), (-0.9, 2.3), (1.6, 0.04)], ids=["z=0", "z=-0.59", "z=8"])
def test_crps_closed_form_against_a_quadrature_of_its_definition(engine, e, v):
    """CRPS(F, y) = int (F(t) - 1{t >= y})^2 dt for F = N(0, v), y = e: one row predicted from the prior, under a kernel with k(x, x) = v / 2
    and noise v / 2.  The quadrature (both tails split at y and at the mean, absolute tolerance 1e-13) bounds its own error below 1e-12;
    the closed form loses a few ulps: rtol 1e-10."""
    sd = np.sqrt(v)
    cdf, sf = (lambda t: scipy.special.ndtr(t / sd) ** 2), (lambda t: scipy.special.ndtr(-t / sd) ** 2)
    lo, hi = min(e, 0.0) - 40.0 * sd, max(e, 0.0) + 40.0 * sd
    kw = dict(epsabs=1e-13, epsrel=1e-13, limit=200)
    crps = scipy.integrate.quad(cdf, lo, e, points=[0.0] if lo < 0.0 < e else None, **kw)[0]
    crps += scipy.integrate.quad(sf, e, hi, points=[0.0] if e < 0.0 < hi else None, **kw)[0]
    np.testing.assert_allclose(-rule_terms("crps", e, v), crps, rtol=1e-10)
    obs = Obs(GP((0.5 * v) * EQ())(engine.tensor(np.array([[0.3]])), 0.5 * v - 1e-12), engine.tensor(np.array([e])))
    value, mean, var = _evaluate(engine, obs, np.array([0]), score="crps")
    print(f"e={e} v={v}: CRPS {-float(value):.15e} (quadrature {crps:.15e})")
    np.testing.assert_allclose(-float(value), crps, rtol=1e-10)
    np.testing.assert_allclose(to_np(var), [v], rtol=1e-12)


N = 33


@pytest.mark.parametrize("name", ["eq_linear", "periodic"])
@pytest.mark.parametrize("which", [None, "ragged", "start"], ids=["loo", "ahead-ragged", "ahead-start"])
@pytest.mark.parametrize("rule", RULES)
def test_kernel_parameter_and_noise_gradients_against_the_complex_step(engine, name, which, rule):
    x, y, noise = layer_data(N, seed=8)
    origin = None if which is None else ORIGINS[which](N)
    theta = THETA[name]
    want_theta = complex_step(lambda t: brute_force(_gram(name, x, t, noise), y, rule, origin)[0], theta)
    want_noise = complex_step(lambda d: brute_force(_gram(name, x, theta.astype(complex), d), y, rule, origin)[0], noise)
    params = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in theta]
    if name == "eq_linear":
        kernel = EQ().stretch(torch.stack(params[:2])).select([0, 1]) + params[2] * Linear().select([0, 1])
    else:
        kernel = library_kernel(name, params)
    noise_t = engine.tensor(noise).clone().requires_grad_(True)
    obs = Obs(GP(kernel)(engine.tensor(x), noise_t), engine.tensor(y))
    with engine.defer_checks():
        value = (obs.loo(score=rule) if origin is None else obs.ahead(origin, score=rule))[0]
        value.backward()
    got = np.array([float(p.grad) for p in params])
    print(f"{name} {which} {rule}: gradients {got} (complex step {want_theta})")
    np.testing.assert_allclose(got, want_theta, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(to_np(noise_t.grad), want_noise, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("which", [None, "ragged"], ids=["loo", "ahead-ragged"])
@pytest.mark.parametrize("rule", RULES)
def test_the_whole_of_w_against_the_complex_step_on_the_entries_of_k(engine, which, rule):
    """7 rows: W_ab = d value / d K_ab with K_ab and K_ba moved together (a != b), 2 d value / d K_aa on the diagonal.  W is what the
    composed route hands to the engine's weighted-sum pass (outside `defer_checks` every engine composes)."""
    n = 7
    x, y, noise = layer_data(n)
    origin = None if which is None else ORIGINS[which](n)
    K = _gram("eq_linear", x, THETA["eq_linear"], noise)
    want = np.zeros((n, n))
    for a in range(n):
        for b in range(a + 1):
            moved = K.astype(complex)
            moved[a, b] += 1e-30j
            if a != b:
                moved[b, a] += 1e-30j
            want[a, b] = np.imag(brute_force(moved, y, rule, origin)[0]) / 1e-30 * (2.0 if a == b else 1.0)
    seen = []
    pass_of_the_engine = engine.kernel_grads
    engine.kernel_grads = lambda ck, xx, W, *args, **kw: (seen.append(to_np(W).copy()), pass_of_the_engine(ck, xx, W, *args, **kw))[1]
    try:
        noise_t = engine.tensor(noise).clone().requires_grad_(True)
        obs = _obs(engine, "eq_linear", THETA["eq_linear"], x, y, noise_t)
        value = (obs.loo(score=rule) if origin is None else obs.ahead(origin, score=rule))[0]
        value.backward()
    finally:
        del engine.kernel_grads
    assert len(seen) == 1
    il = np.tril_indices(n)
    np.testing.assert_allclose(seen[0][il], want[il], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(to_np(noise_t.grad), 0.5 * np.diag(want), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("which", [None, "h5"], ids=["loo", "ahead"])
def test_the_log_score_is_the_call_without_a_score(engine, which):
    x, y, noise = layer_data(N)
    origin = None if which is None else ORIGINS[which](N)
    results = []
    for kw in ({}, {"score": "log"}):
        noise_t = engine.tensor(noise).clone().requires_grad_(True)
        obs = _obs(engine, "eq_linear", THETA["eq_linear"], x, y, noise_t)
        with engine.defer_checks():
            value, mean, var = obs.loo(**kw) if origin is None else obs.ahead(origin, **kw)
            value.backward()
        results.append((value.detach(), mean, var, noise_t.grad))
        results.append(_evaluate(engine, _obs(engine, "eq_linear", THETA["eq_linear"], x, y, engine.tensor(noise)), origin, **kw))
    for plain, scored in ((results[0], results[2]), (results[1], results[3])):
        assert len(plain) == len(scored)
        for a, b in zip(plain, scored):
            assert torch.equal(a.nan_to_num(-1.0), b.nan_to_num(-1.0))
    want = brute_force(_gram("eq_linear", x, THETA["eq_linear"], noise), y, "log", origin)[0]
    np.testing.assert_allclose(float(results[2][0]), want, rtol=1e-10)


def test_regressor_values_follow_from_the_returned_means_and_variances(engine):
    """Four outputs, 10 % missing (rows missing at an earlier output never reach a later layer), outputs not normalised: under "se" the
    value is -nansum((y - mean)^2), under "crps" minus the summed Gaussian CRPS of the returned predictives; the means and variances
    are those of the log score."""
    n, p = 40, 4
    x, y = regressor_data(n, p, seed=13, missing=0.1)
    reg = GPARRegressor(impute=False, **_KW)
    for call, kw in ((reg.loo, {}), (reg.ahead, dict(horizon=3, start=4))):
        _, mean_log, var_log = call(x, y, **kw)
        assert np.isnan(mean_log).any() and not np.isnan(mean_log).all()
        value, mean, var = call(x, y, score="se", **kw)
        assert isinstance(value, np.ndarray) and mean.shape == var.shape == (n, p)
        np.testing.assert_allclose(float(value), -np.nansum((y - mean) ** 2), rtol=1e-12)
        assert np.array_equal(mean, mean_log, equal_nan=True) and np.array_equal(var, var_log, equal_nan=True)
        value, mean, var = call(x, y, score="crps", **kw)
        scored = ~np.isnan(mean)
        np.testing.assert_allclose(float(value), np.sum(rule_terms("crps", (y - mean)[scored], var[scored])), rtol=1e-12)
        assert np.array_equal(mean, mean_log, equal_nan=True) and np.array_equal(var, var_log, equal_nan=True)
        assert isinstance(call(torch.tensor(x), y, score="crps", **kw)[0], torch.Tensor)


@pytest.mark.parametrize("objective,kw", [("loo", {}), ("ahead", dict(horizon=2))], ids=["loo", "ahead"])
def test_fit_with_the_crps_by_the_prepared_and_the_general_route(engine, objective, kw):
    x, y = regressor_data(50, 2, seed=4, missing=0.0)
    finals = {}
    for fast in (True, False):
        reg = GPARRegressor(**_KW)
        reg.fast_fit = fast
        reg.condition(x, y)
        finals[fast] = reg._train(range(2), objective=objective, score="crps", iters=5, **kw)
    print(f"trained {objective} CRPS objectives, prepared / general:", finals[True], finals[False])
    for pi in range(2):
        np.testing.assert_allclose(finals[True][pi], finals[False][pi], rtol=1e-6)
    evaluate = (lambda r: float(r.loo(x, y, score="crps")[0])) if objective == "loo" else (lambda r: float(r.ahead(x, y, score="crps", **kw)[0]))
    before = evaluate(GPARRegressor(**_KW))
    reg = GPARRegressor(**_KW)
    reg.fit(x, y, objective=objective, score="crps", iters=5, **kw)
    after = evaluate(reg)
    assert after > before
    np.testing.assert_allclose(after, -sum(finals[False].values()), rtol=1e-6)   # (fit is the general / prepared route above)


def test_greedy_order_ranks_by_the_trained_crps_value(engine):
    x, y = regressor_data(25, 2, seed=9, missing=0.0)
    reg = GPARRegressor(**_KW)
    order, values = reg.greedy_order(x, y, objective="loo", score="crps", iters=4)
    assert sorted(order) == [0, 1] and all(np.isfinite(values)) and all(v < 0.0 for v in values)   # (minus a CRPS)
    # the first position's value is minus the trained objective of that output as a single layer ...
    single = GPARRegressor(**_KW)
    single.condition(x, y[:, order[:1]])
    final = single._train([0], objective="loo", score="crps", iters=4)[0]
    assert abs(values[0] + float(final)) <= 1e-8 * abs(values[0])
    assert abs(values[0] - float(single.loo(x, y[:, order[:1]], score="crps")[0])) <= 1e-8 * abs(values[0])
    # ... and the chain's values add up to the CRPS value of the chosen chain at its trained hyper-parameters
    chain = GPARRegressor(**_KW)
    chain.vs = reg.greedy_vs_.copy()
    np.testing.assert_allclose(sum(values), float(chain.loo(x, y[:, order], score="crps")[0]), rtol=1e-8)


def test_error_surface(oracle_engine):
    x, y = regressor_data(20, 2, seed=2, missing=0.0)
    reg = GPARRegressor(**_KW)
    for bad in ("mse", "CRPS", None, 1):
        with pytest.raises(ValueError, match="score must be"):
            reg.loo(x, y, score=bad)
        with pytest.raises(ValueError, match="score must be"):
            reg.ahead(x, y, score=bad)
        with pytest.raises(ValueError, match="score must be"):
            reg.fit(x, y, objective="loo", score=bad, iters=1)
        with pytest.raises(ValueError, match="score must be"):
            reg.greedy_order(x, y, objective="loo", score=bad, iters=1)
    for rule in RULES:
        with pytest.raises(ValueError, match="no per-row scoring rule"):
            reg.fit(x, y, score=rule, iters=1)
        with pytest.raises(ValueError, match="no per-row scoring rule"):
            reg.fit(x, y, objective="cv", folds=4, score=rule, iters=1)
        with pytest.raises(ValueError, match="no per-row scoring rule"):
            reg.cv(x, y, folds=4, score=rule)
        with pytest.raises(ValueError, match="no per-row scoring rule"):
            reg.greedy_order(x, y, objective="cv", folds=4, score=rule, iters=1)
        # the restrictions of the objectives are those of the log score
        with pytest.raises(NotImplementedError):
            reg.fit(x, y, objective="loo", score=rule, fix=False, iters=1)
        sparse = GPARRegressor(x_ind=np.linspace(0, 1, 5), **_KW)
        with pytest.raises(ValueError, match="inducing points"):
            sparse.loo(x, y, score=rule)
        with pytest.raises(ValueError, match="inducing points"):
            sparse.fit(x, y, objective="ahead", score=rule, iters=1)
    reg.cv(x, y, folds=4, score="log")
    obs = Obs(GP(EQ())(oracle_engine.tensor(x), 0.1), oracle_engine.tensor(y[:, 0]))
    with pytest.raises(ValueError, match="score must be"):
        obs.loo(score="brier")
    with pytest.raises(ValueError, match="score must be"):
        obs.ahead(np.zeros(20, dtype=int), score="brier")
