"""Purged (hv-block) blocked cross-validation: `Obs.cv(starts, hold)`, `GPAR.cv(gap=)`, `GPARRegressor.cv(gap=)` and
`fit(objective="cv", folds=, gap=)`.

When fold F is held out, the `gap` rows on either side of it - G - are taken out of the conditioning set too, without being scored:
y_F is predicted from the rows outside H = F + G.  The references live in this file, in numpy.  Brute force: for every fold delete H,
condition on the rest, take the joint Gaussian of y_F - its mean, its marginal variances, its log density.  Closed form, as the issue
states it: with P = K^-1, alpha = P y, Dt = P_FF - P_FG P_GG^-1 P_GF, at = alpha_F - P_FG P_GG^-1 alpha_G:  y_F ~ N(y_F - Dt^-1 at, Dt^-1),
and the weights W = alpha u^T + u alpha^T - 2 P C P of the gradient from Sigma = P_HH^-1 (`_closed_form`).  Gradients: the complex-step
derivative of the brute-force value through the numpy kernels of tests/test_loo_gpu.py.  At the conditionings used (noise 0.05 of a
unit signal, the data of tests/test_cv_gpu.py) the two references agree to ~1e-13 (asserted at 1e-11 below); tolerances are the
project's parity rules: values rtol 1e-10, means / variances rtol 1e-8 / atol 1e-10, W and kernel gradients rtol 1e-6 / atol 1e-7, trained
objectives of the two training routes rtol 1e-6.  Tests that take the `engine` fixture run the composed route on the CPU oracle here
and go through the library on the GPU.

Cases are (n, fold size, gap), folds of equal size with the last cut short: (7, 1, 1) and (7, 3, 2); (40, 5, 3); (40, 8, 50) - every
fold from the prior; (65, 16, 24) and (66, 17, 24), whose blocks all touch an end of the data (57 and 58 rows at most); and, for the
sizes those two were meant to reach, (130, 16, 24) - |H| = 64 in the interior, the fused calls' limit - and (130, 17, 24) - |H| = 65,
which takes the composed route on every engine.
"""
import numpy as np
import pytest
import torch

from gpar_amd import fastfit
from gpar_amd.gp import GP, Obs
from gpar_amd.kernels import EQ, Cosine, Linear
from gpar_amd.model import purged_folds
from gpar_amd.regression import GPARRegressor

from .conftest import to_np
from .test_cv import _fold_starts
from .test_loo import _KW, _data
from .test_ahead import SPECTRAL, k_eq_cos, spectral_terms
from .test_loo_gpu import KERNELS

# (one spectral-mixture component over the first two of the three columns beside the kernels of tests/test_loo_gpu.py)
KERNELS = dict(KERNELS, eq_cos=(k_eq_cos, np.array([0.5, 0.7, 0.45, 1.3])))

_LOG_2PI = np.log(2.0 * np.pi)
CASES = [(7, 1, 1), (7, 3, 2), (40, 5, 3), (40, 8, 50), (65, 16, 24), (66, 17, 24), (130, 16, 24), (130, 17, 24)]
LARGEST_BLOCK = {(65, 16, 24): 57, (66, 17, 24): 58, (130, 16, 24): 64, (130, 17, 24): 65}


# ---- numpy references --------------------------------------------------------------------------------------------------------
def _extents(n, fold, gap):
    """(starts, hold_lo, hold_hi) of folds of `fold` rows (the last cut short) purged by `gap` rows on either side."""
    starts = _fold_starts(n, [fold])
    return starts, np.maximum(starts[:-1] - gap, 0), np.minimum(starts[1:] + gap, n)


def _brute_force(K, y, starts, lo, hi):
    """Delete H, condition on the rest, the joint Gaussian of y_F: (value, means, marginal variances).  K may be complex (complex step)."""
    n = len(y)
    value, mean, var = 0.0, np.zeros(n, dtype=K.dtype), np.zeros(n, dtype=K.dtype)
    for s, e, a, b in zip(starts[:-1], starts[1:], lo, hi):
        fold = np.arange(s, e)
        rest = np.concatenate([np.arange(0, a), np.arange(b, n)])
        if rest.size:
            sol = np.linalg.solve(K[np.ix_(rest, rest)], np.concatenate([y[rest, None].astype(K.dtype), K[np.ix_(rest, fold)]], axis=1))
            mu = K[np.ix_(fold, rest)] @ sol[:, 0]
            cov = K[np.ix_(fold, fold)] - K[np.ix_(fold, rest)] @ sol[:, 1:]
        else:
            mu, cov = np.zeros(e - s, dtype=K.dtype), K[np.ix_(fold, fold)]
        r = y[fold] - mu
        sign, logabs = np.linalg.slogdet(cov)
        value = value + -0.5 * (np.log(sign) + logabs + r @ np.linalg.solve(cov, r) + (e - s) * _LOG_2PI)
        mean[fold], var[fold] = mu, np.diag(cov)
    return value, mean, var


def _closed_form(K, y, starts, lo, hi):
    """(value, means, variances, W) from P = K^-1: per fold the Schur complement inside P_HH for the value, Sigma = P_HH^-1 for the weights."""
    n = len(y)
    P = np.linalg.inv(K)
    P = 0.5 * (P + P.T)
    alpha = P @ y
    value, mean, var = -0.5 * n * _LOG_2PI, np.zeros(n), np.zeros(n)
    b, C = np.zeros(n), np.zeros((n, n))
    for s, e, a, h in zip(starts[:-1], starts[1:], lo, hi):
        F, G, H = np.arange(s, e), np.concatenate([np.arange(a, s), np.arange(e, h)]), np.arange(a, h)
        Dt, at = P[np.ix_(F, F)], alpha[F]
        if G.size:
            sol = np.linalg.solve(P[np.ix_(G, G)], np.concatenate([alpha[G, None], P[np.ix_(G, F)]], axis=1))
            Dt, at = Dt - P[np.ix_(F, G)] @ sol[:, 1:], at - P[np.ix_(F, G)] @ sol[:, 0]
        Dinv = np.linalg.inv(Dt)
        bt = Dinv @ at
        mean[F], var[F] = y[F] - bt, np.diag(Dinv)
        value += 0.5 * np.linalg.slogdet(Dt)[1] - 0.5 * at @ bt
        Sigma = np.linalg.inv(P[np.ix_(H, H)])
        ev = Sigma @ alpha[H]
        f = F - a
        q = Dt @ ev[f]
        Sm = np.zeros((H.size, H.size))
        Sm[np.ix_(f, f)] = 0.5 * (Dt - np.outer(q, q))
        bh = Sigma[:, f] @ q
        b[H] += bh
        C[np.ix_(H, H)] += Sigma @ Sm @ Sigma + 0.5 * (np.outer(ev, bh) + np.outer(bh, ev))
    u = P @ b
    return value, mean, var, np.outer(alpha, u) + np.outer(u, alpha) - 2.0 * P @ C @ P


_LAYERS = {}


def layer_case(n, fold, gap, weighted, name="eq_linear"):
    """Inputs and the numpy references of one case (the data of tests/test_cv_gpu.py), computed once and never modified; the two
    references are checked against each other here, where they are made."""
    key = (n, fold, gap, weighted, name)
    if key not in _LAYERS:
        kfun, theta = KERNELS[name]
        rng = np.random.default_rng(1000 * n + weighted)
        x = rng.uniform(0.0, 1.0, (n, 3))
        y = np.sin(5.0 * x[:, 0]) + np.cos(3.0 * x[:, 1]) + 0.5 * x[:, 2] + 0.2 * rng.standard_normal(n)
        noise = 0.05 / rng.uniform(0.5, 2.0, n) if weighted else np.full(n, 0.05)
        starts, lo, hi = _extents(n, fold, gap)
        K = kfun(x, theta) + np.diag(noise) + 1e-12 * np.eye(n)
        value, mean, var = _brute_force(K, y, starts, lo, hi)
        v_closed, m_closed, s_closed, W = _closed_form(K, y, starts, lo, hi)
        assert abs(v_closed - value) <= 1e-11 * abs(value), (key, v_closed, value)
        np.testing.assert_allclose(m_closed, mean, rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(s_closed, var, rtol=1e-9)
        _LAYERS[key] = dict(x=x, y=y, noise=noise, starts=starts, lo=lo, hi=hi, K=K, value=value, mean=mean, var=var, W=W, name=name,
                            logdet=np.linalg.slogdet(K)[1])
    return _LAYERS[key]


def complex_step_grads(case):
    """(d value / d theta, d value / d noise) of the brute-force value by the complex step, once per case."""
    if "grads" not in case:
        kfun, theta = KERNELS[case["name"]]
        x, y, noise, n = case["x"], case["y"], case["noise"], len(case["y"])

        def value(t, d):
            return _brute_force(kfun(x, t) + np.diag(d) + 1e-12 * np.eye(n), y, case["starts"], case["lo"], case["hi"])[0]

        grads, dnoise = np.zeros(theta.size), np.zeros(n)
        for j in range(theta.size):
            moved = theta.astype(complex)
            moved[j] += 1e-30j
            grads[j] = np.imag(value(moved, noise)) / 1e-30
        for j in range(n):
            moved = noise.astype(complex)
            moved[j] += 1e-30j
            dnoise[j] = np.imag(value(theta.astype(complex), moved)) / 1e-30
        case["grads"], case["dnoise"] = grads, dnoise
    return case["grads"], case["dnoise"]


def eq_linear_kernel(theta):
    """The library's kernel of tests/test_loo_gpu.py's `_k_eq_linear` over parameters that may be tensors."""
    return EQ().stretch(torch.stack(list(theta[:2]))).select([0, 1]) + theta[2] * Linear().stretch(theta[3]).select([2])


def eq_cos_kernel(theta):
    return EQ().stretch(torch.stack(list(theta[:2]))).select([0, 1]) * Cosine().stretch(torch.stack(list(theta[2:4]))).select([0, 1])


def _obs(engine, case, theta=None, noise=None):
    theta = [torch.tensor(float(v), dtype=torch.float64) for v in KERNELS[case["name"]][1]] if theta is None else theta
    noise = engine.tensor(case["noise"]) if noise is None else noise
    return Obs(GP((eq_cos_kernel if case["name"] == "eq_cos" else eq_linear_kernel)(theta))(engine.tensor(case["x"]), noise), engine.tensor(case["y"]))


# ---- one layer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
@pytest.mark.parametrize("n,fold,gap", CASES, ids=lambda v: str(v))
def test_obs_cv_with_hold_against_brute_force_deletion(engine, n, fold, gap, weighted):
    case = layer_case(n, fold, gap, weighted)
    if (n, fold, gap) == (40, 8, 50):
        assert np.all(case["lo"] == 0) and np.all(case["hi"] == n)   # every fold is predicted from the prior
        np.testing.assert_allclose(case["mean"], 0.0, atol=1e-12)
    if (n, fold, gap) in LARGEST_BLOCK:
        assert int((case["hi"] - case["lo"]).max()) == LARGEST_BLOCK[(n, fold, gap)]
    with torch.no_grad():
        value, mean, var = _obs(engine, case).cv(case["starts"], (case["lo"], case["hi"]))
    print(f"n={n} fold={fold} gap={gap}: value {float(value):.12e} (brute force {case['value']:.12e})")
    np.testing.assert_allclose(float(value), case["value"], rtol=1e-10)
    np.testing.assert_allclose(to_np(mean), case["mean"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(to_np(var), case["var"], rtol=1e-8, atol=1e-10)


def test_hold_equal_to_the_folds_is_cv_bit_for_bit_through_the_regressor(engine):
    x, y = _data(33, 3, seed=41, missing=0.1)
    reg = GPARRegressor(**_KW)
    want, got = reg.cv(x, y, folds=5), reg.cv(x, y, folds=5, gap=0)
    for a, b in zip(got, want):
        assert np.array_equal(a, b, equal_nan=True)
    # through Obs: the folds' own extents as blocks give the same numbers (another route: not the same bits)
    case = layer_case(40, 5, 3, True)
    with torch.no_grad():
        a = _obs(engine, case).cv(case["starts"])
        b = _obs(engine, case).cv(case["starts"], (case["starts"][:-1], case["starts"][1:]))
    np.testing.assert_allclose(float(b[0]), float(a[0]), rtol=1e-10)
    np.testing.assert_allclose(to_np(b[1]), to_np(a[1]), rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(to_np(b[2]), to_np(a[2]), rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("gap", [1, 7, 100])
def test_one_fold_with_any_gap_is_logpdf(engine, gap):
    x, y = _data(40, 1, seed=42)
    reg = GPARRegressor(**_KW)
    value, mean, var = reg.cv(x, y, folds=1, gap=gap)
    want = float(reg.logpdf(x, y))
    assert abs(float(value) - want) <= 1e-10 * abs(want)
    np.testing.assert_allclose(mean, 0.0, atol=1e-10)


def test_folds_of_one_row_with_no_gap_are_loo_and_with_a_gap_leave_2g_plus_1_out(engine):
    x, y = _data(33, 2, seed=43, missing=0.1)
    reg = GPARRegressor(**_KW)
    want, got = reg.loo(x, y), reg.cv(x, y, folds=33, gap=0)
    assert abs(float(got[0]) - float(want[0])) <= 1e-10 * abs(float(want[0]))
    np.testing.assert_allclose(got[1], want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(got[2], want[2], rtol=1e-8, atol=1e-10)
    # leave-(2 g + 1)-out, score the middle: row r from the rows outside r - g ... r + g
    case = layer_case(40, 1, 2, False)
    K, yv, n = case["K"], case["y"], 40
    for r in (0, 1, 17, 39):
        rest = np.array([j for j in range(n) if abs(j - r) > 2])
        sol = np.linalg.solve(K[np.ix_(rest, rest)], np.stack([yv[rest], K[rest, r]], axis=1))
        assert abs(case["mean"][r] - K[r, rest] @ sol[:, 0]) <= 1e-12 and abs(case["var"][r] - (K[r, r] - K[r, rest] @ sol[:, 1])) <= 1e-12
    with torch.no_grad():
        value, mean, var = _obs(engine, case).cv(case["starts"], (case["lo"], case["hi"]))
    np.testing.assert_allclose(float(value), case["value"], rtol=1e-10)
    np.testing.assert_allclose(to_np(mean), case["mean"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(to_np(var), case["var"], rtol=1e-8, atol=1e-10)


def test_a_gap_beyond_the_data_predicts_every_fold_from_the_prior(engine):
    x, y = _data(24, 1, seed=44)
    reg = GPARRegressor(scale=0.5, linear=False, nonlinear=False, noise=0.05, normalise_y=False)
    value, mean, var = reg.cv(x, y, folds=4, gap=24)
    np.testing.assert_allclose(mean, 0.0, atol=1e-10)
    np.testing.assert_allclose(var, 1.0 + 0.05 + engine.epsilon, rtol=1e-8)   # (the prior variance of an EQ kernel, and the noise)
    K = np.exp(-0.5 * ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1) / 0.5**2) + (0.05 + engine.epsilon) * np.eye(24)
    want = 0.0
    for part in np.array_split(np.arange(24), 4):
        cov = K[np.ix_(part, part)]
        want += -0.5 * (np.linalg.slogdet(cov)[1] + y[part, 0] @ np.linalg.solve(cov, y[part, 0]) + part.size * _LOG_2PI)
    assert abs(float(value) - want) <= 1e-10 * abs(want)


# ---- gradient ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,fold,gap", [(40, 5, 3), (66, 17, 24), (130, 17, 24)], ids=lambda v: str(v))
def test_kernel_parameter_and_noise_gradients_against_the_complex_step(engine, n, fold, gap):
    case = layer_case(n, fold, gap, True)
    want_theta, want_noise = complex_step_grads(case)
    params = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in KERNELS["eq_linear"][1]]
    noise_t = engine.tensor(case["noise"]).clone().requires_grad_(True)
    obs = _obs(engine, case, params, noise_t)
    with engine.defer_checks():
        value = obs.cv(case["starts"], (case["lo"], case["hi"]))[0]
        value.backward()
    got = np.array([float(p.grad) for p in params])
    print(f"n={n} fold={fold} gap={gap}: gradients {got} (complex step {want_theta})")
    np.testing.assert_allclose(float(value), case["value"], rtol=1e-10)
    assert np.max(np.abs(want_theta)) > 1e-2
    np.testing.assert_allclose(got, want_theta, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(to_np(noise_t.grad), want_noise, rtol=1e-6, atol=1e-7)
    # the closed form's weights, the reference of the GPU tests, against the same derivatives: 1/2 diag W is d value / d noise
    np.testing.assert_allclose(0.5 * np.diag(case["W"]), want_noise, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("n,fold,gap", [(40, 5, 3), (66, 17, 24)], ids=lambda v: str(v))
def test_eq_x_cosine_value_and_gradients_against_brute_force_deletion_and_the_complex_step(engine, n, fold, gap):
    """Value, means and variances against the brute force, and the gradients of the envelope's scales, the cosine's periods and the
    noise against its complex step, for one spectral-mixture component."""
    case = layer_case(n, fold, gap, True, name="eq_cos")
    want_theta, want_noise = complex_step_grads(case)
    params = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in KERNELS["eq_cos"][1]]
    noise_t = engine.tensor(case["noise"]).clone().requires_grad_(True)
    with engine.defer_checks():
        value, mean, var = _obs(engine, case, params, noise_t).cv(case["starts"], (case["lo"], case["hi"]))
        value.backward()
    got = np.array([float(p.grad) for p in params])
    np.testing.assert_allclose(float(value), case["value"], rtol=1e-10)
    np.testing.assert_allclose(to_np(mean), case["mean"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(to_np(var), case["var"], rtol=1e-8, atol=1e-10)
    assert np.max(np.abs(want_theta[2:])) > 1e-2   # (the periods matter)
    np.testing.assert_allclose(got, want_theta, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(to_np(noise_t.grad), want_noise, rtol=1e-6, atol=1e-7)


# ---- the public API ----------------------------------------------------------------------------------------------------------
def _missing_data():
    x, y = _data(30, 3, seed=45, missing=0.2)
    y[4:6, 0] = np.nan     # (folds=5 over 30 rows: spans of 6 - the whole window of 2 rows before fold 1 of output 0 is missing ...
    y[6, 0] = 0.3          # ... and its first row is observed: nothing is purged on that side)
    y[12:18, 1] = np.nan   # (fold 2 of output 1 scores nothing: it vanishes)
    return x, y


def test_regressor_cv_with_a_gap_counts_rows_as_given_against_per_output_brute_force(engine):
    _regressor_cv_with_a_gap(engine, {})


def test_spectral_regressor_cv_with_a_gap_against_per_output_brute_force(engine):
    _regressor_cv_with_a_gap(engine, SPECTRAL)


def _regressor_cv_with_a_gap(engine, spectral):
    x, y = _missing_data()
    n, gap = 30, 2
    assert 0.1 < np.isnan(y).mean() < 0.35
    reg = GPARRegressor(scale=0.5, linear=False, nonlinear=False, noise=0.05, normalise_y=False, impute=True, **spectral)
    value, mean, var = reg.cv(x, y, folds=5, gap=gap)
    np.testing.assert_array_equal(np.isnan(mean), np.isnan(y))
    np.testing.assert_array_equal(np.isnan(var), np.isnan(y))
    spans = [(part[0], part[-1] + 1) for part in np.array_split(np.arange(n), 5)]
    total = 0.0
    for i in range(3):
        # (no layer of this model looks at earlier outputs: output i is a GP over x on the rows observed there)
        seen = np.nonzero(~np.isnan(y[:, i]))[0]
        K = np.exp(-0.5 * ((x[seen, None, :] - x[None, seen, :]) ** 2).sum(-1) / 0.5**2) + (0.05 + engine.epsilon) * np.eye(seen.size)
        if spectral:
            K = K + spectral_terms(x[seen], spectral["spectral_period"], spectral["spectral_scale"])
        starts, lo, hi = [0], [], []
        for a, b in spans:
            inside = np.nonzero((seen >= a) & (seen < b))[0]
            if inside.size:
                block = np.nonzero((seen >= a - gap) & (seen < b + gap))[0]
                starts.append(inside[-1] + 1), lo.append(block[0]), hi.append(block[-1] + 1)
        got = purged_folds(np.repeat(np.arange(5), 6), seen, gap)
        np.testing.assert_array_equal(got[0], starts), np.testing.assert_array_equal(got[1][0], lo), np.testing.assert_array_equal(got[1][1], hi)
        if i == 0:
            assert lo[1] == starts[1]   # (the purge window before fold 1 is empty)
        v, m, s = _brute_force(K, y[seen, i], np.array(starts), np.array(lo), np.array(hi))
        total += v
        np.testing.assert_allclose(mean[seen, i], m, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(var[seen, i], s, rtol=1e-8, atol=1e-10)
    assert abs(float(value) - total) <= 1e-10 * abs(total)


# ---- training ----------------------------------------------------------------------------------------------------------------
def test_fit_with_a_gap_by_the_prepared_and_the_general_route(engine):
    x, y = _data(48, 2, seed=46)
    finals, values = {}, {}
    for fast in (True, False):
        reg = GPARRegressor(**_KW)
        before = float(reg.cv(x, y, folds=6, gap=2)[0])
        reg.fast_fit = fast
        reg.condition(x, y)
        finals[fast] = reg._train(range(2), objective="cv", folds=6, gap=2, iters=5)
        values[fast] = float(reg.cv(x, y, folds=6, gap=2)[0])
        assert values[fast] >= before
        np.testing.assert_allclose(-sum(finals[fast].values()), values[fast], rtol=1e-8)
    print("trained purged cross-validation objectives, prepared / general:", finals[True], finals[False])
    for pi in range(2):
        np.testing.assert_allclose(finals[True][pi], finals[False][pi], rtol=1e-6)
    reg = GPARRegressor(**_KW)
    before = float(reg.cv(x, y, folds=6, gap=2)[0])
    reg.fit(x, y, objective="cv", folds=6, gap=2, iters=5)
    assert float(reg.cv(x, y, folds=6, gap=2)[0]) >= before


def test_greedy_order_takes_the_gap(engine):
    x, y = _data(24, 2, seed=47)
    order, values = GPARRegressor(**_KW).greedy_order(x, y, objective="cv", folds=4, gap=1, iters=3)
    assert sorted(order) == [0, 1] and all(np.isfinite(values))


# ---- errors ------------------------------------------------------------------------------------------------------------------
def test_argument_errors(oracle_engine):
    x, y = _data(12, 2, seed=48)
    for bad in (True, 1.0, -1, "2"):
        with pytest.raises(ValueError):
            GPARRegressor(**_KW).cv(x, y, folds=3, gap=bad)
        with pytest.raises(ValueError):
            GPARRegressor(**_KW).fit(x, y, objective="cv", folds=3, gap=bad, iters=1)
    for objective, extra in (("mll", {}), ("loo", {}), ("ahead", {"horizon": 1})):
        with pytest.raises(ValueError, match='gap belongs to objective="cv"'):
            GPARRegressor(**_KW).fit(x, y, objective=objective, gap=1, iters=1, **extra)
    scattered = np.array([0, 0, 1, 1, 0, 0, 2, 2, 2, 3, 3, 3])
    GPARRegressor(**_KW).cv(x, y, folds=scattered, gap=0)   # (no gap: any labelling)
    with pytest.raises(ValueError):
        GPARRegressor(**_KW).cv(x, y, folds=scattered, gap=1)
    with pytest.raises(ValueError):
        GPARRegressor(**_KW).fit(x, y, objective="cv", folds=scattered, gap=1, iters=1)
    sparse = GPARRegressor(x_ind=x[:4], **_KW)
    with pytest.raises(ValueError):
        sparse.cv(x, y, folds=3, gap=1)
    with pytest.raises(ValueError):
        sparse.fit(x, y, objective="cv", folds=3, gap=1, iters=1)
    with pytest.raises(NotImplementedError):
        GPARRegressor(**_KW).fit(x, y, objective="cv", folds=3, gap=1, fix=False, iters=1)
    with pytest.raises(ValueError):
        GPARRegressor(**_KW).cv(x, y, folds=3, gap=1, score="crps")
    with pytest.raises(ValueError):
        fastfit.DenseLayerObjective(None, None, [], None, None, {}, None, None, None, objective="loo", hold=([0], [1]))
    f = GP(EQ().stretch(0.5))
    xs, ys = x, y[:, 0]
    for hold in (([0, 4], [5, 11]), ([0, 5], [4, 12]), ([0, 3], [6, 13]), ([2, 1], [6, 12]), ([0], [12]), ([-1, 3], [6, 12]), ([0.0, 3.0], [6, 12])):
        with pytest.raises(ValueError):
            Obs(f(xs, 0.1), ys).cv([0, 5, 12], hold)
