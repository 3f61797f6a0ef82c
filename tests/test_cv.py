"""Blocked (leave-fold-out) cross-validation: `Obs.cv`, `GPAR.cv`, `GPARRegressor.cv` and `fit(objective="cv", folds=...)`.

The references live in this file, in numpy.  With P = K^-1, alpha = P y and, per fold F, D_F = P[F, F], b_F = D_F^-1 alpha_F:
y_F given all other rows ~ N(y_F - b_F, D_F^-1), value = sum_F [1/2 log|D_F| - 1/2 alpha_F^T b_F] - n/2 log 2 pi (the closed form), and the
same by deleting the fold's rows and conditioning on the rest (brute force).  At the conditionings used here (noise 0.05 - 0.1 of a unit
signal) the two agree to ~1e-12, inside the tolerances, which are the project's parity rules (tests/test_parity_gpu.py): values
rtol 1e-10, predictive moments rtol 1e-8 / atol 1e-10, finite differences as tests/test_loo.py.  Tests that take the `engine` fixture run
on the CPU oracle here and through the library on the GPU.

Fold patterns are lists of sizes taken in a cycle until the rows are used up (the last fold is cut short): [3, 4] over 7 rows is
3 + 4, [1, 2, 31, 32] over 65 rows is 1 + 2 + 31 + 31.
"""
import numpy as np
import pytest
import torch

from gpar_amd import fastfit
from gpar_amd.gp import GP, Obs
from gpar_amd.kernels import EQ, Linear
from gpar_amd.model import per_output
from gpar_amd.optimise import objective_and_gradient
from gpar_amd.regression import GPARRegressor, _construct_gpar, _surviving_rows

from .conftest import to_np
from .test_fastfit import _layer_objectives
from .test_loo import _KW, _SPECTRAL_KW, _data, _eq_linear, _fd, _one_layer, _spectral_first_layer

_LOG_2PI = np.log(2.0 * np.pi)


# ---- numpy references --------------------------------------------------------------------------------------------------------
def _fold_starts(n, pattern):
    """Row offsets of contiguous folds whose sizes cycle through `pattern` until n rows are used (the last fold is cut short)."""
    starts, k = [0], 0
    while starts[-1] < n:
        starts.append(min(n, starts[-1] + pattern[k % len(pattern)]))
        k += 1
    return np.array(starts)


def _closed_form(K, y, starts):
    """(value, means, marginal variances, alpha, K^-1, b, C) of blocked cross-validation under N(0, K)."""
    n = len(y)
    P = np.linalg.inv(K)
    P = 0.5 * (P + P.T)
    alpha = P @ y
    value, b, var, C = -0.5 * n * _LOG_2PI, np.zeros(n), np.zeros(n), np.zeros((n, n))
    for lo, hi in zip(starts[:-1], starts[1:]):
        D = P[lo:hi, lo:hi]
        Dinv = np.linalg.inv(D)
        Dinv = 0.5 * (Dinv + Dinv.T)
        b[lo:hi] = Dinv @ alpha[lo:hi]
        var[lo:hi] = np.diag(Dinv)
        C[lo:hi, lo:hi] = 0.5 * (Dinv + np.outer(b[lo:hi], b[lo:hi]))
        value += 0.5 * np.linalg.slogdet(D)[1] - 0.5 * alpha[lo:hi] @ b[lo:hi]
    return value, y - b, var, alpha, P, b, C


def _brute_force(K, y, starts):
    """The same by deleting one fold at a time and conditioning on the rest: the joint Gaussian log-density of the fold."""
    n = len(y)
    value, mean, var = 0.0, np.zeros(n), np.zeros(n)
    for lo, hi in zip(starts[:-1], starts[1:]):
        fold = np.arange(lo, hi)
        rest = np.delete(np.arange(n), fold)
        if rest.size:
            sol = np.linalg.solve(K[np.ix_(rest, rest)], np.concatenate([y[rest, None], K[np.ix_(rest, fold)]], axis=1))
            mu = K[np.ix_(fold, rest)] @ sol[:, 0]
            cov = K[np.ix_(fold, fold)] - K[np.ix_(fold, rest)] @ sol[:, 1:]
        else:
            mu, cov = np.zeros(hi - lo), K
        r = y[fold] - mu
        value += -0.5 * (np.linalg.slogdet(cov)[1] + r @ np.linalg.solve(cov, r) + (hi - lo) * _LOG_2PI)
        mean[fold], var[fold] = mu, np.diag(cov)
    return value, mean, var


def _cv_weights(K, y, starts):
    """W of dL/dtheta = 1/2 sum_ab W_ab dK_ab/dtheta:  alpha u^T + u alpha^T - 2 P C P with u = P b."""
    _, _, _, alpha, P, b, C = _closed_form(K, y, starts)
    u = P @ b
    return np.outer(alpha, u) + np.outer(u, alpha) - 2.0 * P @ C @ P


# ---- one layer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [False, True], ids=["unit", "weighted"])
@pytest.mark.parametrize("n,pattern", [(7, [3, 4]), (65, [3, 4]), (65, [1, 2, 31, 32])], ids=["7-3.4", "65-3.4", "65-1.2.31.32"])
def test_closed_form_equals_brute_force_deletion_for_one_layer(engine, n, pattern, weights):
    x, y, w = _one_layer(n, weights, seed=n)
    starts = _fold_starts(n, pattern)
    K = _eq_linear(x) + np.diag(0.05 / w) + engine.epsilon * np.eye(n)
    v_brute, m_brute, s_brute = _brute_force(K, y, starts)
    v_closed, m_closed, s_closed = _closed_form(K, y, starts)[:3]
    assert abs(v_closed - v_brute) <= 1e-11 * abs(v_brute)
    np.testing.assert_allclose(m_closed, m_brute, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(s_closed, s_brute, rtol=1e-10)
    f = GP(EQ().stretch(0.5) + 0.3 * Linear())
    with torch.no_grad():
        value, mean, var = Obs(f(x, 0.05 / w), y).cv(starts)
    assert abs(float(value) - v_brute) <= 1e-10 * abs(v_brute)
    np.testing.assert_allclose(to_np(mean), m_brute, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(to_np(var), s_brute, rtol=1e-8, atol=1e-10)


def test_fold_offsets_are_checked(oracle_engine):
    x, y, _ = _one_layer(10, False, seed=3)
    f = GP(EQ().stretch(0.5))
    for bad in ([0, 4], [1, 10], [0, 4, 4, 10], [0, 6, 4, 10], [0, 12]):
        with pytest.raises(ValueError):
            Obs(f(x, 0.1), y).cv(bad)


# ---- the two identities --------------------------------------------------------------------------------------------------------
def test_folds_of_one_row_reproduce_loo(engine):
    x, y = _data(33, 3, seed=31, missing=0.1)
    reg = GPARRegressor(**_KW)
    want = reg.loo(x, y)
    got = reg.cv(x, y, folds=np.arange(33))
    assert abs(float(got[0]) - float(want[0])) <= 1e-10 * abs(float(want[0]))
    np.testing.assert_allclose(got[1], want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(got[2], want[2], rtol=1e-8, atol=1e-10)


def test_one_fold_over_all_rows_reproduces_logpdf_and_its_gradient(engine):
    x, y = _data(40, 1, seed=32)
    reg = GPARRegressor(**_KW)
    value, mean, var = reg.cv(x, y, folds=1)
    assert isinstance(value, np.ndarray) and mean.shape == var.shape == y.shape
    want = float(reg.logpdf(x, y))
    assert abs(float(value) - want) <= 1e-10 * abs(want)
    np.testing.assert_allclose(mean, 0.0, atol=1e-10)   # (nothing is left to condition on: the prior's mean)
    assert torch.is_tensor(reg.cv(torch.tensor(x), y, folds=1)[0])
    names = reg.vs.names
    grads = {}
    for which in ("cv", "logpdf"):
        reg.vs.requires_grad(True)
        gpar = _construct_gpar(reg, reg.vs, 2, 1)
        w = torch.ones(40, 1, dtype=torch.float64)
        val = gpar.cv(x, y, w, np.zeros(40, dtype=int))[0] if which == "cv" else gpar.logpdf(x, y, w)
        val.backward()
        grads[which] = np.concatenate([v.grad.numpy().reshape(-1) for v in reg.vs.get_vars(*names)])
        for v in reg.vs.get_vars(*names):
            v.grad = None
        reg.vs.requires_grad(False)
    assert np.max(np.abs(grads["logpdf"])) > 1e-2
    np.testing.assert_allclose(grads["cv"], grads["logpdf"], rtol=1e-6, atol=1e-7)


# ---- the public API ----------------------------------------------------------------------------------------------------------
def test_unsorted_labels_give_the_result_of_the_sorted_problem_mapped_back(engine):
    x, y = _data(30, 2, seed=33)
    labels = np.random.default_rng(33).choice([7, -2, 11, 4], size=30)
    perm = np.argsort(labels, kind="stable")
    reg = GPARRegressor(**_KW)
    got = reg.cv(x, y, folds=labels)
    want = reg.cv(x[perm], y[perm], folds=labels[perm])
    assert abs(float(got[0]) - float(want[0])) <= 1e-10 * abs(float(want[0]))
    np.testing.assert_allclose(got[1][perm], want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(got[2][perm], want[2], rtol=1e-8, atol=1e-10)
    # the first layer against numpy, through the sorted rows
    single = GPARRegressor(scale=0.5, linear=False, nonlinear=False, noise=0.05, normalise_y=False)
    value, mean, var = single.cv(x, y[:, :1], folds=labels)
    d2 = ((x[perm, None, :] - x[None, perm, :]) ** 2).sum(-1) / 0.5**2
    K = np.exp(-0.5 * d2) + (0.05 + engine.epsilon) * np.eye(30)
    starts = np.concatenate([[0], np.nonzero(np.diff(labels[perm]))[0] + 1, [30]])
    v_ref, m_ref, s_ref = _closed_form(K, y[perm, 0], starts)[:3]
    assert abs(float(value) - v_ref) <= 1e-10 * abs(v_ref)
    np.testing.assert_allclose(mean[perm, 0], m_ref, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var[perm, 0], s_ref, rtol=1e-8, atol=1e-10)


def test_a_number_of_folds_means_the_blocks_of_array_split(engine):
    x, y = _data(23, 2, seed=34)
    reg = GPARRegressor(**_KW)
    labels = np.concatenate([np.full(len(part), j) for j, part in enumerate(np.array_split(np.arange(23), 5))])
    got, want = reg.cv(x, y, folds=5), reg.cv(x, y, folds=labels)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("replace", [False, True])
def test_missing_entries_are_nan_and_contribute_nothing(engine, replace):
    x, y = _data(40, 3, seed=35, missing=0.1)
    y[8:16, 0] = np.nan   # (fold 1 of output 0 is emptied: it vanishes)
    assert np.isnan(y).any()
    labels = np.repeat(np.arange(5), 8)
    reg = GPARRegressor(scale=0.5, linear=False, nonlinear=False, noise=0.05, normalise_y=False, impute=True, replace=replace)
    value, mean, var = reg.cv(x, y, folds=labels)
    np.testing.assert_array_equal(np.isnan(mean), np.isnan(y))
    np.testing.assert_array_equal(np.isnan(var), np.isnan(y))
    assert np.isfinite(value) and np.all(var[~np.isnan(y)] > 0.0)
    # output 0 alone: the observed rows with their labels are the whole problem
    seen = ~np.isnan(y[:, 0])
    first = reg.cv(x, y[:, :1], folds=labels)
    dropped = reg.cv(x[seen], y[seen, :1], folds=labels[seen])
    # (parity tolerances, not equal bits: on the GPU a layer that feeds another one and a last layer take different routes)
    np.testing.assert_allclose(first[0], dropped[0], rtol=1e-10)
    np.testing.assert_allclose(first[1][seen], dropped[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(mean[:, 0], first[1][:, 0], rtol=1e-8, atol=1e-10)
    d2 = ((x[seen, None, :] - x[None, seen, :]) ** 2).sum(-1) / 0.5**2
    K = np.exp(-0.5 * d2) + (0.05 + engine.epsilon) * np.eye(int(seen.sum()))
    starts = np.concatenate([[0], np.nonzero(np.diff(labels[seen]))[0] + 1, [int(seen.sum())]])
    assert len(starts) == 5
    v_ref, m_ref, s_ref = _closed_form(K, y[seen, 0], starts)[:3]
    assert abs(float(first[0]) - v_ref) <= 1e-10 * abs(v_ref)
    np.testing.assert_allclose(mean[seen, 0], m_ref, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var[seen, 0], s_ref, rtol=1e-8, atol=1e-10)


def test_first_layer_of_a_spectral_model_equals_the_closed_form_and_the_brute_force_with_weights(engine):
    """The VALUE of cv, its means and variances for a spectral model against the dense restatement: the closed form and one deletion
    per fold, folds of 3 and 4 rows, weights."""
    x, y = _data(30, 1, seed=37)
    w = np.random.default_rng(37).uniform(0.5, 2.0, y.shape)
    starts = _fold_starts(30, [3, 4])
    labels = np.repeat(np.arange(len(starts) - 1), np.diff(starts))
    value, mean, var = GPARRegressor(**_SPECTRAL_KW).cv(x, y, w, folds=labels)
    K = _spectral_first_layer(x) + np.diag(0.05 / w[:, 0]) + engine.epsilon * np.eye(30)
    v_ref, m_ref, s_ref = _closed_form(K, y[:, 0], starts)[:3]
    v_brute, m_brute, s_brute = _brute_force(K, y[:, 0], starts)
    assert abs(v_ref - v_brute) <= 1e-11 * abs(v_brute)
    assert abs(float(value) - v_brute) <= 1e-10 * abs(v_brute)
    np.testing.assert_allclose(mean[:, 0], m_brute, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var[:, 0], s_brute, rtol=1e-8, atol=1e-10)
    plain = GPARRegressor(scale=0.5, linear=False, nonlinear=False, noise=0.05, normalise_y=False).cv(x, y, w, folds=labels)[0]
    assert abs(float(plain) - v_brute) > 1e-3 * abs(v_brute)


# ---- gradient ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matern,spectral", [(None, None), (1.5, None), (None, 2)], ids=["eq", "matern32", "spectral2"])
def test_autograd_gradient_of_the_cv_value_against_central_differences(engine, matern, spectral):
    x, y = _data(40, 2, seed=36)
    rng = np.random.default_rng(36)
    w = rng.uniform(0.5, 2.0, y.shape)
    labels = rng.integers(0, 6, 40)   # (unsorted: the gradient passes through the permutation)
    # (spectral: two components at periods 0.7 and 0.31 with short envelopes - periods, envelope scales and variances are differentiated)
    reg = GPARRegressor(matern=matern, **_KW, **({} if spectral is None else dict(spectral=spectral, spectral_period=(0.7, 0.31), spectral_scale=0.8)))

    def value():
        return _construct_gpar(reg, reg.vs, 2, 2).cv(x, y, w, labels)[0]

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
    """The reference of the GPU tests checks itself: 1/2 sum W o dK/dtheta against differences of L, for the EQ length scale, and
    1/2 diag W against differences in one noise entry."""
    x, y, w = _one_layer(30, True, seed=6)
    starts = _fold_starts(30, [1, 5, 2, 9])

    def K(scale, bump=0.0):
        noise = 0.1 / w
        noise[7] += bump
        return _eq_linear(x, scale=scale) + np.diag(noise)

    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    dK = np.exp(-0.5 * d2 / 0.5**2) * d2 / 0.5**3
    W = _cv_weights(K(0.5), y, starts)
    h = 1e-5
    want = (_closed_form(K(0.5 + h), y, starts)[0] - _closed_form(K(0.5 - h), y, starts)[0]) / (2.0 * h)
    assert abs(0.5 * np.sum(W * dK) - want) <= 1e-7 * abs(want)
    want = (_closed_form(K(0.5, h), y, starts)[0] - _closed_form(K(0.5, -h), y, starts)[0]) / (2.0 * h)
    assert abs(0.5 * W[7, 7] - want) <= 1e-7 * abs(want)


# ---- training ----------------------------------------------------------------------------------------------------------------
def test_fit_with_the_cv_objective_raises_the_cv_value(engine):
    x, y = _data(40, 2, seed=37)
    reg = GPARRegressor(**_KW)
    before = float(reg.cv(x, y, folds=5)[0])
    reg.fit(x, y, objective="cv", folds=5, iters=15)
    assert float(reg.cv(x, y, folds=5)[0]) > before


def test_greedy_order_ranks_by_the_trained_cv_value(engine):
    x, y = _data(25, 2, seed=38)
    reg = GPARRegressor(**_KW)
    order, values = reg.greedy_order(x, y, objective="cv", folds=5, iters=4)
    assert sorted(order) == [0, 1] and all(np.isfinite(values))
    # the first position's value is the trained cross-validation value of that output as a single layer
    single = GPARRegressor(**_KW)
    single.fit(x, y[:, order[:1]], objective="cv", folds=5, iters=4)
    assert abs(values[0] - float(single.cv(x, y[:, order[:1]], folds=5)[0])) <= 1e-8 * abs(values[0])
    other = GPARRegressor(**_KW)
    other.fit(x, y[:, order[1:]], objective="cv", folds=5, iters=4)
    assert values[0] >= float(other.cv(x, y[:, order[1:]], folds=5)[0])


# ---- host logic of the fast route ---------------------------------------------------------------------------------------------
class NumpyCvObjective(fastfit.DenseLayerObjective):
    """DenseLayerObjective with the device side in numpy: what the library call returns, from the closed form above."""

    def _allocate(self, ck):
        pass

    def _device_eval(self, ck, noise):
        from oracle import kernels as ok

        assert self.objective == "cv"
        spec = ok.spec_to_dict(self.kernel.resolve(self.width))
        X, y, w = self.X.numpy(), self.y.numpy(), self.w.numpy()
        K = ok.gram(spec, X, None, noise_diag=noise / w, jitter=self.eng.epsilon)
        try:
            np.linalg.cholesky(K)
        except np.linalg.LinAlgError:
            return None
        W = _cv_weights(K, y, self.fold_start)
        return _closed_form(K, y, self.fold_start)[0], ok.kernel_grads(spec, X, W), 0.5 * np.diag(W).copy()


def _labels_reaching(reg, eng, pi, labels):
    """The labels of the rows of layer pi's fixed design matrix (rows that earlier layers' masks dropped are gone from it)."""
    y_t = eng.tensor(reg.y).view(reg.y.shape)
    y_t._host_nan = torch.isnan(reg.y).numpy()
    items = list(per_output(y_t, eng.tensor(reg.w), keep=bool(reg.impute)))
    return labels[_surviving_rows(items, pi, reg.n)]


@pytest.mark.parametrize("variant", ["plain", "weights", "missing"])
def test_fast_and_general_routes_agree_on_the_host_side(oracle_engine, variant, monkeypatch):
    rng = np.random.default_rng(10)
    x, y = _data(28, 3, seed=10, missing=0.15 if variant == "missing" else 0.0)
    w = rng.uniform(0.5, 2.0, y.shape) if variant == "weights" else None
    labels = rng.integers(0, 5, 28)
    reg = GPARRegressor(scale=0.5, linear=True, nonlinear=True, rq=True, noise=0.1)
    reg.condition(x, y, w)
    real_build = fastfit.build
    for pi in range(reg.p):
        reaching = _labels_reaching(reg, oracle_engine, pi, labels)
        monkeypatch.setattr(fastfit, "build", lambda *a, **k: real_build(*a, objective="cv", folds=reaching, **k))
        fast, _, x0 = _layer_objectives(reg, oracle_engine, pi, NumpyCvObjective)
        assert fast.objective == "cv" and fast.group is None
        sizes = np.diff(fast.fold_start)
        assert fast.fold_start[0] == 0 and fast.fold_start[-1] == fast.n and np.all(sizes > 0) and len(sizes) <= 5

        def objective(vs, pi=pi, fast=fast):
            f, noise = _construct_gpar(reg, vs, reg.m, pi + 1).layers[pi]()
            return -Obs(f(fast.X, noise / fast.w), fast.y).cv(fast.fold_start)[0]

        general, _, _ = objective_and_gradient(objective, reg.vs, [f"{pi}/*"])
        for trial in range(2):
            xv = x0 + (0.0 if trial == 0 else 0.3 * rng.standard_normal(x0.shape))
            v_fast, g_fast = fast.fg(xv)
            v_ref, g_ref = general(xv)
            assert abs(v_fast - v_ref) <= 1e-9 * max(1.0, abs(v_ref)), (variant, pi, v_fast, v_ref)
            np.testing.assert_allclose(g_fast, g_ref, rtol=1e-6, atol=1e-7 * max(1.0, np.abs(g_ref).max()))
        reg.vs.set_vector(x0, fast.names)


def test_fit_hands_the_folds_to_the_prepared_route_and_trains_the_same_model(oracle_engine, monkeypatch):
    x, y = _data(30, 3, seed=12, missing=0.1)
    labels = np.random.default_rng(12).integers(0, 4, 30)
    built = []
    real_build = fastfit.build

    def build(*args, **kwargs):
        built.append(real_build(*args, cls=NumpyCvObjective, **kwargs))
        return built[-1]

    monkeypatch.setattr(fastfit, "build", build)
    fast, slow = GPARRegressor(**_KW), GPARRegressor(**_KW)
    fast.fit(x, y, objective="cv", folds=labels, iters=6)
    assert len(built) == 3 and all(b is not None and b.objective == "cv" and b.evaluations > 0 and b.fallbacks == 0 for b in built)
    slow.fast_fit = False
    slow.fit(x, y, objective="cv", folds=labels, iters=6)
    assert len(built) == 3
    a, b = fast.get_variables(), slow.get_variables()
    assert sorted(a) == sorted(b)
    for name in a:
        np.testing.assert_allclose(a[name], b[name], rtol=1e-6, atol=1e-9, err_msg=name)


def test_a_fold_larger_than_the_fused_limit_goes_to_the_general_route(oracle_engine, monkeypatch):
    x, y = _data(70, 1, seed=13)
    built = []
    real_build = fastfit.build

    def build(*args, **kwargs):
        built.append(real_build(*args, cls=NumpyCvObjective, **kwargs))
        return built[-1]

    monkeypatch.setattr(fastfit, "build", build)
    reg = GPARRegressor(**_KW)
    labels = np.array([0] * 65 + [1] * 5)
    before = float(reg.cv(x, y, folds=labels)[0])
    reg.fit(x, y, objective="cv", folds=labels, iters=5)
    assert built == [None]
    assert float(reg.cv(x, y, folds=labels)[0]) > before
    reg.fit(x, y, objective="cv", folds=np.array([0] * 64 + [1] * 6), iters=1)
    assert len(built) == 2 and built[1] is not None and int(np.diff(built[1].fold_start).max()) == 64


# ---- errors ------------------------------------------------------------------------------------------------------------------
def test_error_cases(oracle_engine):
    x, y = _data(12, 2, seed=11)
    with pytest.raises(ValueError):
        GPARRegressor(**_KW).fit(x, y, objective="cv", iters=1)
    with pytest.raises(ValueError):
        GPARRegressor(**_KW).fit(x, y, objective="mll", folds=3, iters=1)
    with pytest.raises(ValueError):
        GPARRegressor(**_KW).fit(x, y, objective="loo", folds=3, iters=1)
    with pytest.raises(ValueError):
        GPARRegressor(**_KW).cv(x, y)
    for bad in (np.arange(11), np.zeros((12, 1), dtype=int), np.linspace(0.0, 1.0, 12), 0, 13, -1):
        with pytest.raises(ValueError):
            GPARRegressor(**_KW).cv(x, y, folds=bad)
        with pytest.raises(ValueError):
            GPARRegressor(**_KW).fit(x, y, objective="cv", folds=bad, iters=1)
    sparse = GPARRegressor(x_ind=x[:4], **_KW)
    with pytest.raises(ValueError):
        sparse.fit(x, y, objective="cv", folds=3, iters=1)
    with pytest.raises(ValueError):
        sparse.cv(x, y, folds=3)
    with pytest.raises(NotImplementedError):
        GPARRegressor(**_KW).fit(x, y, objective="cv", folds=3, fix=False, iters=1)
    with pytest.raises(ValueError):
        fastfit.DenseLayerObjective(None, None, [], None, None, {}, None, None, None, objective="cv")
    with pytest.raises(ValueError):
        fastfit.DenseLayerObjective(None, None, [], None, None, {}, None, None, None, objective="loo", fold_start=[0, 1])
