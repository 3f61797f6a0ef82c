"""Streaming conditioning on the CPU oracle engine: `GPARRegressor.update` appends and forgets observations and must leave the regressor
exactly where `condition` on the moved window would, with the output normalisation of the last `condition` kept.

The oracle engine has neither `chol_drop_leading` nor `chol_append_`, so the incremental route runs through the composed fallbacks of
gpar_amd/gp.py here - the same host code that drives the library calls on the GPU (tests/test_update_gpu.py).  Tolerances are the
project's parity rules for well-conditioned problems (tests/test_loo.py, tests/test_parity_gpu.py; noise 0.1 on outputs of variance
~0.5): values rtol 1e-10, posterior moments and samples rtol 1e-8 / atol 1e-10."""
import numpy as np
import pytest
import torch

from gpar_amd import gp
from gpar_amd.regression import GPARRegressor

N0, M, P = 20, 2, 3
CONFIG = dict(scale=0.5, linear=True, nonlinear=True, noise=0.1)


def make_data(rows, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (rows, M))
    y = np.stack([np.sin(6 * x[:, 0]), np.cos(5 * x[:, 1]) * x[:, 0], x[:, 0] - x[:, 1] ** 2], axis=1)
    return x, y + 0.05 * rng.standard_normal(y.shape), rng.uniform(0, 1, (9, M))


def fresh_like(reg, x, y, **kw):
    """A new regressor with reg's hyper-parameter values, conditioned on (x, y)."""
    out = GPARRegressor(**{**CONFIG, "normalise_y": False, **kw})
    out.vs = reg.vs.copy(detach=True)
    out.condition(x, y)
    return out


def run_steps(reg, x, y, steps, lo=0, hi=N0):
    """Apply (drop, append) steps to reg, taking the appended rows from x[hi:], and return the window [lo, hi) reached."""
    for drop, k in steps:
        if k:
            reg.update(x[hi:hi + k], y[hi:hi + k], drop=drop)
        else:
            reg.update(drop=drop)
        lo, hi = lo + drop, hi + k
    return lo, hi


def assert_same_posterior(eng, a, b, xs, x_eval, y_eval):
    np.testing.assert_allclose(a.logpdf(x_eval, y_eval, posterior=True), b.logpdf(x_eval, y_eval, posterior=True), rtol=1e-10)
    eng.seed(7)
    sa = a.sample(xs, posterior=True)
    eng.seed(7)
    sb = b.sample(xs, posterior=True)
    np.testing.assert_allclose(sa, sb, rtol=1e-8, atol=1e-10)


@pytest.fixture
def wide_threshold(monkeypatch):
    """The rank-k route for forgotten rows is opt-in (gpar_amd.regression.update_drop_fraction): these tests are about that route."""
    monkeypatch.setenv("GPAR_UPDATE_DROP_FRACTION", "0.5")


@pytest.mark.parametrize("steps", [[(0, 1)], [(0, 5)], [(3, 0)], [(4, 4)], [(2, 3), (3, 1), (1, 2)]],
                         ids=["append1", "append5", "drop3", "drop4_append4", "three_steps"])
def test_equivalence(oracle_engine, wide_threshold, steps):
    x, y, xs = make_data(40)
    reg = GPARRegressor(**CONFIG, normalise_y=False)
    reg.condition(x[:N0], y[:N0])
    lo, hi = run_steps(reg, x, y, steps)
    assert reg.last_update_incremental_ is True
    assert reg.n == hi - lo
    np.testing.assert_array_equal(reg.x.numpy(), x[lo:hi])
    np.testing.assert_array_equal(reg.y.numpy(), y[lo:hi])
    np.testing.assert_array_equal(reg.w.numpy(), np.ones((hi - lo, P)))
    assert_same_posterior(oracle_engine, reg, fresh_like(reg, x[lo:hi], y[lo:hi]), xs, x[30:], y[30:])


def test_weights_travel_with_the_rows(oracle_engine, wide_threshold):
    x, y, xs = make_data(40)
    w = np.random.default_rng(3).uniform(0.5, 2.0, y.shape)
    reg = GPARRegressor(**CONFIG, normalise_y=False)
    reg.condition(x[:N0], y[:N0], w[:N0])
    reg.update(x[N0:N0 + 4], y[N0:N0 + 4], w[N0:N0 + 4], drop=2)
    assert reg.last_update_incremental_ is True
    np.testing.assert_array_equal(reg.w.numpy(), w[2:N0 + 4])
    ref = GPARRegressor(**CONFIG, normalise_y=False)
    ref.vs = reg.vs.copy(detach=True)
    ref.condition(x[2:N0 + 4], y[2:N0 + 4], w[2:N0 + 4])
    assert_same_posterior(oracle_engine, reg, ref, xs, x[30:], y[30:])


def test_normalisation_is_frozen(oracle_engine, wide_threshold):
    x, y, xs = make_data(40)
    y = 3.0 * y + 2.0
    y[N0:] += 1.5   # the appended rows move the mean: refreshed constants would differ
    reg = GPARRegressor(**CONFIG, normalise_y=True)
    reg.condition(x[:N0], y[:N0])
    reg.update(x[N0:N0 + 5], y[N0:N0 + 5], drop=3)
    assert reg.last_update_incremental_ is True
    lo, hi = 3, N0 + 5
    frozen = fresh_like(reg, x[lo:hi], y[lo:hi], normalise_y=True)
    frozen._normalise_y, frozen._unnormalise_y = reg._normalise_y, reg._unnormalise_y   # forced to the OLD constants
    frozen.y = reg._normalise_y(torch.from_numpy(y[lo:hi]))
    np.testing.assert_array_equal(reg.y.numpy(), frozen.y.numpy())
    assert_same_posterior(oracle_engine, reg, frozen, xs, x[30:], y[30:])
    refreshed = fresh_like(reg, x[lo:hi], y[lo:hi], normalise_y=True)
    assert not np.allclose(reg.y.numpy(), refreshed.y.numpy())


@pytest.mark.parametrize("case", ["nan", "replace", "x_ind"])
def test_fallback(oracle_engine, wide_threshold, case):
    x, y, xs = make_data(40)
    kw = {}
    if case == "nan":
        y[N0 + 1, 1] = np.nan
    elif case == "replace":
        kw["replace"] = True
    else:
        kw["x_ind"] = x[::4][:6].copy()
    reg = GPARRegressor(**CONFIG, normalise_y=False, **kw)
    reg.condition(x[:N0], y[:N0])
    reg.update(x[N0:N0 + 4], y[N0:N0 + 4], drop=2)
    assert reg.last_update_incremental_ is False
    ref = fresh_like(reg, x[2:N0 + 4], y[2:N0 + 4], **kw)
    if case == "replace":
        got, want = reg.predict_moments(xs), ref.predict_moments(xs)
        np.testing.assert_allclose(got[0], want[0], rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(got[1], want[1], rtol=1e-8, atol=1e-10)
    else:
        assert_same_posterior(oracle_engine, reg, ref, xs, x[30:], y[30:])


def test_drop_threshold_is_read_at_call_time(oracle_engine, monkeypatch):
    """By default (the measured crossover) rows are forgotten by conditioning again and appended incrementally; the switch moves it."""
    x, y, xs = make_data(40)
    reg = GPARRegressor(**CONFIG, normalise_y=False)
    reg.condition(x[:N0], y[:N0])
    reg.update(drop=1)
    assert reg.last_update_incremental_ is False
    reg.update(x[N0:N0 + 2], y[N0:N0 + 2])
    assert reg.last_update_incremental_ is True
    monkeypatch.setenv("GPAR_UPDATE_DROP_FRACTION", "0.125")
    reg.update(drop=2)   # 2 <= 21 / 8
    assert reg.last_update_incremental_ is True
    reg.update(drop=5)
    assert reg.last_update_incremental_ is False
    assert_same_posterior(oracle_engine, reg, fresh_like(reg, x[8:N0 + 2], y[8:N0 + 2]), xs, x[30:], y[30:])


@pytest.mark.parametrize("how", ["fit", "condition", "hyper"])
def test_cache_is_dropped(oracle_engine, wide_threshold, how):
    x, y, xs = make_data(40)
    reg = GPARRegressor(**CONFIG, normalise_y=False)
    reg.condition(x[:N0], y[:N0])
    reg.update(x[N0:N0 + 2], y[N0:N0 + 2])
    assert reg._stream_cache is not None and reg._stream_posterior() is not None
    if how == "fit":
        reg.fit(x[:N0], y[:N0], iters=1)
        assert reg._stream_cache is None
    elif how == "condition":
        reg.condition(x[:N0], y[:N0])
        assert reg._stream_cache is None
    else:
        name = next(n for n in reg.vs.names if n.endswith("noise"))
        reg.vs.assign(name, 0.2)
        assert reg._stream_posterior() is None and reg._stream_cache is None
    # and what follows is the ordinary route on the data the regressor holds
    ref = fresh_like(reg, reg.x.numpy(), reg.y.numpy())
    assert_same_posterior(oracle_engine, reg, ref, xs, x[30:], y[30:])


def test_untouched_regressor_never_consults_a_cache(oracle_engine, monkeypatch):
    def boom(self):
        raise AssertionError("a regressor that was never updated looked for kept factors")

    monkeypatch.setattr(GPARRegressor, "_stream_posterior", boom)
    x, y, xs = make_data(40)
    reg = GPARRegressor(**CONFIG, normalise_y=False)
    reg.condition(x[:N0], y[:N0])
    reg.logpdf(x[30:], y[30:], posterior=True)
    reg.sample(xs, posterior=True)
    reg.predict(xs, num_samples=2)
    rep = GPARRegressor(**CONFIG, normalise_y=False, replace=True)
    rep.condition(x[:N0], y[:N0])
    rep.predict_moments(xs)
    assert reg._stream_cache is None and rep._stream_cache is None


def test_errors(oracle_engine):
    x, y, _ = make_data(40)
    reg = GPARRegressor(**CONFIG, normalise_y=False)
    with pytest.raises(RuntimeError):
        reg.update(x[:2], y[:2])
    reg.condition(x[:N0], y[:N0])
    for bad in (-1, N0 + 1):
        with pytest.raises(ValueError):
            reg.update(drop=bad)
    with pytest.raises(ValueError):
        reg.update(drop=N0)   # everything forgotten, nothing appended
    with pytest.raises(ValueError):
        reg.update(x[:2, :1], y[:2])
    with pytest.raises(ValueError):
        reg.update(x[:2], y[:2, :2])
    with pytest.raises(ValueError):
        reg.update(x[:2], None)
    assert reg.n == N0   # nothing moved
    reg.update(x[N0:N0 + 3], y[N0:N0 + 3], drop=N0)   # the whole window replaced: allowed, conditioned in full
    assert reg.n == 3 and reg.last_update_incremental_ is False


@pytest.mark.parametrize("n,k", [(7, 1), (20, 3), (33, 9)])
def test_composed_factor_updates(oracle_engine, n, k):
    """The composed routes against numpy's Cholesky: drop the k leading rows, then append k rows again."""
    eng = oracle_engine
    rng = np.random.default_rng(n)
    x = rng.uniform(0, 1, (n, 1))
    S = np.exp(-0.5 * (x - x.T) ** 2 / 0.3 ** 2) + (0.05 + 1e-12) * np.eye(n)
    y = rng.standard_normal(n)

    def augmented(S_, y_):
        L = np.linalg.cholesky(S_)
        z = np.linalg.solve(L, y_)
        A = np.full((len(y_) + 1, len(y_) + 1), np.nan)
        A[np.tril_indices(len(y_))] = L[np.tril_indices(len(y_))]
        A[-1, :-1], A[-1, -1] = z, -z @ z
        return A, 2.0 * np.sum(np.log(np.diag(L)))

    A, logdet = augmented(S, y)
    want, want_logdet = augmented(S[k:, k:], y[k:])
    out, got_logdet, info = gp.chol_drop_leading(eng, torch.from_numpy(A.copy()), k)
    il = np.tril_indices(n - k + 1)
    assert int(info) == 0
    np.testing.assert_allclose(out.numpy()[il], want[il], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(float(got_logdet), want_logdet, rtol=1e-10)

    n0 = n - k
    B = np.full((n + 1, n + 1), np.nan)
    B[:n0, :n0] = augmented(S[:n0, :n0], y[:n0])[0][:n0, :n0]
    B[n0:n, :n] = S[n0:, :]
    B[n, :n0] = np.linalg.solve(np.linalg.cholesky(S[:n0, :n0]), y[:n0])
    B[n, n0:n] = y[n0:]
    Bt = torch.from_numpy(B)
    old = torch.tensor([augmented(S[:n0, :n0], y[:n0])[1]])
    got_logdet, info = gp.chol_append_(eng, Bt, n0, k, old)
    il = np.tril_indices(n + 1)
    assert int(info) == 0
    np.testing.assert_allclose(Bt.numpy()[il], A[il], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(float(got_logdet), logdet, rtol=1e-10)
