"""Pathwise posterior sampling (`predict(sampler="pathwise")`, `gpar_amd/pathwise.py`, `Obs.pathwise_sample_batch`) on the CPU: the oracle
engine runs the composed route.  What is checked, and against what:

  * the spectral laws of the basis - Phi(z) Phi(z')^T against `oracle.kernels.gram`, within 6 standard errors taken from the per-feature
    products themselves (F = 2^16); the exact features to 1e-12;
  * one layer's draw, with the basis, the weights and the noise draws handed in, against a numpy restatement written here;
  * the update is exact whatever the basis (F = 4 and F = 2048);
  * the law of the samples: against `predict_moments` (`replace=True`) and against the exact sampler (`replace=False`), with the margins of
    tests/test_share_nothing.py;
  * no matrix with two dimensions >= n*; the public surface and its refusals; the shift on time stamps near 1e6.
"""
import math

import numpy as np
import pytest
import torch

from gpar_amd import kernels as K
from gpar_amd.gp import GP, Obs, Stacked
from gpar_amd.pathwise import draw_basis, feature_map
from oracle import kernels as ok


def _spec(kernel, width):
    return ok.spec_to_dict(kernel.resolve(width))


LAWS = {
    "eq": lambda: 1.3 * K.EQ().stretch(0.7).select([0, 1]),
    "rq-0.01": lambda: K.RQ(0.01).stretch(0.5).select([0, 1]),
    "rq-2": lambda: 0.6 * K.RQ(2.0).stretch(0.5).select([0]),
    "matern12": lambda: K.Matern12().stretch(0.8).select([0, 1]),
    "matern32": lambda: 2.0 * K.Matern32().stretch(0.8).select([0, 1]),
    "matern52": lambda: K.Matern52().stretch(0.6).select([1]),
    "eq*cos": lambda: 0.9 * K.EQ().stretch(0.8).select([0]) * K.Cosine().stretch(0.6).select([0]),
    "locally-periodic": lambda: K.EQ().stretch(1.1).select([0]) * K.EQ().stretch(0.7).periodic(0.5).select([0]),
}


@pytest.mark.parametrize("name", list(LAWS))
def test_random_features_follow_the_kernels_spectral_law(name):
    """Phi(z) Phi(z')^T with F = 2^16 frequencies lies within 6 standard errors of the kernel at 12 point pairs.  The estimate is a sum of
    F independent per-frequency products (a cos and a sin feature each): its standard error is sqrt(F) times their sample standard
    deviation - no fixed number.  (A pair at distance zero has no spread and must be exact: the floor 1e-12.)"""
    kernel = LAWS[name]().resolve(2)
    rng = np.random.default_rng(5)
    a, b = rng.uniform(-1, 1, (12, 2)), rng.uniform(-1, 1, (12, 2))
    b[0] = a[0]
    F = 2 ** 16
    basis = draw_basis(kernel, F, np.random.default_rng(17)).with_shift(feature_map(kernel, a))
    assert basis.num_frequencies == F and basis.num_weights == 2 * F
    pa, pb = basis.phi(feature_map(kernel, a)), basis.phi(feature_map(kernel, b))
    per = pa[:, :F] * pb[:, :F] + pa[:, F:] * pb[:, F:]   # 12 x F products
    want = np.array([ok.gram(_spec(kernel, 2), a[i : i + 1], b[i : i + 1])[0, 0] for i in range(12)])
    se = math.sqrt(F) * per.std(axis=1, ddof=1)
    err = np.abs(per.sum(axis=1) - want)
    print(name, "largest error / standard error:", np.max(err[1:] / se[1:]))
    assert np.all(err <= 6.0 * se + 1e-12), (err, se)


def test_exact_features_are_exact():
    """Cos alone (one pair), Linear and the constant reproduce their kernels to 1e-12."""
    rng = np.random.default_rng(2)
    a, b = rng.uniform(-2, 2, (9, 2)), rng.uniform(-2, 2, (11, 2))
    kernel = (0.7 * K.Cosine().stretch([0.6, 1.7]).select([0, 1]) + 1.5 * K.Linear().stretch(2.0).select([0, 1]) + 0.3).resolve(2)
    basis = draw_basis(kernel, 50, np.random.default_rng(0)).with_shift(feature_map(kernel, a))
    assert basis.num_frequencies == 1 and basis.lin_idx.size == 2 and basis.const_amp.size == 1
    got = basis.phi(feature_map(kernel, a)) @ basis.phi(feature_map(kernel, b)).T
    np.testing.assert_allclose(got, ok.gram(_spec(kernel, 2), a, b), rtol=0, atol=1e-12)


def test_terms_without_a_basis_are_named():
    with pytest.raises(ValueError, match="term 1"):
        draw_basis((K.EQ().select([0]) + (K.Linear().select([0]) * K.EQ().select([0])).labelled("mixed")).resolve(1), 8, np.random.default_rng(0))
    with pytest.raises(ValueError, match="term 0"):
        draw_basis((-1.0 * K.EQ().select([0])).resolve(1), 8, np.random.default_rng(0))
    with pytest.raises(ValueError):
        draw_basis(K.EQ().select([0]), 0, np.random.default_rng(0))


def _layer_kernel():
    return 1.3 * K.EQ().stretch(0.5).select([0]) + 0.8 * K.Linear().stretch(2.0).select([1]) + 0.2


def _layer(eng, n, seed):
    """One layer: n observations (after a missing one has been dropped, as the model drops it) with weights, over two columns."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n + 1, 2))
    y = np.sin(5 * x[:, :1]) + 0.5 * x[:, 1:]
    y[rng.integers(n + 1)] = np.nan   # the missing value: its row is not observed
    w = rng.uniform(0.5, 2.0, n + 1)
    keep = ~np.isnan(y[:, 0])
    x, y, w = x[keep], y[keep], w[keep]
    kernel = _layer_kernel()
    f = GP(kernel, engine=eng)
    return kernel, x, y, 0.1 / w, Obs(f(x, 0.1 / w), y)


def _phi_numpy(basis, z):
    """Phi restated: [amp cos | amp sin | linear | constant]."""
    phase = 2.0 * np.pi * ((z - basis.shift) @ basis.omega.T)
    return np.concatenate([np.cos(phase) * basis.amp, np.sin(phase) * basis.amp, z[:, basis.lin_idx] * basis.lin_amp,
                           np.tile(basis.const_amp, (z.shape[0], 1))], axis=1)


def _features_numpy(x):
    """The feature map of `_layer_kernel`, restated: x0 / 0.5 for the EQ factor, x1 / 2 for the linear one."""
    return np.stack([x[:, 0] / 0.5, x[:, 1] / 2.0], axis=1)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("ns", [1, 5])
@pytest.mark.parametrize("n", [1, 7])
def test_a_layers_draw_equals_the_numpy_restatement(oracle_engine, n, ns, S):
    """With the basis, theta and the noise draws handed in, `Obs.pathwise_sample_batch` over S stacked design matrices equals
        Phi(x*_s) theta_s + k(x*_s, X) (K + D + eps I)^-1 (y - Phi(X) theta_s - sqrt(D) e_s) + sqrt(noise*) xi_s
    computed here with numpy (`oracle.kernels.gram`, `np.linalg.solve`), to rtol 1e-10.  Weighted noise, one missing observation."""
    eng = oracle_engine
    kernel, x, y, D, obs = _layer(eng, n, seed=10 * n + ns + S)
    rng = np.random.default_rng(1)
    xs = rng.uniform(0, 1, (S, ns, 2))
    basis = draw_basis(kernel.resolve(2), 16, np.random.default_rng(3)).with_shift(_features_numpy(x))
    theta, e, xi = rng.standard_normal((basis.num_weights, S)), rng.standard_normal((n, S)), rng.standard_normal((ns, S))
    noise_star = rng.uniform(0.05, 0.2, ns)
    got = obs.pathwise_sample_batch(Stacked(torch.from_numpy(xs.reshape(S * ns, 2)), S), noise_star, basis, S, draws=(theta, e, xi)).numpy()
    spec = _spec(kernel, 2)
    Kxx = ok.gram(spec, x, x) + np.diag(D) + eng.epsilon * np.eye(n)
    want = np.empty((ns, S))
    for s in range(S):
        v = np.linalg.solve(Kxx, y[:, 0] - _phi_numpy(basis, _features_numpy(x)) @ theta[:, s] - np.sqrt(D) * e[:, s])
        want[:, s] = _phi_numpy(basis, _features_numpy(xs[s])) @ theta[:, s] + ok.gram(spec, xs[s], x) @ v + np.sqrt(noise_star) * xi[:, s]
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12)
    # one design matrix shared by the draws is the same code with one group
    shared = obs.pathwise_sample_batch(torch.from_numpy(xs[0]), None, basis, S, draws=(theta, e, None)).numpy()
    np.testing.assert_allclose(shared[:, 0], want[:, 0] - np.sqrt(noise_star) * xi[:, 0], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("F", [4, 2048])
def test_the_update_is_exact_whatever_the_basis(oracle_engine, F):
    """At the training inputs a latent draw is f*_s(X) = y - e_s - D v_s with v_s = (K + D)^-1 (y - f_s(X) - e_s): with the noise draws e_s
    handed in as zero, |f*_s(X) - y| <= max D |v_s| row by row, however poor the basis (F = 4) - the right-hand side is computed here.
    (The factor carries the engine's jitter 1e-12 beside D >= 0.05: the bound has room for it, since max D exceeds most rows' D.)"""
    eng = oracle_engine
    n, S = 7, 3
    kernel, x, y, D, obs = _layer(eng, n, seed=4)
    basis = draw_basis(kernel.resolve(2), F, np.random.default_rng(F)).with_shift(_features_numpy(x))
    theta = np.random.default_rng(8).standard_normal((basis.num_weights, S))
    got = obs.pathwise_sample_batch(torch.from_numpy(x), None, basis, S, draws=(theta, np.zeros((n, S)), None)).numpy()
    Kxx = ok.gram(_spec(kernel, 2), x, x) + np.diag(D)
    for s in range(S):
        v = np.linalg.solve(Kxx, y[:, 0] - _phi_numpy(basis, _features_numpy(x)) @ theta[:, s])
        bound = np.max(D) * np.linalg.norm(v)
        assert np.all(np.abs(got[:, s] - y[:, 0]) <= bound), (np.abs(got[:, s] - y[:, 0]).max(), bound)
        np.testing.assert_allclose(got[:, s] - y[:, 0], -D * v, rtol=1e-8, atol=1e-11)


def _problem(n, m, p, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n, m))
    cols = []
    for i in range(p):
        base = np.sin(2 * np.pi * (x @ rng.uniform(0.5, 1.5, m)) + i)
        if cols:
            base = base + 0.5 * cols[-1] ** 2
        cols.append(base + 0.1 * rng.standard_normal(n))
    y = np.stack(cols, axis=1)
    return x, 0.7 + 1.9 * (y - y.mean(0)) / y.std(0)


def check_law_against_the_closed_form(S=1500):
    """`replace=True`, p = 3, n = 40: the means of S pathwise samples within 5 standard errors of `predict_moments`, their spreads
    within 25 % (the margins tests/test_share_nothing.py uses for `predict`).  Runs on whatever engine is installed."""
    from gpar_amd import GPARRegressor

    x, y = _problem(40, 1, 3, seed=11)
    xs = np.linspace(0.05, 0.95, 6)[:, None]
    reg = GPARRegressor(scale=0.5, linear=True, nonlinear=True, noise=0.05, replace=True, impute=True, normalise_y=False)
    reg.condition(x, y)
    want_mean, want_var = reg.predict_moments(xs)
    got = np.stack(reg.sample(xs, posterior=True, num_samples=S, sampler="pathwise"))
    sd = np.sqrt(want_var)
    print("largest |mean error| / standard error:", np.max(np.abs(got.mean(0) - want_mean) / (sd / np.sqrt(S))),
          " spread ratio:", np.min(got.std(0) / sd), np.max(got.std(0) / sd))
    assert np.all(np.abs(got.mean(0) - want_mean) <= 5.0 * sd / np.sqrt(S))
    np.testing.assert_allclose(got.std(0), sd, rtol=0.25)


def test_law_with_means_fed_forward(oracle_engine):
    check_law_against_the_closed_form()


@pytest.mark.parametrize("latent", [False, True], ids=["observed", "latent"])
def test_law_with_samples_fed_forward(oracle_engine, latent):
    """`replace=False`, nonlinear output dependence: against the exact sampler's statistics with the margins of
    tests/test_share_nothing.py - means within 5 standard errors, spreads within 15 %, correlations between consecutive outputs within
    0.16.  (At this seed two runs of the exact sampler with different seeds stay within the same margins: checked before committing.)"""
    from gpar_amd import GPARRegressor

    x, y = _problem(70, 2, 3, seed=75)
    xs = np.random.default_rng(3).uniform(0, 1, (6, 2))
    ws = np.random.default_rng(4).uniform(0.5, 2.0, (6, 3))
    reg = GPARRegressor(scale=0.5, linear=True, nonlinear=True, noise=0.1)
    reg.condition(x, y)
    S = 1500
    want = np.stack(reg.sample(xs, ws, posterior=True, num_samples=S, latent=latent))
    got = np.stack(reg.sample(xs, ws, posterior=True, num_samples=S, latent=latent, sampler="pathwise"))
    assert got.shape == want.shape == (S, 6, 3)
    mg, mw, sg, sw = got.mean(0), want.mean(0), got.std(0), want.std(0)
    assert np.all(np.abs(mg - mw) <= 5.0 * np.sqrt((sg ** 2 + sw ** 2) / S)), np.max(np.abs(mg - mw) / np.sqrt((sg ** 2 + sw ** 2) / S))
    np.testing.assert_allclose(sg, sw, rtol=0.15)
    for i in range(2):
        cg = [np.corrcoef(got[:, j, i], got[:, j, i + 1])[0, 1] for j in range(6)]
        cw = [np.corrcoef(want[:, j, i], want[:, j, i + 1])[0, 1] for j in range(6)]
        np.testing.assert_allclose(cg, cw, atol=0.16)


def test_no_matrix_with_two_large_dimensions(oracle_engine, monkeypatch):
    """n = 30, n* = 3000: no workspace request has two dimensions >= n* (the exact sampler asks for n* x n*)."""
    from gpar_amd import GPARRegressor

    x, y = _problem(30, 1, 2, seed=2)
    reg = GPARRegressor(scale=0.5, linear=True, nonlinear=True, noise=0.1)
    reg.condition(x, y)
    asked, make = [], oracle_engine.new_matrix

    def spy(rows, cols, zero=False):
        asked.append((rows, cols))
        return make(rows, cols, zero=zero)

    monkeypatch.setattr(oracle_engine, "new_matrix", spy)
    ns = 3000
    out = reg.sample(np.linspace(0, 1, ns)[:, None], posterior=True, num_samples=2, sampler="pathwise", features=64)
    assert out[0].shape == (ns, 2) and np.all(np.isfinite(out[0]))
    assert asked and all(min(r, c) < ns for r, c in asked), asked


def test_surface(oracle_engine):
    from gpar_amd import GPARRegressor
    from gpar_amd.parallel import sharded_predict, sharded_sample

    x, y = _problem(30, 1, 2, seed=2)
    xs = np.linspace(0, 1, 5)[:, None]
    reg = GPARRegressor(scale=0.5, linear=True, nonlinear=True, noise=0.1)
    reg.condition(x, y)
    # "exact" is the default path, bit for bit
    oracle_engine.seed(5)
    a = reg.predict(xs, num_samples=7, credible_bounds=True)
    oracle_engine.seed(5)
    b = reg.predict(xs, num_samples=7, credible_bounds=True, sampler="exact")
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    # the same seed gives the same pathwise samples, another seed others
    draws = []
    for seed in (5, 5, 6):
        oracle_engine.seed(seed)
        draws.append(np.stack(reg.sample(xs, posterior=True, num_samples=3, sampler="pathwise", features=32)))
    assert np.array_equal(draws[0], draws[1]) and not np.array_equal(draws[0], draws[2])
    one = reg.sample(xs, posterior=True, sampler="pathwise", features=32)
    assert one.shape == (5, 2)
    # refusals
    for kw in (dict(sampler="pathwise", marginal=True), dict(sampler="matheron"), dict(sampler="pathwise", features=0), dict(features=0)):
        with pytest.raises(ValueError):
            reg.predict(xs, num_samples=3, **kw)
    with pytest.raises(ValueError, match="posterior"):
        reg.sample(xs, p=2, posterior=False, num_samples=3, sampler="pathwise")
    with pytest.raises(ValueError, match="exact sampler"):
        sharded_predict(reg, xs, num_samples=3, sampler="pathwise")
    with pytest.raises(ValueError, match="exact sampler"):
        sharded_sample(reg, xs, num_samples=3, sampler="pathwise")
    sparse = GPARRegressor(scale=0.5, linear=True, nonlinear=True, noise=0.1, x_ind=np.linspace(0, 1, 8)[:, None])
    sparse.condition(x, y)
    with pytest.raises(ValueError, match="inducing"):
        sparse.predict(xs, num_samples=3, sampler="pathwise")


def test_a_kernel_term_outside_the_basis_is_refused(oracle_engine):
    """A layer whose kernel multiplies a linear factor into another has no basis: ValueError from `sample_many`, naming the term."""
    from gpar_amd.model import GPAR

    kernel = K.EQ().stretch(0.5).select([0]) + K.Linear().select([0]) * K.EQ().select([0])
    gpar = GPAR().add_layer(lambda: (GP(kernel), 0.1))
    x, y = np.linspace(0, 1, 9)[:, None], np.sin(np.linspace(0, 3, 9))[:, None]
    post = gpar | (x, y, np.ones((9, 1)))
    with pytest.raises(ValueError, match="term 1"):
        post.sample_many(x[:3], np.ones((3, 1)), 2, sampler="pathwise")
    with pytest.raises(ValueError, match="conditioned"):
        gpar.sample_many(x[:3], np.ones((3, 1)), 2, sampler="pathwise")


def test_the_shift_keeps_the_digits_of_large_time_stamps(oracle_engine):
    """x + 1e6 against x with the basis, theta and the draws handed in (the shift is taken from each problem's own training features).
    The inputs x + 1e6 are rounded to 2^-52 1e6 / 2 each, so differences of featurised coordinates are off by at most
    d = 2^-52 1e6 / scale; a phase 2 pi omega . (z - shift) moves by at most 2 pi dz max|omega| d, a prior value by that times
    sum_j amp_j (|thc_j| + |ths_j|) =: P.  The update carries a change of the prior values at X, and of the kernel values (slope at most 1 per
    unit of z for an EQ factor), into the draw with the gain worked out below.  Without the shift the phase itself would
    be rounded at 1e6 / scale max|omega| 2^-52 ~ 1e-9 per frequency - the same order; what the shift removes is the loss in the
    DIFFERENCES, which is why the bound below can be stated from the rounding of the inputs alone."""
    eng = oracle_engine
    n, ns, S, scale, noise = 12, 9, 2, 0.5, 0.1
    rng = np.random.default_rng(6)
    x, xs = rng.uniform(0, 4, (n, 1)), rng.uniform(0, 4, (ns, 1))
    y = np.sin(2 * x)
    kernel = 1.5 * K.EQ().stretch(scale).select([0])
    basis0 = draw_basis(kernel.resolve(1), 256, np.random.default_rng(1))
    theta, e = rng.standard_normal((basis0.num_weights, S)), rng.standard_normal((n, S))
    draws = []
    for offset in (0.0, 1e6):
        obs = Obs(GP(kernel, engine=eng)(x + offset, noise), y)
        assert basis0.shift is None
        draws.append(obs.pathwise_sample_batch(torch.from_numpy(xs + offset), None, basis0, S, draws=(theta, e, None)).numpy())
    d = 2.0 ** -52 * 1e6 / scale
    F = basis0.num_frequencies
    P = float(np.max(np.sum(basis0.amp[:, None] * (np.abs(theta[:F]) + np.abs(theta[F : 2 * F])), axis=0)))
    prior_move = 2 * np.pi * np.max(np.abs(basis0.omega)) * d * P
    # first order: d(draw) = df* + dk v + k dv with dv = A^-1 (dR - dK v), A = K + D: at most (1 + g) (prior_move + n dk max|v|), g the
    # largest row sum of |k(x*, X) A^-1| - computed here at offset 0
    spec = _spec(kernel, 1)
    A = ok.gram(spec, x, x) + noise * np.eye(n)
    g = np.max(np.sum(np.abs(ok.gram(spec, xs, x) @ np.linalg.inv(A)), axis=1))
    based = basis0.with_shift(x / scale)
    v = np.linalg.solve(A, y - based.phi(x / scale) @ theta - math.sqrt(noise) * e)
    dk = 1.5 * d   # (an EQ factor's slope is below 1 per unit of z)
    bound = (1.0 + g) * (prior_move + n * dk * np.max(np.abs(v)))
    err = np.max(np.abs(draws[0] - draws[1]))
    print("shift: largest difference", err, "bound", bound)
    assert err <= bound
    assert bound < 1e-3   # (the bound means something: draws are of order 1)
