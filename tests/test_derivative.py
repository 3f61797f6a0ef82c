"""Posterior derivatives on the CPU: the numpy restatement (tests/derivative_reference.py) against 50-digit central differences, the
restated layer chain against central differences of predict_moments, the J builder against central differences of the feature map, and
the error surface and the ABI text of GPARRegressor.derivative / gpar_posterior_deriv.  The device kernels themselves are tested in
tests/test_derivative_gpu.py against the restatement that is pinned here."""
import os
import re

import mpmath as mp
import numpy as np
import pytest
import torch

from gpar_amd import GPARRegressor, log_transform
from oracle import gpar_ref, mp_ref
from oracle import kernels as ok

from . import derivative_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f(type_, cols, scales, periods=None, alpha=0.0):
    return {"type": type_, "cols": list(cols), "scales": list(scales), "periods": periods, "alpha": alpha}


def structures():
    """name -> kernel dict over a design matrix of width 3: every factor type alone, and the products the issue names."""
    single = {
        "eq": [_f("eq", [0, 2], [0.7, 1.1])],
        "rq": [_f("rq", [1], [0.9], alpha=0.7)],
        "matern32": [_f("matern32", [0, 1], [0.8, 1.3])],
        "matern52": [_f("matern52", [2], [1.0])],
        "linear": [_f("linear", [0, 1], [2.0, 1.5])],
        "cos": [_f("cos", [1], [0.9])],
    }
    out = {k: {"terms": [{"coef": 1.3, "factors": v}]} for k, v in single.items()}
    out["per_eq_decay"] = {"terms": [{"coef": 0.7, "factors": [_f("eq", [0], [1.0, 1.4], periods=[0.6]), _f("eq", [0], [3.0])]}]}
    out["linear_eq"] = {"terms": [{"coef": 0.5, "factors": [_f("linear", [1, 2], [2.0, 0.8]), _f("eq", [0, 1], [1.2, 0.9])]}]}
    out["linear_linear"] = {"terms": [{"coef": 0.6, "factors": [_f("linear", [0, 1], [1.1, 0.7]), _f("linear", [1, 2], [0.9, 1.6])]}]}
    out["with_constant"] = {"terms": [{"coef": 0.9, "factors": [_f("matern52", [0], [0.8])]}, {"coef": 0.3, "factors": []}]}
    out["cos_two_dims"] = {"terms": [{"coef": 0.4, "factors": [_f("eq", [0, 1], [1.5, 1.5]), _f("cos", [0, 1], [0.5, 0.9])]}]}
    out["sum_of_all"] = {"terms": [t for k in ("eq", "rq", "matern32", "per_eq_decay", "linear_linear", "cos_two_dims", "with_constant")
                                   for t in out[k]["terms"]]}
    return out


def points(seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (4, 3)), rng.uniform(-1, 1, (3, 3)), rng.standard_normal((3, 3))   # x, xs, U


def _shift(xs, U, h):
    return [[mp.mpf(float(v)) + h * mp.mpf(float(u)) for v, u in zip(row, urow)] for row, urow in zip(xs, U)]


# ---- (a) the restatement against central differences in extended precision ---------------------------------------------------------------
# Tolerance: the restatement is fp64 numpy - entries of size <= 10 from a few dozen roundings of 2^-53, differences z - z' of numbers of
# size 1 included: 1e-12 (1 + max |reference|) absolute, the bound tests/test_decompose_gpu.py asserts for Gram entries against numpy.
# The central differences run at 80 digits with steps 1e-20 (first derivative: truncation h^2) and 1e-25 (mixed second derivative:
# truncation h^2, and h for the Matern factors, whose r^3 term is not smooth at r = 0) - far below that bound.
@pytest.mark.parametrize("name", sorted(structures()) + ["matern12"])
def test_cross_rows_against_mpmath_central_differences(name):
    spec = structures().get(name) or {"terms": [{"coef": 1.1, "factors": [_f("matern12", [0, 1], [0.8, 1.2])]}]}   # (nu = 1/2: d exists off r = 0)
    x, xs, U = points()
    got = dr.cross_rows(spec, xs, x, U)
    with mp.workdps(80):
        h = mp.mpf(10) ** -20
        rows = [[mp.mpf(float(v)) for v in row] for row in x]
        up, down = mp_ref.gram(spec, _shift(xs, U, h), rows), mp_ref.gram(spec, _shift(xs, U, -h), rows)
        want = np.array([[float((up[a, b] - down[a, b]) / (2 * h)) for b in range(x.shape[0])] for a in range(xs.shape[0])])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * (1 + np.abs(want).max()))
    alpha = np.array([0.3, -1.2, 0.8, 0.5])
    np.testing.assert_allclose(dr.mean_derivative(spec, xs, x, alpha, U), want @ alpha, rtol=0, atol=1e-12 * (1 + np.abs(want).max()) * 4)


@pytest.mark.parametrize("name", sorted(structures()))
def test_prior_term_against_mpmath_mixed_central_differences(name):
    spec = structures()[name]
    _, xs, U = points()
    got = dr.prior_term(spec, xs, U)
    want = np.zeros(xs.shape[0])
    with mp.workdps(80):
        h = mp.mpf(10) ** -25
        for a in range(xs.shape[0]):
            up, down = _shift(xs[a:a + 1], U[a:a + 1], h), _shift(xs[a:a + 1], U[a:a + 1], -h)
            k = lambda p, q: mp_ref.gram(spec, p, q)[0, 0]
            want[a] = float((k(up, up) - k(up, down) - k(down, up) + k(down, down)) / (4 * h * h))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * (1 + np.abs(want).max()))
    assert np.all(got >= 0.0)   # (the variance of a derivative)


def test_the_restatement_refuses_matern12():
    with pytest.raises(ValueError, match="not differentiable"):
        dr.prior_term({"terms": [{"coef": 1.0, "factors": [_f("matern12", [0], [1.0])]}]}, np.zeros((1, 3)), np.ones((1, 3)))


# ---- (b) the restated layer chain against central differences of predict_moments ------------------------------------------------------------
def _model_data(seed=0, n=30, ns=7, missing=0.1):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n, 2))
    y = np.stack([np.sin(6 * x[:, 0]) + x[:, 1], np.cos(5 * x[:, 1]) * x[:, 0], x[:, 0] - x[:, 1] ** 2], axis=1)
    y = y + 0.05 * rng.standard_normal(y.shape)
    if missing:
        y[rng.uniform(size=y.shape) < missing] = np.nan
        y[0] = [0.3, -0.2, 0.1]
    return x, y, rng.uniform(0.1, 0.9, (ns, 2))


@pytest.mark.parametrize("wrt", [0, 1])
def test_model_mean_derivative_is_the_derivative_of_predict_moments_under_replace(oracle_engine, wrt):
    """Central differences (step 1e-5) of predict_moments(latent=True) on the oracle engine, replace=True, against the restatement's
    analytic total derivative.  The tolerance is not chosen: it is 10 x the discrepancy between the restatement's analytic value and the
    restatement's OWN central difference (oracle.gpar_ref.gpar_predict_moments, the same chain in numpy) at the same step - what a
    central difference of this chain is good for.  Measured here: discrepancy 9.5e-9 (wrt = 0) and 1.1e-8 (wrt = 1) on derivatives of
    size up to 5.6 and 3.2."""
    config = dict(per=True, input_linear=True, spectral=1, nonlinear=True, noise=0.05)
    x, y, xs = _model_data()
    reg = GPARRegressor(replace=True, impute=True, normalise_y=True, **config)
    reg.condition(x, y)
    h = 1e-5
    step = np.zeros_like(xs)
    step[:, wrt] = h
    got = [reg.predict_moments(xs + s * step, latent=True)[0] for s in (1, -1)]
    hypers = reg.get_variables()   # (the variables exist once the layers have been built)
    analytic, _ = dr.model_derivative(x, y, hypers, reg.model_config, xs, wrt, impute=True, replace=True, variance=False, normalise_y=True)
    own = [gpar_ref.gpar_predict_moments(x, y, None, hypers, reg.model_config, xs + s * step, latent=True, impute=True, replace=True)[0] for s in (1, -1)]
    discrepancy = np.abs(analytic - (own[0] - own[1]) / (2 * h)).max()
    print(f"wrt={wrt}: restatement analytic against its own central difference: {discrepancy:.3e}; max |derivative| {np.abs(analytic).max():.3f}")
    assert 0 < discrepancy < 1e-6   # (a central difference at 1e-5: h^2 |f'''| / 6 + 2^-53 |f| / h)
    np.testing.assert_allclose((got[0] - got[1]) / (2 * h), analytic, rtol=0, atol=10 * discrepancy)


# ---- (c) the J builder ------------------------------------------------------------------------------------------------------------------------
def test_feature_directions_against_central_differences_of_the_feature_map():
    """J[c][a][q] = d z_q / d x along U: central differences (step 1e-6) of oracle.kernels.features.  Tolerance 1e-8: truncation
    h^2 freq^3 / 6 / scale = 1e-12 * 10.5^3 / 6 = 2e-10 for the embedded dims, rounding 2^-53 |z| / h = 2e-10."""
    from gpar_amd.hip import feature_directions
    from gpar_amd.kernels import EQ, Cosine, Kernel, Linear, Matern32, compile_kernel

    parts = [1.3 * EQ().stretch(np.array([0.7, 1.1])).select([0, 2]),
             0.7 * (EQ().stretch(np.array([1.0, 1.4, 0.9, 1.2])).periodic(np.array([0.6, 1.7])).select([0, 1]) * EQ().stretch(3.0).select([0])),
             0.5 * (Matern32().stretch(1.0).select([1]) * Linear().stretch(2.0).select([2])),
             0.4 * Cosine().stretch(np.array([0.5, 0.9])).select([0, 1])]
    kernel = Kernel([t for k in parts for t in k.terms])
    ck = compile_kernel(kernel, 3)
    rng = np.random.default_rng(5)
    xs, U = rng.uniform(-1, 1, (6, 3)), rng.standard_normal((2, 6, 3))
    J = feature_directions(ck, torch.tensor(xs), torch.tensor(U)).numpy()
    assert J.shape == (2, 6, ck.dz)
    factors = [f for t in ok.spec_to_dict(ck.kernel)["terms"] for f in t["factors"]]
    feats = lambda pts: np.concatenate([ok.features(f, pts) for f in factors], axis=1)
    assert feats(xs).shape[1] == ck.dz
    h = 1e-6
    for c in range(2):
        want = (feats(xs + h * U[c]) - feats(xs - h * U[c])) / (2 * h)
        np.testing.assert_allclose(J[c], want, rtol=0, atol=1e-8)
    one = feature_directions(ck, torch.tensor(xs), torch.tensor(U[0])).numpy()   # (a single n* x width field)
    np.testing.assert_array_equal(one, J[:1])
    with pytest.raises(ValueError, match="width"):
        feature_directions(ck, torch.tensor(xs), torch.tensor(U[:, :, :2]))


# ---- (d) errors that are raised before any engine call, (e) the engine without the kernel -------------------------------------------------------
def test_error_surface(oracle_engine):
    x, y, xs = _model_data(missing=0)
    with pytest.raises(RuntimeError, match="condition or fit"):
        GPARRegressor().derivative(xs)
    logged = GPARRegressor(transform_y=log_transform)
    logged.condition(x, np.exp(y))
    with pytest.raises(ValueError, match="identity output transform"):
        logged.derivative(xs)
    sparse = GPARRegressor(x_ind=x[:5])
    sparse.condition(x, y)
    with pytest.raises(ValueError, match="inducing points"):
        sparse.derivative(xs)
    rough = GPARRegressor(matern=0.5)
    rough.condition(x, y)
    with pytest.raises(ValueError, match="not differentiable"):
        rough.derivative(xs)
    reg = GPARRegressor()
    reg.condition(x, y)
    for wrt in (-1, 2):
        with pytest.raises(ValueError, match="wrt"):
            reg.derivative(xs, wrt=wrt)


def test_process_level_errors(oracle_engine):
    from gpar_amd.gp import GP, Obs, PseudoObs
    from gpar_amd.kernels import EQ, Matern12

    x, y, xs = _model_data(missing=0)
    U = np.ones_like(xs)
    f = GP(EQ())
    with pytest.raises(ValueError, match="conditioned"):
        f.derivative_moments(xs, U)
    with pytest.raises(ValueError, match="inducing points"):
        (f | PseudoObs(f(x[:5]), f(x, 0.1), y[:, :1])).derivative_moments(xs, U)
    g = GP(Matern12())
    with pytest.raises(ValueError, match="not differentiable"):
        (g | Obs(g(x, 0.1), y[:, :1])).derivative_moments(xs, U)


def test_an_engine_without_the_kernel_raises_not_implemented(oracle_engine):
    x, y, xs = _model_data(missing=0)
    reg = GPARRegressor()
    reg.condition(x, y)
    assert not hasattr(oracle_engine, "posterior_deriv")
    with pytest.raises(NotImplementedError, match="posterior_deriv"):
        reg.derivative(xs)
    with pytest.raises(NotImplementedError, match="posterior_deriv"):
        reg.derivative(xs, wrt=1, variance=False)


# ---- (f) the ABI text -------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_documents_state_abi_21():
    from gpar_amd import _lib

    header = open(os.path.join(ROOT, "include", "gpar_hip.h")).read()
    assert re.findall(r"#define\s+GPAR_ABI_VERSION\s+(\d+)", header) == ["21"]
    assert re.findall(r"#define\s+GPAR_WS_POSTERIOR_DERIV\s+(\d+)", header) == [str(_lib.WS_POSTERIOR_DERIV)] == ["16"]
    assert len(re.findall(r"\bint gpar_posterior_deriv\(", header)) == 1
    assert _lib.ABI_VERSION == 21 and "gpar_posterior_deriv" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["gpar_posterior_deriv"][1]) == 22   # (the header's argument list)
    assert "gpar_posterior_deriv" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "gram_deriv.h" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
