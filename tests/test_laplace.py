"""Hyperparameter uncertainty, the host side: the pseudo-inverse and flat-direction rule of `laplace`, the block assembly over layers, the
refusals of `laplace` / `predict_moments_hyper`, and what the header and the binding state about gpar_gram_grad_rows."""
import os
import re

import numpy as np
import pytest

from gpar_amd import GPARRegressor, HyperPosterior, log_transform
from gpar_amd.regression import block_diagonal, laplace_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(n=12, p=2, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n, 1))
    y = np.stack([np.sin(5 * x[:, 0]) + 0.1 * k * x[:, 0] for k in range(p)], axis=1) + 0.05 * rng.standard_normal((n, p))
    return x, y, rng.uniform(0, 1, (4, 1))


def test_pseudo_inverse_leaves_flat_directions_out():
    """A hand-made 3 x 3 Hessian with eigenvalues (4, 0, -1): one direction is kept, two are flat."""
    q, _ = np.linalg.qr(np.array([[1.0, 2.0, 0.5], [0.3, 1.0, -1.0], [2.0, 0.1, 1.0]]))
    H = q @ np.diag([4.0, 0.0, -1.0]) @ q.T
    sigma, flat, support = laplace_block(H)
    assert flat == 2
    np.testing.assert_allclose(sigma, np.outer(q[:, 0], q[:, 0]) / 4.0, rtol=0, atol=1e-14)
    np.testing.assert_allclose(support, q[:, 0] ** 2, rtol=0, atol=1e-14)
    # a positive-definite Hessian: the plain inverse, nothing flat
    H = q @ np.diag([4.0, 2.0, 0.5]) @ q.T
    sigma, flat, support = laplace_block(H)
    assert flat == 0
    np.testing.assert_allclose(sigma, np.linalg.inv(H), rtol=1e-12)
    np.testing.assert_allclose(support, np.ones(3), rtol=1e-12)
    # the threshold is relative: 1e-10 lambda_max itself is flat, a little above it is kept
    assert laplace_block(np.diag([1.0, 1e-10]))[1] == 1 and laplace_block(np.diag([1.0, 1.1e-10]))[1] == 0
    # a coordinate lying wholly in flat directions has no support
    sigma, flat, support = laplace_block(np.diag([2.0, 0.0]))
    assert flat == 1 and support[1] == 0.0 and sigma[1, 1] == 0.0 and sigma[0, 0] == 0.5
    # nothing positive at all: everything flat, a zero covariance
    sigma, flat, _ = laplace_block(-np.eye(2))
    assert flat == 2 and np.all(sigma == 0.0)
    assert laplace_block(np.zeros((0, 0)))[1] == 0


def test_block_assembly_over_layers():
    a, b, c = np.array([[1.0, 2.0], [3.0, 4.0]]), np.zeros((0, 0)), np.array([[5.0]])
    got = block_diagonal([a, b, c])
    assert got.shape == (3, 3)
    assert np.array_equal(got, np.array([[1.0, 2.0, 0.0], [3.0, 4.0, 0.0], [0.0, 0.0, 5.0]]))
    assert block_diagonal([]).shape == (0, 0)


def test_the_named_object():
    assert HyperPosterior._fields[:5] == ("names", "value", "stderr", "cov", "flat")


def _some_hp():
    return HyperPosterior((), (), (), np.zeros((0, 0)), (), (), ())


def test_refusals(oracle_engine):
    x, y, xs = _data()
    with pytest.raises(RuntimeError, match="condition or fit"):
        GPARRegressor(replace=True).laplace(x, y)
    with pytest.raises(RuntimeError, match="condition or fit"):
        GPARRegressor(replace=True).predict_moments_hyper(xs, _some_hp())
    sparse = GPARRegressor(replace=True, x_ind=np.linspace(0, 1, 5))
    sparse.condition(x, y)
    with pytest.raises(ValueError, match="inducing points"):
        sparse.laplace(x, y)
    with pytest.raises(ValueError, match="inducing points"):
        sparse.predict_moments_hyper(xs, _some_hp())
    warped = GPARRegressor(replace=True, transform_y=log_transform)
    warped.condition(x, np.abs(y) + 1.0)
    with pytest.raises(ValueError, match="identity output transform"):
        warped.predict_moments_hyper(xs, _some_hp())
    rough = GPARRegressor(replace=True, matern=0.5)   # (served with one output: tests/test_laplace_gpu.py)
    rough.condition(x, y)
    with pytest.raises(ValueError, match="matern=0.5 with more than one output"):
        rough.predict_moments_hyper(xs, _some_hp())


def test_an_engine_without_the_kernel_raises_not_implemented(oracle_engine):
    x, y, xs = _data()
    reg = GPARRegressor(replace=True)
    reg.condition(x, y)
    assert not hasattr(oracle_engine, "gram_grad_rows")
    with pytest.raises(NotImplementedError, match="gram_grad_rows"):
        reg.predict_moments_hyper(xs, _some_hp())
    with pytest.raises(NotImplementedError, match="gram_grad_rows"):
        reg.laplace(x, y)


def test_the_process_refuses_an_engine_without_the_kernel(oracle_engine):
    from gpar_amd.gp import GP, Obs
    from gpar_amd.kernels import EQ

    x, y, xs = _data(p=1)
    f = GP(EQ())
    obs = Obs(f(oracle_engine.tensor(x), 0.1), oracle_engine.tensor(y))
    with pytest.raises(NotImplementedError, match="gram_grad_rows"):
        obs.mean_sensitivity((f | obs)._pts(oracle_engine.tensor(xs)), np.ones((1, 4)), np.zeros(1), 0.1)


def test_header_and_binding_state_the_entry_within_abi_21():
    from gpar_amd import _lib

    header = open(os.path.join(ROOT, "include", "gpar_hip.h")).read()
    assert re.findall(r"#define\s+GPAR_ABI_VERSION\s+(\d+)", header) == ["21"]
    assert re.findall(r"#define\s+GPAR_WS_GRAM_GRAD_ROWS\s+(\d+)", header) == [str(_lib.WS_GRAM_GRAD_ROWS)] == ["17"]
    assert len(re.findall(r"\bint gpar_gram_grad_rows\(", header)) == 1
    assert _lib.ABI_VERSION == 21 and "gpar_gram_grad_rows" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["gpar_gram_grad_rows"][1]) == 16
    assert "gpar_gram_grad_rows" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
