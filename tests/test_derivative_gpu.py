"""Posterior derivatives on the GPU: gpar_posterior_deriv through the C ABI (padded leading dimensions and direction strides, every
differentiable factor type and the products tests/test_derivative.py pins, sizes on either side of every 64-tile edge and of a split
boundary) and GPARRegressor.derivative, against the numpy restatement tests/derivative_reference.py.

Tolerances: tests/test_decompose_gpu.py's for posterior means and marginal variances, rtol 1e-8 / atol 1e-10."""
import ctypes

import numpy as np
import pytest
import torch

from . import derivative_reference as dr
from .conftest import make_engine, to_np

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-8, 1e-10
NOISE = 0.1
SENTINEL = 7.25
NS_TRAIN = (1, 63, 64, 65, 130)
NS_TEST = (1, 64, 65, 129)
NDIRS = (1, 3)


@pytest.fixture
def hip():
    from gpar_amd.engine import set_engine

    eng = make_engine("hip")
    previous = set_engine(eng)
    yield eng
    set_engine(previous)


def _structures():
    """The kernel structures of tests/test_derivative.py as product kernels over three input columns, and their sum (8 terms, 10 factors)."""
    from gpar_amd.kernels import EQ, RQ, Cosine, Kernel, Linear, Matern32, Matern52, ZeroKernel

    out = {
        "eq": 1.3 * EQ().stretch(np.array([0.7, 1.1])).select([0, 2]),
        "rq": 1.3 * RQ(0.7).stretch(0.9).select([1]),
        "matern32": 1.3 * Matern32().stretch(np.array([0.8, 1.3])).select([0, 1]),
        "matern52": 1.3 * Matern52().stretch(1.0).select([2]),
        "linear": 1.3 * Linear().stretch(np.array([2.0, 1.5])).select([0, 1]),
        "cos": 1.3 * Cosine().stretch(0.9).select([1]),
        "per_eq_decay": 0.7 * (EQ().stretch(np.array([1.0, 1.4])).periodic(0.6).select([0]) * EQ().stretch(3.0).select([0])),
        "linear_eq": 0.5 * (Linear().stretch(np.array([2.0, 0.8])).select([1, 2]) * EQ().stretch(np.array([1.2, 0.9])).select([0, 1])),
        "linear_linear": 0.6 * (Linear().stretch(np.array([1.1, 0.7])).select([0, 1]) * Linear().stretch(np.array([0.9, 1.6])).select([1, 2])),
        "with_constant": 0.9 * Matern52().stretch(0.8).select([0]) + (ZeroKernel() + 0.3),
        "cos_two_dims": 0.4 * (EQ().stretch(1.5).select([0, 1]) * Cosine().stretch(np.array([0.5, 0.9])).select([0, 1])),
    }
    out["sum_of_all"] = Kernel([t for k in ("eq", "rq", "matern32", "per_eq_decay", "linear_linear", "cos_two_dims", "with_constant")
                                for t in out[k].terms])
    return out


NAMES = ("sum_of_all", "eq", "rq", "matern32", "matern52", "linear", "cos", "per_eq_decay", "linear_eq", "linear_linear", "with_constant",
         "cos_two_dims")


def _data(n, ns, ndir, seed=0):
    rng = np.random.default_rng(seed + 1000 * n + 10 * ns + ndir)
    return rng.uniform(-1, 1, (n, 3)), rng.standard_normal(n), rng.uniform(-1, 1, (ns, 3)), rng.standard_normal((ndir, ns, 3))


def _conditioned(hip, kernel, x, y, noise=NOISE):
    from gpar_amd.gp import GP, Obs

    f = GP(kernel)
    return f, Obs(f(hip.tensor(x), noise), hip.tensor(y))


def _lib_and_stream(eng):
    from gpar_amd import _lib, hip as hipmod

    return _lib.load(), hipmod.stream_ptr(eng.device)


def _padded(rows, cols, ld, device):
    buf = torch.full((max(rows, 1), ld), SENTINEL, dtype=torch.float64, device=device)
    return buf, buf[:rows, :cols]


def _least_workspace(n, ns, ndir, variance=True):
    """One split of the mean pass, the stack of one test row (include/gpar_hip.h)."""
    ldn = (max(n, 1) + 1) & ~1
    return max(ndir * ns, ndir * (ldn + 1) if variance and n > 0 else 0)


def _deriv(hip, obs, p, U, variance=True, ws_doubles=None, pad=3):
    """gpar_posterior_deriv through ctypes: J in a padded buffer (leading dimension dz + 2, a direction stride of one spare row), outputs
    with padded leading dimensions; asserts that the padding is untouched."""
    from gpar_amd import _lib
    from gpar_amd.hip import feature_directions

    lib, stream = _lib_and_stream(hip)
    fac = obs.factor()
    ck, z = obs.fdd.features()
    n, ns, dz = obs.fdd.n, p.n, ck.dz
    ndir = U.shape[0]
    Jbuf = torch.full((ndir, ns + 1, dz + 2), SENTINEL, dtype=torch.float64, device=hip.device)
    Jbuf[:, :ns, :dz] = feature_directions(ck, p.x, hip.tensor(U))
    alpha = fac.alpha().reshape(-1).contiguous()
    if ws_doubles is None:
        ws_doubles = lib.gpar_workspace_doubles(_lib.WS_POSTERIOR_DERIV, n, ns, ndir)
    assert ws_doubles >= _least_workspace(n, ns, ndir, variance)
    ws = torch.empty(ws_doubles + 2, dtype=torch.float64, device=hip.device)
    mbuf, mean = _padded(ndir, ns, ns + pad, hip.device)
    vbuf, var = _padded(ndir, ns, ns + pad + 1, hip.device)
    rc = lib.gpar_posterior_deriv(ctypes.byref(ck.kspec), p.z.data_ptr(), ns, int(p.z.stride(0)), Jbuf.data_ptr(), dz + 2, (ns + 1) * (dz + 2), ndir,
                                  z.data_ptr(), n, int(z.stride(0)), dz, alpha.data_ptr(), fac.L.data_ptr(), int(fac.L.stride(0)) if n > 1 else 1,
                                  mbuf.data_ptr(), ns + pad, vbuf.data_ptr() if variance else None, ns + pad + 1, ws.data_ptr(), int(ws_doubles), stream)
    assert rc == 0, rc
    assert np.all(to_np(mbuf)[:, ns:] == SENTINEL) and np.all(to_np(vbuf)[:, ns:] == SENTINEL)
    if not variance:
        assert np.all(to_np(vbuf) == SENTINEL)
    return to_np(mean).copy(), to_np(var).copy()


def _restated(spec, x, y, xs, U, noise=NOISE):
    parts = [dr.layer_derivative(spec, x, y, noise, xs, U[c]) for c in range(U.shape[0])]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])


# ---- the C ABI against the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS_TRAIN)
def test_posterior_deriv_against_the_restatement(hip, n):
    from oracle import kernels as ok

    structures = _structures()
    for i, (ns, ndir) in enumerate((ns, ndir) for ns in NS_TEST for ndir in NDIRS):
        name = NAMES[(i + NS_TRAIN.index(n) * 5) % len(NAMES)]   # (every structure meets several sizes; the sum of all meets each n)
        kernel = structures[name]
        x, y, xs, U = _data(n, ns, ndir)
        f, obs = _conditioned(hip, kernel, x, y)
        p = f._pts(hip.tensor(xs))
        spec = ok.spec_to_dict(p.ck.kernel)
        want_mean, want_var = _restated(spec, x, y, xs, U)
        what = f"{name} n={n} n*={ns} ndir={ndir}"
        mean, var = _deriv(hip, obs, p, U)
        np.testing.assert_allclose(mean, want_mean, rtol=RTOL, atol=ATOL, err_msg=what)
        np.testing.assert_allclose(var, want_var, rtol=RTOL, atol=ATOL, err_msg=what)
        again = _deriv(hip, obs, p, U)
        np.testing.assert_array_equal(mean, again[0], err_msg=what)   # the same bits every time: no atomics, fixed order
        np.testing.assert_array_equal(var, again[1], err_msg=what)
        np.testing.assert_array_equal(_deriv(hip, obs, p, U, variance=False)[0], mean, err_msg=what)   # var == NULL: the same mean bits
        small = _deriv(hip, obs, p, U, ws_doubles=_least_workspace(n, ns, ndir))   # a chunk of one test row, one split
        np.testing.assert_allclose(small[0], want_mean, rtol=RTOL, atol=ATOL, err_msg=what)
        np.testing.assert_allclose(small[1], want_var, rtol=RTOL, atol=ATOL, err_msg=what)


def test_a_zero_direction_gives_exactly_zero(hip):
    kernel = _structures()["sum_of_all"]
    x, y, xs, U = _data(65, 65, 3)
    U[1] = 0.0
    U[2, 10:40] = 0.0
    f, obs = _conditioned(hip, kernel, x, y)
    mean, var = _deriv(hip, obs, f._pts(hip.tensor(xs)), U)
    assert np.all(mean[1] == 0.0) and np.all(var[1] == 0.0)
    assert np.all(mean[2, 10:40] == 0.0) and np.all(var[2, 10:40] == 0.0)
    assert np.all(mean[0] != 0.0) and np.all(var[0] > 0.0)


def test_no_training_rows_gives_zero_means_and_the_prior_term(hip):
    from gpar_amd.hip import feature_directions
    from oracle import kernels as ok

    lib, stream = _lib_and_stream(hip)
    kernel = _structures()["sum_of_all"]
    _, _, xs, U = _data(0, 65, 3)
    ck = hip.compile(kernel, 3)
    xs_t = hip.tensor(xs)
    zs = hip.features(ck, xs_t)
    J = feature_directions(ck, xs_t, hip.tensor(U))
    ns, ndir = 65, 3
    ws = torch.empty(ndir * ns, dtype=torch.float64, device=hip.device)
    mean = torch.full((ndir, ns), SENTINEL, dtype=torch.float64, device=hip.device)
    var = torch.full((ndir, ns), SENTINEL, dtype=torch.float64, device=hip.device)
    rc = lib.gpar_posterior_deriv(ctypes.byref(ck.kspec), zs.data_ptr(), ns, int(zs.stride(0)), J.data_ptr(), ck.dz, ns * ck.dz, ndir, None, 0, ck.dz,
                                  ck.dz, None, None, 1, mean.data_ptr(), ns, var.data_ptr(), ns, ws.data_ptr(), ndir * ns, stream)
    assert rc == 0
    assert np.all(to_np(mean) == 0.0)
    spec = ok.spec_to_dict(ck.kernel)
    np.testing.assert_allclose(to_np(var), np.stack([dr.prior_term(spec, xs, U[c]) for c in range(ndir)]), rtol=1e-12, atol=1e-13)
    # no test rows: nothing is done
    rc = lib.gpar_posterior_deriv(ctypes.byref(ck.kspec), None, 0, ck.dz, None, ck.dz, 0, ndir, None, 0, ck.dz, ck.dz, None, None, 1, None, 1, None, 1,
                                  None, 0, stream)
    assert rc == 0


def test_argument_errors_touch_nothing(hip):
    from gpar_amd import _lib
    from gpar_amd.hip import feature_directions
    from gpar_amd.kernels import EQ, Matern12

    lib, stream = _lib_and_stream(hip)
    kernel = _structures()["sum_of_all"]
    n, ns, ndir = 20, 9, 2
    x, y, xs, U = _data(n, ns, ndir)
    f, obs = _conditioned(hip, kernel, x, y)
    p = f._pts(hip.tensor(xs))
    fac = obs.factor()
    ck, z = obs.fdd.features()
    dz = ck.dz
    J = feature_directions(ck, p.x, hip.tensor(U))
    alpha = fac.alpha().reshape(-1).contiguous()
    nws = int(lib.gpar_workspace_doubles(_lib.WS_POSTERIOR_DERIV, n, ns, ndir))
    ws = torch.empty(nws, dtype=torch.float64, device=hip.device)
    mean = torch.full((ndir, ns), SENTINEL, dtype=torch.float64, device=hip.device)
    var = torch.full((ndir, ns), SENTINEL, dtype=torch.float64, device=hip.device)
    good = dict(ks=ctypes.byref(ck.kspec), zs=p.z.data_ptr(), ns=ns, ldzs=int(p.z.stride(0)), J=J.data_ptr(), ldj=dz, stride_j=ns * dz, ndir=ndir,
                z=z.data_ptr(), n=n, ldz=int(z.stride(0)), dz=dz, alpha=alpha.data_ptr(), L=fac.L.data_ptr(), ldl=int(fac.L.stride(0)),
                mean=mean.data_ptr(), ldm=ns, var=var.data_ptr(), ldv=ns, ws=ws.data_ptr(), ws_doubles=nws, stream=stream)

    def call(**changes):
        return lib.gpar_posterior_deriv(*{**good, **changes}.values())

    rough = hip.compile(EQ().select([0]) * Matern12().select([1]), 3)
    crowded = _lib.KSpec()   # five factors in one term
    crowded.nterms, crowded.nfactors = 1, 5
    crowded.coef[0] = 1.0
    for i in range(5):
        crowded.factor[i].type, crowded.factor[i].term, crowded.factor[i].off, crowded.factor[i].nd = _lib.K_EQ, 0, i, 1
    bad = [dict(ks=None), dict(ks=ctypes.byref(rough.kspec), dz=rough.dz), dict(ks=ctypes.byref(crowded)), dict(ndir=0), dict(ndir=_lib.GPAR_MAX_TERMS + 1),
           dict(n=-1), dict(ns=-1), dict(dz=-1), dict(dz=_lib.GPAR_MAX_DIMS + 1), dict(dz=dz - 1), dict(ldzs=dz - 1), dict(ldj=dz - 1),
           dict(stride_j=ns * dz - 1), dict(ldz=dz - 1), dict(ldl=n - 1), dict(ldm=ns - 1), dict(ldv=ns - 1), dict(ws=None),
           dict(ws_doubles=ndir * ns - 1), dict(ws_doubles=_least_workspace(n, ns, ndir) - 1), dict(zs=None), dict(J=None), dict(mean=None),
           dict(z=None), dict(alpha=None), dict(L=None)]
    for changes in bad:
        rc = call(**changes)
        assert rc < 0, (changes, rc)
    torch.cuda.synchronize()
    assert np.all(to_np(mean) == SENTINEL) and np.all(to_np(var) == SENTINEL)
    assert lib.gpar_workspace_doubles(_lib.WS_POSTERIOR_DERIV, n, ns, 0) == -1
    assert call(var=None, L=None, ws_doubles=ndir * ns) == 0   # (without variances neither L nor the stack is needed)
    assert call() == 0
    torch.cuda.synchronize()
    assert not np.any(to_np(mean) == SENTINEL) and not np.any(to_np(var) == SENTINEL)


def test_variances_at_the_training_rows_under_small_noise_are_not_negative(hip):
    """Test rows equal to training rows at noise 1e-6: the prior term and the solve's norm cancel to the last digits; the variances stay
    >= -atol.  (A condition, not a measurement.)"""
    for name in ("eq", "matern52", "sum_of_all"):
        x, y, _, U = _data(65, 65, 3)
        f, obs = _conditioned(hip, _structures()[name], x, y, noise=1e-6)
        _, var = _deriv(hip, obs, f._pts(hip.tensor(x)), U)
        assert np.all(np.isfinite(var)) and var.min() >= -ATOL, (name, var.min())


# ---- GPARRegressor.derivative ----------------------------------------------------------------------------------------------------------------
N, NS, P, M = 70, 9, 3, 2
CONFIGS = {"per": dict(per=True), "input_linear": dict(input_linear=True), "spectral": dict(spectral=2), "matern": dict(matern=1.5, nonlinear=True),
           "rq": dict(rq=True, nonlinear=True), "markov": dict(markov=1, nonlinear=True)}


def _model_data(seed=0, missing=0.1, n=N):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n, M))
    y = np.stack([np.sin(6 * x[:, 0]) + x[:, 1], np.cos(5 * x[:, 1]) * x[:, 0], x[:, 0] - x[:, 1] ** 2], axis=1)
    y = y + 0.05 * rng.standard_normal(y.shape)
    if missing:
        y[rng.uniform(size=y.shape) < missing] = np.nan
        y[0] = [0.3, -0.2, 0.1]
    return x, y, rng.uniform(0.05, 0.95, (NS, M))


@pytest.mark.parametrize("replace", [False, True])
@pytest.mark.parametrize("key", sorted(CONFIGS))
def test_regressor_derivative_against_the_restatement(hip, key, replace):
    from gpar_amd import GPARRegressor

    x, y, xs = _model_data()
    reg = GPARRegressor(replace=replace, impute=True, normalise_y=True, noise=0.1, **CONFIGS[key])
    reg.condition(x, y)
    for wrt in range(M):
        mean, var = reg.derivative(xs, wrt=wrt)
        assert mean.shape == var.shape == (NS, P)
        want_mean, want_var = dr.model_derivative(x, y, reg.get_variables(), reg.model_config, xs, wrt, impute=True, replace=replace, normalise_y=True)
        np.testing.assert_allclose(mean, want_mean, rtol=RTOL, atol=ATOL, err_msg=f"{key} wrt={wrt}")
        np.testing.assert_allclose(var, want_var, rtol=RTOL, atol=ATOL, err_msg=f"{key} wrt={wrt}")
        plain = reg.derivative(xs, wrt=wrt, variance=False)
        assert plain[1] is None
        np.testing.assert_array_equal(plain[0], mean)


def test_units_of_y_per_unit_of_x(hip):
    from gpar_amd import GPARRegressor

    x, y, xs = _model_data()
    mean, std = np.nanmean(y, axis=0), np.nanstd(y, axis=0)
    config = dict(replace=True, impute=True, noise=0.1, per=True, input_linear=True, nonlinear=True)
    raw = GPARRegressor(normalise_y=True, **config)
    raw.condition(x, y)
    unit = GPARRegressor(normalise_y=False, **config)
    unit.condition(x, (y - mean) / std)
    a, b = raw.derivative(xs, wrt=1), unit.derivative(xs, wrt=1)
    for i in range(P):
        np.testing.assert_allclose(a[0][:, i], b[0][:, i] * std[i], rtol=RTOL, atol=ATOL * std[i])
        np.testing.assert_allclose(a[1][:, i], b[1][:, i] * std[i] ** 2, rtol=RTOL, atol=ATOL * std[i] ** 2)


def test_after_update_the_derivative_is_that_of_the_moved_window(hip):
    from gpar_amd import GPARRegressor

    config = dict(replace=False, impute=False, normalise_y=False, noise=0.1, per=True, spectral=2, input_linear=True, linear=True, nonlinear=True)
    x, y, xs = _model_data(missing=0, n=N + 6)
    moved = GPARRegressor(**config)
    moved.condition(x[:N], y[:N])
    moved.update(x[N:], y[N:], drop=3)
    assert moved._stream_cache is not None
    fresh = GPARRegressor(**config)
    fresh.condition(x[3:], y[3:])
    a, b = moved.derivative(xs, wrt=0), fresh.derivative(xs, wrt=0)
    np.testing.assert_allclose(a[0], b[0], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(a[1], b[1], rtol=RTOL, atol=ATOL)
