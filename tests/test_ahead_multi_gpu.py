"""Multi-horizon rolling-origin forecast scoring on the GPU: gpar_ahead_multi_dense / gpar_ahead_multi_dense_grad /
gpar_ahead_multi_dense_grad_finish through the C ABI against the brute-force numpy yardstick (one fresh conditioning per scored row and
horizon, the scoring rule applied in numpy; gradients by the complex step of that same weighted value), then `Obs.ahead` with K x n origins,
`GPARRegressor.ahead(horizon=(...))` and `fit(objective="ahead", horizon=(...), horizon_weights=(...))` end to end.

Sizes 1 / 2 / 31 / 32 / 33 / 63 / 64 / 65 / 130: the smallest, around the 32-row tile of the abar and banded kernels (and the chunk of origins
they skip by), around two tiles and the 64 lanes of the row kernel's walk, and several tiles across a 128-wide GEMM tile.  Horizon sets
(1,), (1, 2), (7, 1, 64), (2, 65, n) and (1, ..., 8), the cap: one horizon, two neighbours, an unsorted set whose longest member crosses the
wave, one that reaches the prior, and every register of the row kernel.  Sets whose smallest horizon is not below n predict every row from
the prior in every horizon and are dropped but for a few kept on purpose.  The weights are never uniform and the scoring rule changes
from case to case.  Tolerances: the parity rules (tests/test_ahead_gpu.py) - values rtol 1e-10, means / variances rtol 1e-8 / atol 1e-10,
W and gradients rtol 1e-6 / atol 1e-7, trained objectives of the two training routes rtol 1e-6.
"""
import ctypes

import numpy as np
import pytest
import torch

from .conftest import make_engine
from .test_ahead import _KW, origins_for, ragged_origin, regressor_data
from .test_ahead_multi import multi_brute_force, regressor_multi_brute_force
from .test_loo_gpu import KERNELS, _library_grads, _library_kernel

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 130]
SETS = {"one": (1,), "two": (1, 2), "three": (7, 1, 64), "prior": (2, 65, None), "cap": (1, 2, 3, 4, 5, 6, 7, 8)}   # None: n
RULES = ("log", "crps", "se")


@pytest.fixture
def hip():
    from gpar_amd.engine import set_engine

    eng = make_engine("hip")
    previous = set_engine(eng)
    yield eng
    set_engine(previous)


def horizons_of(key, n):
    return tuple(n if h is None else h for h in SETS[key])


def ragged_origins(n):
    """Three origin arrays: ragged with every third row unscored (in ALL three), a horizon of two from row 5 (rows 1, 2 and 4 unscored in
    this array alone), ragged again with another seed."""
    return np.stack([ragged_origin(n), origins_for(n, 2, start=min(5, n - 1)), ragged_origin(n, seed=9)])


def weights_of(k):
    return 0.5 + 0.75 * np.arange(k)


_CASES = {}


def _case(name, n, key, rule="log", weighted=True):
    """Inputs and the brute-force reference of one case, computed once and shared by the tests (never modified)."""
    ident = (name, n, key, rule, weighted)
    if ident not in _CASES:
        kfun, theta = KERNELS[name]
        rng = np.random.default_rng(1000 * n + weighted)
        t = (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / max(n, 8)
        x = np.stack([t, rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)], axis=1)
        y = np.sin(5.0 * x[:, 0]) + np.cos(3.0 * x[:, 1]) + 0.5 * x[:, 2] + 0.2 * rng.standard_normal(n)
        noise = 0.05 / rng.uniform(0.5, 2.0, n) if weighted else np.full(n, 0.05)
        origins = ragged_origins(n) if key == "ragged" else np.stack([origins_for(n, h) for h in horizons_of(key, n)])
        w = weights_of(len(origins))

        def value(th, d):
            return multi_brute_force(kfun(x, th) + np.diag(d) + 1e-12 * np.eye(n), y, origins, w, rule)[0]

        K = kfun(x, theta) + np.diag(noise) + 1e-12 * np.eye(n)
        val, values, mean, var = multi_brute_force(K, y, origins, w, rule)
        grads = np.zeros(theta.size)
        for j in range(theta.size):
            moved = theta.astype(complex)
            moved[j] += 1e-30j
            grads[j] = np.imag(value(moved, noise)) / 1e-30
        rows = np.arange(n) if n <= 33 else np.unique(np.linspace(0, n - 1, 4).astype(int))
        half = np.zeros(rows.size)
        for i, a in enumerate(rows):   # d value / d noise_a = 1/2 W_aa
            moved = noise.astype(complex)
            moved[a] += 1e-30j
            half[i] = np.imag(value(theta.astype(complex), moved)) / 1e-30
        _CASES[ident] = dict(x=x, y=y, noise=noise, origins=origins, weights=w, K=K, value=val, values=values, mean=mean, var=var, grads=grads,
                             rows=rows, half=half, logdet=np.linalg.slogdet(K)[1], name=name, rule=rule)
    return _CASES[ident]


def _padded(rows, cols, pad, dev, fill=None):
    buf = torch.empty(rows, cols + pad, dtype=torch.float64, device=dev)
    if fill is not None:
        buf.fill_(fill)
    return buf[:, :cols]


def _call(hip, case, mode, pad=0, origins=None, noise=None, prefill=None, nh=None, weights=None, refused=False):
    """One C ABI call with every buffer allocated here (leading dimensions widened by `pad`): "value", "grad", or "finish" (build + batched
    factorisation + gpar_ahead_multi_dense_grad_finish).  `nh`, `weights`: what the call is told instead of the case's.  `refused`: the
    status is returned instead of checked.  Returns a dict of the outputs."""
    from gpar_amd import _lib
    from gpar_amd import hip as lib

    name = case["name"]
    ck = hip.compile(_library_kernel(name, KERNELS[name][1]), 3)
    dev = torch.device("cuda:0")
    n = len(case["y"])
    og_host = np.asarray(case["origins"] if origins is None else origins)
    k = len(og_host)
    nh = k if nh is None else nh
    rows = max(k, nh)   # (a refused nh above the case's: the buffers are still as large as the call is told)
    x = _padded(n, 3, pad, dev)
    x.copy_(torch.tensor(case["x"]))
    y = torch.tensor(case["y"], device=dev)
    nz = torch.tensor(case["noise"] if noise is None else noise, device=dev)
    og = torch.zeros(rows, n, dtype=torch.int32, device=dev)
    og[:k].copy_(torch.tensor(og_host, dtype=torch.int32))
    w_host = np.ones(rows)
    w_host[:k] = case["weights"]
    if weights is not None:
        w_host[:len(weights)] = weights
    w = (ctypes.c_double * rows)(*w_host)
    cdll, nacc = _lib.load(), _lib.GRAD_NACC
    z, zd = _padded(n, 3, pad, dev), _padded(n, 3, pad, dev, fill=0.0)
    A = _padded(n + 1, n + 1, pad + (n + 1) % 2, dev)
    X, W = _padded(n, n, pad + n % 2, dev), _padded(n, n, pad + n % 2, dev)
    nblocks = max(1, min(((n + 63) // 64) * ((n + 63) // 64 + 1) // 2, 1024))
    grad = mode != "value"
    nvec = int(cdll.gpar_workspace_doubles(_lib.WS_AHEAD_MULTI, n, int(grad), rows))
    off_t = 3 * rows * n + 2 * n
    assert nvec == (off_t + off_t % 2 + n * (n + n % 2) if grad else rows * n)
    vec = torch.empty(nvec, dtype=torch.float64, device=dev)
    work, alpha = torch.empty(nblocks * nacc, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    fill = -7.0 if prefill else 0.0
    out = torch.full((2 + nacc,), fill, dtype=torch.float64, device=dev)
    values = torch.full((rows,), fill, dtype=torch.float64, device=dev)
    half = torch.full((n,), fill, dtype=torch.float64, device=dev)
    moments = torch.full((2, rows, n), fill, dtype=torch.float64, device=dev)
    info = torch.zeros(2, dtype=torch.int32, device=dev)
    stream = lib.stream_ptr(dev)
    fs, ks = ctypes.byref(ck.fspec), ctypes.byref(ck.kspec)
    ld = lib._ld
    multi = (og.data_ptr(), nh, w, values.data_ptr(), _lib.SCORES[case["rule"]])
    if mode == "value":
        rc = cdll.gpar_ahead_multi_dense(fs, ks, x.data_ptr(), n, ld(x), y.data_ptr(), 1, nz.data_ptr(), 1e-12, z.data_ptr(), ld(z), A.data_ptr(), ld(A),
                                         vec.data_ptr(), out.data_ptr(), moments[0].data_ptr(), moments[1].data_ptr(), *multi, info.data_ptr(), 0,
                                         stream)
    elif mode == "grad":
        rc = cdll.gpar_ahead_multi_dense_grad(fs, ks, x.data_ptr(), n, ld(x), y.data_ptr(), 1, nz.data_ptr(), 1e-12, z.data_ptr(), zd.data_ptr(), ld(z),
                                              A.data_ptr(), ld(A), X.data_ptr(), ld(X), W.data_ptr(), ld(W), alpha.data_ptr(), vec.data_ptr(),
                                              work.data_ptr(), nblocks, out.data_ptr(), half.data_ptr(), moments[0].data_ptr(),
                                              moments[1].data_ptr(), *multi, info.data_ptr(), 0, stream)
    else:
        logdet = torch.zeros(1, dtype=torch.float64, device=dev)
        _lib.check(cdll.gpar_logpdf_dense_build(fs, ks, x.data_ptr(), n, ld(x), y.data_ptr(), 1, nz.data_ptr(), 1e-12, z.data_ptr(), ld(z), A.data_ptr(),
                                                ld(A), logdet.data_ptr(), info.data_ptr(), stream), "build")
        _lib.check(cdll.gpar_potrf_batch(A.data_ptr(), 1, 0, n + 1, n, ld(A), logdet.data_ptr(), info.data_ptr(), 0, stream), "potrf_batch")
        rc = cdll.gpar_ahead_multi_dense_grad_finish(fs, ks, x.data_ptr(), n, ld(x), y.data_ptr(), 1, z.data_ptr(), zd.data_ptr(), ld(z), A.data_ptr(),
                                                     ld(A), logdet.data_ptr(), info.data_ptr(), X.data_ptr(), ld(X), W.data_ptr(), ld(W),
                                                     alpha.data_ptr(), vec.data_ptr(), work.data_ptr(), nblocks, out.data_ptr(), half.data_ptr(),
                                                     moments[0].data_ptr(), moments[1].data_ptr(), *multi, info[1:].data_ptr(), stream)
    if not refused:
        _lib.check(rc, "gpar_ahead_multi_dense" + {"value": "", "grad": "_grad", "finish": "_grad_finish"}[mode])
    torch.cuda.synchronize()
    return dict(out=out, values=values, half=half, mean=moments[0], var=moments[1], info=info.cpu().tolist(), W=W, ck=ck, rc=rc)


def _check(hip, case, got, grad):
    n, k = len(case["y"]), len(case["origins"])
    out = got["out"].cpu().numpy()
    values = got["values"].cpu().numpy()[:k]
    print(f"  n={n} {case['rule']}: value {out[0]:.12e} (ref {case['value']:.12e}), per horizon {values} (ref {case['values']})")
    np.testing.assert_allclose(values, case["values"], rtol=1e-10)
    np.testing.assert_allclose(out[0], case["value"], rtol=1e-10)
    np.testing.assert_allclose(out[1], case["logdet"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(got["mean"].cpu().numpy()[:k], case["mean"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(got["var"].cpu().numpy()[:k], case["var"], rtol=1e-8, atol=1e-10)
    assert np.array_equal(np.isnan(got["mean"].cpu().numpy()[:k]), case["origins"] < 0)
    if not grad:
        return
    grads = _library_grads(case["name"], hip._grads_from_moments(got["ck"], out[2:], 0.5))
    print(f"  gradients {grads} (ref {case['grads']})")
    np.testing.assert_allclose(grads, case["grads"], rtol=1e-6, atol=1e-7)
    half = got["half"].cpu().numpy()
    np.testing.assert_allclose(half[case["rows"]], case["half"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(half, 0.5 * np.diag(got["W"].cpu().numpy()), rtol=0, atol=0)


PRIOR_ONLY = {(1, "one"), (1, "prior"), (1, "cap"), (2, "prior")}   # kept although no horizon of the set is below n
ABI_CASES = [(n, key) for n in SIZES for key in SETS if min(horizons_of(key, n)) < n or (n, key) in PRIOR_ONLY]


@pytest.mark.parametrize("n,key", ABI_CASES, ids=lambda v: str(v))
def test_the_three_entries_against_the_brute_force(hip, n, key):
    k = len(SETS[key])
    name = "eq_linear" if (n + k) % 2 == 0 else "rq_periodic"
    case = _case(name, n, key, rule=RULES[(n + k) % 3], weighted=n % 2 == 1)
    value_only = _call(hip, case, "value")
    assert value_only["info"] == [0, 0]
    _check(hip, case, value_only, grad=False)
    one_call = _call(hip, case, "grad")
    assert one_call["info"] == [0, 0]
    _check(hip, case, one_call, grad=True)
    if key == "prior":   # the last horizon is n: from the prior, mean 0 and var = diag K
        np.testing.assert_allclose(one_call["mean"].cpu().numpy()[-1], 0.0, atol=1e-10)
        np.testing.assert_allclose(one_call["var"].cpu().numpy()[-1], np.diag(case["K"]), rtol=1e-8)


@pytest.mark.parametrize("n,rule", [(33, "log"), (130, "crps")])
def test_ragged_origins_with_rows_unscored_in_some_horizons_and_in_all(hip, n, rule):
    case = _case("rq_periodic", n, "ragged", rule=rule)
    unscored = case["origins"] < 0
    assert unscored.all(axis=0).any() and (unscored.any(axis=0) & ~unscored.all(axis=0)).any()
    got = _call(hip, case, "grad")
    assert got["info"] == [0, 0]
    _check(hip, case, got, grad=True)
    _check(hip, case, _call(hip, case, "value"), grad=False)


@pytest.mark.parametrize("rule", RULES)
def test_the_whole_of_w_against_the_complex_step_on_the_entries_of_k(hip, rule):
    """7 rows, ragged: W_ab = d value / d K_ab with K_ab and K_ba moved together (a != b), 2 d value / d K_aa on the diagonal."""
    n = 7
    case = _case("eq_linear", n, "ragged", rule=rule)
    W = np.zeros((n, n))
    for a in range(n):
        for b in range(a + 1):
            moved = case["K"].astype(complex)
            moved[a, b] += 1e-30j
            if a != b:
                moved[b, a] += 1e-30j
            W[a, b] = np.imag(multi_brute_force(moved, case["y"], case["origins"], case["weights"], rule)[0]) / 1e-30 * (2.0 if a == b else 1.0)
    got = _call(hip, case, "grad")["W"].cpu().numpy()
    il = np.tril_indices(n)
    np.testing.assert_allclose(got[il], W[il], rtol=1e-6, atol=1e-7)


def test_padded_leading_dimensions(hip):
    case = _case("eq_linear", 65, "three")
    got = _call(hip, case, "grad", pad=5)
    assert got["info"] == [0, 0]
    _check(hip, case, got, grad=True)
    _check(hip, case, _call(hip, case, "value", pad=3), grad=False)


def test_finish_form_gives_the_bits_of_the_one_call_form_and_two_calls_give_the_same_bits(hip):
    for n, key in ((130, "three"), (65, "ragged"), (64, "cap")):
        case = _case("rq_periodic", n, key)
        first, second, finish = _call(hip, case, "grad"), _call(hip, case, "grad"), _call(hip, case, "finish")
        assert first["info"] == [0, 0] and finish["info"] == [0, 0]
        il = torch.tril_indices(n, n)
        for other in (second, finish):
            assert torch.equal(other["out"], first["out"]) and torch.equal(other["half"], first["half"])
            assert torch.equal(other["values"], first["values"])
            assert torch.equal(other["var"].nan_to_num(-1.0), first["var"].nan_to_num(-1.0))
            assert torch.equal(other["mean"].nan_to_num(-1.0), first["mean"].nan_to_num(-1.0))
            assert torch.equal(other["W"][il[0], il[1]], first["W"][il[0], il[1]])


def _untouched(got):
    tail = slice(2, None)
    return (float(got["out"][0]) == -7.0 and bool((got["out"][tail] == -7.0).all()) and bool((got["values"] == -7.0).all())
            and bool((got["mean"] == -7.0).all()) and bool((got["var"] == -7.0).all()) and bool((got["half"] == -7.0).all()))


def test_a_bad_origin_in_a_later_horizon_and_a_matrix_that_is_not_positive_definite_report_and_leave_the_outputs(hip):
    n = 33
    case = _case("eq_linear", n, "three")
    for mode in ("value", "grad", "finish"):
        bad = case["origins"].copy()
        bad[1, 20], bad[2, 25], bad[0, 30] = 21, -2, 31   # (horizons 1 and 2 and, further down, 0: the smallest bad row is the one reported)
        got = _call(hip, case, mode, origins=bad, prefill=True)
        assert got["info"][1 if mode == "finish" else 0] == n + 1 + 20
        assert _untouched(got)
        noise = case["noise"].copy()
        noise[10] = -50.0   # K + D loses its positive definiteness at row 11
        got = _call(hip, case, mode, noise=noise, prefill=True)
        assert got["info"][0] == 11
        assert _untouched(got)


def test_too_many_horizons_and_a_weight_that_is_not_positive_are_argument_errors_that_touch_nothing(hip):
    case = _case("eq_linear", 33, "three")
    for mode in ("value", "grad", "finish"):
        for told, status in ((dict(nh=9), -1015), (dict(nh=0), -1015), (dict(weights=[1.0, 0.0]), -1016), (dict(weights=[-1.0]), -1016),
                             (dict(weights=[1.0, 1.0, float("inf")]), -1016), (dict(weights=[float("nan")]), -1016)):
            got = _call(hip, case, mode, prefill=True, refused=True, **told)
            assert got["rc"] == status, (mode, told, got["rc"])
            assert _untouched(got) and got["info"][-1] == 0


def test_fused_and_composed_routes_agree_through_obs_ahead(hip):
    from gpar_amd.gp import GP, Obs
    from gpar_amd.kernels import EQ, RQ

    n = 130
    case = _case("rq_periodic", n, "three")
    theta = KERNELS["rq_periodic"][1]
    results = {}
    for fused in (True, False):
        params = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in theta]
        kernel = RQ(params[1]).stretch(params[0]).select([0]) * EQ().stretch(params[2]).periodic(params[3]).select([1])
        noise = torch.tensor(case["noise"], device="cuda:0", requires_grad=True)
        obs = Obs(GP(kernel)(hip.tensor(case["x"]), noise), hip.tensor(case["y"]))
        with hip.defer_checks():
            if not fused:
                obs.factor()   # (a factor that exists already: the one-call entry does not apply, the composed route runs)
            value, mean, var = obs.ahead(case["origins"], weights=case["weights"])
            value.backward()
        results[fused] = (float(value.detach()), mean.cpu().numpy(), var.cpu().numpy(), np.array([float(p.grad) for p in params]),
                          noise.grad.cpu().numpy(), obs._held_out_values.cpu().numpy())
    a, b = results[True], results[False]
    np.testing.assert_allclose(a[0], case["value"], rtol=1e-10)
    np.testing.assert_allclose(a[0], b[0], rtol=1e-10)
    np.testing.assert_allclose(a[5], case["values"], rtol=1e-10)
    np.testing.assert_allclose(b[5], case["values"], rtol=1e-10)
    np.testing.assert_allclose(a[1], b[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(a[2], b[2], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(a[3], b[3], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(a[4], b[4], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(a[3], case["grads"], rtol=1e-6, atol=1e-7)


def test_regressor_ahead_on_the_gpu_against_the_brute_force(hip):
    from gpar_amd.regression import GPARRegressor

    n, p, horizons, start, weights = 60, 3, (1, 4, 16), 5, (1.0, 0.5, 2.0)
    x, y = regressor_data(n, p, seed=11, missing=0.1)
    reg = GPARRegressor(impute=False, **_KW)
    value, mean, var = reg.ahead(x, y, horizon=horizons, start=start, horizon_weights=weights)
    want = regressor_multi_brute_force(x, y, horizons, start, weights=weights)
    np.testing.assert_allclose(float(value), want[0], rtol=1e-10)
    np.testing.assert_allclose(reg.ahead_values_, want[1], rtol=1e-10)
    np.testing.assert_allclose(mean, want[2], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var, want[3], rtol=1e-8, atol=1e-10)
    # a scalar horizon returns what the single-horizon entries return: the same moments, the shapes of before
    value_4, mean_4, var_4 = reg.ahead(x, y, horizon=4, start=start)
    assert mean_4.shape == (n, p)
    np.testing.assert_allclose(float(value_4), want[1][1], rtol=1e-10)
    np.testing.assert_allclose(mean_4, want[2][1], rtol=1e-8, atol=1e-10)


def test_fit_on_two_horizons_by_the_prepared_and_the_general_route(hip):
    from gpar_amd.regression import GPARRegressor

    x, y = regressor_data(200, 2, seed=21, missing=0.0)
    finals = {}
    for fast in (True, False):
        reg = GPARRegressor(**_KW)
        reg.fast_fit = fast
        reg.condition(x, y)
        finals[fast] = reg._train(range(2), objective="ahead", horizon=(1, 4), horizon_weights=(1, 2), iters=5)
    print("trained two-horizon objectives, prepared / general:", finals[True], finals[False])
    for pi in range(2):
        np.testing.assert_allclose(finals[True][pi], finals[False][pi], rtol=1e-6)
    before = float(GPARRegressor(**_KW).ahead(x, y, horizon=(1, 4), horizon_weights=(1, 2))[0])
    assert -sum(finals[True].values()) >= before
