"""Pins the CPU oracle (test infrastructure) itself, on CPU:

  * Philox-4x32-10 against the published known-answer vectors of the Random123 distribution;
  * kernel definitions against hand-computed closed-form values;
  * the oracle engine's Cholesky route against a second route that uses no Cholesky (slogdet + solve), for the
    dense log marginal likelihood, posterior moments, the VFE bound and its posterior;
  * analytic kernel gradients against central finite differences;
  * the host orchestration on the oracle engine against the stand-alone numpy GPAR (oracle/gpar_ref.py);
  * the committed golden vectors (tests/golden/gpar_cases.json) against a fresh evaluation.

The reference's own stack (stheno / lab / matrix) is not installable here, so absolute parity with it is
"unpinned" (see oracle/__init__.py); what the reference's tests DO pin — identities and host-logic literals — is
covered in tests/test_gpar_model.py and tests/test_regressor.py.
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import gp_ref, gpar_ref, philox
from oracle import kernels as ok
from oracle.engine import OracleEngine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gpar_cases.json")


def test_philox_known_answer_vectors():
    # Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key) -> output
    kat = [
        ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
    ]
    for ctr, key, expect in kat:
        got = philox.philox4x32_10(*[np.array([c], dtype=np.uint32) for c in ctr], *key)
        assert tuple(int(g[0]) for g in got) == expect


def test_philox_normals_are_standard():
    z = philox.randn(7, 3, 4000, 50)
    assert abs(z.mean()) < 1e-2 and abs(z.std() - 1) < 1e-2
    assert np.array_equal(philox.randn(7, 3, 5, 3), philox.randn(7, 3, 5, 3))
    assert not np.array_equal(philox.randn(7, 3, 5, 3), philox.randn(7, 4, 5, 3))


def _f(type, cols, scales, periods=None, alpha=0.0):
    return {"type": type, "cols": cols, "scales": scales, "periods": periods, "alpha": alpha}


def test_kernel_closed_forms():
    x = np.array([[0.0, 1.0], [3.0, 5.0]])
    eq = {"terms": [{"coef": 2.0, "factors": [_f("eq", [0, 1], [1.0, 2.0])]}]}
    # r2 = 3^2 + (4/2)^2 = 13
    np.testing.assert_allclose(ok.gram(eq, x), [[2.0, 2 * np.exp(-6.5)], [2 * np.exp(-6.5), 2.0]], rtol=1e-15)
    rq = {"terms": [{"coef": 1.0, "factors": [_f("rq", [0, 1], [1.0, 2.0], alpha=0.5)]}]}
    np.testing.assert_allclose(ok.gram(rq, x)[0, 1], (1 + 13 / (2 * 0.5)) ** -0.5, rtol=1e-14)
    lin = {"terms": [{"coef": 1.0, "factors": [_f("linear", [1], [2.0])]}, {"coef": 0.25, "factors": []}]}
    np.testing.assert_allclose(ok.gram(lin, x), np.array([[0.25, 1.25], [1.25, 6.25]]) + 0.25, rtol=1e-15)
    # periodic: invariant under shifts by the period; equals EQ on the (sin, cos) embedding
    per = {"terms": [{"coef": 1.0, "factors": [_f("eq", [0], [0.7, 1.3], periods=[2.0])]}]}
    a, b = np.array([[0.3]]), np.array([[0.3 + 2.0 * 5]])
    np.testing.assert_allclose(ok.gram(per, a, b), [[1.0]], atol=1e-13)
    u, v = 0.3, 1.1
    emb = lambda t: np.array([np.sin(np.pi * t) / 0.7, np.cos(np.pi * t) / 1.3])
    np.testing.assert_allclose(ok.gram(per, np.array([[u]]), np.array([[v]])), [[np.exp(-0.5 * np.sum((emb(u) - emb(v)) ** 2))]], rtol=1e-14)
    # kernels over zero columns (markov=0 quirk): EQ -> 1, Linear -> 0
    zero_w = {"terms": [{"coef": 0.6, "factors": [_f("eq", [], [])]}, {"coef": 1.0, "factors": [_f("linear", [], [])]}]}
    np.testing.assert_allclose(ok.gram(zero_w, x), np.full((2, 2), 0.6))
    np.testing.assert_allclose(ok.gram_diag(eq, x), [2.0, 2.0])
    np.testing.assert_allclose(ok.gram_diag(lin, x), [0.5, 6.5])
    # the Matern kernels at r = sqrt(13) (include/gpar_hip.h), 1 on the diagonal and over zero columns
    for kind, value in (("matern12", np.exp(-np.sqrt(13.0))), ("matern32", (1 + np.sqrt(39.0)) * np.exp(-np.sqrt(39.0))),
                        ("matern52", (1 + np.sqrt(65.0) + 65.0 / 3.0) * np.exp(-np.sqrt(65.0)))):
        mat = {"terms": [{"coef": 2.0, "factors": [_f(kind, [0, 1], [1.0, 2.0])]}]}
        np.testing.assert_allclose(ok.gram(mat, x), [[2.0, 2 * value], [2 * value, 2.0]], rtol=1e-14)
        np.testing.assert_allclose(ok.gram_diag(mat, x), [2.0, 2.0])
        np.testing.assert_allclose(ok.gram({"terms": [{"coef": 0.6, "factors": [_f(kind, [], [])]}]}, x), np.full((2, 2), 0.6))
    # a Matern factor on the periodic embedding: the same (sin, cos) features, r instead of r2; invariant under shifts by the period
    r = np.sqrt(np.sum((emb(u) - emb(v)) ** 2))
    for kind, value in (("matern12", np.exp(-r)), ("matern32", (1 + np.sqrt(3.0) * r) * np.exp(-np.sqrt(3.0) * r)),
                        ("matern52", (1 + np.sqrt(5.0) * r + 5.0 * r * r / 3.0) * np.exp(-np.sqrt(5.0) * r))):
        mper = {"terms": [{"coef": 1.0, "factors": [_f(kind, [0], [0.7, 1.3], periods=[2.0])]}]}
        np.testing.assert_allclose(ok.gram(mper, np.array([[u]]), np.array([[v]])), [[value]], rtol=1e-14)
        np.testing.assert_allclose(ok.gram(mper, np.array([[u]]), np.array([[v + 2.0 * 3]])), [[value]], rtol=1e-12)


def test_unknown_types_raise_everywhere():
    """No branch treats an unnamed factor type as RQ (or as anything else), and `matern` outside 0.5 / 1.5 / 2.5 is refused."""
    from oracle import mp_ref
    from oracle import torch_cpu as tc

    x = np.array([[0.0, 1.0], [3.0, 5.0], [-1.0, 0.5]])
    bad = {"terms": [{"coef": 1.0, "factors": [_f("matern99", [0, 1], [1.0, 2.0])]}]}
    W = np.ones((3, 3))
    for call in (lambda: ok.gram(bad, x), lambda: ok.gram_diag(bad, x), lambda: ok.kernel_grads(bad, x, W),
                 lambda: ok.kernel_input_grads(bad, x, x, W), lambda: mp_ref.gram(bad, x.tolist()),
                 lambda: tc.gram(bad, torch.as_tensor(x))):
        with pytest.raises(ValueError, match="unknown factor type"):
            call()
    # the reference's CPU path has no Matern kernel: it refuses one rather than evaluating it as RQ with alpha = 0
    with pytest.raises(ValueError, match="unknown factor type"):
        tc.gram({"terms": [{"coef": 1.0, "factors": [_f("matern32", [0, 1], [1.0, 2.0])]}]}, torch.as_tensor(x))
    hypers = {"0/input/var": 1.0, "0/input/scales": [1.0], "0/noise": 0.1}
    for nu in (0.7, 3.5, True, "1.5"):
        with pytest.raises((ValueError, TypeError)):
            gpar_ref.layer_spec(hypers, 1, 0, dict(linear=False, matern=nu))
    with pytest.raises(ValueError, match="exclude"):
        gpar_ref.layer_spec(dict(hypers, **{"0/input/alpha": 1.0}), 1, 0, dict(linear=False, matern=1.5, rq=True))


def test_layer_spec_follows_the_regressor_for_matern():
    """config["matern"] selects the type of the two nonlinear factors and of nothing else (gpar_amd/regression.py: the locally
    periodic term keeps its EQ factors), under the variable names of the EQ model."""
    rng = np.random.default_rng(5)
    config = dict(linear=True, nonlinear=True, per=True, input_linear=True)
    for nu, kind in ((None, "eq"), (0.5, "matern12"), (1.5, "matern32"), (2.5, "matern52")):
        cfg = config if nu is None else dict(config, matern=nu)
        import importlib.util

        s = importlib.util.spec_from_file_location("make_golden", os.path.join(os.path.dirname(GOLDEN), "make_golden.py"))
        mod = importlib.util.module_from_spec(s)
        s.loader.exec_module(mod)
        hypers = mod.hypers_for(2, 2, cfg, rng)
        assert set(hypers) == set(mod.hypers_for(2, 2, config, np.random.default_rng(0)))
        spec, _ = gpar_ref.layer_spec(hypers, 2, 1, cfg)
        types = [[f["type"] for f in t["factors"]] for t in spec["terms"]]
        assert types == [[kind], ["eq", "eq"], ["linear"], [], ["linear"], [kind]]


_MATERN_CONFIGS = [dict(linear=True, nonlinear=True, matern=0.5), dict(linear=True, nonlinear=True, matern=1.5, per=True, input_linear=True),
                   dict(linear=True, nonlinear=True, matern=2.5), dict(linear=True, nonlinear=True, matern=0.5, per=True)]


def _smallest_distance(spec, x1, x2=None):
    """Smallest distance, over the stationary factors of `spec`, between two different points in the factor's own (scaled, embedded)
    features.  nu = 1/2 has a kink at r = 0: a finite-difference stencil that reaches across it has no limit, so the tests below
    assert that this is far above the stencil's reach."""
    best = np.inf
    for term in spec["terms"]:
        for f in term["factors"]:
            if f["type"] == "linear" or not len(f["cols"]):
                continue
            z1 = ok.features(f, x1)
            z2 = z1 if x2 is None else ok.features(f, x2)
            d = np.sqrt(np.sum((z1[:, None, :] - z2[None, :, :]) ** 2, axis=2))
            if x2 is None:
                d = d[~np.eye(d.shape[0], dtype=bool)]
            best = min(best, float(np.min(d)))
    return best


def _random_layer(rng, config, m=2, pi=1, p=2):
    import importlib.util

    spec_path = os.path.join(os.path.dirname(GOLDEN), "make_golden.py")
    s = importlib.util.spec_from_file_location("make_golden", spec_path)
    mod = importlib.util.module_from_spec(s)
    s.loader.exec_module(mod)
    hypers = mod.hypers_for(m, p, config, rng)
    return gpar_ref.layer_spec(hypers, m, pi, config)[0]


@pytest.mark.parametrize("config", [dict(linear=True, nonlinear=True), dict(linear=True, nonlinear=True, rq=True, per=True, input_linear=True)]
                         + _MATERN_CONFIGS)
def test_engine_cholesky_route_equals_slogdet_route(config):
    from gpar_amd.engine import set_engine
    from gpar_amd.gp import GP, Obs, PseudoObs
    from gpar_amd.kernels import Kernel

    rng = np.random.default_rng(3)
    spec = _random_layer(rng, config)
    n, ns = 17, 6
    x, xs = rng.standard_normal((n, 3)), rng.standard_normal((ns, 3))
    y = rng.standard_normal(n)
    noise = rng.uniform(0.05, 0.2, n)
    eng = OracleEngine()
    previous = set_engine(eng)
    try:
        f = GP(_kernel_from_spec(spec))
        assert abs(float(f(x, noise).logpdf(y)) - gp_ref.logpdf(spec, x, y, noise)) < 1e-10
        post = f | Obs(f(x, noise), y)
        mean, cov = gp_ref.posterior(spec, x, y, noise, xs)
        np.testing.assert_allclose(post.mean(xs).numpy()[:, 0], mean, rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(post(xs).var().numpy(), cov, rtol=1e-8, atol=1e-10)
        z = rng.standard_normal((7, 3))
        sparse = PseudoObs(f(z), f(x, noise), y)
        assert abs(float(sparse.logpdf()) - gp_ref.vfe_bound(spec, x, y, noise, z)) < 1e-9
        smean, scov = gp_ref.vfe_posterior(spec, x, y, noise, z, xs)
        spost = f | sparse
        np.testing.assert_allclose(spost.mean(xs).numpy()[:, 0], smean, rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose(spost(xs).var().numpy(), scov, rtol=1e-7, atol=1e-9)
        # Z = X: the bound is tight (reference tests/test_model.py:141-149)
        tight = PseudoObs(f(x), f(x, noise), y)
        assert abs(float(tight.logpdf()) - gp_ref.logpdf(spec, x, y, noise)) < 1e-6
    finally:
        set_engine(previous)


def _kernel_from_spec(spec):
    from gpar_amd.kernels import Factor, Kernel, Term

    terms = []
    for t in spec["terms"]:
        fs = [Factor(f["type"], tuple(f["cols"]), np.array(f["scales"]), None if f["periods"] is None else np.array(f["periods"]),
                     f["alpha"] if f["type"] == "rq" else None) for f in t["factors"]]
        terms.append(Term(t["coef"], fs))
    return Kernel(terms)


def test_partial_cholesky_is_schur_complement():
    rng = np.random.default_rng(0)
    N, nf = 9, 5
    M = rng.standard_normal((N, N))
    A = M @ M.T + N * np.eye(N)
    t = torch.tensor(A.copy())
    logdet, info = OracleEngine().potrf_(t, nf=nf)
    S = A[nf:, nf:] - A[nf:, :nf] @ np.linalg.solve(A[:nf, :nf], A[:nf, nf:])
    got = t.numpy()
    il = np.tril_indices(N - nf)
    np.testing.assert_allclose(got[nf:, nf:][il], S[il], rtol=1e-12)
    assert int(info) == 0 and np.isclose(float(logdet), np.linalg.slogdet(A[:nf, :nf])[1])
    bad = A.copy()
    bad[3, 3] = -1.0
    _, info = OracleEngine().potrf_(torch.tensor(bad))
    assert int(info) == 4


@pytest.mark.parametrize("config", [dict(linear=True, nonlinear=True), dict(linear=True, nonlinear=True, rq=True, per=True, input_linear=True)]
                         + _MATERN_CONFIGS)
def test_kernel_gradients_match_finite_differences(config):
    rng = np.random.default_rng(8)
    spec = _random_layer(rng, config)
    n = 9
    x = rng.standard_normal((n, 3))
    W = rng.standard_normal((n, n))
    W = W + W.T
    grads = ok.kernel_grads(spec, x, W)
    h = 1e-6
    # (a parameter step of h moves a feature by ~h |z| / s: four orders below the closest pair)
    assert _smallest_distance(spec, x) > 1e4 * h

    def value(s):
        return 0.5 * np.sum(W * ok.gram(s, x))

    def bump(path, delta):
        import copy

        s = copy.deepcopy(spec)
        ti, fi, key, idx = path
        if key == "coef":
            s["terms"][ti]["coef"] += delta
        elif key == "alpha":
            s["terms"][ti]["factors"][fi]["alpha"] += delta
        else:
            s["terms"][ti]["factors"][fi][key][idx] += delta
        return s

    for ti, term in enumerate(spec["terms"]):
        fd = (value(bump((ti, None, "coef", None), h)) - value(bump((ti, None, "coef", None), -h))) / (2 * h)
        assert abs(fd - grads["coef"][ti]) < 1e-6 * (1 + abs(fd))
        for fi, f in enumerate(term["factors"]):
            g = grads["factors"][ti][fi]
            for key in ("scales", "periods"):
                if g[key] is None:
                    continue
                for idx in range(len(f[key])):
                    fd = (value(bump((ti, fi, key, idx), h)) - value(bump((ti, fi, key, idx), -h))) / (2 * h)
                    assert abs(fd - g[key][idx]) < 1e-5 * (1 + abs(fd)), (ti, fi, key, idx)
            if g["alpha"] is not None:
                fd = (value(bump((ti, fi, "alpha", None), h)) - value(bump((ti, fi, "alpha", None), -h))) / (2 * h)
                assert abs(fd - g["alpha"]) < 1e-5 * (1 + abs(fd))


def test_vfe_bound_gradient_matches_finite_differences(oracle_engine):
    """d(VFE bound)/d(kernel parameters, noise) (gp.PseudoObs.gradients: W_fu, W_uu, diagonal and noise terms) against
    central differences of the bound itself - every kernel family incl. periodic, non-uniform observation weights, a
    scale shared by two factors (torch chains it), on the oracle engine."""
    from gpar_amd.gp import GP, PseudoObs
    from gpar_amd.kernels import EQ, RQ, Linear

    rng = np.random.default_rng(0)
    n, M = 32, 7
    x, z = rng.uniform(0, 1, (n, 2)), rng.uniform(0, 1, (M, 2))
    y = np.sin(4 * x[:, 0]) + x[:, 1] ** 2 + 0.05 * rng.standard_normal(n)
    w = torch.tensor(rng.uniform(0.5, 1.5, n))

    def bound(theta):
        c1, s1, s2, a, c2, ls, noise, period, sp = theta
        k = (
            c1 * EQ().stretch(torch.stack([s1, s2]))
            + c2 * RQ(a).stretch(ls).select([0])
            + Linear().stretch(torch.stack([s2 * 2.0])).select([1])
            + 0.7 * (EQ().stretch(torch.stack([sp, sp])).periodic(torch.stack([period])) * EQ().stretch(torch.stack([s1 * 3.0]))).select([0])
        )
        f = GP(k)
        return PseudoObs(f(z), f(x, noise / w), y).elbo()

    theta = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in [1.3, 0.6, 0.9, 1.7, 0.4, 0.5, 0.08, 0.8, 1.1]]
    bound(theta).backward()
    h = 1e-6
    for i, t in enumerate(theta):
        up = [u.detach().clone() for u in theta]
        dn = [u.detach().clone() for u in theta]
        up[i] += h
        dn[i] -= h
        with torch.no_grad():
            fd = (float(bound(up)) - float(bound(dn))) / (2 * h)
        assert abs(float(t.grad) - fd) <= 2e-6 * (1 + abs(fd)), (i, float(t.grad), fd)


def _load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _nan_array(rows):
    return np.array([[np.nan if v is None else v for v in row] for row in rows], dtype=np.float64)


@pytest.mark.parametrize("case", _load_golden()["gpar_logpdf"], ids=lambda c: c["name"])
def test_golden_vectors_reproduce_and_host_code_agrees(case, oracle_engine):
    """(i) a fresh evaluation of the stand-alone numpy GPAR reproduces the committed value; (ii) the product's host
    orchestration (GPARRegressor on the oracle engine) gives the same number from the same hyper-parameters."""
    from gpar_amd.regression import GPARRegressor

    x, y = np.array(case["x"]), _nan_array(case["y"])
    w = None if case["w"] is None else np.array(case["w"])
    eps, x_ind = case.get("epsilon", 1e-12), case.get("x_ind")
    y_ref = y
    if "train_y" in case:   # the reference un-normalises the argument of logpdf (gpar/regression.py:483, sic)
        ty = _nan_array(case["train_y"])
        y_ref = y * np.array([np.std(c[~np.isnan(c)]) for c in ty.T]) + np.array([np.mean(c[~np.isnan(c)]) for c in ty.T])
    fresh = gpar_ref.gpar_logpdf(x, y_ref, w, case["hypers"], case["config"], impute=case["impute"], replace=case["replace"],
                                 eps=eps, x_ind=None if x_ind is None else np.array(x_ind))
    assert abs(fresh - case["logpdf"]) <= 1e-11 * abs(case["logpdf"])
    oracle_engine.epsilon = eps  # lab's B.epsilon (examples/paper/air_temp.py:18 sets 1e-6)
    reg = regressor_from_case(case)
    got = float(reg.logpdf(x, y, w))
    assert abs(got - case["logpdf"]) <= 1e-9 * abs(case["logpdf"]), (got, case["logpdf"])
    assert set(reg.get_variables()) == set(case["hypers"])  # identical hyper-parameter naming


def regressor_from_case(case):
    """GPARRegressor whose variables are pre-set to the case's hyper-parameters (constructor inits are then ignored:
    get-or-create semantics)."""
    from gpar_amd.regression import GPARRegressor

    x_ind = case.get("x_ind")
    reg = GPARRegressor(replace=case["replace"], impute=case["impute"], normalise_y="train_y" in case,
                        x_ind=None if x_ind is None else np.array(x_ind), **{k: v for k, v in case["config"].items()})
    if "train_y" in case:   # (micro-normalise-quirk: conditioned with normalise_y=True before the prior logpdf is asked for)
        reg.condition(np.array(case["train_x"]), _nan_array(case["train_y"]))
    for name, value in case["hypers"].items():
        value = np.asarray(value, dtype=np.float64)
        if name.endswith("/input/lin/const"):
            reg.vs.get(init=value, name=name)
        elif name.endswith("/alpha"):
            reg.vs.bnd(init=value, lower=1e-3, upper=1e3, name=name)
        elif name.endswith("/noise"):
            reg.vs.bnd(init=value, lower=1e-8, name=name)
        else:
            reg.vs.bnd(init=value, name=name)
    return reg


@pytest.mark.parametrize("config", [dict(linear=True, nonlinear=True), dict(linear=True, nonlinear=True, rq=True, per=True, input_linear=True)]
                         + _MATERN_CONFIGS)
def test_kernel_input_gradients_match_finite_differences(config):
    """oracle/kernels.kernel_input_grads (the reference for the device pass gram_input_grad_kernel): derivative of
    sum_ab W_ab k(x1_a, x2_b) with respect to every entry of x1, against central differences."""
    rng = np.random.default_rng(3)
    m, pi = 2, 2
    spec = _random_layer(rng, config, m=m, pi=pi, p=3)
    x1, x2 = rng.uniform(-1, 1, (7, m + pi)), rng.uniform(-1, 1, (5, m + pi))
    W = rng.standard_normal((7, 5))
    got = ok.kernel_input_grads(spec, x1, x2, W)
    assert _smallest_distance(spec, x1, x2) > 1e4 * 1e-6   # the stencil below moves a point by 1e-6 (features: times omega / s, ~10)
    fd = np.zeros_like(x1)
    for a in range(x1.shape[0]):
        for c in range(x1.shape[1]):
            for sgn in (+1, -1):
                xp = x1.copy()
                xp[a, c] += sgn * 1e-6
                fd[a, c] += sgn * np.sum(W * ok.gram(spec, xp, x2)) / 2e-6
    np.testing.assert_allclose(got, fd, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("kind", ["matern12", "matern32", "matern52"])
def test_matern_gradients_at_coincident_points(kind):
    """The r = 0 convention (include/gpar_hip.h): dk/dr2 of nu = 1/2 is singular at r = 0 and every gradient takes it as 0 there.
    With duplicated rows (and the diagonal, always) the gradients must be finite and equal the sums over the pairs that do not
    coincide, written out pair by pair here; they also equal central differences in the scales and the period, because a coincident
    pair has k = 1 for every value of those parameters (the kink is in the points, not in the parameters)."""
    rng = np.random.default_rng(17)
    n = 8
    x = rng.uniform(-1, 1, (n, 2))
    x[5], x[6], x[2] = x[0], x[1], x[0]
    scales, pscales, period, coef = [0.7, 1.9], [0.8, 1.4], 1.3, 1.6
    spec = {"terms": [{"coef": coef, "factors": [_f(kind, [0, 1], scales)]},
                      {"coef": 0.5, "factors": [_f(kind, [1], pscales, periods=[period])]}]}
    W = rng.standard_normal((n, n))
    W = W + W.T
    grads = ok.kernel_grads(spec, x, W)

    def dk_dr2(r):
        if kind == "matern12":
            return -np.exp(-r) / (2 * r)
        if kind == "matern32":
            return -1.5 * np.exp(-np.sqrt(3.0) * r)
        return -(5.0 / 6.0) * (1 + np.sqrt(5.0) * r) * np.exp(-np.sqrt(5.0) * r)

    expect, coincident = np.zeros(2), 0
    for a in range(n):
        for b in range(n):
            d = (x[a] - x[b]) / np.array(scales)
            r = np.sqrt(np.sum(d * d))
            if r == 0.0:
                coincident += 1
                continue
            expect += 0.5 * W[a, b] * coef * dk_dr2(r) * (-2.0 * d * d / np.array(scales))
    assert coincident == n + 2 * 3 + 2   # the diagonal, the triple (0, 2, 5) and the pair (1, 6)
    got = grads["factors"][0][0]["scales"]
    assert np.all(np.isfinite(got))
    np.testing.assert_allclose(got, expect, rtol=1e-12)
    for g in (grads["factors"][1][0]["scales"], grads["factors"][1][0]["periods"]):
        assert np.all(np.isfinite(g))

    import copy

    h = 1e-6
    for ti, key, idx in [(0, "scales", 0), (0, "scales", 1), (1, "scales", 0), (1, "scales", 1), (1, "periods", 0)]:
        up, dn = copy.deepcopy(spec), copy.deepcopy(spec)
        up["terms"][ti]["factors"][0][key][idx] += h
        dn["terms"][ti]["factors"][0][key][idx] -= h
        fd = 0.5 * np.sum(W * (ok.gram(up, x) - ok.gram(dn, x))) / (2 * h)
        assert abs(fd - grads["factors"][ti][0][key][idx]) < 1e-5 * (1 + abs(fd)), (ti, key, idx)

    # gradients with respect to the points: x1 shares rows with x2; the coincident pairs drop out of the row sums
    x2 = x[:5]
    V = rng.standard_normal((n, 5))
    one = {"terms": [spec["terms"][0]]}
    got = ok.kernel_input_grads(one, x, x2, V)
    expect = np.zeros_like(x)
    for a in range(n):
        for b in range(5):
            d = (x[a] - x2[b]) / np.array(scales)
            r = np.sqrt(np.sum(d * d))
            if r > 0.0:
                expect[a] += V[a, b] * coef * dk_dr2(r) * 2.0 * d / np.array(scales)
    assert np.all(np.isfinite(got))
    np.testing.assert_allclose(got, expect, rtol=1e-12, atol=1e-15)
    assert np.all(np.isfinite(ok.kernel_input_grads(spec, x, x2, V)))


@pytest.mark.parametrize("name", ["matern12-weights", "matern32-markov1", "matern52-per-inputlinear", "matern12-missing-impute",
                                  "matern32-inducing"])
def test_matern_config_is_not_silently_evaluated_as_eq(name, oracle_engine):
    """oracle/gpar_ref.layer_spec reads config["matern"]: the stand-alone numpy GPAR handed the `model_config` of a Matern regressor
    (i) equals the product's host algebra on the oracle engine and (ii) differs, far beyond rounding, from the same call with
    `matern` removed from the configuration - the value of the EQ model, which layer_spec once returned for every Matern model."""
    case = next(c for c in _load_golden()["gpar_logpdf"] if c["name"] == name)
    x, y = np.array(case["x"]), _nan_array(case["y"])
    w = None if case["w"] is None else np.array(case["w"])
    x_ind = None if case.get("x_ind") is None else np.array(case["x_ind"])
    reg = regressor_from_case(case)
    assert reg.model_config["matern"] == case["config"]["matern"]
    kw = dict(impute=case["impute"], replace=case["replace"], x_ind=x_ind)
    ref = gpar_ref.gpar_logpdf(x, y, w, case["hypers"], reg.model_config, **kw)
    got = float(reg.logpdf(x, y, w))
    assert abs(got - ref) <= 1e-9 * abs(ref), (got, ref)
    as_eq = gpar_ref.gpar_logpdf(x, y, w, case["hypers"], {k: v for k, v in reg.model_config.items() if k != "matern"}, **kw)
    assert abs(as_eq - ref) > 1e-3 * abs(ref), (as_eq, ref)


# ---- the cosine factor (include/gpar_hip.h: GPAR_K_COS) and the spectral mixture of GPARRegressor(spectral=Q) -----------------------

def test_cosine_closed_forms_and_argument_errors():
    """cos(2 pi sigma) of the SUM of the scaled differences; 1 on the diagonal exactly; the phase survives large time stamps (2 sigma is
    reduced before pi enters); periods, or no features, are refused everywhere."""
    from oracle import mp_ref

    x = np.array([[0.0, 1.0], [3.0, 5.0]])
    cos = {"terms": [{"coef": 2.0, "factors": [_f("cos", [0, 1], [4.0, 16.0])]}]}
    # sigma = -3/4 - 4/16 = -1: a whole period;  with scales (4, 8): sigma = -5/4, a quarter period: exactly 0
    np.testing.assert_array_equal(ok.gram(cos, x), [[2.0, 2.0], [2.0, 2.0]])
    quarter = {"terms": [{"coef": 2.0, "factors": [_f("cos", [0, 1], [4.0, 8.0])]}]}
    # (the zero is that of cos(pi / 2) with pi rounded to long double: 1e-19, or 1e-16 where long double is float64)
    np.testing.assert_allclose(ok.gram(quarter, x), [[2.0, 0.0], [0.0, 2.0]], rtol=0, atol=2.5e-16)
    np.testing.assert_array_equal(ok.gram_diag(cos, x), [2.0, 2.0])
    eighth = {"terms": [{"coef": 1.0, "factors": [_f("cos", [0], [24.0])]}]}
    np.testing.assert_allclose(ok.gram(eighth, x)[0, 1], np.sqrt(0.5), rtol=1e-15)
    # a Linear factor beside it keeps |z|^2 on the diagonal
    lin = {"terms": [{"coef": 0.5, "factors": [_f("cos", [0], [0.3]), _f("linear", [1], [2.0])]}]}
    np.testing.assert_allclose(ok.gram_diag(lin, x), [0.5 * 0.25, 0.5 * 6.25], rtol=1e-15)
    np.testing.assert_allclose(np.diag(ok.gram(lin, x)), ok.gram_diag(lin, x), rtol=1e-15)
    # time stamps of 2^40 + quarters over the period 1: float64 holds them exactly, and so must the phase be
    t = np.array([[2.0 ** 40], [2.0 ** 40 + 0.25], [2.0 ** 40 + 0.5]])
    unit = {"terms": [{"coef": 1.0, "factors": [_f("cos", [0], [1.0])]}]}
    np.testing.assert_allclose(ok.gram(unit, t), [[1.0, 0.0, -1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 1.0]], rtol=0, atol=1.3e-16)
    # against 50 digits at a large argument, where cos(2 * pi * sigma) in float64 is off by 2 pi |sigma| 2^-52 ~ 1e-10
    big = np.array([[123456.789], [0.123]])
    third = {"terms": [{"coef": 1.0, "factors": [_f("cos", [0], [0.37])]}]}
    exact = float(mp_ref.gram(third, big.tolist())[0, 1])
    z = big[:, 0] * (1.0 / 0.37)        # (the features as both compute them: x times the rounded reciprocal)
    import mpmath as mp

    exact_of_rounded = float(mp.cos(2 * mp.pi * (mp.mpf(float(z[0])) - mp.mpf(float(z[1])))))
    assert abs(ok.gram(third, big)[0, 1] - exact_of_rounded) < 1e-15 + 2 * np.pi * abs(z[0]) * 2.0 ** -53 * 1.01   # one rounding of sigma
    assert abs(exact - exact_of_rounded) < 1e-9   # (what dividing by the scale in 50 digits instead changes: not the oracle's error)
    for bad in ({"terms": [{"coef": 1.0, "factors": [_f("cos", [0], [0.7, 1.3], periods=[2.0])]}]},
                {"terms": [{"coef": 1.0, "factors": [_f("cos", [], [])]}]}):
        W = np.ones((2, 2))
        for call in (lambda: ok.gram(bad, x), lambda: ok.gram_diag(bad, x), lambda: ok.kernel_grads(bad, x, W),
                     lambda: ok.kernel_input_grads(bad, x, x, W), lambda: mp_ref.gram(bad, x.tolist())):
            with pytest.raises(ValueError, match="cosine factor"):
                call()


def test_cosine_equals_linear_on_the_periodic_embedding():
    """cos(2 pi (x - y) / T) = <phi(x), phi(y)>, phi = [sin(2 pi x / T), cos(2 pi x / T)]: Cosine().stretch(T) is Linear().periodic(T)
    with unit scales - what the oracle already had.  Pins the sign, the factor of two and the reading of the scale as a period.

    Tolerance: the embedding rounds each row angle a = 2 pi x / T (the product 2 pi / T, then times x: 2 roundings, then the argument
    reduction of sin / cos inside libm is exact to the rounded a) - an absolute phase error of at most 2 * 2^-53 |a| per row, two rows
    per entry, |a| <= 2 pi 8 / T - and four roundings of values of size <= 1 in forming the inner product, 4 * 2^-53; the cosine
    side's own error (one rounding of x / T and of the difference, the evaluation) is below 2 pi * 2 * 2^-53 * 8 / T + 2^-52.  With a
    factor 2 of slack on the sum."""
    rng = np.random.default_rng(11)
    x = rng.uniform(0.0, 8.0, (40, 1))

    def bound(T):
        amax = 2 * np.pi * 8.0 / T
        return 2 * (2 * (2 * 2.0 ** -53 * amax) + 4 * 2.0 ** -53 + 2 * np.pi * 2 * 2.0 ** -53 * 8.0 / T + 2.0 ** -52)

    assert bound(0.31) < 2.5e-13 and bound(2.7) < 3e-14
    for T in (0.31, 1.0, 2.7):
        cos = {"terms": [{"coef": 1.0, "factors": [_f("cos", [0], [T])]}]}
        lin = {"terms": [{"coef": 1.0, "factors": [_f("linear", [0], [1.0, 1.0], periods=[T])]}]}
        tol = bound(T)
        np.testing.assert_allclose(ok.gram(cos, x), ok.gram(lin, x), rtol=0, atol=tol)
        y = rng.uniform(0.0, 8.0, (7, 1))
        np.testing.assert_allclose(ok.gram(cos, x, y), ok.gram(lin, x, y), rtol=0, atol=tol)
        got = ok.gram(cos, x)
        assert np.array_equal(got, got.T) and np.all(np.diag(got) == 1.0)
    # and through the product's own classes: what `spec_to_dict` makes of Cosine().stretch(T)
    from gpar_amd.kernels import Cosine, Linear

    a = ok.spec_to_dict(Cosine().stretch(np.array([0.8])).resolve(1))
    b = ok.spec_to_dict(Linear().periodic(np.array([0.8])).resolve(1))
    assert [f["type"] for f in a["terms"][0]["factors"]] == ["cos"] and b["terms"][0]["factors"][0]["scales"] == [1.0, 1.0]
    np.testing.assert_allclose(ok.gram(a, x), ok.gram(b, x), rtol=0, atol=bound(0.8))


def test_pure_cosine_gram_is_positive_semidefinite_of_rank_two():
    rng = np.random.default_rng(12)
    n = 40
    x = rng.uniform(0.0, 8.0, (n, 2))
    for scales in ([0.7, 1.9], [0.31, 0.31]):
        K = ok.gram({"terms": [{"coef": 1.0, "factors": [_f("cos", [0, 1], scales)]}]}, x)
        ev = np.linalg.eigvalsh(K)
        assert ev[0] >= -1e-12 * n, ev[0]
        assert np.sum(ev > 1e-10 * n) <= 2, ev[-4:]
        assert abs(np.sum(ev) - n) < 1e-10 * n


def _cosine_structures():
    per = _f("eq", [0], [0.9, 1.4], periods=[0.8])
    return {
        "cos-nd1": [{"coef": 1.3, "factors": [_f("cos", [1], [0.6])]}],
        "cos-nd2": [{"coef": 1.3, "factors": [_f("cos", [0, 2], [0.6, 1.7])]}],
        "cos-nd3": [{"coef": 0.7, "factors": [_f("cos", [0, 1, 2], [0.9, 0.5, 2.3])]}],
        "eq-x-cos": [{"coef": 0.8, "factors": [_f("eq", [0, 1], [0.7, 1.1]), _f("cos", [0, 1], [0.45, 1.3])]}],
        "matern32-x-cos": [{"coef": 1.1, "factors": [_f("matern32", [0, 1], [0.7, 1.1]), _f("cos", [0], [0.45])]}],
        "rq-x-cos": [{"coef": 0.5, "factors": [_f("rq", [1, 2], [0.7, 1.1], alpha=0.8), _f("cos", [0, 1], [0.45, 0.9])]}],
        "linear-x-cos": [{"coef": 0.9, "factors": [_f("linear", [1, 2], [1.5, 2.5]), _f("cos", [0], [0.45])]}],
        "cos-beside-locally-periodic": [{"coef": 0.6, "factors": [_f("eq", [0, 1], [2.0, 2.5]), _f("cos", [0, 1], [0.5, 0.7])]},
                                        {"coef": 1.2, "factors": [per, _f("eq", [0], [3.0])]}],
    }


@pytest.mark.parametrize("name", list(_cosine_structures()))
def test_cosine_kernel_gradients_match_central_differences(name):
    """`kernel_grads` (coefficients, scales - and the neighbours' periods and alphas, whose `rest` products now hold a cosine) and
    `kernel_input_grads`, rectangular and symmetric, against central differences of `gram`.  The cosine has no kink: the stencil needs
    no distance condition.  Fourth-order stencil, h = 1e-3 relative: truncation ~ h^4 (2 pi / T)^5 / 30 < 1e-7 relative at T >= 0.45
    on inputs in [-1, 1], rounding 1e-16 / h = 1e-13."""
    import copy

    rng = np.random.default_rng(19)
    spec = {"terms": _cosine_structures()[name]}
    n = 9
    x = rng.uniform(-1, 1, (n, 3))
    W = rng.standard_normal((n, n))
    W = W + W.T
    grads = ok.kernel_grads(spec, x, W)

    def fd(fn, h):
        return (-fn(2 * h) + 8 * fn(h) - 8 * fn(-h) + fn(-2 * h)) / (12 * h)

    def value_at(ti, fi, key, idx):
        def fn(delta):
            s = copy.deepcopy(spec)
            if fi is None:
                s["terms"][ti]["coef"] += delta
            elif idx is None:
                s["terms"][ti]["factors"][fi][key] += delta
            else:
                s["terms"][ti]["factors"][fi][key][idx] += delta
            return 0.5 * np.sum(W * ok.gram(s, x))
        return fn

    checked = 0
    for ti, term in enumerate(spec["terms"]):
        want = fd(value_at(ti, None, "coef", None), 1e-3)
        assert abs(want - grads["coef"][ti]) < 1e-7 * (1 + abs(want)), (ti, want, grads["coef"][ti])
        for fi, f in enumerate(term["factors"]):
            g = grads["factors"][ti][fi]
            if f["type"] == "cos":
                assert g["periods"] is None and g["alpha"] is None
            for q, s_q in enumerate(f["scales"]):
                want = fd(value_at(ti, fi, "scales", q), 1e-3 * s_q)
                assert abs(want - g["scales"][q]) < 2e-6 * (1 + abs(want)), (ti, fi, q, want, g["scales"][q])
                checked += 1
            if f["periods"] is not None:
                want = fd(value_at(ti, fi, "periods", 0), 1e-3 * f["periods"][0])
                assert abs(want - g["periods"][0]) < 2e-6 * (1 + abs(want))
            if f["type"] == "rq":
                want = fd(value_at(ti, fi, "alpha", None), 1e-3)
                assert abs(want - g["alpha"]) < 1e-7 * (1 + abs(want))
    assert checked >= 1
    # inputs: rectangular, and symmetric as the engine forms it (twice the row sums with the symmetric weights)
    x2 = rng.uniform(-1, 1, (5, 3))
    V = rng.standard_normal((n, 5))
    got = ok.kernel_input_grads(spec, x, x2, V)
    got_sym = 2.0 * ok.kernel_input_grads(spec, x, x, W)
    want, want_sym = np.zeros_like(x), np.zeros_like(x)
    for a in range(n):
        for c in range(3):
            def moved(delta):
                xp = x.copy()
                xp[a, c] += delta
                return xp
            want[a, c] = fd(lambda d: np.sum(V * ok.gram(spec, moved(d), x2)), 1e-3)
            want_sym[a, c] = fd(lambda d: np.sum(W * ok.gram(spec, moved(d))), 1e-3)
    big = max(np.max(np.abs(want)), 1.0)
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-6 * big)
    np.testing.assert_allclose(got_sym, want_sym, rtol=0, atol=2e-6 * max(np.max(np.abs(want_sym)), 1.0))
    used = sorted({c for t in spec["terms"] for f in t["factors"] for c in f["cols"]})
    assert all(np.any(got[:, c] != 0.0) for c in used)


def _spectral_hypers(m, p, config, rng):
    import importlib.util

    s = importlib.util.spec_from_file_location("make_golden", os.path.join(os.path.dirname(GOLDEN), "make_golden.py"))
    mod = importlib.util.module_from_spec(s)
    s.loader.exec_module(mod)
    return mod.hypers_for(m, p, config, rng)


def test_layer_spec_follows_the_regressor_for_spectral():
    """config["spectral"] = Q adds var * EQ(scales) * cos(pers) per component over the input columns, after the locally periodic term;
    the envelope stays EQ under `matern` / `rq`, `scale_tie` does not tie these - and the variables are those the regressor creates."""
    from gpar_amd.engine import set_engine
    from gpar_amd.regression import GPARRegressor

    rng = np.random.default_rng(6)
    base = dict(linear=True, nonlinear=True, per=True, input_linear=True)
    for extra, kind in ((dict(), "eq"), (dict(matern=1.5), "matern32"), (dict(rq=True), "rq"), (dict(scale_tie=True), "eq")):
        cfg = dict(base, spectral=2, **extra)
        hypers = _spectral_hypers(2, 2, cfg, rng)
        spec, _ = gpar_ref.layer_spec(hypers, 2, 1, cfg)
        assert [[f["type"] for f in t["factors"]] for t in spec["terms"]] == [[kind], ["eq", "eq"], ["eq", "cos"], ["eq", "cos"], ["linear"], [],
                                                                              ["linear"], [kind]]
        for q in (0, 1):
            term = spec["terms"][2 + q]
            assert term["coef"] == hypers[f"1/input/sm{q}/var"] and [f["cols"] for f in term["factors"]] == [[0, 1], [0, 1]]
            assert term["factors"][0]["scales"] == hypers[f"1/input/sm{q}/scales"] and term["factors"][1]["scales"] == hypers[f"1/input/sm{q}/pers"]
            assert term["factors"][1]["periods"] is None
    previous = set_engine(OracleEngine())
    try:
        x, y = rng.uniform(0, 1, (12, 2)), rng.standard_normal((12, 2))
        reg = GPARRegressor(normalise_y=False, spectral=2, spectral_period=(0.7, 0.31), spectral_scale=0.8, **base)
        got = float(reg.logpdf(x, y))
        variables = reg.get_variables()
        assert {k for k in variables if "/sm" in k} == {f"{pi}/input/sm{q}/{v}" for pi in (0, 1) for q in (0, 1) for v in ("var", "scales", "pers")}
        np.testing.assert_allclose(variables["1/input/sm1/pers"], [0.31, 0.31])
        np.testing.assert_allclose(variables["0/input/sm0/scales"], [0.8, 0.8])
        want = gpar_ref.gpar_logpdf(x, y, None, variables, reg.model_config)
        assert abs(got - want) <= 1e-10 * abs(want)
    finally:
        set_engine(previous)
    for bad in (0, True, 1.5, "2"):
        with pytest.raises((ValueError, TypeError)):
            gpar_ref.layer_spec(_spectral_hypers(1, 1, dict(linear=False, spectral=1), rng), 1, 0, dict(linear=False, spectral=bad))


@pytest.mark.parametrize("name", ["spectral2-missing-weights", "spectral2-inducing"])
def test_spectral_config_on_the_engine_equals_the_restatement(name, oracle_engine):
    """The stand-alone numpy GPAR handed the `model_config` of a spectral regressor equals the product's host algebra on the oracle
    engine - missing data, weights, `impute`, inducing points - and differs far beyond rounding from the same call without `spectral`."""
    case = next(c for c in _load_golden()["gpar_logpdf"] if c["name"] == name)
    x, y = np.array(case["x"]), _nan_array(case["y"])
    w = None if case["w"] is None else np.array(case["w"])
    x_ind = None if case.get("x_ind") is None else np.array(case["x_ind"])
    reg = regressor_from_case(case)
    assert reg.model_config["spectral"] == case["config"]["spectral"] == 2 and np.isnan(y).any() and case["impute"]
    kw = dict(impute=case["impute"], replace=case["replace"], x_ind=x_ind)
    ref = gpar_ref.gpar_logpdf(x, y, w, case["hypers"], reg.model_config, **kw)
    got = float(reg.logpdf(x, y, w))
    assert abs(got - ref) <= 1e-9 * abs(ref), (got, ref)
    assert abs(ref - case["logpdf"]) <= 1e-12 * abs(ref)
    without = gpar_ref.gpar_logpdf(x, y, w, case["hypers"], {k: v for k, v in reg.model_config.items() if not k.startswith("spectral")}, **kw)
    assert abs(without - ref) > 1e-3 * abs(ref), (without, ref)


def test_spectral_regressor_runs_every_entry_point_on_the_oracle_engine(oracle_engine):
    """GPARRegressor(spectral=2) through logpdf, condition, predict, loo, cv and ahead on the numpy engine, where the oracle raised
    `unknown factor type 'cos'` before it knew the factor."""
    from gpar_amd.regression import GPARRegressor

    rng = np.random.default_rng(21)
    x = np.linspace(0, 1, 30)[:, None]
    y = np.stack([np.sin(2 * np.pi * x[:, 0] / 0.5), np.cos(2 * np.pi * x[:, 0] / 0.31)], axis=1) + 0.05 * rng.standard_normal((30, 2))
    reg = GPARRegressor(spectral=2, spectral_period=(0.5, 0.31), spectral_scale=0.8, replace=True, noise=0.05, normalise_y=False)
    values = [float(reg.logpdf(x, y)), float(reg.loo(x, y)[0]), float(reg.cv(x, y, folds=3)[0]), float(reg.ahead(x, y)[0])]
    assert np.all(np.isfinite(values)), values
    reg.condition(x, y)
    mean = reg.predict(np.linspace(0, 1, 7)[:, None], num_samples=3)
    assert np.all(np.isfinite(np.asarray(mean))) and np.asarray(mean).shape == (7, 2)
    assert np.isfinite(float(reg.logpdf(x, y, posterior=True)))
