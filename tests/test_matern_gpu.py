"""Matern kernels (nu = 1/2, 3/2, 5/2) through libgpar_hip.so on the MI355X.

The reference is scikit-learn's `Matern` / `GaussianProcessRegressor` and the numpy restatement of the three kernels and their
derivatives below (`_phi`, `_dphi_ds`); never the code under test, and not `oracle/` - which has its own restatement of these types,
written independently of this file, and carries them through the parity suites (tests/test_hip_primitives.py, test_parity_gpu.py,
test_fuzz_parity_gpu.py, the golden vectors).

    type         k(s), r = sqrt(s)                        dk/ds
    Matern 1/2   exp(-r)                                  -exp(-r) / (2 r), 0 where r = 0
    Matern 3/2   (1 + sqrt(3) r) exp(-sqrt(3) r)          -(3/2) exp(-sqrt(3) r)
    Matern 5/2   (1 + sqrt(5) r + 5 s / 3) exp(-sqrt(5) r)  -(5/6)(1 + sqrt(5) r) exp(-sqrt(5) r)

The Gram and gradient kernels exist three times - the interpreter (csrc/gram.h), the source generated for a structure and compiled
at run time (csrc/gram_jit.h, grad_jit.h), and the same source compiled at build time into the archive - and the library caches
which one it uses per process: the route tests run their cases in one fresh child process per route.

Tolerances are the project's own: Gram entries rtol 1e-13 / atol 1e-14 (tests/test_hip_primitives.py::test_gram_matches_oracle),
parameter gradients rtol 1e-10 / atol 1e-12 * sum|W| (::test_kernel_gradients_match_oracle), input gradients 1e-11 * max(1,
max|ref|) absolute (::test_kernel_input_gradients_match_oracle), log marginal likelihood rtol 1e-10 and its gradient rtol 1e-8 / atol
1e-9 * max|ref| (tests/test_parity_gpu.py), finite differences rtol 1e-5 / atol 1e-6 * max|ref| with the fourth-order stencil
and step of oracle/gpar_ref.py::fd_gradient (tests/test_share_nothing.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from .conftest import make_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUS = [0.5, 1.5, 2.5]
TYPE = {0.5: "matern12", 1.5: "matern32", 2.5: "matern52"}


# ---- numpy restatement ------------------------------------------------------------------------------------------------------------
def _phi(kind, s):
    r = np.sqrt(s)
    if kind == "eq":
        return np.exp(-0.5 * s)
    if kind == "matern12":
        return np.exp(-r)
    if kind == "matern32":
        return (1.0 + np.sqrt(3.0) * r) * np.exp(-np.sqrt(3.0) * r)
    if kind == "matern52":
        return (1.0 + np.sqrt(5.0) * r + 5.0 * s / 3.0) * np.exp(-np.sqrt(5.0) * r)
    assert kind == "linear"
    return s


def _dphi_ds(kind, s):
    r = np.sqrt(s)
    if kind == "eq":
        return -0.5 * np.exp(-0.5 * s)
    if kind == "matern12":
        return np.where(r == 0.0, 0.0, -np.exp(-r) / (2.0 * np.where(r == 0.0, 1.0, r)))
    if kind == "matern32":
        return -1.5 * np.exp(-np.sqrt(3.0) * r)
    if kind == "matern52":
        return -(5.0 / 6.0) * (1.0 + np.sqrt(5.0) * r) * np.exp(-np.sqrt(5.0) * r)
    return np.ones_like(s)


def _features(f, x):
    """Scaled features of factor f = dict(kind, cols, scales[, periods]) at the rows of x."""
    cols = np.asarray(f["cols"], dtype=int)
    v = x[:, cols]
    if f.get("periods") is not None:
        w = 2.0 * np.pi / np.asarray(f["periods"])
        v = np.concatenate([np.sin(v * w), np.cos(v * w)], axis=1)
    return v / np.asarray(f["scales"])


def _s(f, x1, x2):
    z1, z2 = _features(f, x1), _features(f, x2)
    if f["kind"] == "linear":
        return z1 @ z2.T
    return ((z1[:, None, :] - z2[None, :, :]) ** 2).sum(-1)


def _ref_gram(terms, x1, x2):
    """terms = [(coef, [factor, ...]), ...]"""
    K = np.zeros((x1.shape[0], x2.shape[0]))
    for coef, factors in terms:
        prod = np.full_like(K, coef)
        for f in factors:
            prod = prod * _phi(f["kind"], _s(f, x1, x2))
        K += prod
    return K


def _ref_grads(terms, x1, x2, W):
    """d / d(coef, scales) of sum_ab W_ab k(x1_a, x2_b), and d / d x1 of the same (x2 held fixed); non-periodic factors."""
    coef_g, scale_g = [], []
    dx = np.zeros_like(x1)
    for coef, factors in terms:
        phis = [_phi(f["kind"], _s(f, x1, x2)) for f in factors]
        coef_g.append(float(np.sum(W * np.prod(phis, axis=0)) if phis else np.sum(W)))
        per_factor = []
        for k, f in enumerate(factors):
            rest = np.full_like(W, coef)
            for k2, ph in enumerate(phis):
                if k2 != k:
                    rest = rest * ph
            g = W * rest * _dphi_ds(f["kind"], _s(f, x1, x2))
            z1, z2 = _features(f, x1), _features(f, x2)
            scales = np.asarray(f["scales"], dtype=float)
            out = np.zeros(len(scales))
            for q, c in enumerate(f["cols"]):
                if f["kind"] == "linear":
                    out[q] = np.sum(g * np.outer(z1[:, q], z2[:, q])) * (-2.0 / scales[q])
                    dx[:, c] += (g * z2[None, :, q]).sum(1) / scales[q]
                else:
                    d = z1[:, None, q] - z2[None, :, q]
                    out[q] = np.sum(g * d * d) * (-2.0 / scales[q])
                    dx[:, c] += (2.0 * g * d).sum(1) / scales[q]
            per_factor.append(out)
        scale_g.append(per_factor)
    return coef_g, scale_g, dx


def _kernel_of(terms):
    from gpar_amd import kernels as K

    make = {"eq": K.EQ, "linear": K.Linear, "matern12": K.Matern12, "matern32": K.Matern32, "matern52": K.Matern52}
    total = K.ZeroKernel()
    for coef, factors in terms:
        prod = None
        for f in factors:
            k = make[f["kind"]]().stretch(np.asarray(f["scales"], dtype=float))
            if f.get("periods") is not None:
                k = k.periodic(np.asarray(f["periods"], dtype=float))
            k = k.select(f["cols"])
            prod = k if prod is None else prod * k
        total = total + (coef * prod if prod is not None else coef)
    return total


def _mixed_terms():
    """Three product terms mixing Matern, EQ, periodic and linear factors (+ a constant)."""
    return [
        (1.3, [dict(kind="matern12", cols=[0, 1], scales=[0.7, 1.9])]),
        (0.8, [dict(kind="eq", cols=[0], scales=[0.9, 1.4], periods=[0.6]), dict(kind="matern52", cols=[2, 3], scales=[1.1, 0.6])]),
        (0.45, [dict(kind="linear", cols=[4], scales=[2.5]), dict(kind="matern32", cols=[1], scales=[1.7])]),
        (0.2, []),
    ]


# ---- the three routes, each in a child process of its own -----------------------------------------------------------------------
ROUTES = {
    "interpreter": dict(GPAR_AOT="0", GPAR_GRAM_JIT_MIN_ENTRIES=str(1 << 40), GPAR_GRAD_JIT_MIN_ENTRIES=str(1 << 40)),
    "runtime": dict(GPAR_AOT="0", GPAR_GRAM_JIT_MIN_ENTRIES="1", GPAR_GRAD_JIT_MIN_ENTRIES="1"),
    "archive": dict(GPAR_AOT="1", GPAR_AOT_MIN_ENTRIES="1"),
}


def _stats():
    import ctypes

    from gpar_amd import _lib

    lib = _lib.load()
    j = [ctypes.c_int(), ctypes.c_int(), ctypes.c_int()]
    a = [ctypes.c_int(), ctypes.c_int()]
    lib.gpar_jit_stats(*[ctypes.byref(c) for c in j])
    lib.gpar_aot_stats(*[ctypes.byref(c) for c in a])
    return dict(compiled=j[0].value, failures=j[1].value, cached=j[2].value, entries=a[0].value, loaded=a[1].value)


def _gram_c_abi(ck, x1, x2=None, lower=False):
    """gpar_featurize + gpar_gram through the ctypes binding."""
    from gpar_amd import hip as H

    dev = torch.device("cuda:0")
    z1 = H.featurize(ck, torch.tensor(x1, device=dev))
    z2 = None if x2 is None else H.featurize(ck, torch.tensor(x2, device=dev))
    n1 = x1.shape[0]
    if lower:
        out = torch.full((n1, n1), float("nan"), dtype=torch.float64, device=dev)
        H.gram(ck, z1, None, out=out, lower=True)
        return out.cpu().numpy()
    return H.gram(ck, z1, z2).cpu().numpy()


def _route_gram(route):
    """Child process: the Gram parity cases of one route.  Prints the largest error per case, then asserts."""
    from sklearn.gaussian_process.kernels import Matern

    from gpar_amd.kernels import compile_kernel

    worst = 0.0
    archive = route == "archive"
    for nu in NUS:
        if archive and nu == 0.5:
            continue   # (nu = 1/2 is not a family of the archive: compiled at first use)
        for dz in (1, 3, 8):
            if archive and dz == 8:
                continue   # (the archive's single-factor Matern structures are the first layers of m = 1 .. 4)
            rng = np.random.default_rng(int(10 * nu) + dz)
            scales = rng.uniform(0.5, 2.0, dz)
            terms = [(1.0, [dict(kind=TYPE[nu], cols=list(range(dz)), scales=scales)])]
            ck = compile_kernel(_kernel_of(terms), dz)
            sk = Matern(length_scale=scales if dz > 1 else float(scales[0]), nu=nu)
            before = _stats()
            for n in (1, 63, 64, 257, 1000):
                x1, x2 = rng.standard_normal((n, dz)), rng.standard_normal((max(n // 2, 1) + 3, dz))
                cross, sym = _gram_c_abi(ck, x1, x2), _gram_c_abi(ck, x1, lower=True)
                il = np.tril_indices(n)
                want_c, want_s = sk(x1, x2), sk(x1)
                err = max(np.max(np.abs(cross - want_c) / (1e-14 + 1e-13 * np.abs(want_c))), np.max(np.abs(sym[il] - want_s[il]) / (1e-14 + 1e-13 * np.abs(want_s[il]))))
                print(f"gram {route} nu={nu} dz={dz} n={n}: error / tolerance = {err:.3f}", flush=True)
                worst = max(worst, err)
                assert np.allclose(cross, want_c, rtol=1e-13, atol=1e-14), (route, nu, dz, n)
                assert np.allclose(sym[il], want_s[il], rtol=1e-13, atol=1e-14), (route, nu, dz, n)
                assert np.all(np.diag(sym) == 1.0)
                # the numpy restatement is the same function
                assert np.allclose(_ref_gram(terms, x1, x2), want_c, rtol=1e-13, atol=1e-14)
            after = _stats()
            assert after["failures"] == 0
            if route == "interpreter":
                assert after["compiled"] == 0 and after["loaded"] == 0
            elif route == "runtime":
                assert after["compiled"] > before["compiled"] and after["loaded"] == 0
            else:
                assert after["entries"] >= 300 and after["loaded"] > before["loaded"] and after["compiled"] == before["compiled"]
    if not archive:
        terms = _mixed_terms()
        ck = compile_kernel(_kernel_of(terms), 5)
        rng = np.random.default_rng(99)
        for n in (1, 63, 64, 257, 1000):
            x1, x2 = rng.standard_normal((n, 5)), rng.standard_normal((n // 2 + 3, 5))
            cross, sym = _gram_c_abi(ck, x1, x2), _gram_c_abi(ck, x1, lower=True)
            il = np.tril_indices(n)
            want_c, want_s = _ref_gram(terms, x1, x2), _ref_gram(terms, x1, x1)
            err = max(np.max(np.abs(cross - want_c) / (1e-14 + 1e-13 * np.abs(want_c))), np.max(np.abs(sym[il] - want_s[il]) / (1e-14 + 1e-13 * np.abs(want_s[il]))))
            print(f"gram {route} mixed n={n}: error / tolerance = {err:.3f}", flush=True)
            worst = max(worst, err)
            assert np.allclose(cross, want_c, rtol=1e-13, atol=1e-14), (route, "mixed", n)
            assert np.allclose(sym[il], want_s[il], rtol=1e-13, atol=1e-14), (route, "mixed", n)
    print(json.dumps(dict(route=route, worst=worst, stats=_stats())))


def _route_coincident(route):
    """Child process: exact duplicates among the inputs.  Finite entries, an exact diagonal, finite gradients equal to the numpy
    restatement with dk/ds = 0 at r = 0."""
    from gpar_amd.engine import HipEngine
    from gpar_amd.kernels import compile_kernel

    eng = HipEngine()
    dev = eng.device
    archive = route == "archive"
    worst = 0.0
    for nu in NUS:
        if archive and nu == 0.5:
            continue
        # (the archive's structure: layer 1 of the matern families at m = 2 - input kernel, linear and Matern output kernels)
        terms = [
            (1.7, [dict(kind=TYPE[nu], cols=[0, 1], scales=[0.8, 1.6])]),
            (1.0, [dict(kind="linear", cols=[2], scales=[3.0])]),
            (0.6, [dict(kind=TYPE[nu], cols=[2], scales=[1.2])]),
        ]
        ck = compile_kernel(_kernel_of(terms), 3)
        rng = np.random.default_rng(int(10 * nu))
        n = 150
        x = rng.standard_normal((n, 3))
        x[40:70] = x[:30]            # duplicates across tile boundaries ...
        x[70:75] = x[0]              # ... several copies of one point
        x[100:110, :2] = x[5, :2]    # coincident in one factor only
        before = _stats()
        K = _gram_c_abi(ck, x, lower=True)
        il = np.tril_indices(n)
        want = _ref_gram(terms, x, x)
        assert np.all(np.isfinite(K[il]))
        assert np.allclose(K[il], want[il], rtol=1e-13, atol=1e-14)
        # a pure Matern sum: the diagonal is EXACTLY the sum of the coefficients
        pure = [(1.7, [dict(kind=TYPE[nu], cols=[0, 1], scales=[0.8, 1.6])]), (0.6, [dict(kind=TYPE[nu], cols=[2], scales=[1.2])])]
        Kp = _gram_c_abi(compile_kernel(_kernel_of(pure), 3), x, lower=True)
        assert np.all(np.diag(Kp) == 1.7 + 0.6)
        assert np.all(Kp[40:70, :30][np.arange(30), np.arange(30)] == 1.7 + 0.6)   # duplicates off the diagonal too
        # parameter gradient with symmetric weights
        W = rng.standard_normal((n, n))
        W = W + W.T
        Wdev = torch.tensor(np.tril(W) + np.triu(np.full((n, n), np.nan), 1), device=dev)
        got = eng.kernel_grads(ck, torch.tensor(x, device=dev), Wdev)   # 1/2 sum_ab W_ab dK_ab
        coef_g, scale_g, _ = _ref_grads(terms, x, x, 0.5 * W)
        scale = np.abs(W).sum()
        for t in range(len(terms)):
            assert np.isfinite(got["coef"][t]) and abs(got["coef"][t] - coef_g[t]) <= 1e-12 * scale, (route, nu, "coef", t)
            for fi, g in enumerate(got["factors"][t]):
                assert np.all(np.isfinite(g["scales"]))
                worst = max(worst, float(np.max(np.abs(g["scales"] - scale_g[t][fi]) / (1e-12 * scale + 1e-10 * np.abs(scale_g[t][fi])))))
                assert np.allclose(g["scales"], scale_g[t][fi], rtol=1e-10, atol=1e-12 * scale), (route, nu, "scales", t, fi)
        # input gradient: rectangular weights against a second set that contains copies of the first, and the symmetric form
        x2 = np.concatenate([x[:50], rng.standard_normal((31, 3))])
        Wr = rng.standard_normal((n, x2.shape[0]))
        got_r = eng.kernel_input_grads(ck, torch.tensor(x, device=dev), torch.tensor(x2, device=dev), torch.tensor(Wr, device=dev)).cpu().numpy()
        _, _, want_r = _ref_grads(terms, x, x2, Wr)
        got_s = eng.kernel_input_grads(ck, torch.tensor(x, device=dev), None, Wdev, sym=True).cpu().numpy()
        _, _, want_s = _ref_grads(terms, x, x, W)
        want_s = 2.0 * want_s
        for got_x, want_x in ((got_r, want_r), (got_s, want_s)):
            assert np.all(np.isfinite(got_x))
            tol = 1e-11 * max(1.0, np.max(np.abs(want_x)))
            worst = max(worst, float(np.max(np.abs(got_x - want_x)) / tol))
            assert np.max(np.abs(got_x - want_x)) <= tol, (route, nu)
        after = _stats()
        print(f"coincident {route} nu={nu}: worst gradient error / tolerance so far {worst:.3f}; {after}", flush=True)
        assert after["failures"] == 0
        if route == "interpreter":
            assert after["compiled"] == 0 and after["loaded"] == 0
        elif route == "runtime":
            assert after["compiled"] >= before["compiled"] + 3 and after["loaded"] == 0   # Gram, parameter- and input-gradient kernels
        else:
            assert after["loaded"] >= before["loaded"] + 2   # the Gram and the parameter-gradient kernel of this structure
    print(json.dumps(dict(route=route, worst=worst, stats=_stats())))


def _child(function, route):
    code = ("import sys; sys.path.insert(0, %r); from tests import test_matern_gpu as t; t.%s(%r)" % (ROOT, function, route))
    env = {k: v for k, v in os.environ.items() if k not in ("GPAR_AOT", "GPAR_AOT_MIN_ENTRIES", "GPAR_GRAM_JIT_MIN_ENTRIES", "GPAR_GRAD_JIT_MIN_ENTRIES")}
    env.update(ROUTES[route])
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    print(out.stdout[-6000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("route", list(ROUTES))
def test_gram_matches_scikit_learn_on_every_route(route):
    """gpar_featurize + gpar_gram, each nu, symmetric and cross, anisotropic scales, n in {1, 63, 64, 257, 1000} x dz in {1, 3, 8}
    against sklearn's Matern; a three-term structure mixing Matern, EQ, periodic and linear factors against the numpy restatement.
    The archive route runs the structures the archive holds (nu = 3/2, 5/2; dz = 1, 3) and asserts they were loaded from it."""
    result = _child("_route_gram", route)
    assert result["route"] == route and result["worst"] <= 1.0


@pytest.mark.parametrize("route", list(ROUTES))
def test_coincident_points_on_every_route(route):
    """The nu = 1/2 guard (and the other two): exact duplicates, symmetric Gram, parameter and input gradients.  (The archive holds
    no nu = 1/2 structure and no input-gradient kernel of the Matern families: on that route nu = 3/2 and 5/2 take the archive's Gram
    and parameter-gradient kernels, the input gradient the interpreter.)"""
    result = _child("_route_coincident", route)
    assert result["route"] == route and result["worst"] <= 1.0


# ---- through the model ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def hip():
    from gpar_amd.engine import set_engine

    eng = make_engine("hip")
    previous = set_engine(eng)
    yield eng
    set_engine(previous)


def _matern_draw(nu, n, m, seed, scales, noise, var=1.0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n, m))
    K = var * _phi(TYPE[nu], _s(dict(kind=TYPE[nu], cols=list(range(m)), scales=scales), x, x))
    y = np.linalg.cholesky(K + 1e-10 * np.eye(n)) @ rng.standard_normal(n) + np.sqrt(noise) * rng.standard_normal(n)
    return x, y[:, None]


def _latent_gradient_to_log(reg, name):
    """d / d log(theta) from the autograd gradient with respect to the optimiser's latent of a bounded variable."""
    var = reg.vs._vars[name]
    theta = reg.vs[name].detach().numpy()
    dtheta_dlatent = (theta - var.lower) * (var.upper - theta) / (var.upper - var.lower)
    return var.latent.grad.numpy() / dtheta_dlatent * theta


@pytest.mark.parametrize("nu", NUS)
def test_log_marginal_likelihood_and_gradient_match_scikit_learn(hip, nu):
    """GP(v * Matern(nu).stretch(s)) + noise, n = 300, m = 2, noise = 5 % of the signal variance: value rtol 1e-10, gradient (sklearn's
    is with respect to log parameters: converted) rtol 1e-8 / atol 1e-9 * max.  Then the prepared training objective
    (fastfit.build): it must accept the layer, return the general route's value to the bit and its gradient to 1e-12 of the largest
    component."""
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import ConstantKernel, Matern, WhiteKernel

    from gpar_amd.regression import GPARRegressor

    from .test_fastfit import _layer_objectives

    v, scales, noise = 1.4, np.array([0.3, 0.55]), 0.07
    x, y = _matern_draw(nu, 300, 2, seed=3, scales=scales, noise=noise, var=v)
    reg = GPARRegressor(matern=nu, scale=scales, noise=noise, linear=False, nonlinear=False, normalise_y=False)
    with torch.no_grad():
        reg.logpdf(x, y)
    reg.vs.assign("0/input/var", v)
    reg.vs.requires_grad(True)
    value = reg.logpdf(torch.tensor(x), torch.tensor(y))
    value.backward()
    got = np.concatenate([np.atleast_1d(_latent_gradient_to_log(reg, n)) for n in ("0/input/var", "0/input/scales", "0/noise")])
    reg.vs.requires_grad(False)

    kernel = ConstantKernel(v) * Matern(length_scale=scales, nu=nu) + WhiteKernel(noise)
    gpr = GaussianProcessRegressor(kernel=kernel, optimizer=None, alpha=hip.epsilon).fit(x, y[:, 0])
    want_value, want = gpr.log_marginal_likelihood(gpr.kernel_.theta, eval_gradient=True)
    print(f"nu={nu}: logpdf {float(value.detach())!r} sklearn {want_value!r} rel {abs(float(value.detach()) - want_value) / abs(want_value):.2e}; "
          f"gradient max rel-to-largest error {np.max(np.abs(got - want)) / np.max(np.abs(want)):.2e}")
    assert abs(float(value.detach()) - want_value) <= 1e-10 * abs(want_value)
    np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-9 * np.max(np.abs(want)))

    reg = GPARRegressor(matern=nu, scale=scales, noise=noise, linear=False, nonlinear=False, normalise_y=False)
    reg.condition(x, y)
    fast, fg, x0 = _layer_objectives(reg, hip, 0, None)   # (asserts that fastfit.build took the layer)
    rng = np.random.default_rng(1)
    for trial in range(2):
        xv = x0 + (0.0 if trial == 0 else 0.2 * rng.standard_normal(x0.shape))
        v_fast, g_fast = fast.fg(xv)
        v_ref, g_ref = fg(xv)
        print(f"nu={nu} trial {trial}: prepared {v_fast!r} general {v_ref!r}; gradient difference / largest component {np.max(np.abs(g_fast - g_ref)) / np.max(np.abs(g_ref)):.2e}")
        assert v_fast == v_ref
        assert np.max(np.abs(g_fast - g_ref)) <= 1e-12 * np.max(np.abs(g_ref))
    assert fast.fallbacks == 0


def _fd(f, vector, rel_step=1e-3):
    """Fourth-order central differences, entry by entry; stencil and step of oracle/gpar_ref.py::fd_gradient."""
    grad = np.zeros_like(vector)
    for j in range(vector.size):
        h = rel_step * max(abs(vector[j]), 1e-3)
        vals = {}
        for k in (-2, -1, 1, 2):
            moved = vector.copy()
            moved[j] += k * h
            vals[k] = f(moved)
        grad[j] = (-vals[2] + 8.0 * vals[1] - 8.0 * vals[-1] + vals[-2]) / (12.0 * h)
    return grad


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
    return x, (y - y.mean(0)) / y.std(0)


def _analytic_and_fd(reg, x, y, rel_step=1e-3):
    with torch.no_grad():
        reg.logpdf(x, y)
    names = reg.vs.names
    reg.vs.requires_grad(True)
    reg.logpdf(torch.tensor(x), torch.tensor(y)).backward()
    got = np.concatenate([(v.grad if v.grad is not None else torch.zeros_like(v)).numpy().reshape(-1) for v in reg.vs.get_vars(*names)])
    reg.vs.requires_grad(False)
    x0 = reg.vs.get_vector(names)

    def f(vector):
        reg.vs.set_vector(vector, names)
        with torch.no_grad():
            return float(reg.logpdf(x, y))

    want = _fd(f, x0, rel_step)
    reg.vs.set_vector(x0, names)
    return got, want


@pytest.mark.parametrize("nu", NUS)
def test_full_objective_gradient_matches_finite_differences(hip, nu):
    """GPARRegressor(matern=nu, linear, nonlinear, per), p = 3: a Matern factor in a sum with a periodic product and over output
    columns.  d logpdf / d(every optimiser variable) against central differences of the same logpdf.

    Step: a quarter of fd_gradient's 1e-3.  The objective oscillates in the periods of the locally periodic term (EQ factors, with
    and without `matern`), and at 1e-3 the stencil's own h^4 truncation error exceeds the tolerance there: measured on "2/input/per/pers",
    analytic minus stencil at relative steps 1e-3 / 5e-4 / 2.5e-4 = 3.95e-4 / 2.49e-5 / 1.56e-6 for matern=1.5 and 1.24e-3 /
    7.83e-5 / 4.91e-6 for the default EQ model - a factor 16 per halving, against a tolerance of 3.6e-5.  The wide step of
    fd_gradient exists for the rounding noise of K_zz^-1 with inducing points; this objective is dense."""
    from gpar_amd.regression import GPARRegressor

    x, y = _problem(70, 2, 3, seed=int(10 * nu))
    reg = GPARRegressor(matern=nu, scale=0.5, linear=True, nonlinear=True, per=True, noise=0.1, normalise_y=False)
    got, want = _analytic_and_fd(reg, x, y, rel_step=2.5e-4)
    print(f"nu={nu}: {got.size} variables, largest |fd| {np.max(np.abs(want)):.3e}, max error / largest {np.max(np.abs(got - want)) / np.max(np.abs(want)):.2e}")
    assert np.max(np.abs(want)) > 1e-2
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6 * np.max(np.abs(want)))


@pytest.mark.parametrize("nu", NUS)
def test_vfe_bound_gradient_with_respect_to_inducing_inputs(hip, nu):
    """The objective `fit(optimise_x_ind=True)` hands the optimiser for the LAST layer of a two-layer model: the VFE bound as a function
    of the layer's hyper-parameters and the inducing inputs (the columns appended by the earlier layer fixed, as `fit(fix=True)`
    keeps them) - the input-gradient pass, kind 2, with a Matern factor over the inputs and one over an output column."""
    from gpar_amd.model import per_output
    from gpar_amd.optimise import objective_and_gradient
    from gpar_amd.regression import GPARRegressor, _construct_gpar

    x, y = _problem(90, 2, 2, seed=5 + int(10 * nu))
    x_ind = np.random.default_rng(8).uniform(0.05, 0.95, (12, 2))
    reg = GPARRegressor(matern=nu, scale=0.5, linear=True, nonlinear=True, noise=0.1, normalise_y=False, x_ind=x_ind)
    reg._x_ind_trainable = True
    reg.condition(x, y)
    x_t, y_t, w_t = hip.tensor(reg.x), hip.tensor(reg.y), hip.tensor(reg.w)
    y_cached = {k: list(per_output(y_t, w_t, keep=k)) for k in [True, False]}
    gpar = _construct_gpar(reg, reg.vs, reg.m, 2)
    fixed_x, fixed_x_ind = gpar.logpdf(x_t, y_cached, None, only_last_layer=True, outputs=[0], return_inputs=True)

    def objective(vs):
        g = _construct_gpar(reg, vs, reg.m, 2)
        x_ind_pi = torch.cat([hip.tensor(vs["x_ind"]), fixed_x_ind[:, reg.m:]], dim=1)
        return -g.logpdf(fixed_x, y_cached, None, only_last_layer=True, outputs=[1], x_ind=x_ind_pi)

    fg, names, x0 = objective_and_gradient(objective, reg.vs, ["1/*", "x_ind"])
    assert "x_ind" in names and "1/output/nonlin/scales" in names
    _, got = fg(x0)
    want = _fd(lambda v: fg(v)[0], x0)
    print(f"nu={nu}: {got.size} variables, largest |fd| {np.max(np.abs(want)):.3e}, max error / largest {np.max(np.abs(got - want)) / np.max(np.abs(want)):.2e}")
    assert np.max(np.abs(want[: x_ind.size])) > 1e-2
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6 * np.max(np.abs(want)))


@pytest.mark.parametrize("nu", [1.5, 2.5])
def test_joint_bound_gradient_through_forwarded_inducing_inputs(hip, nu):
    """The JOINT bound of both layers (`logpdf` with trainable inducing inputs): layer 2's inducing inputs are [x_ind, posterior mean of
    layer 1 at x_ind], so the gradient also flows through the forwarded means.  nu = 3/2 and 5/2 only: with nu = 1/2 this objective
    is not differentiable where a forwarded mean crosses an observed value of the first output - exp(-|y_a - mean_j| / scale) over
    ONE output column has a kink there, and with 90 x 12 such pairs some lie inside any usable stencil (measured at nu = 1/2:
    analytic minus stencil for one inducing coordinate -23.6 / -0.09 / 2.6e-8 at relative steps 1e-3 / 2.5e-4 / 6e-5, for another
    -12.5 / -12.6 / -9.5: no limit to compare with).  The analytic gradient there is the derivative away from the kinks; the
    per-layer objective above, where the appended columns are fixed, has no such crossing and covers nu = 1/2."""
    from gpar_amd.regression import GPARRegressor

    x, y = _problem(90, 2, 2, seed=5 + int(10 * nu))
    x_ind = np.random.default_rng(8).uniform(0.05, 0.95, (12, 2))
    reg = GPARRegressor(matern=nu, scale=0.5, linear=True, nonlinear=True, noise=0.1, normalise_y=False, x_ind=x_ind)
    reg._x_ind_trainable = True
    got, want = _analytic_and_fd(reg, x, y)
    assert "x_ind" in reg.vs.names
    print(f"nu={nu}: {got.size} variables, largest |fd| {np.max(np.abs(want)):.3e}, max error / largest {np.max(np.abs(got - want)) / np.max(np.abs(want)):.2e}")
    assert np.max(np.abs(want)) > 1e-2
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6 * np.max(np.abs(want)))


def test_fit_predict_logpdf_end_to_end(hip):
    """Data drawn from a Matern-3/2 GPAR (n = 400, p = 2, fixed seed; the second output depends on the first), fit(iters=20): the
    trained log marginal likelihood is finite and not below its initial value, predictions are finite with ordered bounds, and the
    training data are more likely under matern=1.5 than under the default EQ model trained the same way.

    The last claim was checked first with scikit-learn on the same data (GaussianProcessRegressor, ConstantKernel * kernel +
    WhiteKernel, optimised from the same initial values; sum of the two layers' log marginal likelihoods, layer 2 on inputs
    [x, y1]):  Matern(nu=1.5) 117.86  against  RBF 103.42  - a gap of 14 nats."""
    from gpar_amd.regression import GPARRegressor

    x, y = _matern_gpar_draw()

    def run(**kw):
        reg = GPARRegressor(scale=0.3, linear=True, nonlinear=True, noise=0.05, normalise_y=False, **kw)
        initial = float(reg.logpdf(x, y))
        reg.fit(x, y, iters=20)
        return reg, initial, float(reg.logpdf(x, y))

    matern, m0, m1 = run(matern=1.5)
    eq, e0, e1 = run()
    print(f"matern=1.5: {m0:.3f} -> {m1:.3f};  EQ: {e0:.3f} -> {e1:.3f}")
    assert np.isfinite(m1) and m1 >= m0
    xs = np.linspace(0, 1, 60)[:, None]
    mean, lower, upper = matern.predict(xs, num_samples=50, credible_bounds=True)
    assert mean.shape == lower.shape == upper.shape == (60, 2)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(lower)) and np.all(np.isfinite(upper))
    assert np.all(lower <= mean) and np.all(mean <= upper)
    assert m1 > e1


def _matern_gpar_draw():
    rng = np.random.default_rng(4)
    n = 400
    x = np.sort(rng.uniform(0, 1, n))[:, None]
    f = dict(kind="matern32", cols=[0], scales=[0.15])
    L = np.linalg.cholesky(_phi("matern32", _s(f, x, x)) + 1e-10 * np.eye(n))
    y1 = L @ rng.standard_normal(n) + 0.1 * rng.standard_normal(n)
    y2 = 0.6 * y1 + 0.7 * (L @ rng.standard_normal(n)) + 0.1 * rng.standard_normal(n)
    y = np.stack([y1, y2], axis=1)
    return x, (y - y.mean(0)) / y.std(0)


def test_matern_none_is_the_default_model_to_the_bit(hip):
    """`matern=None` and the argument omitted: the same logpdf bits on a case of tests/golden/gpar_cases.json."""
    from .test_oracle import GOLDEN, _nan_array, regressor_from_case

    from gpar_amd.regression import GPARRegressor

    with open(GOLDEN) as f:
        case = next(c for c in json.load(f)["gpar_logpdf"] if c["name"] == "markov2-4out")
    reg = regressor_from_case(case)
    x, y = _nan_array(case["x"]), _nan_array(case["y"])
    w = None if case.get("w") is None else _nan_array(case["w"])
    omitted = float(reg.logpdf(x, y, w))
    assert abs(omitted - case["logpdf"]) <= 1e-10 * abs(case["logpdf"])
    again = GPARRegressor(replace=case["replace"], impute=case["impute"], normalise_y=False, matern=None, **case["config"])
    again.vs = reg.vs.copy(detach=True)
    assert again.model_config == reg.model_config and "matern" not in again.model_config
    assert float(again.logpdf(x, y, w)) == omitted


def test_predict_moments_sample_and_greedy_order_run(hip):
    """`predict_moments` against a 2000-sample `predict` at the tolerances of
    tests/test_share_nothing.py::test_monte_carlo_predict_converges_to_the_closed_form (mean within 5 standard errors, the width of
    the 95 % band within 25 % of 2 x 1.96 sd, its centre within 0.35 max sd); `sample(posterior=True)` and `greedy_order` return
    finite results of the right shape."""
    from gpar_amd.regression import GPARRegressor

    x, y = _problem(150, 2, 3, seed=11)
    xs = np.random.default_rng(2).uniform(0, 1, (25, 2))
    reg = GPARRegressor(matern=2.5, scale=0.5, linear=True, nonlinear=True, noise=0.1, replace=True, impute=True)
    reg.condition(x, y)
    S = 2000
    mean, lower, upper = reg.predict(xs, num_samples=S, credible_bounds=True)
    want_mean, want_var = reg.predict_moments(xs)
    sd = np.sqrt(want_var)
    assert np.all(np.abs(mean - want_mean) <= 5.0 * sd / np.sqrt(S))
    np.testing.assert_allclose(upper - lower, 2 * 1.96 * sd, rtol=0.25)
    np.testing.assert_allclose(0.5 * (upper + lower), want_mean, atol=0.35 * np.max(sd))

    sample = reg.sample(xs, posterior=True)
    assert np.shape(sample) == (25, 3) and np.all(np.isfinite(sample))
    order, values = GPARRegressor(matern=2.5, scale=0.5, linear=True, nonlinear=True, noise=0.1).greedy_order(x, y, iters=5)
    assert sorted(order) == [0, 1, 2] and len(values) == 3 and np.all(np.isfinite(values))
