"""The cosine factor (GPAR_K_COS) and GPARRegressor(spectral=Q) through libgpar_hip.so on the MI355X.

The reference is the numpy restatement below, which imports nothing from gpar_amd - a second statement beside `oracle/kernels.py`, which
learned the factor later (tests/test_hip_primitives.py, test_parity_gpu.py and test_fuzz_parity_gpu.py compare the device with that one):

    z_d = x[col_d] * (1 / scale_d)                            the feature map as include/gpar_hip.h defines it, in float64
    sigma = ((0 + (z_0 - z'_0)) + (z_1 - z'_1)) + ...          float64, in dim order: the definition of the factor's argument
    phi = cos(2 pi sigma),  d phi / d sigma = -2 pi sin(2 pi sigma)     in LONG DOUBLE, sigma reduced exactly before pi enters

so the Gram tolerance - the one tests/test_matern_gpu.py applies to Matern entries, rtol 1e-13 / atol 1e-14 - is asked of the device's
cospi alone.  (A restatement that formed sigma in another order or precision would differ from ANY float64 implementation by
2 pi nd |sigma| 2^-53, up to 3e-14 at nd = 16: the conditioning of the function, not an error of the kernel.)  Derivatives come from
a complex step through a plain complex-valued restatement (exact to rounding), tolerance 1e-6 of the largest component.

The Gram and gradient kernels exist three times - interpreter, generated at run time, generated at build time (the archive) - and the
library caches its choice per process: the route tests run in one child process per route and hand back digests of their results."""
import hashlib
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
LD = np.longdouble
PI_LD = LD("3.14159265358979323846264338327950288")


# ---- numpy restatement ------------------------------------------------------------------------------------------------------------
def _z(f, x):
    return x[:, np.asarray(f["cols"], dtype=int)] * (1.0 / np.asarray(f["scales"], dtype=np.float64))


def _sigma(f, x1, x2):
    z1, z2 = _z(f, x1), _z(f, x2)
    s = np.zeros((x1.shape[0], x2.shape[0]))
    for d in range(z1.shape[1]):
        s = s + (z1[:, None, d] - z2[None, :, d])
    return s


def _cos2pi_ld(s):
    t = np.fmod(LD(2) * s.astype(LD), LD(2))   # exact
    return np.cos(PI_LD * t)


def _phi(f, x1, x2):
    """Value of one factor (long double)."""
    if f["kind"] == "cos":
        return _cos2pi_ld(_sigma(f, x1, x2))
    z1, z2 = _z(f, x1).astype(LD), _z(f, x2).astype(LD)
    if f["kind"] == "linear":
        return z1 @ z2.T
    return np.exp(-((z1[:, None, :] - z2[None, :, :]) ** 2).sum(-1) / 2)


def _ref_gram(terms, x1, x2):
    K = np.zeros((x1.shape[0], x2.shape[0]), dtype=LD)
    for coef, factors in terms:
        prod = np.full(K.shape, LD(coef))
        for f in factors:
            prod = prod * _phi(f, x1, x2)
        K += prod
    return K.astype(np.float64)


def _weighted_sum_complex(terms, x1, x2, W):
    """sum_ab W_ab k(x1_a, x2_b) for COMPLEX parameters / inputs (the complex step's function: plain complex arithmetic)."""
    total = 0.0
    for coef, factors in terms:
        prod = coef
        for f in factors:
            cols = np.asarray(f["cols"], dtype=int)
            z1, z2 = x1[:, cols] / np.asarray(f["scales"]), x2[:, cols] / np.asarray(f["scales"])
            d = z1[:, None, :] - z2[None, :, :]
            if f["kind"] == "cos":
                prod = prod * np.cos(2.0 * np.pi * d.sum(-1))
            elif f["kind"] == "linear":
                prod = prod * (z1 @ z2.T)
            else:
                prod = prod * np.exp(-0.5 * (d * d).sum(-1))
        total = total + np.sum(W * prod)
    return total


def _complex_step_grads(terms, x1, x2, W, sym=False):
    """(d / d coef, d / d scales per term and factor, d / d x1) of sum W k.  `sym`: x2 is x1 and both arguments move with x1."""
    h = 1e-30
    c1 = x1.astype(complex)
    c2 = c1 if sym else x2.astype(complex)
    coef_g, scale_g = [], []
    for ti, (coef, factors) in enumerate(terms):
        bumped = [(c + 1j * h if t == ti else c, fs) for t, (c, fs) in enumerate(terms)]
        coef_g.append(_weighted_sum_complex(bumped, c1, c2, W).imag / h)
        per_factor = []
        for fi, f in enumerate(factors):
            out = np.zeros(len(f["scales"]))
            for q in range(len(f["scales"])):
                sc = np.asarray(f["scales"], dtype=complex).copy()
                sc[q] += 1j * h
                bumped = [(c, [dict(g, scales=sc) if (t, k) == (ti, fi) else g for k, g in enumerate(fs)]) for t, (c, fs) in enumerate(terms)]
                out[q] = _weighted_sum_complex(bumped, c1, c2, W).imag / h
            per_factor.append(out)
        scale_g.append(per_factor)
    dx = np.zeros_like(x1)
    for a in range(x1.shape[0]):
        for c in range(x1.shape[1]):
            b = c1.copy()
            b[a, c] += 1j * h
            dx[a, c] = _weighted_sum_complex(terms, b, b if sym else c2, W).imag / h
    return coef_g, scale_g, dx


def _kernel_of(terms):
    from gpar_amd import kernels as K

    make = {"eq": K.EQ, "linear": K.Linear, "cos": K.Cosine}
    total = K.ZeroKernel()
    for coef, factors in terms:
        prod = None
        for f in factors:
            k = make[f["kind"]]().stretch(np.asarray(f["scales"], dtype=float)).select(f["cols"])
            prod = k if prod is None else prod * k
        total = total + coef * prod
    return total


def _cos_terms(nd, rng):
    return [(1.0, [dict(kind="cos", cols=list(range(nd)), scales=rng.uniform(0.5, 2.0, nd))])]


def _eq_cos_terms(rng):
    return [(0.8, [dict(kind="eq", cols=[0, 1], scales=rng.uniform(0.8, 2.0, 2)), dict(kind="cos", cols=[0, 1], scales=rng.uniform(0.5, 2.0, 2))]),
            (1.0, [dict(kind="linear", cols=[2], scales=[2.5])])]   # (coefficient 1, as Linear().stretch() has it: see the bit test below)


def _cos_without_exponent_terms(rng):
    """Cosine factors in terms that hold no exponential factor, behind a first term: c * Cosine() and c * Linear() * Cosine()."""
    return [(1.0, [dict(kind="eq", cols=[0], scales=rng.uniform(0.8, 2.0, 1))]),
            (0.7, [dict(kind="cos", cols=[0, 1], scales=rng.uniform(0.5, 2.0, 2))]),
            (0.45, [dict(kind="linear", cols=[2], scales=[2.5]), dict(kind="cos", cols=[1], scales=rng.uniform(0.5, 2.0, 1))])]


def _regressor_terms(m, Q, rng, linear=True):
    """The structure GPARRegressor(spectral=Q) builds for a layer with one previous output: var EQ + sum_q var_q EQ * cos (+ linear)."""
    cols = list(range(m))
    terms = [(1.1, [dict(kind="eq", cols=cols, scales=rng.uniform(0.5, 2.0, m))])]
    for q in range(Q):
        terms.append((1.0 / Q, [dict(kind="eq", cols=cols, scales=rng.uniform(2.0, 6.0, m)), dict(kind="cos", cols=cols, scales=rng.uniform(0.4, 1.5, m))]))
    if linear:
        terms.append((1.0, [dict(kind="linear", cols=[m], scales=[3.0])]))
    return terms


# ---- the three routes, each in a child process of its own -------------------------------------------------------------------------
ROUTES = {
    "interpreter": dict(GPAR_AOT="0", GPAR_GRAM_JIT_MIN_ENTRIES=str(1 << 40), GPAR_GRAD_JIT_MIN_ENTRIES=str(1 << 40)),
    "runtime": dict(GPAR_AOT="0", GPAR_GRAM_JIT_MIN_ENTRIES="0", GPAR_GRAD_JIT_MIN_ENTRIES="0"),
    "archive": dict(GPAR_AOT="1", GPAR_AOT_MIN_ENTRIES="1"),
}
SIZES = (1, 2, 31, 32, 33, 64, 65, 130)


def _stats():
    import ctypes

    from gpar_amd import _lib

    lib = _lib.load()
    j = [ctypes.c_int(), ctypes.c_int(), ctypes.c_int()]
    a = [ctypes.c_int(), ctypes.c_int()]
    lib.gpar_jit_stats(*[ctypes.byref(c) for c in j])
    lib.gpar_aot_stats(*[ctypes.byref(c) for c in a])
    return dict(compiled=j[0].value, failures=j[1].value, cached=j[2].value, entries=a[0].value, loaded=a[1].value)


def _gram_device(ck, x1, x2=None):
    """gpar_featurize + gpar_gram: the rectangular form into a matrix with a padded leading dimension, or (x2 None) the lower triangle."""
    from gpar_amd import hip as H

    dev = torch.device("cuda:0")
    z1 = H.featurize(ck, torch.tensor(x1, device=dev))
    n1 = x1.shape[0]
    if x2 is None:
        out = torch.full((n1, n1 + 6), float("nan"), dtype=torch.float64, device=dev)[:, :n1]
        H.gram(ck, z1, None, out=out, lower=True)
        return out.cpu().numpy()
    z2 = H.featurize(ck, torch.tensor(x2, device=dev))
    out = torch.full((n1, x2.shape[0] + 5), float("nan"), dtype=torch.float64, device=dev)[:, : x2.shape[0]]
    H.gram(ck, z1, z2, out=out)
    return out.cpu().numpy()


def _check_gram(tag, terms, width, n, rng, digests):
    from gpar_amd.kernels import compile_kernel

    ck = compile_kernel(_kernel_of(terms), width)
    x1, x2 = rng.standard_normal((n, width)), rng.standard_normal((n // 2 + 3, width))
    cross, sym = _gram_device(ck, x1, x2), _gram_device(ck, x1)
    il = np.tril_indices(n)
    want_c, want_s = _ref_gram(terms, x1, x2), _ref_gram(terms, x1, x1)
    err = max(np.max(np.abs(cross - want_c) / (1e-14 + 1e-13 * np.abs(want_c))), np.max(np.abs(sym[il] - want_s[il]) / (1e-14 + 1e-13 * np.abs(want_s[il]))))
    print(f"gram {tag} n={n}: error / tolerance = {err:.3f}", flush=True)
    assert np.allclose(cross, want_c, rtol=1e-13, atol=1e-14), (tag, n)
    assert np.allclose(sym[il], want_s[il], rtol=1e-13, atol=1e-14), (tag, n)
    digests[f"{tag} n={n}"] = hashlib.sha256(cross.tobytes() + sym[il].tobytes()).hexdigest()
    return err


def _check_grads(tag, terms, width, n, rng, eng):
    """gpar_gram_grad (SYM), gpar_gram_grad_cross (RECT, DIAG) and gpar_gram_input_grad (RECT, SYM) against the complex step."""
    from gpar_amd.kernels import compile_kernel

    ck = compile_kernel(_kernel_of(terms), width)
    x1, x2 = rng.standard_normal((n, width)), rng.standard_normal((n // 2 + 3, width))
    W = rng.standard_normal((n, x2.shape[0]))
    Ws = rng.standard_normal((n, n))
    Ws = Ws + Ws.T
    wd = rng.standard_normal(n)
    t = lambda a: torch.tensor(a, device=eng.device)  # noqa: E731
    worst = 0.0

    def compare(what, got, want_coef, want_scales):
        nonlocal worst
        flat_g = np.concatenate([np.asarray(got["coef"], dtype=float)] + [np.asarray(g["scales"], dtype=float) for fs in got["factors"] for g in fs])
        flat_w = np.concatenate([np.asarray(want_coef, dtype=float)] + [np.asarray(s, dtype=float) for fs in want_scales for s in fs])
        err = np.max(np.abs(flat_g - flat_w)) / (1e-6 * np.max(np.abs(flat_w)))
        print(f"grad {tag} {what} n={n}: error / tolerance = {err:.2e}", flush=True)
        worst = max(worst, err)
        assert err <= 1.0, (tag, what, n, flat_g, flat_w)

    wc, wsc, wdx = _complex_step_grads(terms, x1, x2, W)
    compare("rect", eng.kernel_grads_weighted(ck, t(x1), t(x2), t(W)), wc, wsc)
    gx = eng.kernel_input_grads(ck, t(x1), t(x2), t(W)).cpu().numpy()
    assert np.max(np.abs(gx - wdx)) <= 1e-6 * np.max(np.abs(wdx)), (tag, "input rect", n)
    wc, wsc, wdx = _complex_step_grads(terms, x1, x1, Ws, sym=True)
    compare("sym", eng.kernel_grads_weighted(ck, t(x1), None, t(np.tril(Ws)), sym=True), wc, wsc)
    half = eng.kernel_grads(ck, t(x1), t(np.tril(Ws)))   # gpar_gram_grad: 1/2 sum W dK
    compare("sym (gpar_gram_grad)", dict(coef=[2.0 * c for c in half["coef"]], factors=[[dict(scales=2.0 * g["scales"]) for g in fs] for fs in half["factors"]]), wc, wsc)
    gx = eng.kernel_input_grads(ck, t(x1), None, t(np.tril(Ws)), sym=True).cpu().numpy()
    assert np.max(np.abs(gx - wdx)) <= 1e-6 * np.max(np.abs(wdx)), (tag, "input sym", n)
    # DIAG: only the pairs (a, a) - a cosine factor is 1 there and does not move with its scales
    wc, wsc, _ = _complex_step_grads(terms, x1, x1, np.diag(wd))
    got = eng.kernel_grads_diag(ck, t(x1), t(wd))
    compare("diag", got, wc, wsc)
    for (coef, factors), fs in zip(terms, got["factors"]):
        for f, g in zip(factors, fs):
            if f["kind"] == "cos":
                assert np.all(np.asarray(g["scales"]) == 0.0)
    return worst


def _route(route):
    """Child process: the Gram and gradient cases of one route.  Prints the error of every case, then one JSON line."""
    from gpar_amd.engine import HipEngine
    from gpar_amd.kernels import compile_kernel

    eng = HipEngine()
    digests, worst = {}, 0.0
    if route != "archive":
        for nd in (1, 2, 3, 16, 17):
            rng = np.random.default_rng(nd)
            terms = _cos_terms(nd, rng)
            before = _stats()
            for n in SIZES:
                worst = max(worst, _check_gram(f"cos nd={nd}", terms, nd, n, rng, digests))
            after = _stats()
            assert after["failures"] == 0 and after["loaded"] == 0
            if route == "interpreter" or nd == 17:   # (17 dims with a cosine factor: no generated Gram kernel, the interpreter serves)
                assert after["compiled"] == before["compiled"], (route, nd)
            else:
                assert after["compiled"] > before["compiled"], (route, nd)
        rng = np.random.default_rng(100)
        terms = _eq_cos_terms(rng)
        for n in SIZES:
            worst = max(worst, _check_gram("eq x cos + linear", terms, 3, n, rng, digests))
        rng = np.random.default_rng(101)
        terms = _cos_without_exponent_terms(rng)
        for n in SIZES:
            worst = max(worst, _check_gram("cos terms without exponent", terms, 3, n, rng, digests))
        gworst = 0.0
        for tag, terms, width in (("cos", _cos_terms(3, np.random.default_rng(7)), 3), ("eq x cos", _eq_cos_terms(np.random.default_rng(8)), 3),
                                  ("regressor Q=2 m=2", _regressor_terms(2, 2, np.random.default_rng(9)), 3)):
            before = _stats()
            for n in (33, 66):
                gworst = max(gworst, _check_grads(tag, terms, width, n, np.random.default_rng(n), eng))
            after = _stats()
            assert after["failures"] == 0
            assert (after["compiled"] > before["compiled"]) == (route == "runtime"), (route, tag, before, after)
        print(json.dumps(dict(route=route, worst=worst, grad_worst=gworst, digests=digests, stats=_stats())))
        return
    # the archive: the structure GPARRegressor(spectral=2) builds at m = 1 (layer 1: with the linear output term; layer 0: without)
    for linear in (True, False):
        rng = np.random.default_rng(200 + linear)
        terms = _regressor_terms(1, 2, rng, linear=linear)
        before = _stats()
        for n in SIZES:
            worst = max(worst, _check_gram(f"regressor Q=2 m=1 linear={linear}", terms, 2 if linear else 1, n, rng, digests))
        ck = compile_kernel(_kernel_of(terms), 2 if linear else 1)
        x = rng.standard_normal((66, ck.width))
        Ws = rng.standard_normal((66, 66))
        Ws = Ws + Ws.T
        wc, wsc, _ = _complex_step_grads(terms, x, x, Ws, sym=True)
        half = eng.kernel_grads(ck, torch.tensor(x, device=eng.device), torch.tensor(np.tril(Ws), device=eng.device))
        got = np.concatenate([2.0 * np.asarray(half["coef"])] + [2.0 * np.asarray(g["scales"]) for fs in half["factors"] for g in fs])
        want = np.concatenate([np.asarray(wc)] + [np.asarray(s) for fs in wsc for s in fs])
        assert np.max(np.abs(got - want)) <= 1e-6 * np.max(np.abs(want))
        after = _stats()
        assert after["failures"] == 0 and after["entries"] >= 300 and after["compiled"] == before["compiled"]
        assert after["loaded"] >= before["loaded"] + 2, (before, after)   # the Gram kernel and the gradient pass came from the archive
    print(json.dumps(dict(route=route, worst=worst, digests=digests, stats=_stats())))


_RESULTS = {}


def _run_route(route):
    if route not in _RESULTS:
        env = dict(os.environ, **ROUTES[route])
        code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_spectral_gpu import _route; _route({route!r})"
        proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        print(proc.stdout[-6000:])
        assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
        _RESULTS[route] = json.loads(proc.stdout.strip().splitlines()[-1])
    return _RESULTS[route]


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_gram_and_gradients_on_every_route(route):
    res = _run_route(route)
    assert res["worst"] <= 1.0
    if route == "archive":
        assert res["stats"]["loaded"] >= 4 and res["stats"]["compiled"] == 0


def test_interpreter_and_generated_kernel_agree_in_bits():
    """Same helpers, same order: the cosine factor alone (1 to 17 dims), in a product with EQ beside a linear term, and in terms without an
    exponential factor behind a first term (0.7 * Cosine(), 0.45 * Linear() * Cosine(): the generator pins their product before the
    addition, which it would otherwise fuse).  (The linear term of the second structure
    carries the coefficient 1 that the regressor's kernels give it: a term of linear factors ALONE with another coefficient is
    coef * s + total, which the generated straight-line code may fuse into one multiply-add and the interpreter's factor loop does not -
    a property of such terms with or without a cosine factor in the kernel, seen here with 0.3 and not pursued.)"""
    a, b = _run_route("interpreter"), _run_route("runtime")
    assert sorted(a["digests"]) == sorted(b["digests"]) and len(a["digests"]) >= 56
    assert [k for k in a["digests"] if a["digests"][k] != b["digests"][k]] == []


# ---- large offsets, the diagonal, symmetry ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from gpar_amd.engine import set_engine

    e = make_engine("hip")
    previous = set_engine(e)
    yield e
    set_engine(previous)


def test_large_offsets_keep_the_phase(eng):
    """Time stamps near 1e6 with a period of 0.37: the differences of the rows are small and nearly exact, the rows' own angles are 2.7e6
    periods.  An implementation through per-row angles (cos A cos A' + sin A sin A') is off by ~1e-9 here."""
    from gpar_amd.kernels import compile_kernel

    rng = np.random.default_rng(3)
    for n in (33, 130):
        x = (1e6 + np.cumsum(rng.uniform(0.01, 0.2, n)))[:, None]
        terms = [(1.0, [dict(kind="cos", cols=[0], scales=[0.37])])]
        ck = compile_kernel(_kernel_of(terms), 1)
        got, want = _gram_device(ck, x, x[: n // 2 + 3]), _ref_gram(terms, x, x[: n // 2 + 3])
        assert np.allclose(got, want, rtol=1e-13, atol=1e-14)
        # ... and the restatement itself means the differences: against exact rational arithmetic of the float64 features
        z = x[:, 0] * (1.0 / 0.37)
        assert np.allclose(want, np.cos(2.0 * np.pi * np.subtract.outer(z, z[: n // 2 + 3])), atol=5e-9)
        A = 2.0 * np.pi * z
        angle_sum = np.outer(np.cos(A), np.cos(A[: n // 2 + 3])) + np.outer(np.sin(A), np.sin(A[: n // 2 + 3]))
        assert np.max(np.abs(angle_sum - want)) > 1e-11   # (what the device must not do)


def test_diagonal_is_one_and_gram_is_symmetric_in_bits(eng):
    from gpar_amd import hip as H
    from gpar_amd.kernels import compile_kernel

    rng = np.random.default_rng(4)
    for terms, width in ((_cos_terms(3, rng), 3), ([(1.0, [dict(kind="eq", cols=[0, 1], scales=[1.3, 0.7]), dict(kind="cos", cols=[0, 1], scales=[0.9, 1.7])])], 2)):
        ck = compile_kernel(_kernel_of(terms), width)
        x = rng.standard_normal((130, width)) * 5.0
        z = H.featurize(ck, torch.tensor(x, device=eng.device))
        assert np.all(H.gram_diag(ck, z).cpu().numpy() == 1.0)
        K = H.gram(ck, z, z.clone()).cpu().numpy()   # two arguments that hold the same rows: the full rectangular build
        assert np.array_equal(K, K.T) and np.all(np.diag(K) == 1.0)


# ---- the regressor ----------------------------------------------------------------------------------------------------------------
def _data(m, n=66, p=3, seed=0):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0, 2, (n, m)), axis=0)
    cols = []
    for i in range(p):
        f = np.sin(2 * np.pi * x.sum(1) / 0.5 + i) + 0.4 * np.sin(2 * np.pi * x[:, 0] / 0.19) + (0.5 * cols[-1] if cols else 0.0)
        cols.append(f + 0.1 * rng.standard_normal(n))
    y = np.stack(cols, axis=1)
    y[rng.random(y.shape) < 0.1] = np.nan
    y[0] = 0.3
    return x, y


def _ref_logpdf(v, x, y, Q):
    """Share-nothing GPAR log-density for impute=False, replace=False, unit weights, no normalisation: layer i sees the rows where
    outputs 0 .. i are all observed, inputs [x, y_0 .. y_{i-1}]; kernel var EQ + sum_q var_q EQ cos + linear over the previous outputs."""
    m, total = x.shape[1], 0.0
    rows = np.arange(x.shape[0])
    for i in range(y.shape[1]):
        rows = rows[~np.isnan(y[rows, i])]
        X = np.concatenate([x[rows], y[rows][:, :i]], axis=1)
        cols = list(range(m))
        terms = [(float(v[f"{i}/input/var"]), [dict(kind="eq", cols=cols, scales=np.reshape(v[f"{i}/input/scales"], -1))])]
        for q in range(Q):
            terms.append((float(v[f"{i}/input/sm{q}/var"]), [dict(kind="eq", cols=cols, scales=np.reshape(v[f"{i}/input/sm{q}/scales"], -1)),
                                                             dict(kind="cos", cols=cols, scales=np.reshape(v[f"{i}/input/sm{q}/pers"], -1))]))
        if i > 0:
            terms.append((1.0, [dict(kind="linear", cols=list(range(m, m + i)), scales=np.reshape(v[f"{i}/output/lin/scales"], -1))]))
        K = _ref_gram(terms, X, X) + (float(v[f"{i}/noise"]) + 1e-12) * np.eye(len(rows))
        yi = y[rows, i]
        total += -0.5 * (np.linalg.slogdet(K)[1] + len(rows) * np.log(2 * np.pi) + yi @ np.linalg.solve(K, yi))
    return total


def _regressor(m, **kw):
    from gpar_amd import GPARRegressor

    return GPARRegressor(spectral=2, spectral_period=(0.5, 0.19), spectral_scale=3.0, scale=0.7, noise=0.05, normalise_y=False, **kw)


@pytest.mark.parametrize("m", [1, 2])
def test_regressor_logpdf_matches_the_numpy_restatement(eng, m):
    x, y = _data(m)
    reg = _regressor(m, impute=False)
    got = float(reg.logpdf(x, y))
    want = _ref_logpdf(reg.get_variables(), x, y, 2)
    print(f"logpdf m={m}: {got!r} against {want!r}")
    assert abs(got - want) <= 1e-10 * abs(want)


@pytest.mark.parametrize("m", [1, 2])
def test_fit_gradient_matches_finite_differences_and_the_general_route(eng, m):
    """The prepared objective's (value, gradient) - what `fit` hands L-BFGS-B - per layer: against central differences of the numpy
    restatement over the latent vector (1e-6 of the largest component) and against the general route (value equal, gradient 1e-11)."""
    from .test_fastfit import _layer_objectives

    x, y = _data(m)
    reg = _regressor(m, impute=False)
    reg.condition(x, y)
    xn, yn = reg.x.numpy(), reg.y.numpy()
    for pi in range(reg.p):
        fast, fg, x0 = _layer_objectives(reg, eng, pi, None)
        xv = x0 + 0.1 * np.random.default_rng(pi).standard_normal(x0.shape)
        v_fast, g_fast = fast.fg(xv)
        v_ref, g_ref = fg(xv)
        assert v_fast == v_ref, (m, pi, v_fast, v_ref)
        np.testing.assert_allclose(g_fast, g_ref, rtol=1e-11, atol=1e-12 * max(1.0, np.abs(g_ref).max()))
        assert fast.fallbacks == 0

        def layer_value(vec):
            reg.vs.set_vector(vec, fast.names)
            v = reg.get_variables()
            return -(_ref_logpdf(v, xn, yn[:, : pi + 1], 2) - (_ref_logpdf(v, xn, yn[:, :pi], 2) if pi else 0.0))

        fd = np.zeros_like(xv)
        for k in range(xv.size):
            e = np.zeros_like(xv)
            e[k] = 1e-5
            fd[k] = (layer_value(xv - 2 * e) - 8 * layer_value(xv - e) + 8 * layer_value(xv + e) - layer_value(xv + 2 * e)) / (12 * 1e-5)
        err = np.max(np.abs(g_fast - fd)) / (1e-6 * np.max(np.abs(fd)))
        print(f"fit gradient m={m} layer {pi}: error / tolerance = {err:.2e}")
        assert err <= 1.0, (m, pi, g_fast, fd)
        reg.vs.set_vector(x0, fast.names)


@pytest.mark.parametrize("objective,kw", [("mll", {}), ("loo", {}), ("cv", dict(folds=4)), ("ahead", dict(horizon=(1, 4))), ("ahead", dict(horizon=1, window=8))])
@pytest.mark.parametrize("m", [1, 2])
def test_five_iterations_of_fit_raise_the_objective(eng, m, objective, kw):
    x, y = _data(m)

    def value(reg):
        if objective == "mll":
            return float(reg.logpdf(x, y))
        if objective == "loo":
            return float(reg.loo(x, y)[0])
        if objective == "cv":
            return float(reg.cv(x, y, **kw)[0])
        return float(np.sum(reg.ahead(x, y, **kw)[0]))

    reg = _regressor(m)
    before = value(reg)
    reg.fit(x, y, iters=5, objective=objective, **kw)
    after = value(reg)
    print(f"fit {objective} {kw} m={m}: {before:.6f} -> {after:.6f}")
    assert np.isfinite(after) and after > before


@pytest.mark.parametrize("m", [1, 2])
def test_the_rest_of_the_interface_runs(eng, m):
    from gpar_amd import GPARRegressor

    x, y = _data(m)
    xs = np.random.default_rng(1).uniform(0, 2, (17, m))
    reg = _regressor(m)
    reg.fit(x, y, iters=2)
    mean, lo, hi = reg.predict(xs, num_samples=20, credible_bounds=True)
    assert np.all(np.isfinite(mean)) and np.all(lo <= mean) and np.all(mean <= hi)
    rep = _regressor(m, replace=True)
    rep.condition(x, y)
    mu, var = rep.predict_moments(xs)
    assert np.all(np.isfinite(mu)) and np.all(var > 0)
    full = np.where(np.isnan(y), 0.1, y)   # (the incremental route of `update` takes complete outputs)
    reg.condition(x[:-4], full[:-4])
    reg.update(x[-4:], full[-4:])
    assert reg.n == 66 and np.array_equal(reg.y.numpy(), full)
    m_upd = reg.predict(xs, num_samples=20)
    assert np.all(np.isfinite(m_upd))
    x_ind, index, trace = reg.select_inducing(x, num=8)
    assert len(set(index.tolist())) == 8 and np.array_equal(x_ind, x[index])
    v = reg.get_variables()
    assert abs(trace[0] - 66 * float(v["0/input/var"] + v["0/input/sm0/var"] + v["0/input/sm1/var"])) <= 1e-9 * trace[0]   # k(x, x) = the sum of the variances
    assert np.all(np.diff(trace) <= 1e-12 * trace[0]) and trace[-1] >= -1e-9 * trace[0]
    sparse = GPARRegressor(spectral=2, spectral_period=(0.5, 0.19), spectral_scale=3.0, scale=0.7, noise=0.05, normalise_y=False, x_ind=x_ind)
    dense = float(_regressor(m).logpdf(x, y))
    bound = float(sparse.logpdf(x, y))
    assert np.isfinite(bound) and bound <= dense + 1e-6 * abs(dense)   # the variational bound lies below the exact value
    sparse.fit(x, y, iters=2, optimise_x_ind=True)
    assert np.isfinite(float(sparse.logpdf(x, y)))


# ---- what the keyword is for -------------------------------------------------------------------------------------------------------
def test_spectral_mixture_forecasts_a_two_tone_signal_better_than_eq(eng):
    """y = sin(2 pi x / 0.2) + 0.3 sin(2 pi x / 0.07) + noise 0.05 on 120 equally spaced rows of [0, 1]: after fit(iters=30) the
    16-rows-ahead score of spectral=2 started at periods (0.21, 0.065) exceeds that of the same model without the keyword.  Qualitative,
    no margin.  Checked beforehand on the CPU with this file's numpy restatement, scipy's L-BFGS-B (30 iterations on the log marginal
    likelihood of the normalised outputs) and seeds 0, 1, 2 of the noise: EQ alone -170.25 each time (16 rows are 0.134 in x, far
    beyond any length scale that fits the signal: the forecast is the prior's, -n/2 log(2 pi e)), the mixture 82.91 / 99.72 / 81.51 with
    learned periods 0.200 and 0.070."""
    from gpar_amd import GPARRegressor

    x = np.linspace(0.0, 1.0, 120)[:, None]
    y = np.sin(2 * np.pi * x / 0.2) + 0.3 * np.sin(2 * np.pi * x / 0.07) + 0.05 * np.random.default_rng(0).standard_normal((120, 1))
    values = {}
    for name, kw in (("eq", {}), ("spectral", dict(spectral=2, spectral_period=(0.21, 0.065)))):
        reg = GPARRegressor(**kw)
        reg.fit(x, y, iters=30)
        values[name] = float(np.sum(reg.ahead(x, y, horizon=16)[0]))
        if kw:
            print("periods:", reg.get_variables()["0/input/sm0/pers"], reg.get_variables()["0/input/sm1/pers"])
    print(f"ahead(horizon=16): EQ {values['eq']:.2f}, spectral=2 {values['spectral']:.2f}")
    assert np.isfinite(values["spectral"]) and values["spectral"] > values["eq"]
