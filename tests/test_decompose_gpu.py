"""The decomposition by kernel component on the GPU: gpar_gram_terms, gpar_gram_terms_diag and gpar_posterior_terms through the C ABI
(padded leading dimensions, every factor type, term counts 1 / 3 / 8, four kinds of grouping), against gpar_gram (bits), the composed
route on the same device, and numpy; and GPARRegressor.decompose with the fused call on and off.

Tolerances: posterior means and marginal variances at tests/test_parity_gpu.py's rtol 1e-8 / atol 1e-10.  Gram entries "to rounding":
sums of at most 8 terms in another order differ by at most 8 ulp of the sum of the terms' magnitudes; against numpy's libm the table
arithmetic of the device kernels is good to 1e-13 relative (tests/test_gram_math_gpu.py) - 1e-12 is asserted."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from .conftest import make_engine, to_np

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-8, 1e-10
EPS = np.finfo(np.float64).eps
NS_ROWS = (1, 2, 31, 32, 33, 64, 65, 130)
NS_TEST = (1, 7, 33, 65)
NOISE = 0.1
SENTINEL = 7.25


@pytest.fixture
def hip():
    from gpar_amd.engine import set_engine

    eng = make_engine("hip")
    previous = set_engine(eng)
    yield eng
    set_engine(previous)


def _terms():
    """Eight product terms over two input columns that hold every factor type: EQ, RQ, the three Matern, linear, a periodic embedding,
    the cosine factor, and a constant term without a factor."""
    from gpar_amd.kernels import EQ, RQ, Cosine, Linear, Matern12, Matern32, Matern52, ZeroKernel

    return [
        1.3 * EQ().stretch(np.array([0.7, 1.1])).select([0, 1]),
        0.8 * RQ(0.7).stretch(0.9).select([1]),
        0.6 * Matern12().stretch(1.2).select([0]),
        0.9 * Matern32().stretch(0.8).select([1]),
        0.5 * (Matern52().stretch(1.0).select([0]) * Linear().stretch(2.0).select([1])),
        0.7 * (EQ().stretch(np.array([1.0, 1.4])).periodic(0.6).select([0]) * EQ().stretch(3.0).select([0])),
        0.4 * (EQ().stretch(1.5).select([0, 1]) * Cosine().stretch(np.array([0.5, 0.9])).select([0, 1])),
        ZeroKernel() + 0.3,
    ]


def _kernel(nterms):
    """The structure with 1, 3 or 8 of the terms (1: Matern 5/2 x linear; 3: periodic, cosine, constant)."""
    from gpar_amd.kernels import Kernel

    terms = _terms()
    pick = {1: [4], 3: [5, 6, 7], 8: list(range(8))}[nterms]
    return Kernel([t for i in pick for t in terms[i].terms])


def _groupings(nterms):
    """(comp, ncomp): identity, all in one, one with -1 entries, a non-contiguous one (with a component that holds no term)."""
    scattered = [2, 0, 2, -1, 1, 0, 1, -1][:nterms]
    return [(list(range(nterms)), nterms), ([0] * nterms, 1), ([0 if t % 2 == 0 else -1 for t in range(nterms)], 2 if nterms > 1 else 1),
            (scattered, 4)]


def _data(n, ns, seed=0):
    rng = np.random.default_rng(seed + 1000 * n + ns)
    return rng.uniform(-1, 1, (n, 2)), rng.standard_normal(n), rng.uniform(-1, 1, (ns, 2))


def _numpy_terms(kernel, a, b):
    """Per term of `kernel` its matrix k_t(a, b), by the numpy oracle kernels."""
    from gpar_amd.kernels import Kernel
    from oracle import kernels as ok

    return [ok.gram(ok.spec_to_dict(Kernel([t]).resolve(2)), a, b) for t in kernel.terms]


def _padded(rows, cols, ld, device):
    buf = torch.full((max(rows, 1), ld), SENTINEL, dtype=torch.float64, device=device)
    return buf, buf[:rows, :cols]


def _comp(comp):
    return (ctypes.c_int * max(len(comp), 1))(*comp)


def _lib_and_stream(eng):
    from gpar_amd import _lib, hip as hipmod

    return _lib.load(), hipmod.stream_ptr(eng.device)


def _cases():
    """Every (n, n*) with the term counts cycling over them, so that each count meets every residue of the sizes."""
    return [(n, ns, (1, 3, 8)[i % 3]) for i, (n, ns) in enumerate(itertools.product(NS_ROWS, NS_TEST))]


# ---- gpar_gram_terms / gpar_gram_terms_diag ------------------------------------------------------------------------------------------------
def test_gram_terms_against_gram_and_numpy(hip):
    lib, stream = _lib_and_stream(hip)
    for n, ns, nterms in _cases():
        kernel = _kernel(nterms)
        ck = hip.compile(kernel, 2)
        x, _, xs = _data(n, ns)
        z, zs = hip.features(ck, hip.tensor(x)), hip.features(ck, hip.tensor(xs))
        whole = to_np(hip.gram(ck, zs, z))
        ref = _numpy_terms(kernel, xs, x)
        magnitude = sum(np.abs(r) for r in ref)
        for (comp, ncomp), ldk in zip(_groupings(nterms), (n + 3, n + (n & 1) + 2, n, n + 1)):   # odd, even, tight, one more
            stride = ns * ldk + (6 if ldk % 2 == 0 else 5)   # (even leading dimension and stride: the 16-byte store path)
            buf = torch.full((ncomp * stride + 8,), SENTINEL, dtype=torch.float64, device=hip.device)
            rc = lib.gpar_gram_terms(ctypes.byref(ck.kspec), _comp(comp), ncomp, zs.data_ptr(), ns, int(zs.stride(0)), z.data_ptr(), n,
                                     int(z.stride(0)), ck.dz, buf.data_ptr(), ldk, stride, stream)
            assert rc == 0, (rc, n, ns, nterms, comp)
            got = to_np(buf)
            blocks = [got[g * stride:g * stride + ns * ldk].reshape(ns, ldk) for g in range(ncomp)]
            for g, block in enumerate(blocks):
                assert np.all(block[:, n:] == SENTINEL) and np.all(got[g * stride + ns * ldk:(g + 1) * stride] == SENTINEL)   # padding untouched
                want = sum((r for r, c in zip(ref, comp) if c == g), np.zeros((ns, n)))
                np.testing.assert_allclose(block[:, :n], want, rtol=1e-12, atol=1e-12 * (1 + np.abs(want).max()), err_msg=f"{n} {ns} {comp} {g}")
                if g not in comp:
                    assert np.all(block[:, :n] == 0.0)
            if ncomp == 1 and -1 not in comp:
                np.testing.assert_array_equal(blocks[0][:, :n], whole, err_msg=f"bits of gpar_gram: n={n} n*={ns} terms={nterms}")
            if comp == list(range(nterms)):
                assert np.all(np.abs(sum(b[:, :n] for b in blocks) - whole) <= 8 * EPS * magnitude), (n, ns, nterms)


def test_gram_terms_diag_against_gram_diag_and_numpy(hip):
    lib, stream = _lib_and_stream(hip)
    for ns, nterms in itertools.product((1, 7, 65, 257), (1, 3, 8)):
        kernel = _kernel(nterms)
        ck = hip.compile(kernel, 2)
        xs = _data(3, ns)[2]
        zs = hip.features(ck, hip.tensor(xs))
        ref = [np.diag(r) for r in _numpy_terms(kernel, xs, xs)]
        for comp, ncomp in _groupings(nterms):
            buf, out = _padded(ncomp, ns, ns + 3, hip.device)
            rc = lib.gpar_gram_terms_diag(ctypes.byref(ck.kspec), _comp(comp), ncomp, zs.data_ptr(), ns, int(zs.stride(0)), ck.dz, buf.data_ptr(),
                                          ns + 3, stream)
            assert rc == 0
            assert np.all(to_np(buf)[:, ns:] == SENTINEL)
            for g in range(ncomp):
                want = sum((r for r, c in zip(ref, comp) if c == g), np.zeros(ns))
                np.testing.assert_allclose(to_np(out)[g], want, rtol=1e-12, atol=1e-14)
            if ncomp == 1 and -1 not in comp:
                np.testing.assert_array_equal(to_np(out)[0], to_np(hip.gram_diag(ck, zs)))


# ---- gpar_posterior_terms ---------------------------------------------------------------------------------------------------------------
def _conditioned(hip, kernel, x, y):
    from gpar_amd.gp import GP, Obs

    f = GP(kernel)
    obs = Obs(f(hip.tensor(x), NOISE), hip.tensor(y))
    return f, obs


def _posterior_terms(hip, obs, p, comp, ncomp, variance=True, ws_doubles=None, pad=3):
    lib, stream = _lib_and_stream(hip)
    from gpar_amd import _lib

    fac = obs.factor()
    ck, z = obs.fdd.features()
    n, ns = obs.fdd.n, p.n
    alpha = fac.alpha().reshape(-1).contiguous()
    if ws_doubles is None:
        ws_doubles = lib.gpar_workspace_doubles(_lib.WS_POSTERIOR_TERMS, n, ns, ncomp)
    ws = torch.empty(ws_doubles + 2, dtype=torch.float64, device=hip.device)
    mbuf, mean = _padded(ncomp, ns, ns + pad, hip.device)
    vbuf, var = _padded(ncomp, ns, ns + pad + 1, hip.device)
    rc = lib.gpar_posterior_terms(ctypes.byref(ck.kspec), _comp(comp), ncomp, p.z.data_ptr(), ns, int(p.z.stride(0)), z.data_ptr(), n,
                                  int(z.stride(0)), ck.dz, alpha.data_ptr(), fac.L.data_ptr(), int(fac.L.stride(0)) if n > 1 else max(n, 1),
                                  mbuf.data_ptr(), ns + pad, vbuf.data_ptr() if variance else None, ns + pad + 1, ws.data_ptr(), int(ws_doubles), stream)
    assert rc == 0, rc
    assert np.all(to_np(mbuf)[:, ns:] == SENTINEL) and np.all(to_np(vbuf)[:, ns:] == SENTINEL)
    if not variance:
        assert np.all(to_np(vbuf) == SENTINEL)
    return to_np(mean).copy(), to_np(var).copy()


def _numpy_posterior(kernel, x, y, xs, comp, ncomp):
    train, cross, prior = _numpy_terms(kernel, x, x), _numpy_terms(kernel, xs, x), _numpy_terms(kernel, xs, xs)
    K = sum(train) + (NOISE + 1e-12) * np.eye(x.shape[0])
    L, alpha = np.linalg.cholesky(K), np.linalg.solve(K, y)
    mean, var = np.zeros((ncomp, xs.shape[0])), np.zeros((ncomp, xs.shape[0]))
    for g in range(ncomp):
        kc = sum((c for c, t in zip(cross, comp) if t == g), np.zeros((xs.shape[0], x.shape[0])))
        kd = sum((np.diag(c) for c, t in zip(prior, comp) if t == g), np.zeros(xs.shape[0]))
        mean[g] = kc @ alpha
        var[g] = kd - (np.linalg.solve(L, kc.T) ** 2).sum(0)
    return mean, var


def test_posterior_terms_against_the_composed_route_and_numpy(hip):
    for n, ns, nterms in _cases():
        kernel = _kernel(nterms)
        x, y, xs = _data(n, ns)
        f, obs = _conditioned(hip, kernel, x, y)
        p = f._pts(hip.tensor(xs))
        for comp, ncomp in _groupings(nterms):
            mean, var = _posterior_terms(hip, obs, p, comp, ncomp)
            again = _posterior_terms(hip, obs, p, comp, ncomp)
            np.testing.assert_array_equal(mean, again[0])   # the same bits every time: no atomics, fixed order
            np.testing.assert_array_equal(var, again[1])
            cm, cv = obs._components_composed(p, comp, ncomp, True)
            rm, rv = _numpy_posterior(kernel, x, y, xs, comp, ncomp)
            what = f"n={n} n*={ns} terms={nterms} comp={comp}"
            np.testing.assert_allclose(mean, to_np(cm), rtol=RTOL, atol=ATOL, err_msg=what)
            np.testing.assert_allclose(var, to_np(cv), rtol=RTOL, atol=ATOL, err_msg=what)
            np.testing.assert_allclose(mean, rm, rtol=RTOL, atol=ATOL, err_msg=what)
            np.testing.assert_allclose(var, rv, rtol=RTOL, atol=ATOL, err_msg=what)
            only_means = _posterior_terms(hip, obs, p, comp, ncomp, variance=False)
            np.testing.assert_array_equal(only_means[0], mean)


def test_posterior_terms_identities_and_chunked_variances(hip):
    """Sum of the components = the layer's posterior mean, one component of every term = its posterior variance; and a workspace that holds
    seven test rows at a time (ten chunks of the variance pass) gives the same moments."""
    n, ns, nterms = 130, 65, 8
    kernel = _kernel(nterms)
    x, y, xs = _data(n, ns)
    f, obs = _conditioned(hip, kernel, x, y)
    post = f | obs
    p = f._pts(hip.tensor(xs))
    want_mean, want_var = post.marginal_moments(hip.tensor(xs))
    each, _ = _posterior_terms(hip, obs, p, list(range(nterms)), nterms)
    one_mean, one_var = _posterior_terms(hip, obs, p, [0] * nterms, 1)
    np.testing.assert_allclose(each.sum(0), to_np(want_mean).reshape(-1), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(one_mean[0], to_np(want_mean).reshape(-1), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(one_var[0], to_np(want_var), rtol=RTOL, atol=ATOL)
    comp, ncomp = [2, 0, 2, -1, 1, 0, 1, -1], 3
    full = _posterior_terms(hip, obs, p, comp, ncomp)
    small = max(ncomp * ns, 7 * ncomp * (n + 3))
    chunked = _posterior_terms(hip, obs, p, comp, ncomp, ws_doubles=small)
    np.testing.assert_allclose(chunked[0], full[0], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(chunked[1], full[1], rtol=RTOL, atol=ATOL)
    np.testing.assert_array_equal(chunked[1], _posterior_terms(hip, obs, p, comp, ncomp, ws_doubles=small)[1])


def test_argument_errors_touch_no_output(hip):
    lib, stream = _lib_and_stream(hip)
    n, ns, nterms = 33, 7, 3
    kernel = _kernel(nterms)
    x, y, xs = _data(n, ns)
    f, obs = _conditioned(hip, kernel, x, y)
    p = f._pts(hip.tensor(xs))
    fac = obs.factor()
    ck, z = obs.fdd.features()
    alpha = fac.alpha().reshape(-1).contiguous()
    ws = torch.full((4096,), SENTINEL, dtype=torch.float64, device=hip.device)
    K = torch.full((3 * ns * n + 64,), SENTINEL, dtype=torch.float64, device=hip.device)
    mean = torch.full((3, ns), SENTINEL, dtype=torch.float64, device=hip.device)
    var, diag = mean.clone(), mean.clone()
    good = dict(comp=[0, 1, 2], ncomp=3, n=n, ns=ns, dz=ck.dz)
    bad = [dict(ncomp=0), dict(ncomp=9), dict(comp=[0, 3, 1]), dict(comp=[0, -2, 1]), dict(n=-1), dict(ns=-1), dict(dz=97), dict(dz=-1)]
    for change in bad:
        a = {**good, **change}
        rcs = [
            lib.gpar_gram_terms(ctypes.byref(ck.kspec), _comp(a["comp"]), a["ncomp"], p.z.data_ptr(), a["ns"], int(p.z.stride(0)), z.data_ptr(), a["n"],
                                int(z.stride(0)), a["dz"], K.data_ptr(), n, ns * n, stream),
            lib.gpar_posterior_terms(ctypes.byref(ck.kspec), _comp(a["comp"]), a["ncomp"], p.z.data_ptr(), a["ns"], int(p.z.stride(0)), z.data_ptr(),
                                     a["n"], int(z.stride(0)), a["dz"], alpha.data_ptr(), fac.L.data_ptr(), int(fac.L.stride(0)), mean.data_ptr(), ns,
                                     var.data_ptr(), ns, ws.data_ptr(), 4096, stream),
        ]
        if "n" not in change:   # (the diagonal has one point set: its row count is the `ns` of this table)
            rcs.append(lib.gpar_gram_terms_diag(ctypes.byref(ck.kspec), _comp(a["comp"]), a["ncomp"], p.z.data_ptr(), a["ns"], int(p.z.stride(0)),
                                                a["dz"], diag.data_ptr(), ns, stream))
        assert all(rc < 0 for rc in rcs), (change, rcs)
    # a workspace that cannot hold one split of the means, leading dimensions below the row count
    assert lib.gpar_posterior_terms(ctypes.byref(ck.kspec), _comp(good["comp"]), 3, p.z.data_ptr(), ns, int(p.z.stride(0)), z.data_ptr(), n,
                                    int(z.stride(0)), ck.dz, alpha.data_ptr(), fac.L.data_ptr(), int(fac.L.stride(0)), mean.data_ptr(), ns,
                                    var.data_ptr(), ns, ws.data_ptr(), 3 * ns - 1, stream) < 0
    assert lib.gpar_posterior_terms(ctypes.byref(ck.kspec), _comp(good["comp"]), 3, p.z.data_ptr(), ns, int(p.z.stride(0)), z.data_ptr(), n,
                                    int(z.stride(0)), ck.dz, alpha.data_ptr(), fac.L.data_ptr(), int(fac.L.stride(0)), mean.data_ptr(), ns - 1,
                                    var.data_ptr(), ns, ws.data_ptr(), 4096, stream) < 0
    assert lib.gpar_gram_terms(ctypes.byref(ck.kspec), _comp(good["comp"]), 3, p.z.data_ptr(), ns, int(p.z.stride(0)), z.data_ptr(), n,
                               int(z.stride(0)), ck.dz, K.data_ptr(), n - 1, ns * n, stream) < 0
    torch.cuda.synchronize()
    for out in (ws, K, mean, var, diag):
        assert bool((out == SENTINEL).all())


# ---- through the regressor: the fused call against the composed route -------------------------------------------------------------------
def test_regressor_decompose_fused_against_composed(hip, monkeypatch):
    from gpar_amd import GPARRegressor

    rng = np.random.default_rng(5)
    n, p = 66, 3
    x = rng.uniform(0, 1, (n, 2))
    y = np.stack([np.sin(6 * x[:, 0]) + x[:, 1], np.cos(5 * x[:, 1]) * x[:, 0], x[:, 0] - x[:, 1] ** 2], axis=1) + 0.05 * rng.standard_normal((n, p))
    y[rng.uniform(size=y.shape) < 0.1] = np.nan
    xs = rng.uniform(0, 1, (19, 2))
    reg = GPARRegressor(replace=True, per=True, spectral=2, input_linear=True, linear=True, nonlinear=True, noise=0.1)
    reg.condition(x, y)
    groups = {"seasonal": ["input/per", "input/sm*"], "trend": ["input/nonlin", "input/lin", "input/const"], "outputs": ["output/*"]}
    results = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("GPAR_FUSED_TERMS", switch)
        results[switch] = (reg.decompose(xs), reg.decompose(xs, groups))
    for fused, composed in zip(results["1"], results["0"]):
        assert fused.names == composed.names
        for i in range(p):
            np.testing.assert_allclose(fused.mean[i], composed.mean[i], rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(fused.var[i], composed.var[i], rtol=RTOL, atol=ATOL)
    mean, _ = reg.predict_moments(xs, latent=True)
    each = results["1"][0]
    for i in range(p):
        np.testing.assert_allclose(each.offset[i] + each.mean[i].sum(0), mean[:, i], rtol=RTOL, atol=ATOL)
