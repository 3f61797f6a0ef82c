"""Scoring rules on the GPU: the six score-taking entries of the C ABI (gpar_loo_dense_score, gpar_loo_dense_grad_score,
gpar_loo_dense_grad_finish_score and their gpar_ahead_* counterparts) called directly, against the composed route of gpar_amd/gp.py on the CPU
oracle engine - value, means, variances, the weights W whole (1/2 diag W among them) and the kernel-parameter gradients the moment sums
give.  The composed route itself is held against the brute force and the complex step in tests/test_scores.py.

Sizes 7 / 33 / 64 / 65 / 130 / 200: below, one over and two of the 32-row tiles of the abar / band / S kernels, the 64-lane wave and one
over it; 130 and 200 rows reach the two-accumulator 128-stride loop of the row kernels (rolling origins: with every origin 0; leave-one-out:
in the first rows).  One case widens every leading dimension and strides y.  Tolerances: those tests/test_loo_gpu.py and
tests/test_ahead_gpu.py use for the same quantities under the log score - values rtol 1e-10, means / variances rtol 1e-8 / atol 1e-10,
W, 1/2 diag W and gradients rtol 1e-6 / atol 1e-7; both new rules meet them as they stand, so none was widened.  The score-taking entries with GPAR_SCORE_LOG must give the bits of the entries without
a rule, and two calls the same bits.
"""
import ctypes

import numpy as np
import pytest
import torch

from .conftest import make_engine
from .test_ahead import origins_for, ragged_origin
from .test_loo_gpu import KERNELS, _library_grads, _library_kernel

pytestmark = pytest.mark.gpu

LOG, CRPS, SE = 0, 1, 2
CODES = {"log": LOG, "crps": CRPS, "se": SE}
# n -> (kernel, origins of the rolling-origin case, noise per row?)
SHAPES = {7: ("eq_linear", "ragged", True), 33: ("rq_periodic", 2, True), 64: ("eq_linear", "ragged", False), 65: ("rq_periodic", 7, True),
          130: ("eq_linear", None, False), 200: ("eq_linear", None, True)}


@pytest.fixture
def hip():
    from gpar_amd.engine import set_engine

    eng = make_engine("hip")
    previous = set_engine(eng)
    yield eng
    set_engine(previous)


_CASES, _REFS = {}, {}


def _case(n):
    """Inputs of one size, made once and never modified."""
    if n not in _CASES:
        name, origin_key, weighted = SHAPES[n]
        rng = np.random.default_rng(1000 * n + weighted)
        t = (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / max(n, 8)
        x = np.stack([t, rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)], axis=1)
        y = np.sin(5.0 * x[:, 0]) + np.cos(3.0 * x[:, 1]) + 0.5 * x[:, 2] + 0.2 * rng.standard_normal(n)
        noise = 0.05 / rng.uniform(0.5, 2.0, n) if weighted else np.full(n, 0.05)
        origin = ragged_origin(n) if origin_key == "ragged" else origins_for(n, n if origin_key is None else origin_key)
        _CASES[n] = dict(n=n, name=name, x=x, y=y, noise=noise, origin=origin)
    return _CASES[n]


def _reference(n, objective, rule):
    """The composed route on the CPU oracle engine, once per case: value, means, variances, W (what it hands to the weighted-sum pass) and
    the kernel-parameter gradients that pass returns."""
    key = (n, objective, rule)
    if key not in _REFS:
        from gpar_amd.engine import set_engine
        from gpar_amd.gp import GP, Obs

        case = _case(n)
        eng = make_engine("oracle")
        previous = set_engine(eng)
        seen = []
        weighted_sum_pass = eng.kernel_grads

        def capture(ck, x, W):
            grads = weighted_sum_pass(ck, x, W)
            seen.append((W.detach().numpy().copy(), grads))
            return grads

        eng.kernel_grads = capture
        try:
            noise = torch.tensor(case["noise"], requires_grad=True)
            obs = Obs(GP(_library_kernel(case["name"], KERNELS[case["name"]][1]))(eng.tensor(case["x"]), noise), eng.tensor(case["y"]))
            value, mean, var = obs.loo(score=rule) if objective == "loo" else obs.ahead(case["origin"], score=rule)
            value.backward()
        finally:
            set_engine(previous)
        (W, grads), = seen
        K = KERNELS[case["name"]][0](case["x"], KERNELS[case["name"]][1]) + np.diag(case["noise"]) + 1e-12 * np.eye(n)
        _REFS[key] = dict(value=float(value.detach()), mean=mean.detach().numpy(), var=var.detach().numpy(), W=W,
                          grads=_library_grads(case["name"], grads), logdet=np.linalg.slogdet(K)[1])
    return _REFS[key]


def _padded(rows, cols, pad, dev, fill=None):
    buf = torch.empty(rows, cols + pad, dtype=torch.float64, device=dev)
    if fill is not None:
        buf.fill_(fill)
    return buf[:, :cols]


def _call(hip, case, objective, mode, score, pad=0, incy=1, noise=None, prefill=None):
    """One C ABI call with every buffer allocated here (leading dimensions widened by `pad`, y strided by `incy`): mode "value", "grad" or
    "finish" (build + batched factorisation + the finish form).  `score`: a GPAR_SCORE_* code for the score-taking entry, None for the
    entry without a rule.  `prefill`: every output buffer starts at that value.  Returns the return code and the buffers."""
    from gpar_amd import _lib
    from gpar_amd import hip as lib

    name, n = case["name"], case["n"]
    ck = hip.compile(_library_kernel(name, KERNELS[name][1]), 3)
    dev = torch.device("cuda:0")
    x = _padded(n, 3, pad, dev)
    x.copy_(torch.tensor(case["x"]))
    ybuf = torch.zeros(n, incy, dtype=torch.float64, device=dev)
    ybuf[:, 0] = torch.tensor(case["y"])
    nz = torch.tensor(case["noise"] if noise is None else noise, device=dev)
    og = torch.tensor(case["origin"], dtype=torch.int32, device=dev)
    cdll, nacc = _lib.load(), _lib.GRAD_NACC
    z, zd = _padded(n, 3, pad, dev), _padded(n, 3, pad, dev, fill=0.0)
    A = _padded(n + 1, n + 1, pad + (n + 1) % 2, dev, fill=prefill)
    X, W = _padded(n, n, pad + n % 2, dev, fill=prefill), _padded(n, n, pad + n % 2, dev, fill=prefill)
    T = _padded(n, n, pad + n % 2, dev)
    nblocks = max(1, min(((n + 63) // 64) * ((n + 63) // 64 + 1) // 2, 1024))
    grad = mode != "value"
    ahead = objective == "ahead"
    nvec = int(cdll.gpar_workspace_doubles(_lib.WS_AHEAD if ahead else _lib.WS_LOO, n, int(grad), 0))
    vec = torch.empty(nvec, dtype=torch.float64, device=dev)
    work = torch.empty(nblocks * nacc, dtype=torch.float64, device=dev)
    alpha = torch.full((n,), 0.0 if prefill is None else prefill, dtype=torch.float64, device=dev)
    out = torch.full((2 + nacc,), 0.0 if prefill is None else prefill, dtype=torch.float64, device=dev)
    vectors = torch.full((3, n), 0.0 if prefill is None else prefill, dtype=torch.float64, device=dev)
    info = torch.zeros(2, dtype=torch.int32, device=dev)
    stream = lib.stream_ptr(dev)
    fs, ks = ctypes.byref(ck.fspec), ctypes.byref(ck.kspec)
    ld = lib._ld
    entry = f"gpar_{objective}_dense" + {"value": "", "grad": "_grad", "finish": "_grad_finish"}[mode] + ("" if score is None else "_score")
    rule = () if score is None else (score,)
    extra = (og.data_ptr(),) if ahead else ()
    head = (fs, ks, x.data_ptr(), n, ld(x), ybuf.data_ptr(), incy)
    moments = (vectors[1].data_ptr(), vectors[2].data_ptr())
    if mode == "value":
        mats = (A.data_ptr(), ld(A)) if ahead else (A.data_ptr(), ld(A), X.data_ptr(), ld(X), T.data_ptr(), ld(T))
        rc = getattr(cdll, entry)(*head, nz.data_ptr(), 1e-12, z.data_ptr(), ld(z), *mats, vec.data_ptr(), out.data_ptr(), *moments, *extra, *rule,
                                  info.data_ptr(), 0, stream)
    elif mode == "grad":
        rc = getattr(cdll, entry)(*head, nz.data_ptr(), 1e-12, z.data_ptr(), zd.data_ptr(), ld(z), A.data_ptr(), ld(A), X.data_ptr(), ld(X), W.data_ptr(),
                                  ld(W), alpha.data_ptr(), vec.data_ptr(), work.data_ptr(), nblocks, out.data_ptr(), vectors[0].data_ptr(), *moments,
                                  *extra, *rule, info.data_ptr(), 0, stream)
    else:
        logdet = torch.zeros(1, dtype=torch.float64, device=dev)
        _lib.check(cdll.gpar_logpdf_dense_build(*head, nz.data_ptr(), 1e-12, z.data_ptr(), ld(z), A.data_ptr(), ld(A), logdet.data_ptr(), info.data_ptr(),
                                                stream), "build")
        _lib.check(cdll.gpar_potrf_batch(A.data_ptr(), 1, 0, n + 1, n, ld(A), logdet.data_ptr(), info.data_ptr(), 0, stream), "potrf_batch")
        rc = getattr(cdll, entry)(*head, z.data_ptr(), zd.data_ptr(), ld(z), A.data_ptr(), ld(A), logdet.data_ptr(), info.data_ptr(), X.data_ptr(), ld(X),
                                  W.data_ptr(), ld(W), alpha.data_ptr(), vec.data_ptr(), work.data_ptr(), nblocks, out.data_ptr(),
                                  vectors[0].data_ptr(), *moments, *extra, *rule, info[1:].data_ptr(), stream)
    torch.cuda.synchronize()
    return dict(rc=rc, out=out, half=vectors[0], mean=vectors[1], var=vectors[2], info=info.cpu().tolist(), W=W, A=A, X=X, alpha=alpha, ck=ck)


def _check(hip, case, ref, got, grad):
    n = case["n"]
    assert got["rc"] == 0 and got["info"] == [0, 0]
    out = got["out"].cpu().numpy()
    np.testing.assert_allclose(out[0], ref["value"], rtol=1e-10)
    np.testing.assert_allclose(out[1], ref["logdet"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(got["mean"].cpu().numpy(), ref["mean"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(got["var"].cpu().numpy(), ref["var"], rtol=1e-8, atol=1e-10)
    if not grad:
        return
    grads = _library_grads(case["name"], hip._grads_from_moments(got["ck"], out[2:], 0.5))
    print(f"  n={n}: value {out[0]:.12e} (composed {ref['value']:.12e}), gradients {grads} (composed {ref['grads']})")
    np.testing.assert_allclose(grads, ref["grads"], rtol=1e-6, atol=1e-7)
    il = np.tril_indices(n)
    W = got["W"].cpu().numpy()
    np.testing.assert_allclose(W[il], ref["W"][il], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(got["half"].cpu().numpy(), 0.5 * np.diag(ref["W"]), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(got["half"].cpu().numpy(), 0.5 * np.diag(W), rtol=0, atol=0)


@pytest.mark.parametrize("n", sorted(SHAPES))
@pytest.mark.parametrize("objective", ["loo", "ahead"])
@pytest.mark.parametrize("rule", ["crps", "se"])
def test_the_three_entries_against_the_composed_route(hip, n, objective, rule):
    case, ref = _case(n), _reference(n, objective, rule)
    for mode in ("value", "grad", "finish"):
        _check(hip, case, ref, _call(hip, case, objective, mode, CODES[rule]), grad=mode != "value")


@pytest.mark.parametrize("objective", ["loo", "ahead"])
def test_padded_leading_dimensions_and_strided_observations(hip, objective):
    case, ref = _case(65), _reference(65, objective, "crps")
    _check(hip, case, ref, _call(hip, case, objective, "grad", CRPS, pad=5, incy=3), grad=True)
    _check(hip, case, ref, _call(hip, case, objective, "finish", CRPS, pad=5, incy=3), grad=True)
    _check(hip, case, ref, _call(hip, case, objective, "value", CRPS, pad=3, incy=2), grad=False)


def _same_bits(a, b, n):
    il = torch.tril_indices(n, n)
    assert a["rc"] == b["rc"] == 0 and a["info"] == b["info"] == [0, 0]
    for key in ("out", "half", "mean", "var", "alpha"):
        assert torch.equal(a[key].nan_to_num(-1.0), b[key].nan_to_num(-1.0)), key
    assert torch.equal(a["W"][il[0], il[1]], b["W"][il[0], il[1]])
    assert torch.equal(a["A"], b["A"])


@pytest.mark.parametrize("objective", ["loo", "ahead"])
@pytest.mark.parametrize("n", [65, 130])
def test_the_log_rule_gives_the_bits_of_the_entries_without_a_rule_and_two_calls_give_the_same_bits(hip, objective, n):
    case = _case(n)
    for mode in ("value", "grad", "finish"):
        _same_bits(_call(hip, case, objective, mode, None, prefill=0.0), _call(hip, case, objective, mode, LOG, prefill=0.0), n)
        _same_bits(_call(hip, case, objective, mode, CRPS, prefill=0.0), _call(hip, case, objective, mode, CRPS, prefill=0.0), n)


@pytest.mark.parametrize("objective", ["loo", "ahead"])
def test_an_unknown_rule_is_an_argument_error_that_touches_nothing(hip, objective):
    case = _case(33)
    for mode in ("value", "grad"):
        for bad in (3, -1):
            got = _call(hip, case, objective, mode, bad, prefill=-7.0)
            assert got["rc"] == -1014 and got["info"] == [0, 0]
            for key in ("out", "half", "mean", "var", "alpha", "W", "A", "X"):
                assert bool((got[key] == -7.0).all()), key
    # the finish form: the factor is the caller's and stays; every output of the call keeps what it held
    got = _call(hip, case, objective, "finish", 3, prefill=-7.0)
    assert got["rc"] == -1014 and got["info"] == [0, 0]
    for key in ("out", "half", "mean", "var", "alpha", "W", "X"):
        assert bool((got[key] == -7.0).all()), key


@pytest.mark.parametrize("rule", ["crps", "se"])
def test_a_matrix_that_is_not_positive_definite_reports_and_leaves_the_outputs(hip, rule):
    """The input tests/test_ahead_gpu.py uses: a noise entry of -50 takes the positive definiteness away at row 11.  The rolling-origin
    entries leave value, moment sums, 1/2 diag W, means and variances as they were: their kernels return on a set info word.  (The
    leave-one-out entries make no such promise under any rule - include/gpar_hip.h - and are not part of this test.)"""
    case = _case(33)
    noise = case["noise"].copy()
    noise[10] = -50.0
    for mode in ("value", "grad", "finish"):
        got = _call(hip, case, "ahead", mode, CODES[rule], noise=noise, prefill=-7.0)
        assert got["rc"] == 0 and got["info"][0] == 11
        assert float(got["out"][0]) == -7.0 and bool((got["out"][2:] == -7.0).all())
        assert bool((got["mean"] == -7.0).all()) and bool((got["var"] == -7.0).all()) and bool((got["half"] == -7.0).all())


@pytest.mark.parametrize("objective,kw", [("loo", {}), ("ahead", dict(horizon=2))], ids=["loo", "ahead"])
def test_fit_with_the_crps_by_the_prepared_and_the_general_route(hip, objective, kw):
    from gpar_amd.regression import GPARRegressor

    from .test_ahead import _KW, regressor_data

    x, y = regressor_data(130, 2, seed=21, missing=0.0)
    finals = {}
    for fast in (True, False):
        reg = GPARRegressor(**_KW)
        reg.fast_fit = fast
        reg.condition(x, y)
        finals[fast] = reg._train(range(2), objective=objective, score="crps", iters=5, **kw)
    print(f"trained {objective} CRPS objectives, prepared / general:", finals[True], finals[False])
    for pi in range(2):
        np.testing.assert_allclose(finals[True][pi], finals[False][pi], rtol=1e-6)
