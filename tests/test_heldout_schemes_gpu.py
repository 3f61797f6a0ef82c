"""The held-out scheme objects on the GPU, for the six families at n = 130 (three 64-row tiles, the last ragged) with two input columns
and the rq_periodic kernel: folds [0, 40, 90, 130], a purged gap of 3, horizon 1, horizons (1, 4, 16) with weights (1, 0.5, 0.25), a
window of 16.

1. The prepared training objective (`fastfit.DenseLayerObjective`, its scheme made by `heldout.scheme_of` as `fastfit.build` makes it)
   and the wrapper `hip.<family>_dense_grad` call the same entry with the same arguments in other buffers: value, moment sums and
   1/2 diag W are equal to the bit (the entries are deterministic: tests/test_cv_gap_gpu.py asserts run-to-run equality).
2. Through `Obs`, each side of each limit of the fused calls - a fold of 64 / 65 rows, a purged block of 64 / 65, 8 / 9 horizons, a
   window of 64 / 65 rows - takes the fused or the composed route as `fits()` says (a spy on the engine instance), and the two routes
   agree to the parity rules of tests/test_ahead_window_gpu.py: values rtol 1e-10, means / variances rtol 1e-8 / atol 1e-10, gradients
   rtol 1e-6 / atol 1e-7.
3. A scheme uploads its arrays once: a second evaluation, and a second `Obs` that shares the scheme, reuse them.
"""
import numpy as np
import pytest
import torch

from .conftest import make_engine
from .test_heldout_schemes import FAMILIES, LIMITS, gradients_of, keywords, layer_data, limit_keywords, parametrised_obs, through_obs

pytestmark = pytest.mark.gpu

N, FOLDS, GAP, HORIZONS, WEIGHTS, WINDOW = 130, [0, 40, 90, 130], 3, (1, 4, 16), (1.0, 0.5, 0.25), 16


@pytest.fixture
def hip():
    from gpar_amd.engine import set_engine

    eng = make_engine("hip")
    previous = set_engine(eng)
    yield eng
    set_engine(previous)


def _wrapper_arguments(family, kw):
    """What `hip.<family>_dense_grad` takes behind `periodic`, from the keywords of `keywords`."""
    if family == "loo":
        return ()
    if family.startswith("cv"):
        return (kw["fold_start"],) + ((kw["hold"],) if family == "cv_gap" else ())
    return {"ahead": (kw["origin"],), "ahead_multi": (kw["origin"], kw.get("weights")), "ahead_window": (kw.get("lo"), kw["origin"])}[family]


@pytest.mark.parametrize("family", FAMILIES)
def test_the_prepared_objective_and_the_wrapper_give_the_same_bits(hip, family):
    from gpar_amd import _lib, fastfit
    from gpar_amd import hip as lib
    from gpar_amd.kernels import EQ, RQ, compile_kernel
    from gpar_amd.vars import Vars

    x, y, noise = layer_data(N)
    vs = Vars()
    tracer = fastfit._TracingVars(vs)
    s, alpha, sp, period = (tracer.bnd(float(v), name=name) for v, name in zip((0.6, 1.5, 0.8, 1.3), ("s", "alpha", "sp", "period")))
    noise_holder = tracer.bnd(0.05, name="noise")
    kernel = RQ(alpha).stretch(s).select([0]) * EQ().stretch(sp).periodic(period).select([1])
    X, yt, w = hip.tensor(x), hip.tensor(y), hip.tensor(0.05 / noise)   # (weights in 0.5 ... 2: the noise vector is noise / w)
    kw = keywords(family, N, FOLDS, GAP, HORIZONS, WEIGHTS, WINDOW)
    score = {} if family.startswith("cv") else {"score": "crps" if family == "ahead" else "log"}
    fast = fastfit.DenseLayerObjective(hip, vs, ["s", "alpha", "sp", "period", "noise"], kernel, noise_holder, tracer.holders, X, yt, w,
                                       **kw, **score)
    ck = compile_kernel(kernel, 2)
    value, _, half = fast._device_eval(ck, float(noise_holder))
    nacc = _lib.GRAD_NACC
    sums = fast.res_np[2:2 + nacc].copy()
    flags = {} if family == "ahead_window" else {"lookahead": True, "fused": True}
    out, *rest = getattr(lib, family + "_dense_grad")(ck, X, yt, fast.noise_vec, hip.epsilon, fast.periodic, *_wrapper_arguments(family, kw),
                                                      **flags, **score)
    want_half = rest[1] if family == "ahead_multi" else rest[0]
    info = rest[-2] if family == "ahead_window" else rest[-3]
    assert int(info.cpu()) == 0
    out = out.cpu().numpy()
    print(f"  {family}: value {value!r} / {out[0]!r}; largest moment-sum difference {np.abs(sums - out[2:]).max():.3e}; "
          f"largest 1/2 diag W difference {np.abs(half - want_half.cpu().numpy()).max():.3e}")
    assert fast.periodic and np.isfinite(value) and np.any(sums != 0.0)
    assert value == out[0]
    np.testing.assert_array_equal(sums, out[2:])
    np.testing.assert_array_equal(half, want_half.cpu().numpy())


def _routed(hip, scheme, x, y, noise, deferred):
    """(called the fused entry?, value, mean, var, parameter gradients, noise gradient) of one evaluation with gradients through `Obs`:
    with checks deferred the one-call form applies where the scheme fits; outside, no one-call form applies - the composed route."""
    import contextlib

    obs, params, noise_t = parametrised_obs(hip, x, y, noise, device="cuda:0")
    name = scheme.family + "_dense_grad"
    calls, real = [], getattr(hip, name)

    def spy(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)

    setattr(hip, name, spy)
    try:
        with (hip.defer_checks() if deferred else contextlib.nullcontext()):
            value, mean, var = through_obs(obs, scheme)
            grads, noise_grad = gradients_of(value, params, noise_t)
    finally:
        delattr(hip, name)
    return bool(calls), float(value.detach()), mean.cpu().numpy(), var.cpu().numpy(), grads, noise_grad


@pytest.mark.parametrize("kind,size", LIMITS)
def test_each_side_of_each_limit_takes_the_route_fits_names(hip, kind, size):
    from gpar_amd import heldout

    x, y, noise = layer_data(N)
    kw = limit_keywords(kind, size, N)
    scheme = heldout.scheme_of(**kw)
    fused, *got = _routed(hip, scheme, x, y, noise, deferred=True)
    assert fused == scheme.fits() == (size in (8, 64))
    composed, *want = _routed(hip, heldout.scheme_of(**kw), x, y, noise, deferred=False)
    assert not composed
    print(f"  {kind} {size}: {'fused' if fused else 'composed'} {got[0]!r}, composed {want[0]!r}")
    np.testing.assert_allclose(got[0], want[0], rtol=1e-10)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(got[2], want[2], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(got[3], want[3], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(got[4], want[4], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("family", FAMILIES[1:])   # (leave-one-out has nothing to upload)
def test_a_scheme_uploads_its_arrays_once(hip, family):
    from gpar_amd import heldout

    x, y, noise = layer_data(N)
    scheme = heldout.scheme_of(**keywords(family, N, FOLDS, GAP, HORIZONS, WEIGHTS, WINDOW))
    fused, first, *_ = _routed(hip, scheme, x, y, noise, deferred=True)
    assert fused
    uploaded = scheme.device(N, torch.device("cuda:0"))
    assert uploaded and all(isinstance(a, torch.Tensor) and a.is_cuda for a in uploaded[:1])

    def refuse(n, dev):
        raise AssertionError("the scheme uploaded its arrays a second time")

    scheme._upload = refuse
    for _ in range(2):   # (`_routed` makes a new `Obs` each time: two more `Obs` that share the scheme)
        fused, again, *_ = _routed(hip, scheme, x, y, noise, deferred=True)
        assert fused and again == first
        assert scheme.device(N, torch.device("cuda:0")) is uploaded
