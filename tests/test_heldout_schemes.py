"""The held-out scheme objects (gpar_amd/heldout.py) on the host: `scheme_of` maps the keywords of `fit(objective=...)` to a scheme and
raises the messages `DenseLayerObjective` always raised for a misplaced one; `fits()` holds at the limits of the fused calls (a fold or
a purged block of 64 / 65 rows, 8 / 9 horizons, a window of 64 / 65 rows); the one assembler of the entries' argument lists
(`hip.held_out_call`) produces, for every family and both forms, as many arguments of the kinds `_lib.SIGNATURES` declares; and on the
numpy oracle engine, which has no fused methods, every scheme takes the composed route through `Obs`, where an evaluation is not
disturbed by what an earlier one on the same `Obs` left pending.  The GPU side is tests/test_heldout_schemes_gpu.py, which shares the
helpers below."""
import ctypes

import numpy as np
import pytest
import torch

from gpar_amd import _lib, fastfit

FAMILIES = ["loo", "cv", "cv_gap", "ahead", "ahead_multi", "ahead_window"]
THETA = np.array([0.6, 1.5, 0.8, 1.3])   # the rq_periodic kernel of tests/test_loo_gpu.py: RQ scale, RQ alpha, periodic scale, period


def layer_data(n, seed=0):
    """x (n x 2, the first column a jittered time), y, a noise vector."""
    rng = np.random.default_rng(seed)
    t = (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / max(n, 8)
    x = np.stack([t, rng.uniform(0.0, 1.0, n)], axis=1)
    y = np.sin(5.0 * x[:, 0]) + np.cos(3.0 * x[:, 1]) + 0.2 * rng.standard_normal(n)
    return x, y, 0.05 / rng.uniform(0.5, 2.0, n)


def purged_hold(folds, gap, n):
    folds = np.asarray(folds)
    return np.maximum(folds[:-1] - gap, 0), np.minimum(folds[1:] + gap, n)


def keywords(family, n, folds, gap, horizons, weights, window):
    """The keywords `scheme_of` and `DenseLayerObjective` take for a family, from complete rows in time order."""
    from gpar_amd.model import rolling_origins

    if family == "loo":
        return dict(objective="loo")
    if family == "cv":
        return dict(objective="cv", fold_start=np.asarray(folds))
    if family == "cv_gap":
        return dict(objective="cv", fold_start=np.asarray(folds), hold=purged_hold(folds, gap, n))
    if family == "ahead_multi":
        return dict(objective="ahead", origin=np.stack([rolling_origins(np.arange(n), h, 0) for h in horizons]), weights=weights)
    origin = rolling_origins(np.arange(n), 1, 0)
    if family == "ahead_window":
        return dict(objective="ahead", origin=origin, lo=np.clip(np.arange(n) - window, 0, None))
    return dict(objective="ahead", origin=origin)


def through_obs(obs, scheme):
    """(value, mean, var) of `scheme` through the public method of `Obs` that takes it."""
    if scheme.family == "loo":
        return obs.loo()
    return obs.cv(scheme) if scheme.family.startswith("cv") else obs.ahead(scheme)


def parametrised_obs(eng, x, y, noise, device=None):
    """(obs, the kernel's four parameters, the noise vector): the rq_periodic kernel over tensors that require gradients."""
    from gpar_amd.gp import GP, Obs
    from gpar_amd.kernels import EQ, RQ

    params = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in THETA]
    kernel = RQ(params[1]).stretch(params[0]).select([0]) * EQ().stretch(params[2]).periodic(params[3]).select([1])
    noise = torch.tensor(noise, device=device, requires_grad=True)
    return Obs(GP(kernel)(eng.tensor(x), noise), eng.tensor(y)), params, noise


def gradients_of(value, params, noise):
    value.backward()
    got = np.array([float(p.grad) for p in params]), noise.grad.cpu().numpy().copy()
    for t in (*params, noise):
        t.grad = None
    return got


# ---- scheme_of ------------------------------------------------------------------------------------------------------------------
MISPLACED = [
    (dict(objective="elbo"), 'objective must be "mll", "loo", "cv" or "ahead"'),
    (dict(objective="cv"), 'fold_start belongs to objective="cv"'),
    (dict(objective="loo", fold_start=[0, 1]), 'fold_start belongs to objective="cv"'),
    (dict(objective="mll", fold_start=[0, 1]), 'fold_start belongs to objective="cv"'),
    (dict(objective="loo", hold=([0], [1])), 'hold belongs to objective="cv"'),
    (dict(objective="ahead"), 'origin belongs to objective="ahead"'),
    (dict(objective="loo", origin=[0, 1]), 'origin belongs to objective="ahead"'),
    (dict(objective="ahead", origin=[0, 1], weights=[1.0]), "weights belong to a K x n origin array"),
    (dict(objective="loo", weights=[1.0]), "weights belong to a K x n origin array"),
    (dict(objective="ahead", origin=[[0, 1], [0, 0]], lo=[0, 0]), "lo belongs to one array of origins"),
    (dict(objective="cv", fold_start=[0, 2], lo=[0, 0]), "lo belongs to one array of origins"),
]


@pytest.mark.parametrize("kw,message", MISPLACED, ids=lambda v: v if isinstance(v, str) else "-".join(v))
def test_a_misplaced_keyword_is_the_error_it_always_was(kw, message):
    from gpar_amd import heldout

    with pytest.raises(ValueError) as raised:
        heldout.scheme_of(**kw)
    assert str(raised.value) == message
    with pytest.raises(ValueError) as raised:
        fastfit.DenseLayerObjective(None, None, [], None, None, {}, None, None, None, **kw)
    assert str(raised.value) == message


def test_scheme_of_names_the_six_families():
    from gpar_amd import heldout

    assert heldout.scheme_of("mll") is None
    for family in FAMILIES:
        scheme = heldout.scheme_of(**keywords(family, 20, [0, 7, 13, 20], 2, (1, 2, 4), (1.0, 0.5, 0.25), 5))
        assert scheme.family == family
        assert scheme.takes_score == (family not in ("cv", "cv_gap"))
        assert scheme.factored == (family != "ahead_window")
        assert scheme.horizons == (3 if family == "ahead_multi" else None)
    with pytest.raises(ValueError):
        fastfit.DenseLayerObjective(None, None, [], None, None, {}, None, None, None, objective="cv", fold_start=[0, 2], score="crps")


# ---- fits() at the limits of the fused calls ---------------------------------------------------------------------------------------
def limit_keywords(kind, size, n=130):
    """The keywords of a scheme whose largest fold / purged block / number of horizons / longest window is `size`."""
    if kind == "fold":
        return keywords("cv", n, [0, size, 2 * size, n] if 2 * size < n else [0, size, n], 0, None, None, None)
    if kind == "block":   # (a gap of 3 on either side of the middle fold: the largest block)
        return keywords("cv_gap", n, [0, size - 6, 2 * size - 12, n], 3, None, None, None)
    if kind == "horizons":
        return keywords("ahead_multi", n, None, None, tuple(range(1, size + 1)), None, None)
    return keywords("ahead_window", n, None, None, None, None, size)


LIMITS = [(kind, size) for kind in ("fold", "block", "horizons", "window") for size in ((8, 9) if kind == "horizons" else (64, 65))]


@pytest.mark.parametrize("kind,size", LIMITS)
def test_fits_holds_up_to_the_limit_of_the_fused_call(kind, size):
    from gpar_amd import heldout

    scheme = heldout.scheme_of(**limit_keywords(kind, size))
    measured = {"fold": lambda s: int(np.diff(s.starts).max()), "block": lambda s: int((s.hi - s.lo).max()),
                "horizons": lambda s: s.horizons, "window": lambda s: s.longest}[kind](scheme)
    assert measured == size   # (the case is the boundary it claims to be)
    limit = {"fold": _lib.CV_MAX_FOLD, "block": _lib.CV_MAX_FOLD, "horizons": _lib.AHEAD_MAX_HORIZONS, "window": _lib.AHEAD_WINDOW_MAX}[kind]
    assert scheme.fits() == (size <= limit)
    if not scheme.fits():   # the upload refuses what the call does not take, in the words it always used
        upload = {"fold": "the fused cross-validation takes", "block": "the fused purged cross-validation takes",
                  "horizons": "the fused multi-horizon entries take", "window": "the fused sliding-window entries take"}[kind]
        with pytest.raises(ValueError, match=upload):
            scheme.device(130, "cpu")


# ---- the argument lists against the declared signatures ------------------------------------------------------------------------------
class _RecordingLibrary:
    """Stands where the loaded library stands: every entry records its arguments and succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0

        return entry


def _kind(argtype):
    if argtype in (ctypes.c_int, ctypes.c_long, ctypes.c_longlong):
        return "int"
    return "float" if argtype is ctypes.c_double else "pointer"


# ("mll": the log marginal likelihood goes through the same assembler, in its gradient form alone)
@pytest.mark.parametrize("family,grad", [(f, g) for f in FAMILIES for g in (False, True)] + [("mll", True)])
def test_the_argument_list_of_every_entry_matches_its_declaration(family, grad):
    from gpar_amd import heldout, hip
    from gpar_amd.kernels import EQ, RQ, compile_kernel

    n = 20
    scheme = None if family == "mll" else heldout.scheme_of(**keywords(family, n, [0, 7, 13, 20], 2, (1, 2, 4), (1.0, 0.5, 0.25), 5))
    ck = compile_kernel(RQ(THETA[1]).stretch(THETA[0]).select([0]) * EQ().stretch(THETA[2]).periodic(THETA[3]).select([1]), 2)
    names = ("x ldx y incy noise z ldz A lda out info mean var vec zd X ldxw W ldw alpha work half T ldt").split()
    p = {name: (16 if name.startswith("ld") or name == "incy" else 4096 + 64 * i) for i, name in enumerate(names)}
    values = torch.zeros(3, dtype=torch.float64)
    trailing = () if scheme is None else hip.held_out_trailing(scheme, n, "cpu", values, "crps")
    lib = _RecordingLibrary()
    hip.held_out_call(lib, scheme, grad, ck, p, n, 1e-12, 3, trailing, 0, ctypes.c_void_p(0))
    (name, args), = lib.calls
    assert name == ("gpar_logpdf_dense_grad" if scheme is None else scheme.entry(grad))
    declared = _lib.SIGNATURES[name][1]
    assert len(args) == len(declared)
    for at, (arg, argtype) in enumerate(zip(args, declared)):
        kind = _kind(argtype)
        if kind == "int":
            assert isinstance(arg, int) and not isinstance(arg, bool) and abs(arg) < 4096, (name, at, arg)   # (a count, never an address)
        elif kind == "float":
            assert isinstance(arg, float), (name, at, arg)
        else:
            assert arg is None or isinstance(arg, (ctypes.c_void_p, ctypes.Array)) or type(arg).__name__ == "CArgObject" or arg >= 4096, (name, at, arg)
    if scheme is not None and scheme.takes_score:
        assert _lib.SCORES["crps"] in args


# ---- the composed route on an engine without fused methods ---------------------------------------------------------------------------
@pytest.mark.parametrize("leave_pending", [False, True], ids=["backward-between", "first-left-pending"])
@pytest.mark.parametrize("family", FAMILIES)
def test_the_second_of_two_evaluations_on_one_obs_is_undisturbed(oracle_engine, family, leave_pending):
    from gpar_amd import heldout

    n = 20
    x, y, noise = layer_data(n)

    def scheme(name):
        return heldout.scheme_of(**keywords(name, n, [0, 7, 13, 20], 2, (1, 2, 4), (1.0, 0.5, 0.25), 5))

    other = FAMILIES[(FAMILIES.index(family) + 2) % len(FAMILIES)]   # (an earlier evaluation under another scheme, of another kind of W)
    for name in (family, other):
        assert not hasattr(oracle_engine, name + "_dense") and not hasattr(oracle_engine, name + "_dense_grad")
    fresh, fresh_params, fresh_noise = parametrised_obs(oracle_engine, x, y, noise)
    want_value, want_mean, want_var = through_obs(fresh, scheme(family))
    want = gradients_of(want_value, fresh_params, fresh_noise)
    obs, params, noise_t = parametrised_obs(oracle_engine, x, y, noise)
    first, _, _ = through_obs(obs, scheme(other))
    if not leave_pending:
        gradients_of(first, params, noise_t)
    value, mean, var = through_obs(obs, scheme(family))
    got = gradients_of(value, params, noise_t)
    assert float(value.detach()) == float(want_value.detach())
    np.testing.assert_array_equal(np.asarray(mean), np.asarray(want_mean))
    np.testing.assert_array_equal(np.asarray(var), np.asarray(want_var))
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert np.all(np.isfinite(got[0])) and np.any(got[0] != 0.0)
