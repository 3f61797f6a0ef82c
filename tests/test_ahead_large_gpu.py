"""Rolling-origin forecast scoring past one workgroup's reach: the expanding, the multi-horizon and the sliding-window entries of the
C ABI at n = 255 / 256 / 257 / 513 (300 too for the window form) - one below, at and one above the 256 rows a single 256-thread
workgroup covers in one pass (ahead_check_kernel, ahead_multi_check_kernel, the scan of ahead_window_gather_kernel; two rows a thread
in ahead_window_check_kernel), and two passes plus one row (three rows a thread).  The calls, the checks and the input recipe are those
of tests/test_ahead_gpu.py, test_ahead_multi_gpu.py and test_ahead_window_gpu.py, imported; the yardstick is tests/ahead_reference.py
(one factorisation instead of one solve per scored row; held against the brute force by tests/test_ahead_reference.py): np.longdouble
for values, log-determinants, means and variances, the complex step in complex128 for gradients.  What each case is there for - a second
pass, chunks without a scored row, a scan that breaks in one thread and goes on in another - is asserted from n, lo and origin alone in
tests/test_ahead_reference.py, on the CPU.

Tolerances: the parity rules (tests/test_cv_gpu.py) - values and the log-determinant rtol 1e-10, means / variances rtol 1e-8 / atol 1e-10,
W, 1/2 diag W and parameter gradients rtol 1e-6 / atol 1e-7, `torch.equal` where bits are compared.  Every comparison prints its
largest error over its tolerance (`-s`; collected in profiles/ahead_large_parity.txt).
"""
import numpy as np
import pytest
import torch

from . import ahead_reference as ref
from . import test_ahead_gpu as single
from . import test_ahead_multi_gpu as multi
from . import test_ahead_window_gpu as windowed
from .test_ahead import complex_step, origins_for, ragged_origin
from .test_ahead_gpu import hip  # noqa: F401  (the fixture)
from .test_ahead_window import window_starts
from .test_loo_gpu import KERNELS

pytestmark = pytest.mark.gpu

SIZES = [255, 256, 257, 513]
HORIZONS = [1, 7, 300, None, "ragged"]   # None: n
LATE_SIZES = [257, 513]
MULTI_SIZES = [257, 513]
MULTI_SETS = {"three": (7, 1, 64), "cap": (1, 2, 3, 4, 5, 6, 7, 8), "far": (1, 300)}
MULTI_RULES = ("log", "crps")
WINDOW_SIZES = [256, 257, 300, 513]
WINDOWS = [(1, 1), (7, 7), (64, 1), (64, 65)]   # (window, horizon)


# ---- the cases: inputs and index arrays, numpy alone (tests/test_ahead_reference.py reads them too) ----------------------------------
def kernel_of(n, salt):
    return "eq_linear" if (n + salt) % 2 == 0 else "rq_periodic"


def late_origin(n):
    """Rows below 200 unscored; row r >= 200 predicted from rows 0 ... max(192, r - 40) - 1: the chunks 0 ... 5 hold no scored row and no
    scored chunk has an origin left of column 192."""
    r = np.arange(n)
    return np.where(r < 200, -1, np.maximum(192, r - 40))


def origin_of(n, key):
    if isinstance(key, str):
        return {"ragged": ragged_origin, "late": late_origin}[key](n)
    return origins_for(n, n if key is None else key)


JUMP = 258   # the scored row at which lo of `ragged_window_large` jumps


def ragged_window_large(n, seed=7):
    """(lo, origin): every third row unscored (the middle one of the three rows a thread of the check kernel walks at n = 513), origins
    that advance by 0 - 2 rows a row, windows of 0 ... 64 rows - as long as they may be up to row 150, 40 rows and more from there to
    row JUMP, where lo jumps to the origin (a window of 0 rows, a step of more than 32), any length behind it -, lo and origin
    non-decreasing."""
    rng = np.random.default_rng(seed)
    origin = np.minimum(np.arange(n), np.cumsum(rng.integers(0, 3, n)))
    u = rng.integers(0, 65, n)
    u[JUMP] = 0
    lag = np.where(np.arange(n) < 150, 64, np.where(np.arange(n) < JUMP, 40 + u % 25, u))
    lo = np.maximum.accumulate(np.maximum(0, origin - lag))
    origin[1::3] = -1
    return lo, origin


def window_arrays(n, window, horizon):
    if window == "ragged":
        return ragged_window_large(n)
    return window_starts(n, horizon, window), origins_for(n, horizon)


def expanding_bad_origins(n=513):
    """{kind: (origin, the row that must be reported)} on horizon 2."""
    base = origins_for(n, 2)
    out = {}
    for kind, moves, row in (("row 511 alone", {511: 512}, 511), ("rows 300 and 270", {300: -2, 270: 271}, 270),
                             ("rows 256 and 45", {256: 257, 45: -2}, 45), ("rows 301 and 45, one thread", {301: 302, 45: 46}, 45)):
        bad = base.copy()
        for r, o in moves.items():
            bad[r] = o
        out[kind] = (bad, row)
    return out


def window_bad_arrays(n=513):
    """{kind: (lo, origin, the row that must be reported)}: one change each to well-formed arrays."""
    lo7, og7 = window_arrays(n, 7, 1)       # lo = max(0, r - 7), origin = r
    lo64, og64 = window_arrays(n, 64, 1)    # lo = max(0, r - 64), origin = r

    def moved(array, changes):
        out = array.copy()
        for r, v in changes.items():
            out[r] = v
        return out

    return {"lo decreases from row 383 to row 384": (moved(lo7, {384: lo7[383] - 1}), og7, 384),
            "origin decreases from row 300 to row 301": (lo7, moved(og7, {301: og7[300] - 1}), 301),
            "a window of 65 rows at row 500": (moved(lo64, {500: lo64[499]}), og64, 500),
            "rows 400 and 130": (moved(lo7, {130: og7[130] + 1}), moved(og7, {400: 401}), 130)}


_INPUTS = {}


def inputs(name, n, weighted):
    """x, y, noise by the recipe of tests/test_ahead_gpu.py's `_case`, K in float64 and the function (theta, noise) -> K: computed once,
    shared by every case on these inputs (as are the longdouble matrix and factor `long_factor` adds), never modified."""
    key = (name, n, weighted)
    if key not in _INPUTS:
        kfun, theta = KERNELS[name]
        rng = np.random.default_rng(1000 * n + weighted)
        t = (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / max(n, 8)
        x = np.stack([t, rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)], axis=1)
        y = np.sin(5.0 * x[:, 0]) + np.cos(3.0 * x[:, 1]) + 0.5 * x[:, 2] + 0.2 * rng.standard_normal(n)
        noise = 0.05 / rng.uniform(0.5, 2.0, n) if weighted else np.full(n, 0.05)

        def K(th, d):   # (longdouble noise: the whole matrix in longdouble)
            xx = x.astype(np.longdouble) if np.asarray(d).dtype == np.longdouble else x
            return kfun(xx, th) + np.diag(d) + 1e-12 * np.eye(n)

        _INPUTS[key] = dict(name=name, x=x, y=y, noise=noise, theta=theta, Kfun=K, K=K(theta, noise))
    return _INPUTS[key]


def long_matrix(inp):
    """K in longdouble (cached in the inputs)."""
    if "Kld" not in inp:
        inp["Kld"] = inp["Kfun"](inp["theta"].astype(np.longdouble), inp["noise"].astype(np.longdouble))
    return inp["Kld"]


def long_factor(inp):
    """K in longdouble and its factor with a = L^-1 y; the log-determinant goes into the inputs (all cached there)."""
    if "fac" not in inp:
        inp["fac"] = ref.factor(long_matrix(inp), inp["y"].astype(np.longdouble))
        inp["logdet"] = float(2.0 * np.sum(np.log(np.diagonal(inp["fac"][0]))))
    return inp["Kld"], inp["fac"]


def half_rows(n):
    """12 rows for 1/2 diag W: 0, the rows around 256 where they exist, n - 1, the others spread."""
    rows = [r for r in (0, 255, 256, 257, n - 1) if r < n]
    for r in np.linspace(0, n - 1, 23).astype(int)[1::2]:
        if len(set(rows)) < 12:
            rows.append(int(r))
    return np.array(sorted(set(rows)))


def _half(value, inp, rows):
    """d value / d noise_a = 1/2 W_aa at `rows`, by the complex step; `value(theta, noise)` on complex arguments."""
    out = np.zeros(len(rows))
    for i, a in enumerate(rows):
        moved_noise = inp["noise"].astype(complex)
        moved_noise[a] += 1e-30j
        out[i] = np.imag(value(inp["theta"].astype(complex), moved_noise)) / 1e-30
    return out


_CASES = {}


def expanding_case(n, key):
    ident = ("expanding", n, key)
    if ident not in _CASES:
        inp = inputs(kernel_of(n, key if isinstance(key, int) else 0), n, n % 2 == 1)
        origin = origin_of(n, key)
        Kld, fac = long_factor(inp)
        val, mean, var = ref.expanding(Kld, inp["y"], origin, fac=fac)

        def value(th, d):
            return ref.expanding(inp["Kfun"](th, d), inp["y"], origin)[0]

        rows = half_rows(n)
        _CASES[ident] = dict(inp, origin=origin, value=float(val), mean=mean.astype(float), var=var.astype(float),
                             grads=complex_step(lambda th: value(th, inp["noise"]), inp["theta"]), rows=rows, half=_half(value, inp, rows))
    return _CASES[ident]


def multi_case(n, key, rule, weights=None):
    ident = ("multi", n, key, rule, weights is None)
    if ident not in _CASES:
        horizons = MULTI_SETS[key] if isinstance(key, str) else key
        k = len(horizons)
        inp = inputs(kernel_of(n, k), n, n % 2 == 1)
        origins = np.stack([origins_for(n, h) for h in horizons])
        w = multi.weights_of(k) if weights is None else np.asarray(weights, dtype=float)
        Kld, fac = long_factor(inp)
        val, values, mean, var = ref.expanding_multi(Kld, inp["y"], origins, w.astype(np.longdouble), rule, fac=fac)

        def value(th, d):
            return ref.expanding_multi(inp["Kfun"](th, d), inp["y"], origins, w, rule)[0]

        rows = half_rows(n)
        _CASES[ident] = dict(inp, origins=origins, weights=w, rule=rule, value=float(val), values=values.astype(float), mean=mean.astype(float),
                             var=var.astype(float), grads=complex_step(lambda th: value(th, inp["noise"]), inp["theta"]), rows=rows,
                             half=_half(value, inp, rows))
    return _CASES[ident]


def window_case(n, window, horizon):
    ident = ("window", n, window, horizon)
    if ident not in _CASES:
        salt = 0 if window == "ragged" else window + horizon
        inp = inputs(kernel_of(n, salt), n, n % 2 == 1)
        lo, origin = window_arrays(n, window, horizon)
        val, mean, var = ref.window(long_matrix(inp), inp["y"].astype(np.longdouble), lo, origin)

        def value(th, d):
            return ref.window(inp["Kfun"](th, d), inp["y"], lo, origin)[0]

        rows = half_rows(n)
        half = np.zeros(len(rows))   # (K_aa moves the blocks that hold row a alone)
        for i, a in enumerate(rows):
            half[i] = 0.5 * ref.w_entries(lambda M, p, q: ref.window(M, inp["y"], lo, origin, rows=rows_holding(lo, origin, p, q))[0], inp["K"],
                                          [(a, a)])[0]
        _CASES[ident] = dict(inp, lo=lo, origin=origin, score="log", value=float(val), mean=mean.astype(float), var=var.astype(float),
                             grads=complex_step(lambda th: value(th, inp["noise"]), inp["theta"]), rows=rows, half=half)
    return _CASES[ident]


def rows_holding(lo, origin, a, b):
    """The scored rows whose block lo[r] ... origin[r] - 1, r holds both a and b."""
    r = np.arange(len(origin))
    inside = [(r == i) | ((lo <= i) & (i < origin)) for i in (a, b)]
    return np.flatnonzero((origin >= 0) & inside[0] & inside[1])


def late_entries(n):
    """24 entries (a, b), a >= b, of W for `late_origin`: across column 192 and row 256, an unscored row, and the corners."""
    rows = [r for r in (199, 200, 255, 256, 257 if n > 257 else 250) if r < n]
    cols = [190, 191, 192, 193]
    entries = [(a, b) for a in rows for b in cols] + [(0, 0), (n - 1, 0), (n - 1, n - 1), (n - 1, 192)]
    assert len(entries) == 24 and all(a >= b for a, b in entries)
    return entries


def window_entries(n, lo, origin, extra=()):
    """24 entries (a, b), a >= b, of W for a window case: rows 254 ... 259 (where they exist; then the rows before) against themselves, their neighbour, the
    first column of their block, the one before it (outside every block: zero) and the middle; the corners; `extra` first."""
    entries = list(extra)
    for a in (255, 256, 257, 254, 258, 259, 253, 252, 251, 250, 249, 248):
        if a >= n:
            continue
        first = int(lo[a])
        entries += [(a, a), (a, a - 1), (a, first), (a, max(first - 1, 0)), (a, (a + first) // 2)]
    entries += [(0, 0), (n - 1, n - 1), (n - 1, 0), (n - 1, n - 2), (1, 0), (n // 2, n // 2), (n // 2, n // 2 - 1)]
    entries += [(a, a - 2) for a in range(n - 2, 2, -37)]
    unique = []
    for e in entries:
        if e not in unique and e[0] >= e[1] >= 0:
            unique.append(e)
    assert len(unique) >= 24
    return unique[:24]


# ---- what is printed and collected -----------------------------------------------------------------------------------------------------
def _ratio(label, what, got, want, rtol, atol=0.0):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    both = ~(np.isnan(got) & np.isnan(want))
    worst = float(np.max(np.abs(got[both] - want[both]) / (atol + rtol * np.abs(want[both])))) if both.any() else 0.0
    print(f"ahead_large parity | {label} | {what} | error / tolerance {worst:.3g}")
    return worst


def _report(hip, label, case, got, grad, k=None):
    """Largest error over tolerance of every quantity `_check` holds (printed only: `_check` asserts)."""
    out = got["out"].cpu().numpy()
    _ratio(label, "value", out[0], case["value"], 1e-10)
    if "logdet" in case and k != "window":
        _ratio(label, "logdet", out[1], case["logdet"], 1e-10, 1e-12)
    mean, var = got["mean"].cpu().numpy(), got["var"].cpu().numpy()
    if isinstance(k, int):
        mean, var = mean[:k], var[:k]
        _ratio(label, "values", got["values"].cpu().numpy()[:k], case["values"], 1e-10)
    _ratio(label, "mean", mean, case["mean"], 1e-8, 1e-10)
    _ratio(label, "var", var, case["var"], 1e-8, 1e-10)
    if grad:
        grads = single._library_grads(case["name"], hip._grads_from_moments(got["ck"], out[2:], 0.5))
        _ratio(label, "gradient", grads, case["grads"], 1e-6, 1e-7)
        _ratio(label, "half diag W", got["half"].cpu().numpy()[case["rows"]], case["half"], 1e-6, 1e-7)


def _w_against(label, W, want, entries):
    got = np.array([W[a, b] for a, b in entries])
    _ratio(label, "W entries", got, want, 1e-6, 1e-7)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7)


# ---- the expanding form ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", HORIZONS, ids=lambda v: str(v))
@pytest.mark.parametrize("n", SIZES)
def test_expanding_form_three_modes_against_the_restatement(hip, n, key):
    case = expanding_case(n, key)
    label = f"expanding n={n} origin={key}"
    for mode in ("value", "grad", "finish"):
        got = single._call(hip, case, mode)
        assert got["info"] == [0, 0]
        _report(hip, f"{label} {mode}", case, got, grad=mode != "value")
        single._check(hip, case, got, grad=mode != "value")
        assert np.array_equal(np.isnan(got["mean"].cpu().numpy()), case["origin"] < 0)
        assert np.array_equal(np.isnan(got["var"].cpu().numpy()), case["origin"] < 0)
    K, y = case["K"], case["y"]
    if key == 1:   # the marginal likelihood: its value and its weights, whole
        Kinv = np.linalg.inv(K)
        alpha = Kinv @ y
        mll = -0.5 * (case["logdet"] + y @ alpha + n * np.log(2.0 * np.pi))
        np.testing.assert_allclose(got["out"].cpu().numpy()[0], mll, rtol=1e-10)
        il = np.tril_indices(n)
        _ratio(label, "W whole", got["W"].cpu().numpy()[il], (np.outer(alpha, alpha) - Kinv)[il], 1e-6, 1e-7)
        np.testing.assert_allclose(got["W"].cpu().numpy()[il], (np.outer(alpha, alpha) - Kinv)[il], rtol=1e-6, atol=1e-7)
    prior = np.flatnonzero(case["origin"] == 0)
    if key is None or key == 300:   # from the prior: mean 0, var = diag K - every row, or rows 0 ... 299
        assert prior.size == (n if key is None else min(n, 300)) and np.array_equal(prior, np.arange(prior.size))
        np.testing.assert_allclose(got["mean"].cpu().numpy()[prior], 0.0, atol=1e-10)
        np.testing.assert_allclose(got["var"].cpu().numpy()[prior], np.diag(K)[prior], rtol=1e-8)
    if key == 300 and n == 513:
        assert np.array_equal(case["origin"][300:], np.arange(300, n) - 299)
    if key == "ragged":
        assert (case["origin"] < 0).any()


@pytest.mark.parametrize("n", LATE_SIZES)
def test_late_origins_leave_whole_chunks_unscored_and_w_is_right_across_column_192_and_row_256(hip, n):
    case = expanding_case(n, "late")
    label = f"expanding n={n} origin=late"
    for mode in ("value", "grad", "finish"):
        got = single._call(hip, case, mode)
        assert got["info"] == [0, 0]
        _report(hip, f"{label} {mode}", case, got, grad=mode != "value")
        single._check(hip, case, got, grad=mode != "value")
        mean, var = got["mean"].cpu().numpy(), got["var"].cpu().numpy()
        assert np.isnan(mean[:200]).all() and np.isnan(var[:200]).all() and not np.isnan(mean[200:]).any() and not np.isnan(var[200:]).any()
    entries = late_entries(n)
    want = ref.w_entries(lambda M, a, b: ref.expanding(M, case["y"], case["origin"])[0], case["K"], entries)
    assert np.max(np.abs(want)) > 1e-2   # (the entries are not all lost in the absolute tolerance)
    _w_against(label, got["W"].cpu().numpy(), want, entries)


def test_expanding_form_bad_origins_behind_row_256_report_the_first_row_and_leave_the_outputs(hip):
    n = 513
    case = expanding_case(n, 7)
    for mode in ("value", "grad", "finish"):
        for kind, (bad, row) in expanding_bad_origins(n).items():
            got = single._call(hip, case, mode, origin=bad, prefill=True)
            assert got["info"][1 if mode == "finish" else 0] == n + 1 + row, (mode, kind, got["info"])
            assert float(got["out"][0]) == -7.0 and bool((got["out"][2:] == -7.0).all()), (mode, kind)
            assert bool((got["mean"] == -7.0).all()) and bool((got["var"] == -7.0).all()) and bool((got["half"] == -7.0).all()), (mode, kind)


def _same_bits(first, other, n, keys=("out", "half")):
    il = torch.tril_indices(n, n)
    for key in keys:
        assert torch.equal(other[key], first[key]), key
    assert torch.equal(other["var"].nan_to_num(-1.0), first["var"].nan_to_num(-1.0))
    assert torch.equal(other["mean"].nan_to_num(-1.0), first["mean"].nan_to_num(-1.0))
    assert torch.equal(other["W"][il[0], il[1]], first["W"][il[0], il[1]])


@pytest.mark.parametrize("n,key", [(513, 7), (257, "ragged")], ids=lambda v: str(v))
def test_expanding_finish_form_gives_the_bits_of_the_one_call_form_and_two_calls_give_the_same_bits(hip, n, key):
    case = expanding_case(n, key)
    first, second, finish = single._call(hip, case, "grad"), single._call(hip, case, "grad"), single._call(hip, case, "finish")
    assert first["info"] == [0, 0] and second["info"] == [0, 0] and finish["info"] == [0, 0]
    _same_bits(first, second, n)
    _same_bits(first, finish, n)


def test_expanding_form_with_padded_leading_dimensions(hip):
    case = expanding_case(257, 7)
    got = single._call(hip, case, "grad", pad=5)
    assert got["info"] == [0, 0]
    single._check(hip, case, got, grad=True)
    single._check(hip, case, single._call(hip, case, "value", pad=3), grad=False)


# ---- several horizons ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", MULTI_RULES)
@pytest.mark.parametrize("key", list(MULTI_SETS))
@pytest.mark.parametrize("n", MULTI_SIZES)
def test_multi_horizon_three_modes_against_the_restatement(hip, n, key, rule):
    case = multi_case(n, key, rule)
    k = len(case["origins"])
    label = f"multi n={n} horizons={MULTI_SETS[key]} {rule}"
    for mode in ("value", "grad", "finish"):
        got = multi._call(hip, case, mode)
        assert got["info"] == [0, 0]
        _report(hip, f"{label} {mode}", case, got, grad=mode != "value", k=k)
        multi._check(hip, case, got, grad=mode != "value")
    if key == "far" and n == 513:   # a row whose walk starts 300 columns back while its other horizon starts at the row itself
        assert case["origins"][0, 512] == 512 and case["origins"][1, 512] == 213


def test_one_horizon_of_weight_one_gives_the_bits_of_the_single_horizon_entry(hip):
    n = 513
    case = multi_case(n, (7,), "log", weights=(1.0,))
    lone = dict(case, origin=case["origins"][0])
    for mode in ("value", "grad", "finish"):
        a, b = single._call(hip, lone, mode), multi._call(hip, case, mode)
        assert a["info"] == [0, 0] and b["info"] == [0, 0]
        assert torch.equal(a["out"], b["out"]) and float(b["values"][0]) == float(a["out"][0])
        assert torch.equal(a["mean"], b["mean"][0]) and torch.equal(a["var"], b["var"][0])
        if mode != "value":
            il = torch.tril_indices(n, n)
            assert torch.equal(a["half"], b["half"]) and torch.equal(a["W"][il[0], il[1]], b["W"][il[0], il[1]])


def test_multi_horizon_bad_origin_in_the_second_array_alone_at_row_400(hip):
    n = 513
    case = multi_case(n, "three", "log")
    bad = case["origins"].copy()
    bad[1, 400] = 401
    for mode in ("value", "grad", "finish"):
        got = multi._call(hip, case, mode, origins=bad, prefill=True)
        assert got["info"][1 if mode == "finish" else 0] == n + 1 + 400, (mode, got["info"])
        assert multi._untouched(got), mode


# ---- the window form -------------------------------------------------------------------------------------------------------------------
def _window_w(label, case, got, extra=()):
    lo, origin = case["lo"], case["origin"]
    entries = window_entries(len(case["y"]), lo, origin, extra)
    want = ref.w_entries(lambda M, a, b: ref.window(M, case["y"], lo, origin, rows=rows_holding(lo, origin, a, b))[0], case["K"], entries)
    assert np.max(np.abs(want)) > 1e-2 and (want == 0.0).any()   # (entries inside the band, and outside it)
    _w_against(label, got["W"].cpu().numpy(), want, entries)


@pytest.mark.parametrize("window,horizon", WINDOWS, ids=lambda v: str(v))
@pytest.mark.parametrize("n", WINDOW_SIZES)
def test_window_form_two_modes_against_the_restatement(hip, n, window, horizon):
    case = window_case(n, window, horizon)
    label = f"window n={n} window={window} horizon={horizon}"
    value_only = windowed._call(hip, case, "value")
    assert value_only["info"] == [0]
    _report(hip, f"{label} value", case, value_only, grad=False, k="window")
    windowed._check(hip, case, value_only, grad=False)
    got = windowed._call(hip, case, "grad")
    assert got["info"] == [0]
    _report(hip, f"{label} grad", case, got, grad=True, k="window")
    windowed._check(hip, case, got, grad=True)
    _window_w(label, case, got)


def test_ragged_windows_with_unscored_rows_inside_a_thread_and_a_jump_of_lo(hip):
    n = 513
    case = window_case(n, "ragged", None)
    label = f"window n={n} ragged"
    value_only = windowed._call(hip, case, "value")
    assert value_only["info"] == [0]
    _report(hip, f"{label} value", case, value_only, grad=False, k="window")
    windowed._check(hip, case, value_only, grad=False)
    got = windowed._call(hip, case, "grad")
    assert got["info"] == [0]
    _report(hip, f"{label} grad", case, got, grad=True, k="window")
    windowed._check(hip, case, got, grad=True)
    unscored = case["origin"] < 0
    assert unscored.any() and np.array_equal(np.isnan(got["mean"].cpu().numpy()), unscored)
    lo = case["lo"]
    before = JUMP - 2 if unscored[JUMP - 1] else JUMP - 1   # the scored row before the jump
    across = [(JUMP, JUMP), (JUMP, JUMP - 1), (before, int(lo[before])), (JUMP + 2, JUMP), (JUMP + 2, int(lo[JUMP + 2])), (JUMP + 2, int(lo[before]))]
    _window_w(label, case, got, extra=across)


def test_malformed_windows_behind_row_256_report_the_first_offending_row_and_leave_the_outputs(hip):
    n = 513
    case = window_case(n, 7, 7)
    for mode in ("value", "grad"):
        for kind, (bad_lo, bad_origin, row) in window_bad_arrays(n).items():
            got = windowed._call(hip, case, mode, lo=bad_lo, origin=bad_origin, prefill=True)
            assert got["info"] == [n + 1 + row], (mode, kind, got["info"])
            assert windowed._untouched(got), (mode, kind)


@pytest.mark.parametrize("n,window,horizon", [(513, 64, 65), (513, "ragged", None)], ids=lambda v: str(v))
def test_window_form_two_calls_give_the_same_bits(hip, n, window, horizon):
    case = window_case(n, window, horizon)
    first, second = windowed._call(hip, case, "grad"), windowed._call(hip, case, "grad")
    assert first["info"] == [0] and second["info"] == [0]
    _same_bits(first, second, n)
