"""tests/ahead_reference.py - the restatement of rolling-origin scoring the GPU tests at n = 255 ... 513 are held to
(tests/test_ahead_large_gpu.py) - against the brute force of tests/test_ahead.py, test_ahead_multi.py and test_ahead_window.py (one fresh
solve per scored row) at n = 33 and 65, for every kind of origin array those GPU tests use, with the complex step of both on the kernel
parameters; then its own float64 against its longdouble at n = 513 on every GPU case; and, from n, lo and origin alone, that every GPU
case does what it is there for (a second pass of a 256-thread loop, chunks without a scored row, a scan that breaks in one thread and
goes on in another ...).  All on the CPU.

The restatement must agree with the brute force at least a factor 100 inside the GPU tolerances: value rtol 1e-12, means / variances
rtol 1e-10 / atol 1e-12, gradients rtol 1e-8 / atol 1e-9.  Largest discrepancies found (error over THAT tolerance, so 1 would be a
hundredth of the GPU tolerance; `-s` prints them):

    quantity          expanding   multi-horizon   window
    value             8.9e-3      8.1e-4          5.5e-3       (relative 8.9e-15 at worst)
    value, longdouble 8.3e-3      2.0e-3          9.1e-4
    per-horizon value -           5.2e-3          -
    mean              8.2e-3      3.0e-3          1.2e-3
    variance          1.9e-4      8.1e-5          9.9e-5
    gradient          4.7e-5      1.8e-5          5.2e-6
    W entries         2.2e-6      -               2.8e-5

float64 against longdouble restatement at n = 513, worst relative difference in value over every GPU case (must be below 1e-11, so
that the GPU's rtol 1e-10 on values measures the GPU and not the yardstick):

    1.9e-14 (17 cases: 6 expanding, 6 multi-horizon, 5 window)
"""
import numpy as np
import pytest

from . import ahead_reference as ref
from . import test_ahead_large_gpu as large
from .test_ahead import KFUN, THETA, brute_force, complex_step, layer_data, origins_for, ragged_origin
from .test_ahead_multi import multi_brute_force
from .test_ahead_multi_gpu import weights_of
from .test_ahead_window import window_brute_force, window_starts
from .test_ahead_window_gpu import ragged_window

AH_T, AH_NONE, AW_T, THREADS = 32, 0x7FFFFFFF, 32, 256   # gpar_amd/csrc/ahead.h, ahead_window.h


# ---- against the brute force ---------------------------------------------------------------------------------------------------------
def small_inputs(source, n):
    """(kfun(theta, noise) -> K, theta, y, noise): the GPU tests' recipe with the kernels of tests/test_loo_gpu.py ("gpu:..."), or
    tests/test_ahead.py's layer data with its k_* functions ("ahead:...")."""
    where, name = source.split(":")
    if where == "gpu":
        inp = large.inputs(name, n, n % 2 == 1)
        return inp["Kfun"], inp["theta"], inp["y"], inp["noise"]
    x, y, noise = layer_data(n, seed=8)
    return (lambda th, d: KFUN[name](x, th) + np.diag(d) + 1e-12 * np.eye(n)), THETA[name], y, noise


SOURCES = ["gpu:eq_linear", "gpu:rq_periodic", "ahead:eq_linear", "ahead:periodic"]


def small_late(n):
    """`late_origin` scaled to n rows: the first half unscored, then origins that stay at n / 2 - 4 before they follow the row."""
    r = np.arange(n)
    return np.where(r < n // 2, -1, np.maximum(n // 2 - 4, r - 6))


EXPANDING = {"h1": lambda n: origins_for(n, 1), "h7": lambda n: origins_for(n, 7), "h30": lambda n: origins_for(n, 30),
             "hn": lambda n: origins_for(n, n), "ragged": ragged_origin, "late": small_late}
MULTI = {"three": (7, 1, 64), "cap": (1, 2, 3, 4, 5, 6, 7, 8), "far": (1, 30)}
WINDOW = {"w1h1": (1, 1), "w7h7": (7, 7), "w64h1": (64, 1), "w64h65": (64, 65), "ragged": None}

_WORST = {}


def _hold(kind, what, got, want, rtol, atol=0.0):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    both = ~np.isnan(want)
    ratio = float(np.max(np.abs(got[both] - want[both]) / (atol + rtol * np.abs(want[both])))) if both.any() else 0.0
    _WORST[(kind, what)] = max(_WORST.get((kind, what), 0.0), ratio)
    print(f"restatement against brute force | {kind} | {what} | error / tolerance {ratio:.3g} (worst so far {_WORST[(kind, what)]:.3g})")
    assert ratio <= 1.0, (kind, what, ratio)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("which", list(EXPANDING))
@pytest.mark.parametrize("n", [33, 65])
def test_expanding_form_against_the_brute_force(n, which, source):
    kfun, theta, y, noise = small_inputs(source, n)
    origin = EXPANDING[which](n)
    K = kfun(theta, noise)
    want, got = brute_force(K, y, origin), ref.expanding(K, y, origin)
    _hold("expanding", "value", got[0], want[0], 1e-12)
    _hold("expanding", "mean", got[1], want[1], 1e-10, 1e-12)
    _hold("expanding", "var", got[2], want[2], 1e-10, 1e-12)
    long = ref.expanding(kfun(theta.astype(np.longdouble), noise.astype(np.longdouble)), y.astype(np.longdouble), origin)
    _hold("expanding", "value, longdouble", long[0], want[0], 1e-12)
    g_want = complex_step(lambda th: brute_force(kfun(th, noise), y, origin)[0], theta)
    g_got = complex_step(lambda th: ref.expanding(kfun(th, noise), y, origin)[0], theta)
    _hold("expanding", "gradient", g_got, g_want, 1e-8, 1e-9)


@pytest.mark.parametrize("source", SOURCES[:2])
@pytest.mark.parametrize("rule", ["log", "crps", "se"])
@pytest.mark.parametrize("key", list(MULTI))
@pytest.mark.parametrize("n", [33, 65])
def test_multi_horizon_form_against_the_brute_force(n, key, rule, source):
    kfun, theta, y, noise = small_inputs(source, n)
    origins = np.stack([origins_for(n, h) for h in MULTI[key]])
    w = weights_of(len(origins))
    K = kfun(theta, noise)
    want, got = multi_brute_force(K, y, origins, w, rule), ref.expanding_multi(K, y, origins, w, rule)
    _hold("multi", "value", got[0], want[0], 1e-12)
    _hold("multi", "values", got[1], want[1], 1e-12)
    _hold("multi", "mean", got[2], want[2], 1e-10, 1e-12)
    _hold("multi", "var", got[3], want[3], 1e-10, 1e-12)
    ld = np.longdouble
    long = ref.expanding_multi(kfun(theta.astype(ld), noise.astype(ld)), y.astype(ld), origins, w.astype(ld), rule)
    _hold("multi", "value, longdouble", long[0], want[0], 1e-12)
    g_want = complex_step(lambda th: multi_brute_force(kfun(th, noise), y, origins, w, rule)[0], theta)
    g_got = complex_step(lambda th: ref.expanding_multi(kfun(th, noise), y, origins, w, rule)[0], theta)
    _hold("multi", "gradient", g_got, g_want, 1e-8, 1e-9)
    # the comparison discriminates: a restatement that ignores one origin array is far outside it
    short = ref.expanding_multi(K, y, origins[:-1], w[:-1], rule)[0]
    assert abs(short - want[0]) > 1e-3 * abs(want[0])


@pytest.mark.parametrize("source", SOURCES[:2])
@pytest.mark.parametrize("which", list(WINDOW))
@pytest.mark.parametrize("n", [33, 65])
def test_window_form_against_the_brute_force(n, which, source):
    kfun, theta, y, noise = small_inputs(source, n)
    lo, origin = ragged_window(n) if which == "ragged" else (window_starts(n, WINDOW[which][1], WINDOW[which][0]), origins_for(n, WINDOW[which][1]))
    K = kfun(theta, noise)
    for rule in ("log", "crps"):
        want, got = window_brute_force(K, y, lo, origin, rule), ref.window(K, y, lo, origin, rule)
        _hold("window", "value", got[0], want[0], 1e-12)
        _hold("window", "mean", got[1], want[1], 1e-10, 1e-12)
        _hold("window", "var", got[2], want[2], 1e-10, 1e-12)
    ld = np.longdouble
    long = ref.window(kfun(theta.astype(ld), noise.astype(ld)), y.astype(ld), lo, origin, "crps")
    _hold("window", "value, longdouble", long[0], want[0], 1e-12)
    g_want = complex_step(lambda th: window_brute_force(kfun(th, noise), y, lo, origin)[0], theta)
    g_got = complex_step(lambda th: ref.window(kfun(th, noise), y, lo, origin)[0], theta)
    _hold("window", "gradient", g_got, g_want, 1e-8, 1e-9)
    # single entries of K, through the rows that hold them alone, against the brute force over every row
    entries = [(n - 1, n - 1), (n - 1, n - 2), (n // 2, n // 2 - 1), (n // 2, 0), (5, 5)]
    w_want = ref.w_entries(lambda M, a, b: window_brute_force(M, y, lo, origin)[0], K, entries)
    w_got = ref.w_entries(lambda M, a, b: ref.window(M, y, lo, origin, rows=large.rows_holding(lo, origin, a, b))[0], K, entries)
    _hold("window", "W entries", w_got, w_want, 1e-8, 1e-9)


def test_single_entries_of_k_in_the_expanding_form_against_the_brute_force():
    n = 33
    kfun, theta, y, noise = small_inputs("gpu:eq_linear", n)
    K, origin = kfun(theta, noise), small_late(n)
    entries = [(n - 1, n - 1), (n - 1, 0), (0, 0), (n // 2, n // 2 - 4), (n // 2 + 1, n // 2 - 5), (20, 3)]
    w_want = ref.w_entries(lambda M, a, b: brute_force(M, y, origin)[0], K, entries)
    w_got = ref.w_entries(lambda M, a, b: ref.expanding(M, y, origin)[0], K, entries)
    _hold("expanding", "W entries", w_got, w_want, 1e-8, 1e-9)


def test_erf_series_against_scipy_in_float64_and_in_longdouble():
    import scipy.special

    z = np.linspace(-9.0, 9.0, 721)
    # in longdouble the series is good to ~1e-18: against scipy within scipy's own 1 - 2 ulp of float64; in float64 its up to 260 terms
    # carry three roundings each (the terms shrink geometrically behind the largest, so a few dozen count): 1e-14
    np.testing.assert_allclose(ref.erf(z.astype(np.longdouble)).astype(float), scipy.special.erf(z), rtol=4.5e-16, atol=0)
    np.testing.assert_allclose(ref.erf(z), scipy.special.erf(z), rtol=1e-14, atol=0)


# ---- float64 against longdouble at the GPU cases ---------------------------------------------------------------------------------------
def _gpu_cases(n):
    """(label, function of the dtype -> value) of every GPU case at n rows."""
    cases = []

    def matrices(inp, dtype):
        if dtype == np.longdouble:
            return large.long_matrix(inp), inp["y"].astype(dtype)
        return inp["K"], inp["y"]

    for key in large.HORIZONS + (["late"] if n in large.LATE_SIZES else []):
        if n in large.SIZES:
            inp = large.inputs(large.kernel_of(n, key if isinstance(key, int) else 0), n, n % 2 == 1)
            cases.append((f"expanding n={n} {key}", lambda dt, inp=inp, key=key: ref.expanding(*matrices(inp, dt), large.origin_of(n, key))[0]))
    for key, horizons in large.MULTI_SETS.items():
        for rule in large.MULTI_RULES:
            if n in large.MULTI_SIZES:
                inp = large.inputs(large.kernel_of(n, len(horizons)), n, n % 2 == 1)
                origins = np.stack([origins_for(n, h) for h in horizons])
                w = weights_of(len(horizons))
                cases.append((f"multi n={n} {key} {rule}", lambda dt, inp=inp, origins=origins, w=w, rule=rule:
                              ref.expanding_multi(*matrices(inp, dt), origins, w.astype(dt), rule)[0]))
    for window, horizon in large.WINDOWS + ([("ragged", None)] if n == 513 else []):
        if n in large.WINDOW_SIZES:
            inp = large.inputs(large.kernel_of(n, 0 if window == "ragged" else window + horizon), n, n % 2 == 1)
            lo, origin = large.window_arrays(n, window, horizon)
            cases.append((f"window n={n} {window} {horizon}", lambda dt, inp=inp, lo=lo, origin=origin: ref.window(*matrices(inp, dt), lo, origin)[0]))
    return cases


def test_float64_restatement_against_the_longdouble_one_at_513():
    worst = 0.0
    for label, value in _gpu_cases(513):
        a, b = float(value(float)), value(np.longdouble)
        rel = float(abs(a - b) / abs(b))
        worst = max(worst, rel)
        print(f"float64 against longdouble | {label} | value {a:.15e} | relative difference {rel:.3g}")
    print(f"float64 against longdouble | worst {worst:.3g}")
    assert worst < 1e-11


# ---- every GPU case does what it is there for: from n, lo and origin alone ----------------------------------------------------------------
def _cmin(origins, n):
    origins = np.atleast_2d(origins)
    return [min([int(o) for o in origins[:, k * AH_T:(k + 1) * AH_T].ravel() if o >= 0], default=AH_NONE) for k in range((n + AH_T - 1) // AH_T)]


def test_the_expanding_cases_reach_a_second_pass_and_skip_whole_chunks():
    assert [(n + THREADS - 1) // THREADS for n in large.SIZES] == [1, 1, 2, 3]   # passes of `for (r = t; r < n; r += 256)`
    assert min(large.MULTI_SIZES) > THREADS and min(large.LATE_SIZES) > THREADS
    for n in large.LATE_SIZES:
        cmin = _cmin(large.late_origin(n), n)
        assert cmin[:6] == [AH_NONE] * 6 and all(192 <= c < AH_NONE for c in cmin[6:]) and len(cmin) > 8
        for c0 in range(0, 160, AH_T):   # these tiles skip every chunk
            assert all(c > c0 + AH_T - 1 for c in cmin)
        assert any(c <= 192 + AH_T - 1 for c in cmin)   # ... and the tile of column 192 does not
        entries = large.late_entries(n)
        assert {b for _, b in entries} >= {191, 192} and {a for a, _ in entries} >= {255, 256} and {(0, 0), (n - 1, 0), (n - 1, n - 1)} <= set(entries)
    # horizon 300 at 513: 17 chunks, ten of them with a row from the prior (no tile skips them); the tiles left of column 192 skip the last
    cmin = _cmin(origins_for(513, 300), 513)
    assert len(cmin) == 17 and cmin[:10] == [0] * 10 and cmin[16] == 512 - 299 and cmin[16] > 5 * AH_T + AH_T - 1
    # several horizons: the (1, 300) set makes row 512 walk from column 213 while its other horizon starts at 512
    origins = np.stack([origins_for(513, h) for h in large.MULTI_SETS["far"]])
    assert origins[0, 512] - origins[1, 512] == 299


def _first_bad_by_threads(origins, n):
    """(the row reported, {thread: [its bad rows]}) of the expanding checks: thread t walks rows t, t + 256, ..."""
    origins = np.atleast_2d(origins)
    bad = {}
    for r in range(n):
        if ((origins[:, r] < -1) | (origins[:, r] > r)).any():
            bad.setdefault(r % THREADS, []).append(r)
    return min(rows[0] for rows in bad.values()), bad


def test_the_bad_origins_lie_in_the_passes_they_are_meant_for():
    n = 513
    cases = large.expanding_bad_origins(n)
    for kind, (origin, row) in cases.items():
        first, bad = _first_bad_by_threads(origin, n)
        assert first == row == ref.expanding_check(origin), kind
    assert _first_bad_by_threads(cases["row 511 alone"][0], n)[1] == {255: [511]}                     # pass 2, the last thread
    assert _first_bad_by_threads(cases["rows 300 and 270"][0], n)[1] == {44: [300], 14: [270]}        # two threads, both in pass 2
    assert _first_bad_by_threads(cases["rows 256 and 45"][0], n)[1] == {0: [256], 45: [45]}           # two threads, passes 2 and 1
    assert _first_bad_by_threads(cases["rows 301 and 45, one thread"][0], n)[1] == {45: [45, 301]}    # one thread: its first stays
    origins = np.stack([origins_for(n, h) for h in large.MULTI_SETS["three"]])
    origins[1, 400] = 401
    assert ref.expanding_check(origins) == 400 and ref.expanding_check(origins[[0, 2]]) == -1 and 400 >= THREADS


def _window_threads(n):
    length = (n + THREADS - 1) // THREADS
    return length, lambda r: r // length


def test_the_window_cases_give_every_thread_of_the_check_several_rows():
    assert [_window_threads(n)[0] for n in large.WINDOW_SIZES] == [1, 2, 2, 3]
    n = 513
    length, thread = _window_threads(n)
    lo, origin = large.ragged_window_large(n)
    scored = origin >= 0
    assert ref.window_check(lo, origin) == -1
    # an unscored row inside the run of three rows of every thread; lo and origin non-decreasing over the scored rows
    assert all((~scored[t * length:(t + 1) * length]).any() and scored[t * length:(t + 1) * length].any() for t in range(n // length))
    assert (np.diff(lo[scored]) >= 0).all() and (np.diff(origin[scored]) >= 0).all()
    lengths = (origin - lo)[scored]
    assert lengths.min() == 0 and lengths.max() == 64 and len(set(lengths.tolist())) >= 40
    rows = np.flatnonzero(scored)
    jumps = np.diff(lo[rows])
    assert jumps.max() > 32 and rows[1:][np.argmax(jumps)] == large.JUMP
    # the error cases: the twin finds the stated rows; without its running-maximum condition it does not find the decreases
    cases = large.window_bad_arrays(n)
    for kind, (bad_lo, bad_origin, row) in cases.items():
        assert ref.window_check(bad_lo, bad_origin) == row, kind
    for kind in ("lo decreases from row 383 to row 384", "origin decreases from row 300 to row 301"):
        assert ref.window_check(*cases[kind][:2], monotone=False) == -1, kind
    assert thread(383) == 127 and thread(384) == 128 and 383 % length == length - 1   # across two threads
    assert thread(300) == thread(301) == 100                                           # inside one thread's run
    assert thread(400) != thread(130)
    bad_lo, bad_origin, _ = cases["a window of 65 rows at row 500"]
    assert bad_origin[500] - bad_lo[500] == 65 and bad_lo[500] >= bad_lo[499] and ref.window_check(bad_lo, bad_origin, window_max=65) == -1


def _gather_scan(lo, origin, n, i0, j1):
    """What the scan of one tile of the gather kernel does: per thread the passes it enters and the pass it breaks in (or None)."""
    entered, broke = np.zeros(THREADS, dtype=int), [None] * THREADS
    for t in range(THREADS):
        for p, r in enumerate(range(i0 + t, n, THREADS)):
            entered[t] = p + 1
            if origin[r] < 0:
                continue
            if lo[r] > j1:
                broke[t] = p
                break
    return entered, broke


def test_the_gather_scan_of_the_window_cases_takes_several_passes():
    n = 513
    for window, horizon in large.WINDOWS + [("ragged", None)]:
        lo, origin = large.window_arrays(n, window, horizon)
        # tile row 0: rows 0 ... 512 lie before its threads, which enter up to three passes
        entered, broke = _gather_scan(lo, origin, n, 0, AW_T - 1)
        assert entered.max() >= 2 and (n - 0 > THREADS)
        some = False
        for bi in range((n + AW_T - 1) // AW_T):
            for bj in range(bi + 1):
                entered, broke = _gather_scan(lo, origin, n, bi * AW_T, min(n, bj * AW_T + AW_T) - 1)
                some = some or (any(b == 0 for b in broke) and any(e >= 2 and b != 0 for e, b in zip(entered, broke)))
        assert some, (window, horizon)   # a thread that breaks in its first pass while another goes on to a second
    lo, origin = large.ragged_window_large(n)
    entered, broke = _gather_scan(lo, origin, n, 0, AW_T - 1)
    assert entered.max() == 3   # (an unscored row in the second pass is stepped over: row 1, 257, 513 - 256 = ... of thread 1)
    # the jump of lo: a tile whose columns lie in the gap, its rows before the jump - threads behind the jump break at once
    before = lo[large.JUMP - 1]
    j0 = (before // AW_T + 1) * AW_T
    assert lo[large.JUMP] > j0 + AW_T - 1 > before
    entered, broke = _gather_scan(lo, origin, n, 32, j0 + AW_T - 1)
    assert broke[large.JUMP - 32] == 0 and any(b != 0 and e >= 2 for e, b in zip(entered, broke))
