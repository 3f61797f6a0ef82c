"""tests/cv_reference.py - the yardstick of tests/test_cv_large_gpu.py - held to account on the CPU.

  deletion     at n = 1 / 2 / 7 / 17 / 33, both kernels of tests/test_loo_gpu.py, weighted and unweighted, every fold and hold generator
               of the GPU tests: the one-factorisation forms against `*_brute` (delete, condition, score; a solve each) in np.longdouble
               on values, means and variances, and 1/2 sum W o dK/dtheta against the complex step of the BRUTE-FORCE value - W is derived
               from the closed forms, so this is what makes it a quantity of its own and not a restatement of the device's algebra.
               Bounds: a hundredth of the GPU's parity tolerances (value rtol 1e-12, means / variances rtol 1e-10 / atol 1e-12, gradients
               rtol 1e-8 / atol 1e-9), so that what the yardstick itself is off by does not show in them.
  condition    for every GPU case the float64 evaluation of the closed form stays within SHARE = 1/8 of each parity tolerance of the
               longdouble evaluation (values, log-determinant, means, variances, W, 1/2 diag W; the gradients 1/2 sum W o dK against the
               complex step): the GPU's tolerances then measure the GPU.  The worst share per quantity is printed (`-s`).
  geometry     every reason a GPU case is in the table for (test_cv_large_gpu.REASONS), from n, fold_start, hold_lo, hold_hi and
               max_fold alone.
"""
import numpy as np
import pytest

from . import cv_reference as ref
from . import test_cv_large_gpu as large
from .test_loo_gpu import KERNELS

SMALL = [1, 2, 7, 17, 33]
SHARE = 1.0 / 8.0
_WORST = {}


def _hold(kind, what, got, want, rtol, atol=0.0):
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    ratio = float(np.max(np.abs(got - want) / (atol + rtol * np.abs(want))))
    _WORST[(kind, what)] = max(_WORST.get((kind, what), 0.0), ratio)
    print(f"closed form against deletion | {kind} | {what} | error / tolerance {ratio:.3g} (worst so far {_WORST[(kind, what)]:.3g})")
    assert ratio <= 1.0, (kind, what, ratio)


def small_inputs(name, n, weighted):
    """(S(theta, noise), theta, y, noise, dK/dtheta_j): the GPU tests' recipe for any kernel and weighting."""
    kfun, theta = KERNELS[name]
    rng = np.random.default_rng(1000 * n + weighted)
    x = rng.uniform(0.0, 1.0, (n, 3))
    y = np.sin(5.0 * x[:, 0]) + np.cos(3.0 * x[:, 1]) + 0.5 * x[:, 2] + 0.2 * rng.standard_normal(n)
    noise = 0.05 / rng.uniform(0.5, 2.0, n) if weighted else np.full(n, 0.05)

    def S(th, d):
        xx = x.astype(np.longdouble) if np.asarray(d).dtype == np.longdouble else x
        return kfun(xx, th) + np.diag(d) + 1e-12 * np.eye(n)

    dK = []
    for j in range(theta.size):
        moved = theta.astype(complex)
        moved[j] += 1e-30j
        dK.append(kfun(x, moved).imag / 1e-30)
    return S, theta, y, noise, dK


FORMS = [("loo", rule) for rule in large.RULES] + [("cv", kind) for kind in large.BLOCKED if kind != "loose"] + [("cv_gap", kind) for kind in large.PURGED]


def _extents(family, kind, n):
    if family == "loo":
        return None
    if family == "cv":
        starts = large.BLOCKED[kind][0](n)
        return starts, starts[:-1], starts[1:]
    return large.PURGED[kind][0](n)


def _closed(family, kind, S, y, ext, weights=True):
    if family == "loo":
        return ref.loo(S, y, kind, weights=weights)
    if family == "cv":
        return ref.blocked(S, y, ext[0], weights=weights)
    return ref.purged(S, y, *ext, weights=weights)


def _brute(family, kind, S, y, ext):
    if family == "loo":
        return ref.loo_brute(S, y, kind)
    if family == "cv":
        return ref.blocked_brute(S, y, ext[0])
    return ref.purged_brute(S, y, *ext)


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
@pytest.mark.parametrize("name", sorted(KERNELS))
@pytest.mark.parametrize("n", SMALL)
def test_one_factorisation_forms_equal_deletion_and_w_is_the_derivative_of_the_brute_force_value(n, name, weighted):
    S, theta, y, noise, dK = small_inputs(name, n, weighted)
    long = np.longdouble
    S_long, y_long = S(theta.astype(long), noise.astype(long)), y.astype(long)
    S_double = S(theta, noise)
    for family, kind in FORMS:
        ext = _extents(family, kind, n)
        if ext is not None:   # the generators give well-formed extents at every n
            starts, lo, hi = ext
            assert starts[0] == 0 and starts[-1] == n and np.all(np.diff(starts) >= 1) and np.all(lo <= starts[:-1]) and np.all(hi >= starts[1:])
            assert np.all(lo >= 0) and np.all(hi <= n) and np.all(np.diff(lo) >= 0) and np.all(np.diff(hi) >= 0) and int((hi - lo).max()) <= 64
        value, logdet, mean, var, _ = _closed(family, kind, S_long, y_long, ext, weights=False)
        b_value, b_mean, b_var = _brute(family, kind, S_long, y_long, ext)
        label = f"{family} {kind} n={n}"
        _hold(label, "value", value, b_value, 1e-12)
        _hold(label, "mean", mean, b_mean, 1e-10, 1e-12)
        _hold(label, "var", var, b_var, 1e-10, 1e-12)
        # numpy's own log-determinant: 52 bits against the longdouble factor's
        _hold(label, "logdet", logdet, np.linalg.slogdet(S_double)[1], 1e-12, 1e-13 * n)
        # W of the closed form against the complex step of the deletion's value
        W = _closed(family, kind, S_double, y, ext)[4]
        want = ref.complex_step(lambda th: _brute(family, kind, S(th, noise), y, ext)[0], theta)
        _hold(label, "gradient", [0.5 * np.sum(W * d) for d in dK], want, 1e-8, 1e-9)
        assert np.max(np.abs(want)) > 1e-3 or n <= 2   # (from 7 rows on the gradients are not lost in the absolute tolerance)
        np.testing.assert_allclose(W, W.T, rtol=0, atol=1e-12 * np.max(np.abs(W)))


def test_the_rules_and_their_sensitivities_agree_with_the_complex_step():
    """q = -dterm/de and s = -dterm/dv of cv_reference.sensitivities against the complex step through ahead_reference.term."""
    e, v = np.array([-2.5, -0.3, 0.0, 0.4, 3.0]), np.array([0.2, 1.0, 0.05, 2.0, 0.7])
    for rule in large.RULES:
        q, s = ref.sensitivities(rule, e, v)
        np.testing.assert_allclose(q, -np.imag(ref.term(rule, e + 1e-30j, v.astype(complex))) / 1e-30, rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(s, -np.imag(ref.term(rule, e.astype(complex), v + 1e-30j)) / 1e-30, rtol=1e-13, atol=1e-15)


# ---- the condition of the GPU cases --------------------------------------------------------------------------------------------------------
_SHARES = {}


def _share(c):
    label = f"{c['family']} {c['kind'] or c['rule']} n={c['n']}"
    for what in ("value", "logdet", "mean", "var", "W", "half", "grads"):
        share = large.over_tolerance(what, c["double"][what], c[what])
        _SHARES[what] = max(_SHARES.get(what, 0.0), share)
        print(f"float64 against longdouble | {label} | {what} | share of the tolerance {share:.3g} (worst so far {_SHARES[what]:.3g})")
        assert share <= SHARE, (label, what, share)


@pytest.mark.parametrize("n", large.SIZES)
def test_float64_closed_forms_stay_within_an_eighth_of_the_parity_tolerances_on_every_gpu_case(n):
    for m, rule in large.LOO_CASES:
        if m == n:
            _share(large.case("loo", None, n, rule))
    for family, cases in (("cv", large.BLOCKED_CASES), ("cv_gap", large.PURGED_CASES)):
        for m, kind in cases:
            if m == n:
                _share(large.case(family, kind, n))


# ---- what every GPU case is there for --------------------------------------------------------------------------------------------------------
def holds(reason, n, starts, lo, hi, bound):
    """Whether `reason` is true of the geometry."""
    blocks = hi - lo
    return {"m*m > 256 in some fold": int(blocks.max()) ** 2 > 256,
            "nfolds > 256": len(starts) - 1 > 256,
            "ceil(n/256) = 2": -(-n // 256) == 2,
            "some H equals its neighbour's": bool(np.any((np.diff(lo) == 0) & (np.diff(hi) == 0))),
            "max_fold exceeds the largest fold": bound > int(blocks.max()),
            "2 max_hold - 1 > n": 2 * bound - 1 > n,
            "last row block of 32 ragged": n % 32 != 0,
            "n odd, so cvg_ldp(n) = n + 1": n % 2 == 1 and n + (n & 1) == n + 1}[reason]


def test_every_gpu_case_is_what_the_table_says_it_is_there_for():
    cases = [("loo", None, n) for n in large.SIZES] + [("cv", kind, n) for n, kind in large.BLOCKED_CASES]
    cases += [("cv_gap", kind, n) for n, kind in large.PURGED_CASES]
    seen = set()
    for family, kind, n in cases:
        starts, lo, hi, bound = large.geometry(family, kind, n)
        assert starts[0] == 0 and starts[-1] == n and np.all(np.diff(starts) >= 1) and 1 <= bound <= 64 and int((hi - lo).max()) <= bound
        assert np.all(lo <= starts[:-1]) and np.all(hi >= starts[1:]) and np.all(np.diff(lo) >= 0) and np.all(np.diff(hi) >= 0)
        for reason in large.claimed(family, kind, n):
            assert holds(reason, n, starts, lo, hi, bound), (family, kind, n, reason)
            seen.add(reason)
    assert seen == set(large.ANY_KIND) | {r for table in large.REASONS.values() for r in table}   # (every reason is claimed somewhere)
    # the sizes and the fold patterns the issue names
    assert np.array_equal(np.diff(large.geometry("cv", "full", 257)[0]), [64, 64, 64, 64, 1])
    assert np.diff(large.geometry("cv", "full", 255)[0])[-1] == 63
    assert np.array_equal(np.diff(large.geometry("cv", "sq", 33)[0]), [16, 17])
    assert np.array_equal(np.diff(large.geometry("cv", "odd5", 15)[0])[:4], [5, 3, 1, 5]) and large.geometry("cv", "odd5", 15)[3] == 5
    assert large.geometry("cv", "loose", 15)[3] == 64
    assert [k for m, k in large.BLOCKED_CASES if m == 1] == ["ones"] and sorted(k for m, k in large.BLOCKED_CASES if m == 2) == ["full", "ones"]
    assert np.array_equal(large.geometry("cv", "full", 2)[0], [0, 2]) and np.array_equal(large.geometry("cv", "ones", 2)[0], [0, 1, 2])
    starts, lo, hi, bound = large.geometry("cv_gap", "f2g31", 257)
    assert bound == 64 and np.all(np.diff(starts)[:-1] == 2)
    starts, lo, hi, bound = large.geometry("cv_gap", "f64g0", 257)
    assert np.array_equal(lo, starts[:-1]) and np.array_equal(hi, starts[1:]) and bound == 64
    starts, lo, hi, bound = large.geometry("cv_gap", "left", 257)
    assert np.array_equal(hi, starts[1:]) and np.any(lo < starts[:-1])
    starts, lo, hi, bound = large.geometry("cv_gap", "right", 257)
    assert np.array_equal(lo, starts[:-1]) and np.any(hi > starts[1:])
    starts, lo, hi, bound = large.geometry("cv_gap", "plateau", 257)
    assert len(set(zip(lo[:3], hi[:3]))) == 1 and len(set(zip(lo[-3:], hi[-3:]))) == 1 and (lo[3], hi[3]) != (lo[2], hi[2])
    starts, lo, hi, bound = large.geometry("cv_gap", "short", 33)
    assert np.all(lo == 0) and np.all(hi == 33) and 2 * bound - 1 == 65
