"""The elementary functions of gpar_amd/csrc/gram_math.inc on the MI355X, over their whole range: bit for bit against the
operation-by-operation CPU model (tests/gram_math_emulation.py) and, with derived budgets, against mpmath at 256 bits.

One-term, one-factor kernels over one input column - coef * EQ, coef * RQ(alpha), coef * Matern12 / 32 / 52, each
.stretch([l]).select([0]) - so that an entry is one call of the function under test.  coef and alpha are read back out of the
compiled specification and the feature rows out of H.featurize: the doubles the device uses, featurisation rounding outside the
comparison.  The rows are generated with fixed seeds; that they reach every table entry was checked on the CPU when this file
was written, with the features computed engine-free as x * fl(1 / l) (what featurize_kernel does for a non-periodic dim), and is
asserted here on the features the device returns (test_arguments_reach_every_table_entry).

Budgets (eps = 2^-53; derivations in tests/test_gram_math.py):
  exph       4.5e-16 absolute per unit coefficient, 1e-13 relative above 2^-1000 (em.exph_budget)
  log1p      8.1 eps relative for u >= 2^-7, 17 * 2^-62 absolute below (em.log1p_budget)
  value      coef * (exph budget + k * 2 alpha * log1p budget), k the factor's value.  (d k / d L = -alpha k: the factor 2 leaves room
             for the two roundings of u = fl(s * fl(0.5 / alpha)), which move k by at most k alpha 2 eps u / (1 + u) - no more than
             k alpha times the log1p budget, since u / (1 + u) <= L and 2 eps u < 17 * 2^-62 below 2^-7.)
             Matern: coef * |polynomial| * exph budget + (4 + 2 c r) eps relative (tests/test_gram_math.py::matern_budget).
  derivative |2 d| * coef * |F| * (budget of the exponential part) + 4 eps relative, with d k / d s = coef * F * exponential part; plus
             |2 d| * 2^-1074: both routes form g = W coef d k / d s before they multiply by (z_a - z_b), and beyond d ~ 1e150 that g is
             a denormal (spacing 2^-1074) although the product is not."""
import ctypes
import functools
import math
import random

import mpmath as mp
import numpy as np
import pytest

from . import gram_math_emulation as em
from .test_gram_math import PREC, matern_closed_forms, rq_alpha_budget

pytestmark = pytest.mark.gpu

COEF = 1.3
SCALE = 0.7
ALPHAS = [0.05, 0.4, 1.5, 40.0, 1e4]
CASES = [("eq", None)] + [("rq", a) for a in ALPHAS] + [("matern12", None), ("matern32", None), ("matern52", None)]
IDS = [k if a is None else f"{k}-{a:g}" for k, a in CASES]
N_LOWER = 130
TINY = [1e-170, 2.3e-162, 1e-160, 1e-150]   # feature units: d^2 underflows to 0, is the smallest denormal, 1e-320, 1e-300


def _rq_u_list():
    """About 870 of the arguments of the CPU sweep (em.log1p_arguments): the edge where 1 + u rounds to 1, for every table interval
    j the three doubles around w = 2^e (1 + j / 128) at one exponent e (cycling through 0, 1, 10, 52, 100, 1000), the powers of two,
    a log-uniform fill of [1e-8, 1e8], the far end."""
    out = [5e-324, 1e-300, 2.0 ** -54, math.nextafter(2.0 ** -53, 0.0), 2.0 ** -53, math.nextafter(2.0 ** -53, 1.0), 2.0 ** -52]
    exps = (0, 1, 10, 52, 100, 1000)
    for j in range(128):
        w0 = math.ldexp(1.0 + (j + 0.5) / 128.0, exps[j % 6])   # mid-interval: the achieved u is not exactly the asked one
        out.append(w0 - 1.0 if w0 < 2.0 ** 53 else w0)
        w0 = math.ldexp(1.0 + j / 128.0, exps[(j + 3) % 6])
        for w in (math.nextafter(w0, 0.0), w0, math.nextafter(w0, math.inf)):
            if w >= 1.0:
                out.append(w - 1.0 if w < 2.0 ** 53 else w)
    for k in range(1, 61):
        out += [2.0 ** k - 1.0, 2.0 ** k]
    rng = random.Random(11)
    out += [10.0 ** rng.uniform(-8.0, 8.0) for _ in range(230)]
    out += [1e100, 1e300]
    return out


def feature_targets(kind, alpha):
    """Distances to row 0 in feature units (row 0 is at 0), fixed order: row 0, the shared edge rows, then the kind's own list shuffled
    with a fixed seed (so that the first N_LOWER rows, whose lower triangle is built, are a mixed sample)."""
    shared = [0.0, 0.0, 0.37, 0.37, 1e14] + TINY   # two pairs of exactly coincident rows (rows 0, 1 and 2, 3); 1e14 feature units
    if kind == "eq":      # the list of tests/test_hip_primitives.py::test_gram_exponential_over_its_whole_range
        rng = np.random.default_rng(3)
        half = np.concatenate([rng.uniform(0, 1, 80), rng.uniform(0, 40, 400), rng.uniform(600, 800, 150), [745.1, 746.0, 1e6]])
        own = [math.sqrt(2.0 * h) for h in half]
    elif kind == "rq":    # (no distance whose square overflows: nothing is claimed there)
        own = [math.sqrt(2.0 * alpha * u) for u in _rq_u_list() if 2.0 * alpha * u < 1e307]
    else:
        c = em.MATERN_C[em.NU2[kind]]
        rng = random.Random(5)
        own = [10.0 ** rng.uniform(-10.0, 3.0) for _ in range(300)] + [rng.uniform(0.0, 800.0) / c for _ in range(450)]
        own += [cr / c for cr in (700.0, 708.0, 709.0, 744.0, 745.0, 745.13, 745.2, 746.0, 1e3, 1e7)]
    random.Random(7).shuffle(own)
    return shared + own


def _kernel(kind, alpha):
    from gpar_amd import kernels as gk

    base = {"eq": gk.EQ, "matern12": gk.Matern12, "matern32": gk.Matern32, "matern52": gk.Matern52}
    k = gk.RQ(alpha) if kind == "rq" else base[kind]()
    return gk.compile_kernel((COEF * k.stretch(np.array([SCALE]))).select([0]), 1)


def exp_part(kind, alpha, s):
    """(X, budget of X) at mpmath precision: the exponential part of the factor at squared distance s (an exact double) and the
    absolute error the table functions are allowed in it."""
    s = mp.mpf(s)
    if kind == "eq":
        X = mp.exp(-s / 2)
        return X, em.exph_budget(float(X))
    if kind == "rq":
        a = mp.mpf(alpha)
        u = s / (2 * a)
        L = mp.log1p(u)
        X = mp.exp(-a * L)
        return X, em.exph_budget(float(X)) + float(X) * 2.0 * alpha * em.log1p_budget(float(u), float(L))
    c = mp.sqrt(em.NU2[kind])
    cr = c * mp.sqrt(s)
    X = mp.exp(-cr)
    return X, em.exph_budget(float(X)) + 2.0 * float(cr) * em.EPS * float(X)


def algebraic_parts(kind, alpha, s):
    """(P, F): k = coef P X and d k / d s = coef F X."""
    s = mp.mpf(s)
    if kind == "eq":
        return mp.mpf(1), -mp.mpf(1) / 2
    if kind == "rq":
        return mp.mpf(1), -mp.mpf(1) / (2 * (1 + s / (2 * mp.mpf(alpha))))
    nu2 = em.NU2[kind]
    k, dk = matern_closed_forms(nu2, s)
    X = mp.exp(-mp.sqrt(nu2) * mp.sqrt(s))
    return k / X, dk / X


@functools.lru_cache(maxsize=None)
def case_data(kind, alpha):
    """Everything of a case that both routes share, computed once: the device's features, coefficient and alpha, the emulated column
    and lower triangle, the mpmath values with their budgets."""
    import torch

    from gpar_amd import hip as H

    dev = torch.device("cuda:0")
    ck = _kernel(kind, alpha)
    coef = float(ck.kspec.coef[0])
    a = float(ck.kspec.factor[0].alpha) if kind == "rq" else None
    per_unit = float(H.featurize(ck, torch.tensor([[1.0]], dtype=torch.float64, device=dev)).cpu()[0, 0])
    x = np.array(feature_targets(kind, alpha))[:, None] / per_unit
    z = H.featurize(ck, torch.tensor(x, dtype=torch.float64, device=dev))[:, :1].contiguous()
    zf = [float(v) for v in z.cpu().numpy()[:, 0]]
    assert zf[0] == 0.0 and zf[1] == 0.0 and zf[2] == zf[3] and abs(zf[4] - 1e14) < 1e-1
    col = np.array([em.entry(kind, coef, a, zi, zf[0]) for zi in zf])
    low = np.array([em.entry(kind, coef, a, zf[i], zf[j]) for i in range(N_LOWER) for j in range(i + 1)])
    with mp.workprec(PREC):
        ref, budget = [], []
        for zi in zf:
            s = em.sqdist(zi, zf[0])
            X, bx = exp_part(kind, a, s)
            P, _ = algebraic_parts(kind, a, s)
            ref.append(coef * P * X)
            if kind.startswith("matern"):
                cr = float(mp.sqrt(em.NU2[kind]) * mp.sqrt(mp.mpf(s)))
                budget.append(coef * float(P) * em.exph_budget(float(X)) + (4.0 + 2.0 * cr) * em.EPS * float(coef * P * X))
            else:
                budget.append(coef * bx)
    return dict(ck=ck, coef=coef, alpha=a, z=z, zf=zf, col=col, low=low, ref=ref, budget=budget)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.view(np.int64) == b.view(np.int64)


def _jit_counts():
    from gpar_amd import _lib

    cs = [ctypes.c_int(), ctypes.c_int(), ctypes.c_int()]
    assert not _lib.load().gpar_jit_stats(*[ctypes.byref(c) for c in cs])
    return tuple(c.value for c in cs)


def reached(kind, alpha, zf):
    """(log1p intervals j, w == 1 seen, e >= 2 seen, exponential table entries k mod 64) that the rows zf reach against row 0."""
    js, w_one, e_big, hit = set(), False, False, set()
    for zi in zf:
        s = em.sqdist(zi, zf[0])
        if kind == "eq":
            E = 0.0 + s
        elif kind == "rq":
            u = s * (0.5 / alpha)
            e, j, one = em.log1p_index(u)
            js.add(j)
            w_one, e_big = w_one or (one and u > 0.0), e_big or e >= 2
            E = em.rq_expo(s, alpha)
        else:
            E = em.matern_expo_lin(em.NU2[kind], s)[0]
        if E < 1400.0:   # (a normal, non-zero result: beyond, the table entry hardly matters)
            hit.add(em.exp_index(E) & 63)
    return js, w_one, e_big, hit


def test_arguments_reach_every_table_entry():
    """Coverage is a condition of the tests below: by the emulation's own index arithmetic on the features the device returned, every
    RQ case reaches all 128 intervals of the log1p table, w == 1 and exponents e >= 2 of w; EQ, every Matern kernel and the RQ cases
    together each reach all 64 entries of the exponential table."""
    exp_hit = {}
    for kind, alpha in CASES:
        d = case_data(kind, alpha)
        js, w_one, e_big, hit = reached(kind, d["alpha"], d["zf"])
        exp_hit.setdefault(kind, set()).update(hit)
        if kind == "rq":
            assert js == set(range(128)) and w_one and e_big, (alpha, sorted(set(range(128)) - js), w_one, e_big)
    for kind, hit in exp_hit.items():
        assert hit == set(range(64)), (kind, sorted(set(range(64)) - hit))
    print("[gram_math_gpu] coverage: 128 / 128 log1p intervals, w == 1 and e >= 2 in each of the five RQ cases; 64 / 64 exponential table "
          "entries for each of " + ", ".join(sorted(exp_hit)))


@pytest.mark.parametrize("kind,alpha", CASES, ids=IDS)
def test_values_match_the_emulation_to_the_bit(kind, alpha, monkeypatch):
    """H.gram(ck, z, z[:1]) (about 900 x 1: ragged row tiles of one column) and the lower triangle of H.gram(ck, z[:130], None,
    lower=True), from the interpreter (GPAR_GRAM_JIT_MIN_ENTRIES=-1) and from the generated kernel (=0): every entry has the bits of
    em.entry, the diagonal and every coincident pair is exactly coef, everything is finite and >= 0 - and the same device values meet
    the value budget (module docstring) against mpmath.  No sub-case is relaxed."""
    import torch

    from gpar_amd import hip as H

    d = case_data(kind, alpha)
    ck, z = d["ck"], d["z"]
    n = z.shape[0]
    il = np.tril_indices(N_LOWER)
    for route, setting in (("interpreter", "-1"), ("generated", "0")):
        monkeypatch.setenv("GPAR_GRAM_JIT_MIN_ENTRIES", setting)
        before = _jit_counts()
        col = H.gram(ck, z, z[:1]).cpu().numpy()[:, 0]
        low = H.gram(ck, z[:N_LOWER], None, lower=True, out=torch.zeros(N_LOWER, N_LOWER, dtype=torch.float64, device=z.device)).cpu().numpy()
        after = _jit_counts()
        assert after[1] == before[1], "a generated kernel failed to compile"
        if route == "generated":
            assert after[2] >= 1
        assert np.isfinite(col).all() and np.isfinite(low).all() and (col >= 0.0).all() and (low >= 0.0).all()
        assert (np.diag(low) == d["coef"]).all() and col[0] == col[1] == d["coef"] and low[3, 2] == d["coef"]
        same_col, same_low = _same_bits(col, d["col"]), _same_bits(low[il], d["low"])
        with mp.workprec(PREC):
            worst = max(float(abs(mp.mpf(float(g)) - r)) / b for g, r, b in zip(col, d["ref"], d["budget"]))
        print(f"[gram_math_gpu] values {kind} alpha={alpha} {route}: {n + il[0].size} entries compared, {int(same_col.sum() + same_low.sum())} "
              f"bit-identical to the emulation; worst error / value budget against mpmath = {worst:.3g}")
        problems = []   # (both properties are evaluated before either fails the test)
        if not same_col.all():
            problems.append(("bits differ from the emulation", [(i, d["zf"][i], col[i], d["col"][i]) for i in np.nonzero(~same_col)[0][:5]]))
        if not same_low.all():
            problems.append(("bits of the lower triangle differ from the emulation", int((~same_low).sum())))
        if not worst <= 1.0:
            problems.append(("value budget against mpmath exceeded", worst))
        assert not problems, (route, problems)
        if kind == "eq":   # the relative bound of the existing whole-range test, on these values too
            with mp.workprec(PREC):
                rel = max(float(abs(mp.mpf(float(g)) - r) / r) for g, r in zip(col, d["ref"]) if r > mp.mpf(2) ** -1000)
            assert rel < em.EXPH_REL, rel


@pytest.mark.parametrize("kind,alpha", CASES, ids=IDS)
def test_per_entry_derivative_against_mpmath(kind, alpha, monkeypatch):
    """With z2 a single row and W a column of ones, H.gram_input_grad(..., GRAD_RECT) is d k / d z_i = 2 (z_i - z_0) k'(s_i) entry by
    entry: against mpmath, from the interpreter's libm forms (GPAR_GRAD_JIT_MIN_ENTRIES=-1) and from the generated kernel's table
    forms (=0: gram_exp8, gram_matern_grad8, the RQ form).  Budget: the derivative budget of the module docstring.  At coincident
    rows the result is exactly 0; so it is for nu = 1/2 where d^2 underflows to 0 (d = 1e-170): the guarded divisor treats such a
    pair as coincident, where the true derivative tends to -sign(d) coef."""
    import torch

    from gpar_amd import hip as H

    d = case_data(kind, alpha)
    ck, z, zf, coef = d["ck"], d["z"], d["zf"], d["coef"]
    W = torch.ones(z.shape[0], 1, dtype=torch.float64, device=z.device)
    with mp.workprec(PREC):
        ref, budget = [], []
        for zi in zf:
            dz = zi - zf[0]
            s = em.sqdist(zi, zf[0])
            X, bx = exp_part(kind, d["alpha"], s)
            if s == 0.0 and kind == "matern12":
                ref.append(mp.mpf(0))
                budget.append(0.0)
                continue
            _, F = algebraic_parts(kind, d["alpha"], s)
            r = 2 * mp.mpf(dz) * coef * F * X
            ref.append(r)
            budget.append(abs(2.0 * dz) * coef * abs(float(F)) * bx + 4.0 * em.EPS * abs(float(r)) + abs(2.0 * dz) * 2.0 ** -1074)
        for route, setting in (("libm forms", "-1"), ("generated", "0")):
            monkeypatch.setenv("GPAR_GRAD_JIT_MIN_ENTRIES", setting)
            before = _jit_counts()
            got = H.gram_input_grad(ck, z, z[:1], W, H.GRAD_RECT).cpu().numpy()[:, 0]
            assert _jit_counts()[1] == before[1], "a generated kernel failed to compile"
            assert np.isfinite(got).all()
            assert got[0] == 0.0 and got[1] == 0.0
            if kind == "matern12":
                assert zf[5] != 0.0 and got[5] == 0.0   # d = 1e-170: treated as coincident
            worst, where = 0.0, None
            for i, (g, r, b) in enumerate(zip(got, ref, budget)):
                err = float(abs(mp.mpf(float(g)) - r))
                ratio = err / b if b > 0.0 else (0.0 if err == 0.0 else math.inf)
                if ratio > worst:
                    worst, where = ratio, (i, zf[i], float(g), float(r))
            print(f"[gram_math_gpu] derivative {kind} alpha={alpha} {route}: {len(ref)} entries, worst error / budget = {worst:.3g} at {where}")
            assert worst <= 1.0, (route, worst, where)


@pytest.mark.parametrize("alpha", ALPHAS, ids=[f"{a:g}" for a in ALPHAS])
def test_rq_alpha_and_scale_gradients_per_decade(alpha, monkeypatch):
    """The parameter-gradient pass in rectangular mode (H.gram_grad_cross, GRAD_RECT) against a single row, weights 1, one launch per
    decade of u = s / 2 alpha from 1e-8 to 1e8 (48 rows each), turned into gradients by HipEngine._grads_from_moments, against
    mpmath sums; both routes.
      alpha gradient  sum_i coef k_i g(u_i), g = u / (1 + u) - log1p(u).  Tolerance: sum_i |w_i| coef * (log1p budget + one rounding
                      of u / (1 + u)) - absolute by design: this is the test that decides whether the cancellation in the generated
                      kernel's `tq / base - lg` (relative error of g 3.6e-2 at u = 1e-8, CPU emulation) is acceptable.  It is: the
                      term's ABSOLUTE error is the log1p budget, 3.7e-18 per unit weight, and the series -tq^2 / 2 + ... is not needed.
      scale gradient  sum_i coef k_i (2 alpha / l) u_i / (1 + u_i) - the alpha form's first term times 2 alpha / l, so the same per-entry
                      budget cannot hold for it as stated (one rounding of an entry of size 2 alpha u / l is already larger): it is
                      (2 alpha / l) * sum_i |w_i| * (u_i / (1 + u_i)) * (value budget + 4 eps k_i), the per-entry derivative budget."""
    import torch

    from gpar_amd import hip as H
    from gpar_amd.engine import HipEngine

    d = case_data("rq", alpha)
    ck, coef, a = d["ck"], d["coef"], d["alpha"]
    dev = d["z"].device
    scale = float(ck.kernel.terms[0].factors[0].scales_value()[0])
    per_unit = float(H.featurize(ck, torch.tensor([[1.0]], dtype=torch.float64, device=dev)).cpu()[0, 0])
    rng = random.Random(13)
    worst = {}
    for decade in range(-8, 8):
        us = [10.0 ** rng.uniform(decade, decade + 1) for _ in range(48)]
        x = np.array([0.0] + [math.sqrt(2.0 * a * u) for u in us])[:, None] / per_unit
        z = H.featurize(ck, torch.tensor(x, dtype=torch.float64, device=dev))[:, :1].contiguous()
        zf = [float(v) for v in z.cpu().numpy()[:, 0]]
        W = torch.ones(z.shape[0], 1, dtype=torch.float64, device=dev)
        with mp.workprec(PREC):
            al_ref = sc_ref = mp.mpf(0)
            al_tol = sc_tol = 0.0
            for zi in zf:
                s = mp.mpf(em.sqdist(zi, zf[0]))
                u = s / (2 * mp.mpf(a))
                L = mp.log1p(u)
                k = mp.exp(-mp.mpf(a) * L)
                al_ref += coef * k * (u / (1 + u) - L)
                sc_ref += coef * k * (2 * mp.mpf(a) / mp.mpf(scale)) * u / (1 + u)
                al_tol += coef * rq_alpha_budget(float(u), float(L)) if u > 0 else 0.0
                vb = em.exph_budget(float(k)) + float(k) * 2.0 * a * em.log1p_budget(float(u), float(L))
                sc_tol += (2.0 * a / scale) * coef * float(u / (1 + u)) * (vb + 4.0 * em.EPS * float(k))
        for route, setting in (("libm forms", "-1"), ("generated", "0")):
            monkeypatch.setenv("GPAR_GRAD_JIT_MIN_ENTRIES", setting)
            before = _jit_counts()
            raw = H.gram_grad_cross(ck, z, None, z[:1], None, W, H.GRAD_RECT).cpu().numpy()
            assert _jit_counts()[1] == before[1], "a generated kernel failed to compile"
            g = HipEngine._grads_from_moments(ck, raw, 1.0)["factors"][0][0]
            r_al = float(abs(mp.mpf(float(g["alpha"])) - al_ref)) / al_tol
            r_sc = float(abs(mp.mpf(float(g["scales"][0])) - sc_ref)) / sc_tol
            w = worst.setdefault(route, [0.0, 0.0])
            w[0], w[1] = max(w[0], r_al), max(w[1], r_sc)
            assert r_al <= 1.0 and r_sc <= 1.0, (route, decade, r_al, r_sc, float(g["alpha"]), float(al_ref), float(g["scales"][0]), float(sc_ref))
    for route, w in worst.items():
        print(f"[gram_math_gpu] rq alpha={alpha} {route}: 16 decades x 48 entries, worst error / tolerance: alpha gradient {w[0]:.3g}, scale gradient {w[1]:.3g}")
