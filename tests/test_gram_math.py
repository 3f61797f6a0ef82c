"""Whole-range accuracy of the hand-written elementary functions of gpar_amd/csrc/gram_math.inc, on the CPU.

tests/gram_math_emulation.py restates every device function operation by operation (tests/test_gram_math_gpu.py asserts that the
MI355X agrees with it to the last bit), so the dense sweeps against mpmath (256 bits) run here and cost no GPU time.  Every test
prints its worst measured error / bound ratio (pytest -s shows it); every figure quoted in a docstring below is either derived
there or was measured with this CPU emulation."""
import importlib.util
import math
import os
import random

import mpmath as mp
import pytest

from . import gram_math_emulation as em

PREC = 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rounded(x):
    """The double nearest to the mpmath number x."""
    return float(x)


def test_tables_are_correctly_rounded():
    """All 320 entries of GRAM_TAB: 2^(j/64); v_j = 1 / c_j with c_j = (1 + (j + 1/2) / 128) / 2; log(2 / v_j) of the ROUNDED v_j -
    each the correctly rounded double.  tools/gen_gram_tables.py reproduces the literals."""
    with mp.workprec(PREC):
        tab = em.load_table()
        assert len(tab) == 320
        wrong = []
        for j in range(64):
            if tab[j] != _rounded(mp.mpf(2) ** (mp.mpf(j) / 64)):
                wrong.append(("exp", j))
        for j in range(128):
            c = (1 + (mp.mpf(j) + mp.mpf(1) / 2) / 128) / 2
            v, lv = tab[64 + 2 * j], tab[64 + 2 * j + 1]
            if v != _rounded(1 / c):
                wrong.append(("v", j))
            if lv != _rounded(mp.log(2 / mp.mpf(v))):
                wrong.append(("log", j))
        assert not wrong, wrong
    before = mp.mp.prec
    try:   # (the generator sets mpmath's working precision when it is imported: put it back)
        spec = importlib.util.spec_from_file_location("_gen_gram_tables", os.path.join(ROOT, "tools", "gen_gram_tables.py"))
        gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gen)
        vals = gen.table()
    finally:
        mp.mp.prec = before
    assert vals == tab
    print("[gram_math] tables: 320 / 320 entries correctly rounded, generator reproduces them")


def test_log1p_pos_against_mpmath():
    """gram_log1p_pos against mp.log1p at tests/gram_math_emulation.py::log1p_arguments.  With eps = 2^-53, L = log1p(u), w = fl(1 + u)
    = m 2^e, r = m v_j - 1 (|r| <= 1 / 257, largest at j = 0), the errors of  lg = fma(e - 1, LN2HI, T_j) + (poly + small):

      source                                                   absolute size          u >= 2^-7: / (eps L)      u < 2^-7: / 2^-62
      final sum, one rounding                                  eps |lg|               1                        2   (|lg| < 2^-7)
      fma(e - 1, LN2HI, T_j), one rounding (|.| <= L + 2^-8)   eps (L + 2^-8)         1.502                    0   (e = 1: T_0 itself)
      T_j = log(2 / v_j) rounded to a double                   eps T_j <= eps (L + 2^-8)   1.502               1   (T_0 < 2^-8)
      poly + small, one rounding (|.| <= 2^-8)                 eps 2^-8               0.502                    1   (half an ulp below 2^-8)
      poly = fma(r r, q, r), one rounding                      eps 2^-8               0.502                    1
      r = fma(m, v_j, -1), one rounding (|r| < 2^-8)           eps 2^-9               0.251                    1
      roundings inside q and r r (they scale r^2 / 2)          3 eps 2^-17            0.002                    0.03
      degree-6 truncation, r^7 / 7 / (1 - |r|)                 1.94e-18               2.25                     8.95
      c / w taken as c v_j 2^-e (|c| <= eps w, v_j m = 1 + r)  eps 2^-8               0.502                    2
      LN2LO's own rounding, the rounding of `small`            < 1e-25                0                        0
                                                                                      ---------                -----
                                                                                      8.02 -> 8.1              16.98 -> 17

    (L >= log1p(2^-7) = 0.00778 turns eps 2^-8 into 0.502 eps L.)  Hence: relative error <= 8.1 * 2^-53 = 9.0e-16 for u >= 2^-7,
    absolute error <= 17 * 2^-62 = 3.7e-18 below - inside the 1e-15 / 1e-17 that a Gram entry's rtol 1e-13 at an exponent of 100 can
    afford (alpha L delta).  Measured with the CPU emulation over these 4433 arguments: 1.93 * 2^-53 relative (at u = 2.39) and
    12.1 * 2^-62 = 2.63e-18 absolute (at u = 4.9e-8): the truncation term dominates below 2^-7, as derived.  u == 0 gives exactly 0.
    Below u ~ 1e-17 the result is the correction c / w alone plus T_0 + poly(r_0), which is 1.7e-18 and not 0: the RELATIVE error
    is unbounded there (log1p_pos(5e-324) = 1.7e-18), the absolute bound is what holds, and the result is never negative on this sweep."""
    with mp.workprec(PREC):
        args = em.log1p_arguments()
        assert em.log1p_pos(0.0) == 0.0 and math.copysign(1.0, em.log1p_pos(0.0)) == 1.0
        worst_rel = worst_abs = 0.0
        hit = set()
        for u in args:
            got = em.log1p_pos(u)
            assert math.isfinite(got) and got >= 0.0, (u, got)
            L = mp.log1p(mp.mpf(u))
            err = float(abs(mp.mpf(got) - L))
            ratio = err / em.log1p_budget(u, float(L)) if u > 0.0 else err
            if u >= 2.0 ** -7:
                worst_rel = max(worst_rel, ratio)
            else:
                worst_abs = max(worst_abs, ratio)
            assert ratio <= 1.0, (u, got, float(L), ratio)
            hit.add(em.log1p_index(u)[1])
        assert hit == set(range(128))
    assert em.LOG1P_REL <= 1e-15 and em.LOG1P_ABS <= 1e-17   # the cap: alpha L delta must stay inside rtol 1e-13 at exponents of 100
    print(f"[gram_math] log1p_pos: {len(args)} arguments, worst error / bound: relative part {worst_rel:.3g} (bound {em.LOG1P_REL:.3g}), "
          f"absolute part {worst_abs:.3g} (bound {em.LOG1P_ABS:.3g})")


def _exph_arguments():
    rng = random.Random(1)
    args = [1600.0 * i / 8000 for i in range(8001)]
    args += [rng.uniform(0.0, 80.0) for _ in range(2000)]
    args += [rng.uniform(1416.0, 1492.0) for _ in range(2500)]            # results in the denormal range, and the step to 0
    args += [2.0 * 708.0, 2.0 * 708.4, 2.0 * 745.1, 2.0 * 745.2, 2.0 * 746.0, 5e-324, 1e-300, 1e-17]
    return args


def test_exph_against_mpmath():
    """gram_exph8 against mp.exp(-E / 2) for E in [0, 1600]: every table entry (k mod 64), the denormal results and the step to 0.
    The bounds are the ones tests/test_hip_primitives.py::test_gram_exponential_over_its_whole_range asserts on the device: absolute
    error 4.5e-16 per unit coefficient, relative error 1e-13 above 2^-1000."""
    with mp.workprec(PREC):
        args = _exph_arguments()
        worst_abs = worst_rel = 0.0
        hit = set()
        denormal = 0
        for E in args:
            got = em.exph(E)
            assert math.isfinite(got) and got >= 0.0, (E, got)
            want = mp.exp(-mp.mpf(E) / 2)
            err = abs(mp.mpf(got) - want)
            worst_abs = max(worst_abs, float(err) / em.EXPH_ABS)
            if want > mp.mpf(2) ** -1000:
                worst_rel = max(worst_rel, float(err / want) / em.EXPH_REL)
            denormal += 0.0 < got < 2.0 ** -1022
            hit.add(em.exp_index(E) & 63)
        assert em.exph(0.0) == 1.0
        assert hit == set(range(64)) and denormal > 500
        assert worst_abs <= 1.0 and worst_rel <= 1.0, (worst_abs, worst_rel)
    print(f"[gram_math] exph: {len(args)} arguments ({denormal} denormal results), worst error / bound: absolute {worst_abs:.3g}, relative {worst_rel:.3g}")


def matern_closed_forms(nu2, s):
    """(k(s), dk / ds) of the Matern kernel of smoothness nu2 / 2 at mpmath's working precision; dk / ds := 0 at s = 0 for nu = 1/2."""
    s = mp.mpf(s)
    r = mp.sqrt(s)
    if nu2 == 1:
        return mp.exp(-r), (-mp.exp(-r) / (2 * r) if r != 0 else mp.mpf(0))
    c = mp.sqrt(nu2)
    if nu2 == 3:
        return (1 + c * r) * mp.exp(-c * r), -mp.mpf(3) / 2 * mp.exp(-c * r)
    return (1 + c * r + mp.mpf(5) / 3 * s) * mp.exp(-c * r), -mp.mpf(5) / 6 * (1 + c * r) * mp.exp(-c * r)


def matern_budget(factor, expv, cr):
    """Absolute error allowed to  factor * exp(-c r)  where `factor` is the algebraic part (polynomial, -3/2, 1 / 2r ...), expv the true
    exponential: the exponential's own budget times |factor|, plus (4 + 2 c r) eps relative - at most four roundings in forming the
    factor and the product, and the two relative roundings of c r = fl(C fl(sqrt(s))) (C itself is rounded too, within the same
    2 eps: 0.5 each for C and the product, 0.5 for the square root, rounded up), which move exp(-c r) by c r times as much."""
    factor, expv = abs(float(factor)), float(expv)
    return factor * em.exph_budget(expv) + (4.0 + 2.0 * cr) * em.EPS * factor * expv


def _matern_arguments(nu2):
    rng = random.Random(2)
    c = em.MATERN_C[nu2]
    s = [0.0, 5e-324, 1e-320, 1e-300]
    s += [10.0 ** rng.uniform(-20.0, 6.0) for _ in range(1500)]
    s += [(cr / c) ** 2 for cr in (700.0, 708.0, 709.0, 730.0, 744.0, 745.0, 745.13, 745.2, 746.0, 800.0, 1e3, 1e7)]
    return s


@pytest.mark.parametrize("nu2", [1, 3, 5])
def test_matern_forms_against_closed_forms(nu2):
    """gram_maternh8 followed by gram_exph8 (the value path) and gram_matern_grad8 (value and dk / ds of the generated gradient
    kernels) against the closed forms, from s = 0 through denormal s to c r beyond the exponential's underflow (745.13).  s = 0 gives
    exactly phi = 1 and dk = 0 (nu = 1/2: the guarded divisor), -1.5, -5/6; nothing is ever non-finite.  Budget: matern_budget."""
    with mp.workprec(PREC):
        expo, lin = em.matern_expo_lin(nu2, 0.0)
        assert em.fma(lin, em.exph(expo), 0.0) == 1.0
        phi0, dk0 = em.matern_grad(nu2, 0.0)
        assert phi0 == 1.0 and dk0 == {1: 0.0, 3: -1.5, 5: -0.5 * em.GRAM_5_3}[nu2]
        assert abs(-0.5 * em.GRAM_5_3 + 5.0 / 6.0) < 2e-16
        worst = 0.0
        for s in _matern_arguments(nu2):
            expo, lin = em.matern_expo_lin(nu2, s)
            val = em.fma(lin, em.exph(expo), 0.0)
            phi, dk = em.matern_grad(nu2, s)
            assert math.isfinite(val) and math.isfinite(phi) and math.isfinite(dk), (s, val, phi, dk)
            assert val >= 0.0 and phi >= 0.0 and dk <= 0.0, (s, val, phi, dk)
            if s == 0.0:
                continue
            k_ref, dk_ref = matern_closed_forms(nu2, s)
            c = mp.sqrt(nu2)
            cr = float(c * mp.sqrt(mp.mpf(s)))
            expv = mp.exp(-c * mp.sqrt(mp.mpf(s)))
            for got, ref in ((val, k_ref), (phi, k_ref), (dk, dk_ref)):
                budget = matern_budget(ref / expv, expv, cr)
                ratio = float(abs(mp.mpf(got) - ref)) / budget
                worst = max(worst, ratio)
                assert ratio <= 1.0, (nu2, s, got, float(ref), ratio)
    print(f"[gram_math] matern nu2={nu2}: worst error / budget = {worst:.3g}")


def rq_alpha_budget(u, L):
    """Absolute error allowed to g(u) = u / (1 + u) - log1p(u): the log1p budget plus one rounding of u / (1 + u)."""
    return em.log1p_budget(u, L) + em.EPS * u / (1.0 + u)


def test_rq_alpha_form_against_mpmath():
    """g(u) = u / (1 + u) - log1p_pos(u), the per-entry factor of the RQ alpha moment as the generated gradient kernel forms it
    (tq * (1 / base) - lg), over the arguments of the log1p sweep.  g ~ -u^2 / 2 for small u, so the ABSOLUTE error of log1p_pos
    (3.7e-18 by the analysis above) becomes a large RELATIVE error of g: measured with the CPU emulation, 2.6e-10 at u = 1e-4, 3.5e-6
    at u = 1e-6, 3.6e-2 at u = 1e-8 (absolute: 1.3e-18, 1.8e-18, 1.8e-18).  What is asserted is the absolute bound - the log1p budget
    plus one rounding of u / (1 + u) - which is what a weighted sum over entries needs (tests/test_gram_math_gpu.py sums it)."""
    with mp.workprec(PREC):
        worst = 0.0
        for u in em.log1p_arguments():
            got = em.rq_alpha_form(u)
            assert math.isfinite(got)
            x = mp.mpf(u)
            L = mp.log1p(x)
            want = x / (1 + x) - L
            ratio = float(abs(mp.mpf(got) - want)) / rq_alpha_budget(u, float(L)) if u > 0.0 else float(abs(mp.mpf(got) - want))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (u, got, float(want), ratio)
        loss = {}
        for u in (1e-4, 1e-6, 1e-8):
            x = mp.mpf(u)
            want = x / (1 + x) - mp.log1p(x)
            loss[u] = float(abs((mp.mpf(em.rq_alpha_form(u)) - want) / want))
    print(f"[gram_math] rq alpha form: worst error / budget = {worst:.3g}; relative loss at 1e-4, 1e-6, 1e-8: "
          + ", ".join(f"{loss[u]:.2g}" for u in (1e-4, 1e-6, 1e-8)))
