"""Plain-Python model of gpar_amd/csrc/gram_math.inc: one function per device function, the same IEEE operations in the same order.

The device functions use only fused multiply-adds, sums, products, `rint`, `frexp`, `ldexp`, the correctly rounded square root, a
correctly rounded division and table loads, with contraction switched off - so this model is meant to agree with the GPU to the
last bit (tests/test_gram_math_gpu.py asserts that), and the dense accuracy sweeps can run on the CPU (tests/test_gram_math.py).

  fma(a, b, c)   the exact rational a b + c rounded once (fractions.Fraction -> float is correctly rounded in CPython)
  rint           round half to even (Python's round())
  math.frexp     stands for frexp_mant / frexp_exp,   math.ldexp for v_ldexp (rounds to nearest even into the denormals)
  math.sqrt      the correctly rounded square root

The tables are parsed out of the source text; the scalar constants are written out again by hand below."""
import math
import os
import re
import struct
from fractions import Fraction

INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpar_amd", "csrc", "gram_math.inc")

GRAM_EXP_TAB = 64
NR32L2 = float.fromhex("-0x1.71547652b82fep+5")   # -32 / ln2
L32 = float.fromhex("0x1.62e42fefa39efp-6")       # ln2 / 32
LN2HI = float.fromhex("0x1.62e42fefa2000p-1")
LN2LO = float.fromhex("0x1.9ef35793c7673p-41")
GRAM_SQRT3 = float.fromhex("0x1.bb67ae8584caap+0")
GRAM_SQRT5 = float.fromhex("0x1.1e3779b97f4a8p+1")
GRAM_5_3 = float.fromhex("0x1.aaaaaaaaaaaabp+0")
MATERN_C = {1: 1.0, 3: GRAM_SQRT3, 5: GRAM_SQRT5}


def load_table(path=INC):
    """The 320 doubles of GRAM_TAB, from the hexadecimal literals of the source."""
    src = open(path).read()
    body = src[src.index("GRAM_TAB[GRAM_TAB_DOUBLES] = {"):]
    body = body[body.index("{") + 1: body.index("}")]
    lits = re.findall(r"0x1\.[0-9a-f]{13}p[+-]\d+", body)
    assert len(lits) == 320, len(lits)
    return [float.fromhex(t) for t in lits]


TAB = load_table()


def fma(a, b, c):
    """a b + c with one rounding."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        return a * b + c   # (the product is exact here: this gives the zero its IEEE sign)
    try:
        return float(exact)
    except OverflowError:
        return math.inf if exact > 0 else -math.inf


def rint(x):
    return float(round(x)) if math.isfinite(x) else x


def to_int(x):
    """double -> int32 as the device converts: towards zero, saturating, NaN to 0."""
    if x != x:
        return 0
    return int(max(-2.0 ** 31, min(2.0 ** 31 - 1, x)))


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def exp_index(E):
    """k = 64 e + j of gram_exph8's reduction for the argument E."""
    return to_int(rint(E * NR32L2))


def exph(E, tab=TAB):
    """gram_exph8: exp(-E / 2), E >= 0."""
    k = rint(E * NR32L2)
    ki = to_int(k)
    tj = tab[ki & (GRAM_EXP_TAB - 1)]
    r = fma(k, L32, E)
    p = fma(-1.0 / 3840.0, r, 1.0 / 384.0)
    p = fma(p, r, -1.0 / 48.0)
    p = fma(p, r, 0.125)
    p = fma(p, r, -0.5)
    p = fma(p, r, 1.0)
    return math.ldexp(p * tj, ki >> 6)


def exp_neg(x, tab=TAB):
    """gram_exp8: exp(x), x <= 0."""
    return exph(x * -2.0, tab)


def log1p_index(u):
    """(e, j, w == 1) of gram_log1p_pos's reduction: w = fl(1 + u) = m 2^e, j the top seven mantissa bits of m."""
    w = 1.0 + u
    m, e = math.frexp(w)
    return e, (bits(m) >> 45) & 127, w == 1.0


def log1p_pos(u, tab=TAB, shift=45, third=1.0 / 3.0):
    """gram_log1p_pos: log1p(u), u >= 0.  (`shift` and `third` exist so that a test can show that it notices a wrong one.)"""
    w = 1.0 + u
    c = u - (w - 1.0)
    m, e = math.frexp(w)
    j = (bits(m) >> shift) & 127
    v, lv = tab[GRAM_EXP_TAB + 2 * j], tab[GRAM_EXP_TAB + 2 * j + 1]
    r = fma(m, v, -1.0)
    q = fma(-1.0 / 6.0, r, 0.2)
    q = fma(q, r, -0.25)
    q = fma(q, r, third)
    q = fma(q, r, -0.5)
    poly = fma(r * r, q, r)
    ed = float(e - 1)
    small = fma(ed, LN2LO, math.ldexp(c * v, -e))
    lg = fma(ed, LN2HI, lv) + (poly + small)
    return 0.0 if u == 0.0 else lg


def rq_expo(s, alpha, expo=0.0, tab=TAB):
    """gram_rqh8: the doubled exponent E += 2 alpha log1p(s / 2 alpha)."""
    h2a, a2 = 0.5 / alpha, 2.0 * alpha
    return fma(a2, log1p_pos(s * h2a, tab), expo)


def matern_expo_lin(nu2, s, expo=0.0, lin=1.0):
    """gram_maternh8<NU2>: (E + 2 c r, lin * polynomial)."""
    cr = MATERN_C[nu2] * math.sqrt(s)
    expo = fma(2.0, cr, expo)
    if nu2 == 3:
        lin = lin * (1.0 + cr)
    if nu2 == 5:
        lin = lin * fma(GRAM_5_3, s, 1.0 + cr)
    return expo, lin


def matern_grad(nu2, s, tab=TAB, guard=True):
    """gram_matern_grad8<NU2>: (phi, dk) = (k(s), dk / ds).  (`guard=False` drops the r == 0 selection of nu = 1/2: tests only.)"""
    cr = MATERN_C[nu2] * math.sqrt(s)
    phi = exph(2.0 * cr, tab)
    if nu2 == 1:
        if guard:
            dk = 0.0 if cr == 0.0 else -0.5 * phi / (1.0 if cr == 0.0 else cr)
        else:
            dk = -0.5 * phi / cr if cr != 0.0 else math.copysign(math.inf, -1.0) * phi
    elif nu2 == 3:
        dk = -1.5 * phi
        phi = phi * (1.0 + cr)
    else:
        dk = (-0.5 * GRAM_5_3) * (1.0 + cr) * phi
        phi = phi * fma(GRAM_5_3, s, 1.0 + cr)
    return phi, dk


KINDS = ("eq", "rq", "matern12", "matern32", "matern52")
NU2 = {"matern12": 1, "matern32": 3, "matern52": 5}


def sqdist(za, zb):
    """gram_accum over one feature dim: s = fma(d, d, 0), d = za - zb."""
    d = za - zb
    return fma(d, d, 0.0)


def entry(kind, coef, alpha, za, zb, tab=TAB, third=1.0 / 3.0):
    """One Gram entry of a one-term, one-factor kernel over one feature dim, composed as gram_kernel (gram.h) does: the exponent
    into `expo` starting from 0, lin = coef * polynomial, total = fma(lin, exph(expo), 0)."""
    s = sqdist(za, zb)
    expo, lin = 0.0, coef
    if kind == "eq":
        expo = expo + s
    elif kind == "rq":
        h2a, a2 = 0.5 / alpha, 2.0 * alpha
        expo = fma(a2, log1p_pos(s * h2a, tab, third=third), expo)
    else:
        expo, lin = matern_expo_lin(NU2[kind], s, expo, lin)
    return fma(lin, exph(expo, tab), 0.0)


def rq_alpha_form(u, tab=TAB):
    """The RQ alpha moment's per-entry factor as grad_jit.h's generated text forms it: u / (1 + u) - log1p(u) = tq * (1 / base) - lg."""
    base = 1.0 + u
    ib = 1.0 / base
    return u * ib - log1p_pos(u, tab)


# ---- error budgets (derived in tests/test_gram_math.py::test_log1p_pos_against_mpmath) ------------------------------------------------
EPS = 2.0 ** -53
LOG1P_REL = 8.1 * EPS          # relative, u >= 2^-7
LOG1P_ABS = 17.0 * 2.0 ** -62  # absolute, u < 2^-7
EXPH_ABS = 4.5e-16             # gram_exph8, absolute (per unit coefficient) ...
EXPH_REL = 1e-13               # ... and relative above 2^-1000


def log1p_budget(u, L):
    """Absolute error allowed to gram_log1p_pos at the argument u, L = log1p(u)."""
    return LOG1P_REL * L if u >= 2.0 ** -7 else LOG1P_ABS


def exph_budget(val):
    """Absolute error allowed to gram_exph8 where the true value is val (per unit coefficient)."""
    return min(EXPH_ABS, EXPH_REL * val) if val > 2.0 ** -1000 else EXPH_ABS


def log1p_arguments(seed=0):
    """The arguments u >= 0 at which gram_log1p_pos is swept: zero and the denormals, the edge where 1 + u rounds to 1, both sides
    of every table interval at several exponents of w = fl(1 + u), the powers of two, a log-uniform fill, the far end."""
    import random

    out = [0.0, 5e-324, 1e-300, 2.0 ** -54, math.nextafter(2.0 ** -53, 0.0), 2.0 ** -53, math.nextafter(2.0 ** -53, 1.0), 2.0 ** -52]
    for e in (0, 1, 10, 52, 100, 1000):
        for j in range(128):
            w0 = math.ldexp(1.0 + j / 128.0, e)
            for w in (math.nextafter(w0, 0.0), w0, math.nextafter(w0, math.inf)):
                if w < 1.0:
                    continue
                out.append(w - 1.0 if w < 2.0 ** 53 else w)   # (w - 1 is exact below 2^53; above 2^54, fl(1 + w) = w)
    for k in range(1, 61):
        out += [2.0 ** k - 1.0, 2.0 ** k]
    rng = random.Random(seed)
    out += [10.0 ** rng.uniform(-8.0, 8.0) for _ in range(2000)]
    out += [1e100, 1e300]
    return out
