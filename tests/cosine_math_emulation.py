"""Plain-numpy model of the cosine factor's written form in gpar_amd/csrc/gram_math.inc (gram_cosh8, gram_cos_grad8):

    phi(s) = cospi(2 s),      d phi / d s = -2 pi sinpi(2 s)       (s: the sum of the scaled differences of one pair)

`cospi` / `sinpi` reduce their argument in units of half periods, which is EXACT in binary floating point: t = 2 s is exact, t mod 2
is exact (fmod), and so is the fold of the remainder onto [-1/2, 1/2] - only then is pi multiplied in, on an argument of size at most
1/2.  The form cos(2 pi s) rounds 2 pi s first, an absolute error of |s| 2^-52 in the phase.  This model makes the same reduction
with float64 operations (each of them exact) and evaluates the folded argument with numpy's float64 cos / sin; `reference` does the
reduction in long double (exact again: a float64 is a long double) and evaluates there.  Where long double is no wider than double
(some platforms) the comparison still checks the reduction, with the tolerance of two float64 evaluations."""
import numpy as np

TWO_PI = float.fromhex("0x1.921fb54442d18p+2")   # GRAM_2PI of gram_math.inc


def _fold(t, one):
    """t (any float type; `one` carries it) -> (r, sign) with cos(pi t) = sign * cos(pi r), sin(pi t) = sign * sin(pi r), |r| <= 1/2.
    Every step is exact: fmod, a subtraction of nearby numbers (Sterbenz) and a negation."""
    r = np.fmod(t, 2 * one)                       # (-2, 2), the sign of t
    r = np.where(r > one, r - 2 * one, r)
    r = np.where(r < -one, r + 2 * one, r)        # [-1, 1]
    sign = np.where(np.abs(r) > one / 2, -one, one)
    r = np.where(r > one / 2, r - one, r)
    r = np.where(r < -one / 2, r + one, r)        # [-1/2, 1/2]:  cos(pi (r +- 1)) = -cos(pi r), sin likewise
    return r, sign


def cospi2(s):
    """cospi(2 s) as the device forms it, in float64."""
    s = np.asarray(s, dtype=np.float64)
    r, sign = _fold(2.0 * s, np.float64(1.0))
    return sign * np.cos(np.pi * r)


def dcospi2(s):
    """-2 pi sinpi(2 s) as the device forms it, in float64."""
    s = np.asarray(s, dtype=np.float64)
    r, sign = _fold(2.0 * s, np.float64(1.0))
    return -TWO_PI * (sign * np.sin(np.pi * r))


def naive(s):
    """cos(2 pi s): the form the device does NOT use."""
    s = np.asarray(s, dtype=np.float64)
    return np.cos(TWO_PI * s)


def reference(s):
    """(cos(2 pi s), -2 pi sin(2 pi s)) in long double, the argument reduced exactly before pi enters."""
    ld = np.longdouble
    s = np.asarray(s, dtype=np.float64).astype(ld)
    r, sign = _fold(ld(2) * s, ld(1))
    pi = ld("3.14159265358979323846264338327950288")
    return sign * np.cos(pi * r), -(2 * pi) * (sign * np.sin(pi * r))
