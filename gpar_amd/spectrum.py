"""Host side of the periodogram initialisation of spectral-mixture layers (`GPARRegressor.periodogram`, `spectral_period="auto"`): the
default frequency grid, the preparation of irregular data with missing values for `gpar_periodogram`, and the choice of Q frequencies
from a periodogram.  Pure numpy: the periodogram itself is the engine's (`HipEngine.periodogram`; there is no CPU fallback)."""
import collections

import numpy as np

__all__ = ["Periodogram", "periodogram_grid", "periodogram_inputs", "spectral_peaks"]

#: What `GPARRegressor.periodogram` returns: the F frequencies (cycles per unit of x) and the p x F generalised Lomb-Scargle powers.
Periodogram = collections.namedtuple("Periodogram", "freq power")


def periodogram_grid(span, n_obs, oversample=5, nyquist=1.0):
    """The default frequency grid for time stamps that cover `span` with `n_obs` observed rows (of the best-observed output): multiples
    k / (oversample span), k = 1 .. F, of the step 1 / (oversample span) - `oversample` points per Rayleigh resolution 1 / span -, up to
    nyquist n_obs / (2 span), the Nyquist frequency the same number of equally spaced rows would have; at least one frequency."""
    span, oversample, nyquist = float(span), float(oversample), float(nyquist)
    if not span > 0 or not np.isfinite(span):
        raise ValueError("the time stamps must span a positive, finite range: a periodogram of one instant has no frequencies")
    if not oversample > 0 or not nyquist > 0:
        raise ValueError("oversample and nyquist must be positive")
    step = 1.0 / (oversample * span)
    top = nyquist * float(n_obs) / (2.0 * span)
    count = max(int(np.floor(top / step * (1.0 + 1e-12))), 1)
    return step * np.arange(1, count + 1, dtype=np.float64)


def periodogram_inputs(x, y, w=None):
    """(t, y, omega) as `gpar_periodogram` takes them, from inputs x (n x 1 or 1-D), outputs y (n x p or 1-D; NaN = missing) and observation
    weights w (the shape of y; default ones): omega = w where y is observed and 0 elsewhere, y = 0 where it is missing.  ValueError: more
    than one input column (a frequency vector in m dimensions needs an m-dimensional grid), fewer than 3 rows, shapes that do not agree,
    negative or non-finite weights, non-finite time stamps."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2 and x.shape[1] != 1:
        raise ValueError(f"the periodogram takes one input column (time); x has {x.shape[1]}: a frequency vector over several inputs needs a "
                         "grid in as many dimensions")
    if x.ndim > 2:
        raise ValueError("x must be n x 1 or 1-D")
    t = x.reshape(-1)
    y = np.asarray(y, dtype=np.float64)
    y = y.reshape(-1, 1) if y.ndim < 2 else y
    if y.ndim != 2 or y.shape[0] != t.size:
        raise ValueError("y must hold one row per time stamp")
    if t.size < 3:
        raise ValueError(f"the periodogram needs at least 3 rows ({t.size} given): a sinusoid with a floating mean fits any three values")
    if not np.all(np.isfinite(t)):
        raise ValueError("the time stamps must be finite")
    w = np.ones_like(y) if w is None else np.asarray(w, dtype=np.float64)
    w = w.reshape(-1, 1) if w.ndim < 2 else w
    if w.shape != y.shape:
        raise ValueError("w must have the shape of y")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("the observation weights must be finite and not negative")
    missing = np.isnan(y)
    return t, np.where(missing, 0.0, y), np.where(missing, 0.0, w)


def spectral_peaks(freq, power, Q, span):
    """Q frequencies at which to start the components of a spectral mixture, strongest first, from one output's periodogram `power` (F
    values) on the ascending grid `freq`; `span` is the range the time stamps cover.  Deterministic:

    * the candidates are the local maxima of `power` with positive power: an interior point that exceeds its left neighbour and is not
      below its right one (of a plateau, its lowest frequency), an end point of the grid that exceeds its one neighbour, the one point of
      a one-point grid;
    * repeatedly the highest remaining candidate is taken - of equal ones the lowest frequency - and every frequency within 1 / span of
      it, the Rayleigh resolution, is struck: one physical line, whose main lobe is that wide, is not picked twice;
    * if fewer than Q candidates exist, the remaining components get the harmonics 2 f1, 3 f1, ... of the strongest pick f1 - the
      ladder a scalar `spectral_period` gives, not copies of one line.

    ValueError: no candidate at all (a periodogram that is zero or constant everywhere)."""
    freq = np.asarray(freq, dtype=np.float64).reshape(-1)
    power = np.asarray(power, dtype=np.float64).reshape(-1)
    Q = int(Q)
    if freq.size != power.size or freq.size == 0:
        raise ValueError("freq and power must hold the same, positive number of values")
    if freq.size > 1 and np.any(np.diff(freq) <= 0):
        raise ValueError("freq must ascend")
    if Q < 1:
        raise ValueError("Q must be at least 1")
    if not float(span) > 0:
        raise ValueError("span must be positive")
    F = freq.size
    if F == 1:
        candidate = power > 0
    else:
        candidate = np.zeros(F, dtype=bool)
        candidate[1:-1] = (power[1:-1] > power[:-2]) & (power[1:-1] >= power[2:])
        candidate[0], candidate[-1] = power[0] > power[1], power[-1] > power[-2]
        candidate &= power > 0
    picks = []
    alive = candidate.copy()
    while len(picks) < Q and alive.any():
        k = int(np.argmax(np.where(alive, power, -np.inf)))   # (argmax returns the first, so the lowest frequency, of equal values)
        picks.append(float(freq[k]))
        alive &= np.abs(freq - freq[k]) > 1.0 / float(span)
    if not picks:
        raise ValueError("the periodogram has no peak: its power is zero or constant over the grid")
    harmonic = 2
    while len(picks) < Q:
        picks.append(picks[0] * harmonic)
        harmonic += 1
    return np.array(picks, dtype=np.float64)
