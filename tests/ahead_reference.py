"""A numpy restatement of rolling-origin forecast scoring that scales to n = 513: what the expanding, the multi-horizon and the
sliding-window entries compute, from the dense matrix K, y and the origin arrays, by ONE factorisation where tests/test_ahead.py's
`brute_force` takes one solve per scored row.  It is a yardstick for the GPU tests at sizes the brute force cannot reach
(tests/test_ahead_large_gpu.py) and is itself held against the brute force at n = 33 and 65 by tests/test_ahead_reference.py.

Everything works in float64, np.longdouble and complex128 (the complex step: no conjugate anywhere, sqrt / log / exp / erf analytic):

  cholesky        hand-written, left-looking, column by column, the update of a column one matrix-vector product; a stack of matrices
                  is factored in lock-step (the window form's blocks);
  expanding form  a = L^-1 y,  e_r = y_r - mean_r = sum_{c = o_r .. r} L_rc a_c,  v_r = var_r = sum_{c = o_r .. r} L_rc^2
                  (the factor of a leading block is the leading block of the factor); K origin arrays with weights share L and a;
  window form     per scored row the block J = lo[r] .. origin[r] - 1 followed by r, K_JJ = G G^T, z = G^-1 y_J,
                  e_r = G_tt z_t, v_r = G_tt^2 (the last row of the block's factor);
  rules           the table in the comment of gpar_amd/csrc/score.h, with e = y - mean, v = var, sd = sqrt v, z = e / sd:
                  log  -1/2 [log 2 pi + log v + e^2 / v],   crps  -sd [z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt pi],   se  -e^2,
                  2 Phi(z) - 1 = erf(z / sqrt 2), phi the standard normal density;
  gradients       `complex_step` of tests/test_ahead.py through these functions: kernel parameters, single noise entries, single
                  entries of K (`w_entries`).

Nothing here is computed from the code under test.
"""
import numpy as np
import scipy.special

from .test_ahead import complex_step  # noqa: F401  (the gradients of the restatement: re-exported for its users)


def _pi(dtype):
    return np.pi if dtype != np.longdouble else np.longdouble(4.0) * np.arctan(np.longdouble(1.0))


def erf(z):
    """erf for real (any precision: the series 2 / sqrt pi exp(-z^2) sum_k 2^k z^(2k+1) / (2k+1)!!, all terms of one sign) and complex
    arrays (scipy's, which is analytic)."""
    z = np.asarray(z)
    if np.iscomplexobj(z):
        return scipy.special.erf(z)
    a = np.minimum(np.abs(z), 7.0)   # (erf(7) = 1 to 1e-22)
    term, total = a.copy(), a.copy()
    for k in range(1, 260):
        term = term * (2.0 * a * a) / (2 * k + 1)
        total = total + term
    return np.sign(z) * np.minimum(2.0 / np.sqrt(_pi(z.dtype)) * np.exp(-a * a) * total, 1.0)


def term(rule, e, v):
    """What one scored entry with error e and variance v adds to the value (score.h's table)."""
    if rule == "se":
        return -(e * e)
    pi = _pi(np.asarray(v).dtype)
    if rule == "log":
        return -0.5 * (np.log(2.0 * pi) + np.log(v) + e * e / v)
    if rule != "crps":
        raise ValueError(rule)
    sd = np.sqrt(v)
    z = e / sd
    two_cdf_minus_one, pdf = erf(z / np.sqrt(np.asarray(2.0, dtype=sd.dtype))), np.exp(-0.5 * z * z) / np.sqrt(2.0 * pi)
    return -sd * (z * two_cdf_minus_one + 2.0 * pdf - 1.0 / np.sqrt(pi))


def cholesky(K):
    """Lower factor of K (... x n x n), K = L L^T WITHOUT conjugates, column by column: column j is K[j:, j] minus the product of the rows
    j.. of the columns so far with row j, over the root of its first entry."""
    K = np.asarray(K)
    n = K.shape[-1]
    L = np.zeros_like(K)
    for j in range(n):
        col = K[..., j:, j] - np.matmul(L[..., j:, :j], L[..., j, :j, None])[..., 0]
        root = np.sqrt(col[..., :1])
        L[..., j:, j] = col / root
        L[..., j, j] = root[..., 0]
    return L


def forward(L, y):
    """L^-1 y (... x n), column by column."""
    a = np.array(y, dtype=L.dtype)
    n = L.shape[-1]
    for k in range(n):
        a[..., k] = a[..., k] / L[..., k, k]
        a[..., k + 1:] = a[..., k + 1:] - L[..., k + 1:, k] * a[..., k, None]
    return a


def factor(K, y):
    """(L, a = L^-1 y): what every expanding-form evaluation on K shares."""
    L = cholesky(K)
    return L, forward(L, np.asarray(y))


def expanding_moments(L, a, y, origin):
    """(e, v, mean, var) of one origin array; NaN moments and e = v = 0 on unscored rows."""
    n = L.shape[0]
    origin = np.asarray(origin)
    cols = np.arange(n)
    inside = (cols[None, :] >= origin[:, None]) & (cols[None, :] <= cols[:, None]) & (origin[:, None] >= 0)
    Lm = np.where(inside, L, 0)
    e, v = Lm @ a, np.sum(Lm * Lm, axis=1)
    scored = origin >= 0
    nan = np.full(n, np.nan, dtype=L.dtype)
    return e, v, np.where(scored, np.asarray(y) - e, nan), np.where(scored, v, nan)


def expanding(K, y, origin, rule="log", fac=None):
    """(value, mean, var) as `brute_force(K, y, origin)` returns them.  `fac`: `factor(K, y)` where several calls share it."""
    L, a = factor(K, y) if fac is None else fac
    e, v, mean, var = expanding_moments(L, a, y, origin)
    scored = np.asarray(origin) >= 0
    return np.sum(term(rule, e[scored], v[scored])), mean, var


def expanding_multi(K, y, origins, weights, rule="log", fac=None):
    """(weighted value, the K values, K x n means, K x n variances) as `multi_brute_force` returns them: one factor, K origin arrays."""
    fac = factor(K, y) if fac is None else fac
    parts = [expanding(K, y, o, rule, fac) for o in origins]
    values = np.array([p[0] for p in parts])
    return np.sum(np.asarray(weights) * values), values, np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts])


def window(K, y, lo, origin, rule="log", rows=None):
    """(value, mean, var) as `window_brute_force` returns them: per scored row the factor of K_JJ, J = lo[r] .. origin[r] - 1 then r, and
    e, v from its last row.  Rows with blocks of one size are factored as one stack.  `rows`: only these rows (the others as unscored)."""
    K, y = np.asarray(K), np.asarray(y)
    n = len(y)
    lo, origin = np.asarray(lo), np.asarray(origin)
    mean, var = np.full(n, np.nan, dtype=K.dtype), np.full(n, np.nan, dtype=K.dtype)
    take = np.flatnonzero(origin >= 0) if rows is None else np.array([r for r in rows if origin[r] >= 0], dtype=int)
    value = 0.0
    for m in np.unique(origin[take] - lo[take]):
        rs = take[origin[take] - lo[take] == m]
        J = np.concatenate([lo[rs, None] + np.arange(m)[None, :], rs[:, None]], axis=1)   # len(rs) x (m + 1)
        G = cholesky(K[J[:, :, None], J[:, None, :]])
        z = forward(G, y[J])
        gtt = G[:, m, m]
        e, v = gtt * z[:, m], gtt * gtt
        mean[rs], var[rs] = y[rs] - e, v
        value = value + np.sum(term(rule, e, v))
    return value, mean, var


def w_entries(value_of_K, K, entries):
    """W_ab = d value / d K_ab with K_ab and K_ba moved together (a != b), 2 d value / d K_aa on the diagonal, at the (a, b) of `entries`,
    by the complex step through `value_of_K` (a function of the complex matrix, or of (matrix, a, b))."""
    out = np.zeros(len(entries))
    for i, (a, b) in enumerate(entries):
        moved = np.asarray(K).astype(complex)
        moved[a, b] += 1e-30j
        if a != b:
            moved[b, a] += 1e-30j
        out[i] = np.imag(value_of_K(moved, a, b)) / 1e-30 * (2.0 if a == b else 1.0)
    return out


def window_check(lo, origin, window_max=64, monotone=True):
    """A numpy twin of the window form's argument check: the first row r that is not well-formed - 0 <= lo[r] <= origin[r] <= r,
    origin[r] - lo[r] <= window_max, and neither lo[r] nor origin[r] below the running maximum over the scored rows before it - or -1.
    `monotone` False drops the running-maximum condition (tests/test_ahead_reference.py: the error cases need it)."""
    top_l = top_o = -1
    for r in range(len(origin)):
        o, l = int(origin[r]), int(lo[r])
        if o == -1:
            continue
        if o < -1 or o > r or l < 0 or l > o or o - l > window_max or (monotone and (l < top_l or o < top_o)):
            return r
        top_l, top_o = max(top_l, l), max(top_o, o)
    return -1


def expanding_check(origins):
    """The first row with an origin outside -1 ... r in any of the arrays, or -1."""
    origins = np.atleast_2d(origins)
    r = np.arange(origins.shape[1])
    bad = np.flatnonzero(((origins < -1) | (origins > r[None, :])).any(axis=0))
    return int(bad[0]) if bad.size else -1
