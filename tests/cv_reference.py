"""A numpy restatement of the held-out scoring family that shares the dense-objective chain: leave-one-out under the three scoring
rules, blocked and purged blocked cross-validation - what gpar_loo_dense*[_score], gpar_cv_dense* and gpar_cv_gap_dense* compute, from
the symmetric matrix S = K + diag(noise) + jitter I, y and the index arrays.  It is the yardstick of tests/test_cv_large_gpu.py and is
itself held to account by tests/test_cv_reference.py: against deletion (`*_brute`), and its W against the complex step of the deletion's
value.

Everything works in float64, np.longdouble and complex128 (the complex step: no conjugate anywhere, sqrt / log / exp / erf analytic);
the Cholesky factor, the forward substitution and the rules' terms are those of tests/ahead_reference.py.

  one factorisation   S = L L^T, P = S^-1 = L^-T L^-1, alpha = P y, log det S = 2 sum log L_ii  (`factor`; several forms may share it);
  loo                 d = diag P, e = alpha / d, v = 1 / d:  mean = y - e, var = v, value = sum term(rule, e, v) (score.h's table), and with
                      the rule's q = -dterm/de, s = -dterm/dv:  b = q v, c = q e v + s v^2, u = P b,
                      W = alpha u^T + u alpha^T - 2 P diag(c) P            (the comment above loo_row_write in gpar_hip.hip);
  blocked             per fold F: D = P_FF = G G^T, b_F = D^-1 alpha_F, mean = y_F - b_F, var = diag D^-1,
                      value = sum_F [sum log G_ii - 1/2 alpha_F^T b_F] - n/2 log 2 pi, C = blockdiag 1/2 (D^-1 + b_F b_F^T), u = P b,
                      W = alpha u^T + u alpha^T - 2 P C P                  (the comment above cv_chol_lower);
  purged              per fold F inside its block H, G = H \\ F: P_HH ordered (G, F) = L L^T, N = L^-1, w = N alpha_H, e = N^T w,
                      mean = y_F - e_F, var = diag(N_F^T N_F) on F, term = sum_F log L_ii - 1/2 |w_F|^2, b_H = N_F^T w_F, g = e - b_H,
                      C_H = 1/2 (N_F^T N_F + e e^T - g g^T), b = sum E_H b_H, C = sum E_H C_H E_H^T, W as above   (cv_gap.h);
  *_brute             the definitions: per fold delete the rows of H (of F; the row), condition on the rest, score F - a solve each;
  gradients           `complex_step` (tests/test_ahead.py) through the one-factorisation forms, dL/dtheta = 1/2 sum W o dK/dtheta.

Nothing here is computed from the code under test.
"""
import numpy as np

from .ahead_reference import _pi, cholesky, erf, forward, term
from .test_ahead import complex_step  # noqa: F401  (the gradients of the restatement: re-exported for its users)


def backward(L, a):
    """L^-T a (... x n), row by row from the last."""
    a = np.array(a, dtype=L.dtype)
    for k in range(L.shape[-1] - 1, -1, -1):
        a[..., k] = a[..., k] / L[k, k]
        a[..., :k] = a[..., :k] - L[k, :k] * a[..., k, None]
    return a


def solve(A, B):
    """A^-1 B for a symmetric A (B: n or n x k), by the conjugate-free factor and two substitutions."""
    L = cholesky(A)
    B = np.asarray(B)
    return backward(L, forward(L, B.T.astype(L.dtype))).T


def inverse_factor(L):
    """N = L^-1 (the rows of the forward substitution on the identity are its columns)."""
    return forward(L, np.eye(L.shape[-1], dtype=L.dtype)).T


def factor(S, y):
    """What every form on S shares: L, P = S^-1, alpha = P y and log det S."""
    S = np.asarray(S)
    L = cholesky(S)
    N = inverse_factor(L)
    P = N.T @ N
    return dict(P=P, alpha=P @ np.asarray(y).astype(S.dtype), logdet=2.0 * np.sum(np.log(np.diagonal(L))))


def sensitivities(rule, e, v):
    """(q, s) = (-dterm/de, -dterm/dv) of score.h's table."""
    if rule == "log":
        q = e / v
        return q, 0.5 * (1.0 / v - q * q)
    if rule == "se":
        return 2.0 * e, 0.0 * e
    if rule != "crps":
        raise ValueError(rule)
    pi = _pi(np.asarray(v).dtype)
    sd = np.sqrt(v)
    z = e / sd
    two_pdf = 2.0 * np.exp(-0.5 * z * z) / np.sqrt(2.0 * pi)
    return erf(z / np.sqrt(np.asarray(2.0, dtype=sd.dtype))), (two_pdf - 1.0 / np.sqrt(pi)) / (2.0 * sd)


def _weights(P, alpha, b, C):
    u = P @ b
    return alpha[:, None] * u[None, :] + u[:, None] * alpha[None, :] - 2.0 * (P @ C @ P)


def loo(S, y, rule="log", fac=None, weights=True):
    """(value, log det S, means, variances, W) of leave-one-out under `rule`."""
    fac = factor(S, y) if fac is None else fac
    P, alpha = fac["P"], fac["alpha"]
    d = np.diagonal(P)
    e, v = alpha / d, 1.0 / d
    value = np.sum(term(rule, e, v))
    W = None
    if weights:
        q, s = sensitivities(rule, e, v)
        W = _weights(P, alpha, q * v, np.diag(q * e * v + s * v * v))
    return value, fac["logdet"], np.asarray(y) - e, v, W


def blocked(S, y, fold_start, fac=None, weights=True):
    """(value, log det S, means, variances, W) of blocked cross-validation over the folds [fold_start[f], fold_start[f + 1])."""
    fac = factor(S, y) if fac is None else fac
    P, alpha = fac["P"], fac["alpha"]
    n = len(alpha)
    value = -0.5 * n * np.log(2.0 * _pi(P.dtype))
    b, var, C = np.zeros(n, dtype=P.dtype), np.zeros(n, dtype=P.dtype), np.zeros((n, n), dtype=P.dtype)
    for lo, hi in zip(fold_start[:-1], fold_start[1:]):
        G = cholesky(P[lo:hi, lo:hi])
        Ginv = inverse_factor(G)
        Dinv = Ginv.T @ Ginv
        b[lo:hi] = Dinv @ alpha[lo:hi]
        var[lo:hi] = np.diagonal(Dinv)
        C[lo:hi, lo:hi] = 0.5 * (Dinv + b[lo:hi, None] * b[None, lo:hi])
        value = value + np.sum(np.log(np.diagonal(G))) - 0.5 * np.sum(alpha[lo:hi] * b[lo:hi])
    return value, fac["logdet"], np.asarray(y) - b, var, _weights(P, alpha, b, C) if weights else None


def purged(S, y, fold_start, hold_lo, hold_hi, fac=None, weights=True):
    """(value, log det S, means, variances, W) of purged blocked cross-validation: fold f scores [fold_start[f], fold_start[f + 1]) from
    the rows outside [hold_lo[f], hold_hi[f])."""
    fac = factor(S, y) if fac is None else fac
    P, alpha = fac["P"], fac["alpha"]
    n = len(alpha)
    value = -0.5 * n * np.log(2.0 * _pi(P.dtype))
    y = np.asarray(y)
    mean, var = np.zeros(n, dtype=P.dtype), np.zeros(n, dtype=P.dtype)
    b, C = np.zeros(n, dtype=P.dtype), np.zeros((n, n), dtype=P.dtype)
    for s, e, a, h in zip(fold_start[:-1], fold_start[1:], hold_lo, hold_hi):
        order = np.concatenate([np.arange(a, s), np.arange(e, h), np.arange(s, e)]).astype(int)   # (G left, G right, F)
        g = len(order) - (e - s)
        L = cholesky(P[np.ix_(order, order)])
        N = inverse_factor(L)
        w = N @ alpha[order]
        NF, wF = N[g:], w[g:]
        ev = N.T @ w
        bH = NF.T @ wF
        gv = ev - bH
        NN = NF.T @ NF
        mean[s:e], var[s:e] = y[s:e] - ev[g:], np.diagonal(NN)[g:]
        value = value + np.sum(np.log(np.diagonal(L)[g:])) - 0.5 * np.sum(wF * wF)
        if weights:
            b[order] += bH
            C[np.ix_(order, order)] += 0.5 * (NN + ev[:, None] * ev[None, :] - gv[:, None] * gv[None, :])
    return value, fac["logdet"], mean, var, _weights(P, alpha, b, C) if weights else None


# ---- the definitions: deletion -----------------------------------------------------------------------------------------------------------
def _conditional(S, y, fold, rest):
    """Mean and covariance of y_fold given y_rest under N(0, S)."""
    if not len(rest):
        return np.zeros(len(fold), dtype=S.dtype), S[np.ix_(fold, fold)]
    sol = solve(S[np.ix_(rest, rest)], np.concatenate([y[rest, None].astype(S.dtype), S[np.ix_(rest, fold)]], axis=1))
    return S[np.ix_(fold, rest)] @ sol[:, 0], S[np.ix_(fold, fold)] - S[np.ix_(fold, rest)] @ sol[:, 1:]


def loo_brute(S, y, rule="log"):
    """(value, means, variances): row by row, delete it, condition on the rest, score it."""
    S, y = np.asarray(S), np.asarray(y)
    n = len(y)
    value, mean, var = 0.0, np.zeros(n, dtype=S.dtype), np.zeros(n, dtype=S.dtype)
    for i in range(n):
        mu, cov = _conditional(S, y, np.array([i]), np.delete(np.arange(n), i))
        mean[i], var[i] = mu[0], cov[0, 0]
        value = value + term(rule, y[i] - mu[0], cov[0, 0])
    return value, mean, var


def purged_brute(S, y, fold_start, hold_lo, hold_hi):
    """(value, means, variances): per fold delete the rows of H, condition on the rest, the joint Gaussian log density of y_F."""
    S, y = np.asarray(S), np.asarray(y)
    n = len(y)
    value, mean, var = 0.0, np.zeros(n, dtype=S.dtype), np.zeros(n, dtype=S.dtype)
    log_2pi = np.log(2.0 * _pi(S.dtype))
    for s, e, a, h in zip(fold_start[:-1], fold_start[1:], hold_lo, hold_hi):
        fold = np.arange(s, e)
        mu, cov = _conditional(S, y, fold, np.concatenate([np.arange(0, a), np.arange(h, n)]).astype(int))
        Lc = cholesky(cov)
        z = forward(Lc, (y[fold] - mu).astype(S.dtype))
        value = value - 0.5 * (2.0 * np.sum(np.log(np.diagonal(Lc))) + np.sum(z * z) + (e - s) * log_2pi)
        mean[fold], var[fold] = mu, np.diagonal(cov)
    return value, mean, var


def blocked_brute(S, y, fold_start):
    """(value, means, variances): per fold delete its rows, condition on the rest, the joint log density of the fold."""
    fold_start = np.asarray(fold_start)
    return purged_brute(S, y, fold_start, fold_start[:-1], fold_start[1:])
