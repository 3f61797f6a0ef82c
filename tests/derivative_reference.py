"""Posterior derivatives restated in plain numpy (a helper module, like tests/gram_math_emulation.py): what gpar_posterior_deriv and
GPARRegressor.derivative are compared against.  Everything is in DESIGN space: a direction u is a row over the columns of the design
matrix; the feature map's Jacobian is applied here, independently of the product's J builder.

- The cross-covariance rows d[a, b] = u_a . grad_x k(x*_a, x_b) and the means come from oracle.kernels.kernel_input_grads, which returns
  gradients with respect to the DESIGN columns (d z / d x - 1 / scale and the derivative of the periodic embedding - already chained), so
  a row of d is its result for the pair weights that pick one training row, dotted with u.
- The prior term u^T [grad_x grad_x'^T k](x*, x*) u is a closed form written here from the kernels' definitions (oracle/kernels.py's
  docstring), as an explicit width x width matrix per point.  tests/test_derivative.py checks it, and d, against central differences of
  oracle.mp_ref.gram in 50-digit arithmetic.
- The layer chain follows oracle.gpar_ref.gpar_predict_moments (the conditioning rules of `impute` / `replace`), with the plug-in test
  inputs [x*, latent means of the layers before] and the direction (e_wrt, derivatives of those means) carried alongside.
"""
import numpy as np
import scipy.linalg

from oracle import gpar_ref
from oracle import kernels as ok

EPS = 1e-12   # the engines' jitter


def cross_rows(spec, xs, x, U):
    """d (n* x n): d[a, b] = sum_c U[a, c] d k(xs_a, x_b) / d xs[a, c]."""
    xs, x, U = np.asarray(xs, dtype=np.float64), np.asarray(x, dtype=np.float64), np.asarray(U, dtype=np.float64)
    d = np.zeros((xs.shape[0], x.shape[0]))
    one = np.ones((xs.shape[0], 1))
    for b in range(x.shape[0]):
        d[:, b] = (U * ok.kernel_input_grads(spec, xs, x[b:b + 1], one)).sum(axis=1)
    return d


def mean_derivative(spec, xs, x, alpha, U):
    """sum_b d[a, b] alpha[b], from ONE call with the pair weights 1 alpha^T."""
    xs = np.asarray(xs, dtype=np.float64)
    W = np.ones((xs.shape[0], 1)) * np.asarray(alpha, dtype=np.float64)[None, :]
    return (np.asarray(U, dtype=np.float64) * ok.kernel_input_grads(spec, xs, x, W)).sum(axis=1)


def _feature_jacobian(factor, xrow, width):
    """A (nd x width): d z_q / d x_c of one factor's features at one design row."""
    cols, scales, periods = list(factor["cols"]), np.asarray(factor["scales"], dtype=np.float64), factor.get("periods")
    ncol = len(cols)
    A = np.zeros((scales.shape[0], width))
    for q in range(scales.shape[0]):
        c = cols[q % ncol] if ncol else 0
        if periods is None:
            slope = 1.0
        else:
            omega = 2.0 * np.pi / float(periods[q % ncol])
            slope = omega * np.cos(omega * xrow[c]) if q < ncol else -omega * np.sin(omega * xrow[c])
        A[q, c] = slope / scales[q]
    return A


def prior_hessian(spec, xrow):
    """M (width x width): [grad_x grad_x'^T k](x, x) at one design row.  On the diagonal a stationary factor phi(r2) has value 1, no
    gradient and the feature-space block -2 phi'(0) I; a cosine factor value 1, no gradient and 4 pi^2 1 1^T (cos(2 pi sum (z - z'))
    differentiated once in z and once in z'); a linear factor <z, z'> value |z|^2, both gradients z and the block I.  A product term
    c prod_f phi_f has, by the product rule in z and in z',
        c [sum_f H_f prod_{g != f} v_g + sum_{f != g} (grad_z phi_f)(grad_z' phi_g)^T prod_{h != f, g} v_h]."""
    xrow = np.asarray(xrow, dtype=np.float64)
    width = xrow.shape[0]
    M = np.zeros((width, width))
    for term in spec["terms"]:
        values, grads, blocks = [], [], []
        for f in term["factors"]:
            A = _feature_jacobian(f, xrow, width)
            z = ok.features(f, xrow[None, :])[0]
            nd = z.shape[0]
            if f["type"] == "linear":
                values.append(float(z @ z))
                grads.append(A.T @ z)
                blocks.append(A.T @ A)
            elif f["type"] == "cos":
                values.append(1.0)
                grads.append(np.zeros(width))
                blocks.append(4.0 * np.pi ** 2 * (A.T @ np.ones((nd, nd)) @ A))
            else:
                if f["type"] == "matern12":
                    raise ValueError("a Matern 1/2 process is not differentiable")
                slope0 = float(ok._stationary(f, np.zeros((1, 1)))[1][0, 0])   # d phi / d r2 at r2 = 0
                values.append(1.0)
                grads.append(np.zeros(width))
                blocks.append(-2.0 * slope0 * (A.T @ A))
        nf = len(values)
        total = np.zeros((width, width))
        for f in range(nf):
            total += blocks[f] * np.prod([values[g] for g in range(nf) if g != f])
            for g in range(nf):
                if g != f:
                    total += np.outer(grads[f], grads[g]) * np.prod([values[h] for h in range(nf) if h not in (f, g)])
        M += float(term["coef"]) * total
    return M


def prior_term(spec, xs, U):
    xs, U = np.asarray(xs, dtype=np.float64), np.asarray(U, dtype=np.float64)
    return np.array([U[a] @ prior_hessian(spec, xs[a]) @ U[a] for a in range(xs.shape[0])])


def layer_derivative(spec, x, y, noise_diag, xs, U, variance=True):
    """(dmean, dvar, mean) of one dense layer conditioned on (x, y) with noise diagonal `noise_diag`: derivative moments along the
    design-space directions U (n* x width) and the latent posterior mean at xs."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = x.shape[0]
    K = ok.gram(spec, x) + np.diag(np.broadcast_to(np.asarray(noise_diag, dtype=np.float64), (n,)) + EPS)
    L = np.linalg.cholesky(K)
    alpha = scipy.linalg.cho_solve((L, True), y)
    mean = ok.gram(spec, xs, x) @ alpha
    dmean = mean_derivative(spec, xs, x, alpha, U)
    if not variance:
        return dmean, None, mean
    half = scipy.linalg.solve_triangular(L, cross_rows(spec, xs, x, U).T, lower=True)
    return dmean, prior_term(spec, xs, U) - (half ** 2).sum(axis=0), mean


def layer_derivatives(spec, x, y, noise_diag, xs, U):
    """(dmean, dvar, prior), each ndir x n*: `layer_derivative` for a stack of directions U (ndir x n* x width) - the same formulas from the
    same helpers, with what does not depend on the direction (the factorisation, the gradients of k(x*_a, x_b) with respect to the design
    columns, the matrix of `prior_hessian` per test row) formed once.  `prior` is the term u^T [grad grad'^T k] u alone."""
    x, y, xs, U = (np.asarray(a, dtype=np.float64) for a in (x, y, xs, U))
    n, ns = x.shape[0], xs.shape[0]
    K = ok.gram(spec, x) + np.diag(np.broadcast_to(np.asarray(noise_diag, dtype=np.float64), (n,)) + EPS)
    L = np.linalg.cholesky(K)
    alpha = scipy.linalg.cho_solve((L, True), y)
    one = np.ones((ns, 1))
    G = np.stack([ok.kernel_input_grads(spec, xs, x[b:b + 1], one) for b in range(n)], axis=1)   # n* x n x width
    H = [prior_hessian(spec, xs[a]) for a in range(ns)]
    dmean, dvar, prior = np.zeros(U.shape[:2]), np.zeros(U.shape[:2]), np.zeros(U.shape[:2])
    for c in range(U.shape[0]):
        d = np.einsum("aw,abw->ab", U[c], G)
        dmean[c] = d @ alpha
        prior[c] = [U[c, a] @ H[a] @ U[c, a] for a in range(ns)]
        dvar[c] = prior[c] - (scipy.linalg.solve_triangular(L, d.T, lower=True) ** 2).sum(axis=0)
    return dmean, dvar, prior


def model_derivative(x, y, hypers, config, xs, wrt, impute, replace, variance=True, normalise_y=False):
    """(dmean, dvar), each n* x p, in the units of y: GPAR.derivative restated.  Conditioning as oracle.gpar_ref.gpar_predict_moments
    (rows kept per layer, the next input column = observed values, imputed / replaced by posterior means); prediction along the plug-in
    path: x*_{i+1} = [x*_i, mean_i(x*_i)], u_{i+1} = [u_i, dmean_i]."""
    x, xs = np.asarray(x, dtype=np.float64), np.asarray(xs, dtype=np.float64)
    x = x[:, None] if x.ndim == 1 else x
    xs = xs[:, None] if xs.ndim == 1 else xs
    y = np.asarray(y, dtype=np.float64)
    m, p = x.shape[1], y.shape[1]
    offset, scale = gpar_ref._normalisation(y, normalise_y)
    y = (y - offset) / scale
    available = ~np.isnan(y)
    U = np.zeros_like(xs)
    U[:, wrt] = 1.0
    dmeans, dvars = [], []
    for i in range(p):
        mask = available[:, i].copy()
        if impute and i < p - 1:
            mask |= available[:, i + 1:].any(axis=1)
        x, yi = x[mask], y[mask, i]
        y, available = y[mask], available[mask]
        spec, noise = gpar_ref.layer_spec(hypers, m, i, config)
        have = ~np.isnan(yi)
        dmean, dvar, mean = layer_derivative(spec, x[have], yi[have], noise, xs, U, variance)
        dmeans.append(dmean * scale[i])
        if variance:
            dvars.append(dvar * scale[i] ** 2)
        if i < p - 1:
            col = yi.copy()
            if (impute and (~have).any()) or replace:
                K = ok.gram(spec, x[have]) + (noise + EPS) * np.eye(int(have.sum()))
                mean_x = ok.gram(spec, x, x[have]) @ np.linalg.solve(K, yi[have])
                if impute:
                    col[~have] = mean_x[~have]
                if replace:
                    col[have] = mean_x[have]
            x = np.concatenate([x, col[:, None]], axis=1)
            xs = np.concatenate([xs, mean[:, None]], axis=1)
            U = np.concatenate([U, dmean[:, None]], axis=1)
    return np.stack(dmeans, axis=1), (np.stack(dvars, axis=1) if variance else None)
