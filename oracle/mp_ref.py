"""Oracle (TEST INFRASTRUCTURE): the same closed forms as oracle/gp_ref.py and oracle/gpar_ref.py in 50-digit arithmetic
(mpmath), to bound the floating-point error of the fp64 oracle routes that produced the golden vectors.  Tiny problems
only (n <= 30: a few seconds; the inducing-point layer below, in its M x M form, up to n = 130, M = 65).  Not a second opinion on the FORMULAS - those are pinned by closed forms, finite
differences and scikit-learn (oracle/__init__.py) - but on their evaluation: whatever the fp64 routes lose to
cancellation or conditioning shows up as a difference from these values.
"""
import mpmath as mp

mp.mp.dps = 50

__all__ = ["gram", "logpdf", "posterior", "vfe_bound", "gpar_logpdf", "sparse_bound", "sparse_bounds", "sparse_posterior",
           "sparse_bound_derivatives"]


def _features(factor, x):
    cols = list(factor["cols"])
    rows = []
    periods = factor.get("periods")
    scales = [mp.mpf(s) for s in factor["scales"]]
    for row in x:
        sel = [mp.mpf(row[c]) for c in cols]
        if periods is not None:
            freq = [2 * mp.pi / mp.mpf(t) for t in periods]
            sel = [mp.sin(v * f) for v, f in zip(sel, freq)] + [mp.cos(v * f) for v, f in zip(sel, freq)]
        rows.append([v / s for v, s in zip(sel, scales)])
    return rows


def _factor_entry(factor, za, zb):
    if factor["type"] == "linear":
        return mp.fsum(a * b for a, b in zip(za, zb))
    if factor["type"] == "cos":   # the cosine factor of include/gpar_hip.h: the cosine of the SUM of the scaled differences
        if factor.get("periods") is not None or len(za) == 0:
            raise ValueError("a cosine factor takes no periods and needs at least one feature")
        return mp.cos(2 * mp.pi * mp.fsum(a - b for a, b in zip(za, zb)))
    r2 = mp.fsum((a - b) ** 2 for a, b in zip(za, zb))
    if factor["type"] == "eq":
        return mp.exp(-r2 / 2)
    if factor["type"] == "rq":
        alpha = mp.mpf(factor["alpha"])
        return (1 + r2 / (2 * alpha)) ** (-alpha)
    # the Matern kernels of smoothness 1/2, 3/2, 5/2 (include/gpar_hip.h) in r = sqrt(r2)
    if factor["type"] == "matern12":
        return mp.exp(-mp.sqrt(r2))
    if factor["type"] == "matern32":
        a = mp.sqrt(3 * r2)
        return (1 + a) * mp.exp(-a)
    if factor["type"] == "matern52":
        a = mp.sqrt(5 * r2)
        return (1 + a + 5 * r2 / 3) * mp.exp(-a)
    raise ValueError(f"unknown factor type {factor['type']!r}")


def gram(spec, x1, x2=None, noise_diag=None, jitter=0):
    sym = x2 is None
    x2 = x1 if sym else x2
    n1, n2 = len(x1), len(x2)
    out = mp.zeros(n1, n2)
    for term in spec["terms"]:
        feats = [(f, _features(f, x1), _features(f, x2)) for f in term["factors"]]
        coef = mp.mpf(term["coef"])
        for a in range(n1):
            for b in range(n2):
                v = coef
                for f, z1, z2 in feats:
                    v *= _factor_entry(f, z1[a], z2[b])
                out[a, b] += v
    if sym:
        for a in range(n1):
            if noise_diag is not None:
                out[a, a] += mp.mpf(noise_diag[a])
            out[a, a] += mp.mpf(jitter)
    return out


def _mvn_logpdf(S, r):
    L = mp.cholesky(S)
    z = mp.lu_solve(L, r)  # L is triangular: exact elimination
    logdet = 2 * mp.fsum(mp.log(L[i, i]) for i in range(S.rows))
    return -(logdet + S.rows * mp.log(2 * mp.pi) + mp.fsum(v * v for v in z)) / 2


def _solve(S, B):
    """S^-1 B for a matrix B, column by column."""
    out = mp.zeros(B.rows, B.cols)
    for j in range(B.cols):
        col = mp.lu_solve(S, B[:, j])
        for i in range(B.rows):
            out[i, j] = col[i]
    return out


def _col(v):
    return mp.matrix([mp.mpf(float(a)) for a in v])


def logpdf(spec, x, y, noise, eps=1e-12):
    n = len(y)
    noise = [float(noise)] * n if not hasattr(noise, "__len__") else list(noise)
    return _mvn_logpdf(gram(spec, x, None, noise, eps), _col(y))


def posterior(spec, x, y, noise, xs, eps=1e-12):
    n = len(y)
    noise = [float(noise)] * n if not hasattr(noise, "__len__") else list(noise)
    S = gram(spec, x, None, noise, eps)
    Ksx = gram(spec, xs, x)
    mean = Ksx * mp.lu_solve(S, _col(y))
    cov = gram(spec, xs) - Ksx * _solve(S, Ksx.T)
    return mean, cov


def vfe_bound(spec, x, y, noise, z, eps=1e-12):
    n = len(y)
    d = [mp.mpf(float(noise))] * n if not hasattr(noise, "__len__") else [mp.mpf(float(v)) for v in noise]
    Kzz = gram(spec, z, None, None, eps)
    Kxz = gram(spec, x, z)
    Q = Kxz * _solve(Kzz, Kxz.T)
    S = Q.copy()
    for a in range(n):
        S[a, a] += d[a]
    kdiag = [gram(spec, [x[a]])[0, 0] for a in range(n)]
    return _mvn_logpdf(S, _col(y)) - mp.fsum((kdiag[a] - Q[a, a]) / d[a] for a in range(n)) / 2


def gpar_logpdf(x, y, w, hypers, config, impute=False, replace=False, eps=1e-12):
    """oracle/gpar_ref.gpar_logpdf in 50 digits (dense path; NaN = missing)."""
    import numpy as np

    from . import gpar_ref

    x = np.asarray(x, dtype=np.float64)
    x = x[:, None] if x.ndim == 1 else x
    y = np.asarray(y, dtype=np.float64)
    w = np.ones_like(y) if w is None else np.asarray(w, dtype=np.float64)
    m, p = x.shape[1], y.shape[1]
    rows = [[mp.mpf(float(v)) for v in row] for row in x]
    available = ~np.isnan(y)
    total = mp.mpf(0)
    for i in range(p):
        mask = available[:, i].copy()
        if impute and i < p - 1:
            mask |= available[:, i + 1:].any(axis=1)
        rows = [r for r, keep in zip(rows, mask) if keep]
        yi, wi = y[mask, i], w[mask, i]
        y, w, available = y[mask], w[mask], available[mask]
        spec, noise = gpar_ref.layer_spec(hypers, m, i, config)
        have = ~np.isnan(yi)
        xh = [r for r, h in zip(rows, have) if h]
        nh = [mp.mpf(noise) / mp.mpf(float(v)) for v in wi[have]]
        total += _mvn_logpdf(gram(spec, xh, None, nh, eps), _col(yi[have]))
        if i < p - 1:
            col = [mp.mpf(float(v)) if h else None for v, h in zip(yi, have)]
            if (impute and (~have).any()) or (replace and have.any()):
                S = gram(spec, xh, None, nh, eps)
                mean = gram(spec, rows, xh) * mp.lu_solve(S, _col(yi[have]))
                for k, h in enumerate(have):
                    if (impute and not h) or (replace and h):
                        col[k] = mean[k]
            rows = [r + [c if c is not None else mp.nan] for r, c in zip(rows, col)]
    return total


# ---- the whole inducing-point layer (gp.PseudoObs: VFE, FITC, DTC) ---------------------------------------------------------------------
# From the definitions in the PseudoObs docstring, with K_zz + eps I as the product uses it:
#     Q = K_xz (K_zz + eps I)^-1 K_zx,   e = d [FITC: d + max(k_aa - q_aa, 0)],
#     VFE   log N(y; 0, Q + diag e) - 1/2 sum_a (k_aa - q_aa) / d_a,     DTC / FITC   log N(y; 0, Q + diag e),
#     posterior  mean* = K_*z Sigma^-1 K_zx E^-1 y,   cov* = K_** - K_*z (K_zz + eps I)^-1 K_z* + K_*z Sigma^-1 K_z*,
#     Sigma = K_zz + eps I + K_zx E^-1 K_xz.
# Evaluated in the M x M form (matrix-determinant lemma and Woodbury on Sigma = L_z A L_z^T, A = I + B E^-1 B^T, B = L_z^-1 K_zx), which
# keeps n = 130 affordable; at 50 digits the form costs no accuracy (tests/test_sparse_precision.py holds it to the n x n `vfe_bound`
# above to 40 digits).  Plain lists of mpf instead of mp.matrix: element access dominates otherwise.
_METHODS = ("vfe", "fitc", "dtc")


def _rows(K):
    return [[K[i, j] for j in range(K.cols)] for i in range(K.rows)]


def _noise_list(noise, n):
    """Scalar or per-point noise as n mpf (entries that are mpf already - a perturbation of 1e-20 - are kept as they are)."""
    keep = lambda v: v if isinstance(v, mp.mpf) else mp.mpf(float(v))
    return [keep(noise)] * n if not hasattr(noise, "__len__") else [keep(v) for v in noise]


def _chol_rows(S):
    """Lower Cholesky factor of the symmetric matrix whose lower triangle is in the rows of S."""
    n = len(S)
    L = [[mp.mpf(0)] * n for _ in range(n)]
    for i in range(n):
        Li = L[i]
        for j in range(i):
            Li[j] = (S[i][j] - mp.fdot(Li[:j], L[j][:j])) / L[j][j]
        pivot = S[i][i] - mp.fdot(Li[:i], Li[:i])
        if pivot <= 0:
            raise ValueError("matrix is not positive definite")
        Li[i] = mp.sqrt(pivot)
    return L


def _fwd(L, b):
    """L^-1 b by forward substitution."""
    out = []
    for i, bi in enumerate(b):
        out.append((bi - mp.fdot(L[i][:i], out)) / L[i][i])
    return out


def _sparse_core(spec, x, z, eps):
    """What all three methods share: L_z, B = L_z^-1 K_zx (by rows of x), q_aa = |B_:a|^2 and k_aa."""
    Lz = _chol_rows(_rows(gram(spec, z, None, None, eps)))
    B = [_fwd(Lz, row) for row in _rows(gram(spec, x, z))]
    return {"Lz": Lz, "B": B, "q": [mp.fdot(b, b) for b in B], "kdiag": [gram(spec, [row])[0, 0] for row in x]}


def _effective_noise(core, d, method):
    if method != "fitc":
        return d
    return [da + max(k - q, mp.mpf(0)) for da, k, q in zip(d, core["kdiag"], core["q"])]


def _sparse_solve(core, y, e):
    """L_A = chol(I + B E^-1 B^T), u = L_A^-1 B E^-1 y and log N(y; 0, Q + diag e) from them."""
    B = core["B"]
    n, M = len(B), len(core["Lz"])
    cols = [[B[a][i] for a in range(n)] for i in range(M)]
    scaled = [[v / ea for v, ea in zip(col, e)] for col in cols]
    A = [[mp.fdot(scaled[i], cols[j]) + (1 if i == j else 0) for j in range(i + 1)] for i in range(M)]
    La = _chol_rows(A)
    u = _fwd(La, [mp.fdot(col, y) for col in scaled])
    logdet = mp.fsum(mp.log(v) for v in e) + 2 * mp.fsum(mp.log(La[i][i]) for i in range(M))
    quad = mp.fsum(v * v / ea for v, ea in zip(y, e)) - mp.fdot(u, u)
    return La, u, -(logdet + n * mp.log(2 * mp.pi) + quad) / 2


def sparse_bounds(spec, x, y, noise, z, methods=_METHODS, eps=1e-12):
    """{method: bound} for several methods at once (they share L_z and B; VFE and DTC share everything but the trace term)."""
    yv = [mp.mpf(float(v)) for v in y]
    d = _noise_list(noise, len(yv))
    core = _sparse_core(spec, x, z, eps)
    out, plain = {}, None
    for method in methods:
        if method not in _METHODS:
            raise ValueError(f"unknown inducing-point method {method!r}")
        if method == "fitc":
            out[method] = _sparse_solve(core, yv, _effective_noise(core, d, method))[2]
            continue
        if plain is None:
            plain = _sparse_solve(core, yv, d)[2]
        out[method] = plain
        if method == "vfe":
            out[method] = plain - mp.fsum((k - q) / da for k, q, da in zip(core["kdiag"], core["q"], d)) / 2
    return out


def sparse_bound(spec, x, y, noise, z, method="vfe", eps=1e-12):
    return sparse_bounds(spec, x, y, noise, z, (method,), eps)[method]


def sparse_posterior(spec, x, y, noise, z, xs, method="vfe", eps=1e-12):
    """(mean, full covariance) of the latent function at xs, as (list, list of rows)."""
    yv = [mp.mpf(float(v)) for v in y]
    core = _sparse_core(spec, x, z, eps)
    La, u, _ = _sparse_solve(core, yv, _effective_noise(core, _noise_list(noise, len(yv)), method))
    P = [_fwd(core["Lz"], row) for row in _rows(gram(spec, xs, z))]
    R = [_fwd(La, p) for p in P]
    Kss = gram(spec, xs)
    mean = [mp.fdot(r, u) for r in R]
    ns = len(P)
    cov = [[Kss[s, t] - mp.fdot(P[s], P[t]) + mp.fdot(R[s], R[t]) for t in range(ns)] for s in range(ns)]
    return mean, cov


def _perturbed(spec, x, noise, z, wrt, t):
    """The arguments with `wrt` moved by t times its unit: see `sparse_bound_derivatives`.  Returns (spec, x, noise, z, unit)."""
    import copy

    kind = wrt["kind"]
    x = [[mp.mpf(float(v)) for v in row] for row in x]
    z = [[mp.mpf(float(v)) for v in row] for row in z]
    unit = mp.mpf(1)
    if kind == "coef":
        spec = copy.deepcopy(spec)
        value = mp.mpf(float(spec["terms"][wrt["term"]]["coef"]))
        unit = abs(value)
        spec["terms"][wrt["term"]]["coef"] = value + t * unit
    elif kind in ("scales", "periods", "alpha"):
        spec = copy.deepcopy(spec)
        factor = spec["terms"][wrt["term"]]["factors"][wrt["factor"]]
        if kind == "alpha":
            value = mp.mpf(float(factor["alpha"]))
            unit = abs(value)
            factor["alpha"] = value + t * unit
        else:
            values = [mp.mpf(float(v)) for v in factor[kind]]
            unit = abs(values[wrt["index"]])
            values[wrt["index"]] += t * unit
            factor[kind] = values
    elif kind == "noise":
        n = len(x)
        values = _noise_list(noise, n)
        index = wrt.get("index")
        unit = abs(values[0] if index is None else values[index])
        noise = [v + t * unit if index is None or a == index else v for a, v in enumerate(values)]
    elif kind in ("x", "z"):
        rows = x if kind == "x" else z
        value = rows[wrt["row"]][wrt["col"]]
        unit = abs(value) if value != 0 else mp.mpf(1)
        rows[wrt["row"]][wrt["col"]] = value + t * unit
    elif kind in ("xdir", "zdir"):
        rows = x if kind == "xdir" else z
        for i, drow in enumerate(wrt["direction"]):
            for j, dv in enumerate(drow):
                rows[i][j] += t * mp.mpf(float(dv))
    else:
        raise ValueError(f"cannot differentiate with respect to {kind!r}")
    return spec, x, noise, z, unit


def sparse_bound_derivatives(spec, x, y, noise, z, wrt, methods=_METHODS, eps=1e-12, step=1e-20, dps=80):
    """{method: [d bound / d argument for every entry of `wrt`]} by central differences IN mp ARITHMETIC - no analytic derivative code, so the
    values are independent of `gp.PseudoObs.gradients`.  The step is `step` (1e-20) of the argument's size and the working precision
    `dps` (80) digits: truncation ~ step^2 = 1e-40 relative, rounding ~ 10^-dps / step = 1e-60.

    An entry of `wrt` is a dict: {"kind": "coef", "term": t} | {"kind": "scales" | "periods", "term": t, "factor": f, "index": k} |
    {"kind": "alpha", "term": t, "factor": f} | {"kind": "noise"} (every entry moved together: a scalar noise) | {"kind": "noise",
    "index": a} | {"kind": "x" | "z", "row": i, "col": j} | {"kind": "xdir" | "zdir", "direction": matrix} (the gradient contracted
    with a fixed direction)."""
    out = {m: [] for m in methods}
    with mp.workdps(dps):
        h = mp.mpf(step)
        for entry in wrt:
            values = []
            for sign in (1, -1):
                s, xp, nz, zp, unit = _perturbed(spec, x, noise, z, entry, sign * h)
                values.append((sparse_bounds(s, xp, y, nz, zp, methods, eps), unit))
            (plus, unit), (minus, _) = values
            for m in methods:
                out[m].append((plus[m] - minus[m]) / (2 * h * unit))
    return {m: [+v for v in vals] for m, vals in out.items()}
