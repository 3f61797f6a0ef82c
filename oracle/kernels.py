"""Oracle (TEST INFRASTRUCTURE): Gram matrices of GPAR's composite layer kernels in numpy fp64.

Restates the public definitions of the mlkernels kernels that the reference composes in
/root/reference/gpar/regression.py:92-180 (the packages themselves are not vendored; see
oracle/__init__.py, "parity unpinned"):

    EQ            k(x, y) = exp(-|x - y|^2 / 2)                     (regression.py:109,128,165)
    RQ(alpha)     k(x, y) = (1 + |x - y|^2 / (2 alpha))^-alpha      (regression.py:107,156-163)
    Linear        k(x, y) = <x, y>                                  (regression.py:138,146)
    k.stretch(s)  k(x / s, y / s)                                   (regression.py:110,128,138,146,166)
    k.periodic(T) k(phi(x), phi(y)), phi(x) = [sin(2 pi x / T), cos(2 pi x / T)]  (regression.py:128)
    k.select(i)   k(x[:, i], y[:, i])                               (regression.py:178)
    c * k, k + k', k * k', k + c                                    (regression.py:110,127-129,138)

and the Matern kernels of include/gpar_hip.h, which the reference lacks (Rasmussen & Williams 2006, eq. 4.14-4.17), in
r = sqrt(|x - y|^2):

    matern12      k = exp(-r)                                        dk/dr2 = -exp(-r) / (2 r), TAKEN AS 0 AT r = 0
    matern32      k = (1 + sqrt(3) r) exp(-sqrt(3) r)                dk/dr2 = -(3/2) exp(-sqrt(3) r)
    matern52      k = (1 + sqrt(5) r + 5 r^2 / 3) exp(-sqrt(5) r)    dk/dr2 = -(5/6) (1 + sqrt(5) r) exp(-sqrt(5) r)

(nu = 1/2 has a kink at r = 0: its derivative with respect to r2 is singular there, and every gradient - here as in the
product - leaves coincident pairs out of the sums.)

and the cosine factor of include/gpar_hip.h (the oscillating factor of a spectral mixture, Wilson & Adams 2013; the reference lacks
it as well), in sigma = ((0 + (z_0 - z'_0)) + (z_1 - z'_1)) + ..., the SUM of the scaled differences in dim order:

    cos           k = cos(2 pi sigma)                                dk/dsigma = -2 pi sin(2 pi sigma)
                  d sigma / d s_q = -(z_q - z'_q) / s_q,  d sigma / d x[a, c] = 1 / s_q  (q the feature of column c);  k(x, x) = 1

(2 sigma is reduced to [-1/2, 1/2] half periods exactly - fmod and the fold round nothing, tests/cosine_math_emulation.py - BEFORE
pi enters, and the remainder is evaluated in long double where that is wider than float64.  cos(2 * pi * sigma) in float64 would
round the phase by 2 pi |sigma| 2^-52 first.  No periods - `.stretch(T)` makes a scale the period - and at least one feature.)

A kernel is handed around as a plain dict (no product classes are imported here):

    {"terms": [{"coef": float,
                "factors": [{"type": "eq" | "rq" | "linear" | "matern12" | "matern32" | "matern52" | "cos",
                             "cols": [int, ...],        # columns of the design matrix
                             "scales": [float, ...],    # one per feature (2 * len(cols) if periodic)
                             "periods": None | [float, ...],   # one per column
                             "alpha": float}]}]}

The squared distance is computed from explicit differences, sum_d ((x_d - y_d) / s_d)^2, which is exactly
symmetric and exactly zero on the diagonal; the HIP kernel uses the same formula.
"""
import numpy as np

__all__ = ["features", "factor_matrix", "gram", "gram_diag", "spec_to_dict"]

STATIONARY = ("eq", "rq", "matern12", "matern32", "matern52")   # functions of r2 alone, 1 at r2 = 0


def _stationary(factor, r2):
    """(k, dk/dr2) of a stationary factor at the matrix of squared distances `r2`."""
    kind = factor["type"]
    if kind == "eq":
        F = np.exp(-0.5 * r2)
        return F, -0.5 * F
    if kind == "rq":
        alpha = float(factor["alpha"])
        F = np.exp(-alpha * np.log1p(r2 / (2.0 * alpha)))
        return F, -0.5 * F / (1.0 + r2 / (2.0 * alpha))
    if kind == "matern12":
        r = np.sqrt(r2)
        F = np.exp(-r)
        away = r > 0.0
        dF = np.zeros_like(F)
        dF[away] = -F[away] / (2.0 * r[away])
        return F, dF
    if kind == "matern32":
        a = np.sqrt(3.0) * np.sqrt(r2)
        e = np.exp(-a)
        return (1.0 + a) * e, -1.5 * e
    if kind == "matern52":
        a = np.sqrt(5.0) * np.sqrt(r2)
        e = np.exp(-a)
        return (1.0 + a + 5.0 * r2 / 3.0) * e, -(5.0 / 6.0) * (1.0 + a) * e
    raise ValueError(f"unknown factor type {kind!r}")


_LD = np.longdouble
_LD_PI = _LD("3.14159265358979323846264338327950288")


def _cos_check(factor):
    if factor.get("periods") is not None:
        raise ValueError("a cosine factor takes no periods: it is the cosine of a sum of differences of the columns themselves")
    if len(factor["cols"]) == 0 or len(factor["scales"]) == 0:
        raise ValueError("a cosine factor needs at least one feature")


def _cos_sigma(z1, z2):
    """sigma[a, b] = ((0 + (z1[a, 0] - z2[b, 0])) + (z1[a, 1] - z2[b, 1])) + ... in float64, in dim order."""
    sigma = np.zeros((z1.shape[0], z2.shape[0]))
    for d in range(z1.shape[1]):
        sigma = sigma + (z1[:, d][:, None] - z2[:, d][None, :])
    return sigma


def _cos_pair(sigma):
    """(cos(2 pi sigma), -2 pi sin(2 pi sigma)) of float64 sigma: t = 2 sigma, t mod 2 and the fold onto [-1/2, 1/2] are exact in
    binary floating point (done in float64: nothing to gain from more digits); pi multiplies the remainder, of size at most 1/2, in long
    double, and the result is rounded to float64 once."""
    t = 2.0 * np.asarray(sigma, dtype=np.float64)
    r = np.fmod(t, 2.0)                           # (-2, 2)
    r = np.where(r > 1.0, r - 2.0, r)
    r = np.where(r < -1.0, r + 2.0, r)            # [-1, 1]
    sign = np.where(np.abs(r) > 0.5, -1.0, 1.0)
    r = np.where(r > 0.5, r - 1.0, r)
    r = np.where(r < -0.5, r + 1.0, r)            # [-1/2, 1/2]: cos(pi (r +- 1)) = -cos(pi r), sin likewise
    angle = _LD_PI * r.astype(_LD)
    value = sign * np.cos(angle)
    slope = -(2 * _LD_PI) * (sign * np.sin(angle))
    return value.astype(np.float64), slope.astype(np.float64)


def features(factor, x):
    """Feature rows of one factor: select -> (periodic embedding) -> stretch."""
    x = np.asarray(x, dtype=np.float64)
    cols = list(factor["cols"])
    sel = x[:, cols] if len(cols) else np.zeros((x.shape[0], 0))
    periods = factor.get("periods")
    if periods is not None:
        freq = 2.0 * np.pi / np.asarray(periods, dtype=np.float64)
        sel = np.concatenate([np.sin(sel * freq[None, :]), np.cos(sel * freq[None, :])], axis=1)
    scales = np.asarray(factor["scales"], dtype=np.float64)
    if sel.shape[1] != scales.shape[0]:
        raise ValueError("scales do not match the number of features")
    return sel * (1.0 / scales)[None, :]


def factor_matrix(factor, x1, x2):
    if factor["type"] not in ("linear", "cos") and factor["type"] not in STATIONARY:
        raise ValueError(f"unknown factor type {factor['type']!r}")
    if factor["type"] == "cos":
        _cos_check(factor)
    z1, z2 = features(factor, x1), features(factor, x2)
    if factor["type"] == "cos":
        return _cos_pair(_cos_sigma(z1, z2))[0]
    if factor["type"] == "linear":
        out = np.zeros((z1.shape[0], z2.shape[0]))
        for d in range(z1.shape[1]):
            out += z1[:, d][:, None] * z2[:, d][None, :]
        return out
    r2 = np.zeros((z1.shape[0], z2.shape[0]))
    for d in range(z1.shape[1]):
        diff = z1[:, d][:, None] - z2[:, d][None, :]
        r2 += diff * diff
    return _stationary(factor, r2)[0]


def gram(spec, x1, x2=None, noise_diag=None, jitter=0.0):
    """K[a, b] = k(x1[a], x2[b]); for x2 None the symmetric Gram, optionally + diag(noise_diag) + jitter I."""
    x1 = np.asarray(x1, dtype=np.float64)
    sym = x2 is None
    x2 = x1 if sym else np.asarray(x2, dtype=np.float64)
    out = np.zeros((x1.shape[0], x2.shape[0]))
    for term in spec["terms"]:
        prod = np.full_like(out, float(term["coef"]))
        for factor in term["factors"]:
            prod = prod * factor_matrix(factor, x1, x2)
        out += prod
    if sym:
        idx = np.arange(out.shape[0])
        if noise_diag is not None:
            out[idx, idx] += np.asarray(noise_diag, dtype=np.float64)
        if jitter:
            out[idx, idx] += jitter
    return out


def gram_diag(spec, x):
    """k(x_a, x_a): every stationary factor (EQ, RQ, the Matern kernels) and the cosine factor (sigma = 0 exactly) is 1 on the
    diagonal, a linear factor |z_a|^2."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros(x.shape[0])
    for term in spec["terms"]:
        prod = np.full_like(out, float(term["coef"]))
        for factor in term["factors"]:
            if factor["type"] == "linear":
                z = features(factor, x)
                prod = prod * np.sum(z * z, axis=1)
            elif factor["type"] == "cos":
                _cos_check(factor)
            elif factor["type"] not in STATIONARY:
                raise ValueError(f"unknown factor type {factor['type']!r}")
        out += prod
    return out


def spec_to_dict(kernel):
    """Duck-typed conversion of a product-side kernel object (anything exposing `.terms` with
    `.coef`/`.factors`, factors exposing type/cols/scales/periods/alpha) into the oracle's dict."""
    if isinstance(kernel, dict):
        return kernel
    terms = []
    for term in kernel.terms:
        factors = []
        for f in term.factors:
            factors.append(
                {
                    "type": str(f.type),
                    "cols": [int(c) for c in f.cols],
                    "scales": [float(s) for s in np.asarray(f.scales_value(), dtype=np.float64).reshape(-1)],
                    "periods": None
                    if f.periods is None
                    else [float(s) for s in np.asarray(f.periods_value(), dtype=np.float64).reshape(-1)],
                    "alpha": float(f.alpha_value()) if f.alpha is not None else 0.0,
                }
            )
        terms.append({"coef": float(term.coef_value()), "factors": factors})
    return {"terms": terms}


def kernel_grads(spec, x, W):
    """d/d(theta) of  1/2 sum_ab W_ab K_ab(theta)  for every parameter of the kernel `spec` (W symmetric, n x n):
    term coefficients, per-feature length scales, per-column periods and RQ alphas (the Matern kernels and the cosine factor have
    none beyond their scales; nu = 1/2 contributes nothing at r = 0, see the module docstring).  Each derivative matrix
    dK/dtheta is formed explicitly (test sizes only) — deliberately a different route from the HIP kernel, which
    accumulates per-feature moment sums in one pass.  Verified against central finite differences in
    tests/test_oracle.py."""
    x = np.asarray(x, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    out = {"coef": [], "factors": []}
    for term in spec["terms"]:
        mats = [factor_matrix(f, x, x) for f in term["factors"]]
        full = np.ones((x.shape[0], x.shape[0]))
        for m_ in mats:
            full = full * m_
        out["coef"].append(0.5 * np.sum(W * full))
        fgrads = []
        for fi, f in enumerate(term["factors"]):
            rest = np.full_like(full, float(term["coef"]))
            for fj, m_ in enumerate(mats):
                if fj != fi:
                    rest = rest * m_
            z = features(f, x)
            scales = np.asarray(f["scales"], dtype=np.float64)
            nd = z.shape[1]
            g = {"scales": np.zeros(nd), "periods": None, "alpha": None}
            if f["type"] == "linear":
                for q in range(nd):
                    dF = -2.0 * (z[:, q][:, None] * z[:, q][None, :]) / scales[q]
                    g["scales"][q] = 0.5 * np.sum(W * rest * dF)
            elif f["type"] == "cos":
                _cos_check(f)
                slope = _cos_pair(_cos_sigma(z, z))[1]           # d phi / d sigma
                for q in range(nd):
                    # d sigma / d s_q = -(z_q - z'_q) / s_q
                    dsigma = -(z[:, q][:, None] - z[:, q][None, :]) / scales[q]
                    g["scales"][q] = 0.5 * np.sum(W * rest * slope * dsigma)
            else:
                r2 = np.zeros_like(full)
                diffs = []
                for q in range(nd):
                    d = z[:, q][:, None] - z[:, q][None, :]
                    diffs.append(d)
                    r2 += d * d
                F, dF_dr2 = _stationary(f, r2)
                if f["type"] == "rq":
                    alpha = float(f["alpha"])
                    t = r2 / (2 * alpha)
                    g["alpha"] = 0.5 * np.sum(W * rest * F * (t / (1 + t) - np.log1p(t)))
                for q in range(nd):
                    # d r2 / d s_q = -2 diff_q^2 / s_q
                    g["scales"][q] = 0.5 * np.sum(W * rest * dF_dr2 * (-2.0 * diffs[q] ** 2 / scales[q]))
                if f.get("periods") is not None:
                    periods = np.asarray(f["periods"], dtype=np.float64)
                    cols = list(f["cols"])
                    ncol = len(cols)
                    g["periods"] = np.zeros(ncol)
                    for j in range(ncol):
                        omega = 2 * np.pi / periods[j]
                        xc = x[:, cols[j]]
                        # z_sin = sin(omega x)/s, z_cos = cos(omega x)/s';  d omega / d T = -omega / T
                        dz_sin = np.cos(omega * xc) * xc * (-omega / periods[j]) / scales[j]
                        dz_cos = -np.sin(omega * xc) * xc * (-omega / periods[j]) / scales[j + ncol]
                        dr2 = 2 * diffs[j] * (dz_sin[:, None] - dz_sin[None, :]) + 2 * diffs[j + ncol] * (
                            dz_cos[:, None] - dz_cos[None, :]
                        )
                        g["periods"][j] = 0.5 * np.sum(W * rest * dF_dr2 * dr2)
            fgrads.append(g)
        out["factors"].append(fgrads)
    return out


def kernel_input_grads(spec, x1, x2, W):
    """G[a, c] = sum_b W[a, b] d k(x1_a, x2_b) / d x1[a, c]  (x2 held fixed), through explicit per-column derivative matrices
    of every factor (test sizes only) - a different route from the HIP kernel, which works in feature space with row sums."""
    x1, x2, W = np.asarray(x1, dtype=np.float64), np.asarray(x2, dtype=np.float64), np.asarray(W, dtype=np.float64)
    n1, width = x1.shape
    out = np.zeros((n1, width))
    for term in spec["terms"]:
        mats = [factor_matrix(f, x1, x2) for f in term["factors"]]
        for fi, f in enumerate(term["factors"]):
            rest = np.full((n1, x2.shape[0]), float(term["coef"]))
            for fj, m_ in enumerate(mats):
                if fj != fi:
                    rest = rest * m_
            z1, z2 = features(f, x1), features(f, x2)
            cols = list(f["cols"])
            scales = np.asarray(f["scales"], dtype=np.float64)
            periods = f.get("periods")
            ncol = len(cols)
            if f["type"] == "cos":
                _cos_check(f)
                slope = _cos_pair(_cos_sigma(z1, z2))[1]         # d phi / d sigma; d sigma / d z1[:, q] = 1 for every feature
            elif f["type"] != "linear":
                r2 = np.zeros_like(rest)
                for q in range(z1.shape[1]):
                    r2 += (z1[:, q][:, None] - z2[:, q][None, :]) ** 2
                dF_dr2 = _stationary(f, r2)[1]
            for q in range(z1.shape[1]):
                j = q % ncol if ncol else 0
                c = cols[j]
                # d z1[:, q] / d x1[:, c]
                if periods is None:
                    dz = np.full(n1, 1.0 / scales[q])
                else:
                    omega = 2 * np.pi / float(periods[j])
                    dz = (omega * np.cos(omega * x1[:, c]) if q < ncol else -omega * np.sin(omega * x1[:, c])) / scales[q]
                if f["type"] == "linear":
                    dF = z2[:, q][None, :] * np.ones((n1, 1))            # d <z1, z2> / d z1[q]
                elif f["type"] == "cos":
                    dF = slope
                else:
                    dF = dF_dr2 * 2.0 * (z1[:, q][:, None] - z2[:, q][None, :])
                out[:, c] += np.sum(W * rest * dF, axis=1) * dz
    return out
