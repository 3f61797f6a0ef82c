"""Per-row parameter gradients of a weighted kernel row sum restated in plain numpy long double (a helper module, like
tests/derivative_reference.py): what gpar_gram_grad_rows, pushed through the host chain rule `HipEngine._grads_from_moments`, is compared
against.  For inputs x1 (n1 x width), x2 (n2 x width), weights v (n2) and a kernel spec dict (oracle.kernels.spec_to_dict)

    g_a(theta) = sum_b v_b k_theta(x1_a, x2_b),

`row_gradients` returns, for every NATURAL parameter theta - each term's coefficient, every length scale, every period, every RQ alpha -,
d g_a / d theta and the magnitude sum S_a = sum_b |v_b| |d k_theta(x1_a, x2_b) / d theta|, each as {name: array of n1}.  Names:
"coef/t", "scales/t/f/q", "periods/t/f/c", "alpha/t/f" (term t, factor f of the term, feature q or design column c of the factor).

Written from the kernels' published definitions (include/gpar_hip.h; oracle/kernels.py's docstring states the same ones), in closed form:
a term is c prod_f phi_f, and with the features z = sel(x) / scale (sel the selected columns, or their embedding (sin(w x), cos(w x)), w =
2 pi / period), d = z1 - z2 per feature, r2 = sum d^2,
    linear      phi = sum z1 z2                      d phi / d scale_q = -2 z1_q z2_q / scale_q
    cos         phi = cos(2 pi sum d)                d phi / d scale_q = 2 pi sin(2 pi sum d) d_q / scale_q
    stationary  phi = f(r2)                          d phi / d scale_q = f'(r2) (-2 d_q^2 / scale_q)
                                                     d phi / d period_c = f'(r2) sum_{q in {c, ncol + c}} 2 d_q (dz1_q - dz2_q) / d period_c
      eq        f = exp(-r2 / 2)                     f' = -f / 2
      rq        f = (1 + r2 / (2 alpha))^-alpha      f' = -(1 + r2 / (2 alpha))^(-alpha - 1) / 2
                                                     d f / d alpha = f (t / (1 + t) - log(1 + t)),  t = r2 / (2 alpha)
      matern12  f = exp(-r)                          f' = -exp(-r) / (2 r)   (at r = 0 every d_q is 0 and so is d phi / d scale_q)
      matern32  f = (1 + a) exp(-a), a = sqrt(3 r2)  f' = -3 exp(-a) / 2
      matern52  f = (1 + a + a^2 / 3) exp(-a), a = sqrt(5 r2)      f' = -5 (1 + a) exp(-a) / 6
tests/test_grad_rows_limits.py checks every one of them against central differences of oracle.mp_ref.gram in 50-digit arithmetic.

This module imports numpy alone: nothing from gpar_amd, and nothing from the oracle.  The arithmetic of the dynamic LDS the kernel asks
for (`rows_lds_doubles`, `slots_used`) is restated here too, with its constants; the same CPU test checks them against the sources."""
import numpy as np

LD = np.longdouble
TWO_PI = 8 * np.arctan(LD(1))   # (to the long double's own precision: np.pi is a double)

# ---- the dynamic LDS of gram_grad_rows_kernel (csrc/gram_grad_rows.h rows_lds_bytes), in doubles ------------------------------------------------
GRAM_T, GRAM_LD = 64, 68
MAX_TERMS, MAX_FACTORS, MAX_DIMS, MAXF = 8, 12, 96, 4
GRAD_NACC = MAX_TERMS + MAX_FACTORS + 2 * MAX_DIMS
K_RQ, K_LINEAR, K_COS = 1, 2, 6            # the factor types the slot plan tells apart (include/gpar_hip.h)
LDS_48K, LDS_160K = 48 * 1024 // 8, 160 * 1024 // 8


def rows_lds_doubles(dz, zd, nused):
    """(2, with zd 4) tile images of max(dz, 1) x GRAM_LD features, GRAM_LD weights, GRAM_T accumulators per used slot and the slot map
    of GRAD_NACC ints.  The launch opts in to large LDS when this EXCEEDS LDS_48K; the entry refuses when it EXCEEDS LDS_160K."""
    return (4 if zd else 2) * max(dz, 1) * GRAM_LD + GRAM_LD + GRAM_T * nused + GRAD_NACC // 2


def slots_used(kspec, zd):
    """The raw slots (C_t, Al_f, A_q, P_q at 0, MAX_TERMS, + MAX_FACTORS, + MAX_DIMS) a compiled kernel specification uses, sorted: its
    terms, its RQ factors, the dims under a factor and - when zd is given - the dims under a stationary factor again (rows_check)."""
    used = set(range(kspec.nterms))
    for f in range(kspec.nfactors):
        fa = kspec.factor[f]
        if fa.type == K_RQ:
            used.add(MAX_TERMS + f)
        for d in range(fa.off, fa.off + fa.nd):
            used.add(MAX_TERMS + MAX_FACTORS + d)
            if zd and fa.type not in (K_LINEAR, K_COS):
                used.add(MAX_TERMS + MAX_FACTORS + MAX_DIMS + d)
    return sorted(used)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
def _features(factor, x):
    """(z, dz / d period): n x nd each; the second is None without periods (its column c then belongs to features c and ncol + c)."""
    cols = list(factor["cols"])
    scales = np.asarray(factor["scales"], dtype=LD)
    sel = np.asarray(x, dtype=LD)[:, cols]
    periods = factor.get("periods")
    if periods is None:
        return sel / scales, None
    T = np.asarray(periods, dtype=LD)
    w = TWO_PI / T
    dw = -TWO_PI / (T * T)                                    # d w / d period
    arg = sel * w
    emb = np.concatenate([np.sin(arg), np.cos(arg)], axis=1)
    demb = np.concatenate([sel * np.cos(arg) * dw, -sel * np.sin(arg) * dw], axis=1)
    return emb / scales, demb / scales


def _stationary(kind, r2, alpha):
    """(f, f', d f / d alpha or None) at r2."""
    if kind == "eq":
        f = np.exp(-r2 / 2)
        return f, -f / 2, None
    if kind == "rq":
        t = r2 / (2 * alpha)
        f = np.exp(-alpha * np.log1p(t))
        return f, -f / (2 * (1 + t)), f * (t / (1 + t) - np.log1p(t))
    if kind == "matern12":
        r = np.sqrt(r2)
        f = np.exp(-r)
        slope = np.zeros_like(r)
        np.divide(-f, 2 * r, out=slope, where=r > 0)
        return f, slope, None
    if kind == "matern32":
        a = np.sqrt(3 * r2)
        return (1 + a) * np.exp(-a), -LD(3) / 2 * np.exp(-a), None
    if kind == "matern52":
        a = np.sqrt(5 * r2)
        return (1 + a + a * a / 3) * np.exp(-a), -LD(5) / 6 * (1 + a) * np.exp(-a), None
    raise ValueError(f"unknown factor type {kind!r}")


def _factor(factor, x1, x2):
    """(phi, {name suffix: d phi / d parameter}), every array n1 x n2."""
    kind = factor["type"]
    scales = np.asarray(factor["scales"], dtype=LD)
    z1, p1 = _features(factor, x1)
    z2, p2 = _features(factor, x2)
    nd = scales.shape[0]
    grads = {}
    if kind == "linear":
        prod = z1[:, None, :] * z2[None, :, :]
        for q in range(nd):
            grads[f"scales/{q}"] = -2 * prod[:, :, q] / scales[q]
        return prod.sum(axis=2), grads
    d = z1[:, None, :] - z2[None, :, :]
    if kind == "cos":
        if p1 is not None or nd == 0:
            raise ValueError("a cosine factor takes no periods and needs at least one feature")
        arg = TWO_PI * d.sum(axis=2)
        for q in range(nd):
            grads[f"scales/{q}"] = TWO_PI * np.sin(arg) * d[:, :, q] / scales[q]
        return np.cos(arg), grads
    alpha = LD(factor["alpha"]) if kind == "rq" else None
    f, slope, dalpha = _stationary(kind, (d * d).sum(axis=2), alpha)
    for q in range(nd):
        grads[f"scales/{q}"] = slope * (-2 * d[:, :, q] ** 2 / scales[q])
    if p1 is not None:
        ncol = len(factor["cols"])
        dp = p1[:, None, :] - p2[None, :, :]
        for c in range(ncol):
            grads[f"periods/{c}"] = slope * 2 * (d[:, :, c] * dp[:, :, c] + d[:, :, ncol + c] * dp[:, :, ncol + c])
    if dalpha is not None:
        grads["alpha"] = dalpha
    return f, grads


def pair_gradients(spec, x1, x2):
    """{name: d k(x1_a, x2_b) / d theta, n1 x n2, long double} for every natural parameter, in the order of the spec."""
    n1, n2 = np.asarray(x1).shape[0], np.asarray(x2).shape[0]
    out = {}
    for t, term in enumerate(spec["terms"]):
        parts = [_factor(f, x1, x2) for f in term["factors"]]
        coef = LD(term["coef"])
        whole = np.ones((n1, n2), dtype=LD)
        for phi, _ in parts:
            whole = whole * phi
        out[f"coef/{t}"] = whole
        for i, (_, grads) in enumerate(parts):
            rest = np.full((n1, n2), coef, dtype=LD)
            for j, (phi, _) in enumerate(parts):
                if j != i:
                    rest = rest * phi
            for suffix, g in grads.items():
                what, _, index = suffix.partition("/")
                out[f"{what}/{t}/{i}" + (f"/{index}" if index else "")] = rest * g
    return out


def row_gradients(spec, x1, x2, v):
    """({name: d g_a / d theta}, {name: S_a}), arrays of n1 long doubles (module docstring)."""
    v = np.asarray(v, dtype=LD).reshape(-1)
    pairs = pair_gradients(spec, x1, x2)
    return {k: g @ v for k, g in pairs.items()}, {k: np.abs(g) @ np.abs(v) for k, g in pairs.items()}
