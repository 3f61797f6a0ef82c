"""Leave-one-out, blocked and purged blocked cross-validation at the tile edges and past one workgroup's reach: the entries
gpar_loo_dense*_score, gpar_cv_dense* and gpar_cv_gap_dense* of the C ABI at n = 1 / 2 / 15 / 16 / 17 / 31 / 32 / 33 (CVG_R = 16 rows of
cvg_band_kernel, the 32-wide tiles of the three weight and mirror kernels, the first odd cvg_ldp) and n = 255 / 256 / 257 (the 256 strided
partial sums of loo_sum_terms, the second block of columns of loo_rank2_kernel, the second pass of the `idx += 256` loops, more than 256
folds).  Value-only, one-call gradient and build + batched factorisation + finish form of every case, every buffer allocated here with a
sentinel in its padding and behind its last word.  Kernel and weights alternate with the parity of n (tests/test_ahead_gpu.py's habit);
the data recipe is tests/test_loo_gpu.py's (noise 0.05, jitter 1e-12).

The yardstick is tests/cv_reference.py in np.longdouble (held against deletion and the complex step by tests/test_cv_reference.py, which
also asserts from n and the index arrays alone what every case below is in the table for - REASONS).  Per case:

  parity      values and the log-determinant rtol 1e-10, means / variances rtol 1e-8 / atol 1e-10, W (lower triangle), 1/2 diag W and the
              parameter gradients (complex step) rtol 1e-6 / atol 1e-7 - the rules of tests/test_cv_gpu.py;
  ownership   value, log-determinant, means and variances: the device's distance from longdouble (largest error over the largest entry)
              is at most MARGIN = 8 times the float64 restatement's, with a floor of 8 n 2^-52 - the margin of tests/test_update_gpu.py:
              the device forms S^-1 and then products of it, a chain of roundings a few times longer than the restatement's;
              for W and the gradients the ratio is printed, not asserted;
  bits        finish form = one-call form, two calls = the same bits (`torch.equal`); `loose` (max_fold = 64 over folds of 5, 3, 1) gives
              the value, means and variances of `odd5` bit for bit;
  padding     every padding column and every word behind n comes back as the sentinel.

Every comparison prints its largest error over its tolerance and the ownership ratio (`-s`; collected in profiles/cv_large_parity.txt).
Worst lines of that run, per entry (error / tolerance; in brackets the largest device / float64 distance, asserted <= 8 for the first four,
printed only for W and the gradients):

    loo     value 7.7e-4 (1.4)   logdet 7.0e-6 (0.80)   mean 2.8e-4 (0.45)   var 2.9e-6 (1.0)   W 1.5e-4 (2.8)   gradient 1.5e-6 (8.1)
    cv      value 7.5e-4 (1.3)   logdet 7.0e-6 (0.80)   mean 2.8e-4 (1.1)    var 3.1e-6 (1.3)   W 1.7e-4 (2.3)   gradient 2.2e-6 (9.5)
    cv_gap  value 9.2e-4 (1.3)   logdet 7.0e-6 (0.80)   mean 3.2e-4 (3.0)    var 3.3e-6 (2.9)   W 2.2e-4 (6.4)   gradient 1.5e-5 (10.9)

No case exceeds the margin of 8 on an asserted quantity.
"""
import ctypes

import numpy as np
import pytest
import torch

from . import cv_reference as ref
from .test_cv import _fold_starts
from .test_loo_gpu import KERNELS, _library_grads, _library_kernel
from .test_loo_gpu import hip  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

EDGE, REACH = [1, 2, 15, 16, 17, 31, 32, 33], [255, 256, 257]
SIZES = EDGE + REACH
RULES = ["log", "crps", "se"]
CODES = {"log": 0, "crps": 1, "se": 2}
MARGIN = 8.0
SENTINEL = -7.0
TOL = {"value": (1e-10, 0.0), "logdet": (1e-10, 0.0), "mean": (1e-8, 1e-10), "var": (1e-8, 1e-10), "W": (1e-6, 1e-7), "half": (1e-6, 1e-7),
       "grads": (1e-6, 1e-7)}


# ---- the cases: inputs and index arrays, numpy alone (tests/test_cv_reference.py reads them too) --------------------------------------
def kernel_of(n):
    return "eq_linear" if n % 2 == 0 else "rq_periodic"


def _cycle(n, pattern):
    return _fold_starts(n, pattern)


def _odd5(n):
    return _cycle(n, [5, 3, 1])


# blocked: kind -> (fold offsets of n rows, the smallest n it is run at, max_fold handed over: None = the largest fold)
BLOCKED = {"ones": (lambda n: np.arange(n + 1), 1, None), "full": (lambda n: _cycle(n, [64]), 2, None), "sq": (lambda n: _cycle(n, [16, 17]), 33, None),
           "odd5": (_odd5, 15, None), "loose": (_odd5, 15, 64)}


def _gap(fold, gap, left=True, right=True):
    def extents(n):
        starts = _cycle(n, [fold])
        lo = np.maximum(starts[:-1] - gap, 0) if left else starts[:-1].copy()
        hi = np.minimum(starts[1:] + gap, n) if right else starts[1:].copy()
        return starts, lo, hi
    return extents


def _one_sided(left):
    def extents(n):   # folds of 5 rows (of one row where n has fewer than 15), 30 rows purged on one side only
        return _gap(5 if n >= 15 else 1, 30, left=left, right=not left)(n)
    return extents


def _plateau(n, fold=8, gap=20):
    """Blocks of fold + 2 gap = 48 rows around their fold, pushed inside [0, n): the first three folds share [0, 48), the last three
    [n - 48, n) (every fold the whole layer where n <= 48)."""
    starts = _cycle(n, [fold])
    width = min(n, fold + 2 * gap)
    lo = np.clip(starts[:-1] - gap, 0, n - width)
    return starts, lo, lo + width


# purged: kind -> (extents of n rows, the sizes it is run at)
PURGED = {"f1g0": (_gap(1, 0), SIZES), "f2g31": (_gap(2, 31), SIZES[1:]), "f64g0": (_gap(64, 0), SIZES[1:]), "f16g24": (_gap(16, 24), SIZES[2:]),
          "f17g5": (_gap(17, 5), SIZES[2:]), "left": (_one_sided(True), SIZES[1:]), "right": (_one_sided(False), SIZES[1:]),
          "plateau": (_plateau, SIZES[2:]), "short": (_gap(5, 40), [33])}

LOO_CASES = [(n, rule) for n in SIZES for rule in RULES]
BLOCKED_CASES = [(n, kind) for kind, (_, least, _) in BLOCKED.items() for n in SIZES if n >= least]
PURGED_CASES = [(n, kind) for kind, (_, sizes) in PURGED.items() for n in sizes]

# What each case is in the table for, by family and kind: reason -> the sizes at which it is claimed ("all": every size the kind runs at).
# tests/test_cv_reference.py asserts every claim from n, fold_start, hold_lo, hold_hi and max_fold alone.
ANY_KIND = {"ceil(n/256) = 2": [257], "last row block of 32 ragged": [n for n in SIZES if n % 32], "n odd, so cvg_ldp(n) = n + 1": [n for n in SIZES if n % 2]}
REASONS = {
    ("cv", "ones"): {"nfolds > 256": [257]},
    ("cv", "full"): {"m*m > 256 in some fold": [n for n in SIZES if n >= 17]},
    ("cv", "sq"): {"m*m > 256 in some fold": "all"},
    ("cv", "odd5"): {},
    ("cv", "loose"): {"max_fold exceeds the largest fold": "all"},
    ("cv_gap", "f1g0"): {"nfolds > 256": [257]},
    ("cv_gap", "f2g31"): {"m*m > 256 in some fold": [n for n in SIZES if n >= 17], "2 max_hold - 1 > n": [n for n in SIZES if 2 <= n <= 33],
                          "some H equals its neighbour's": [n for n in SIZES if 15 <= n <= 33]},
    ("cv_gap", "f64g0"): {"m*m > 256 in some fold": [n for n in SIZES if n >= 17]},
    ("cv_gap", "f16g24"): {"m*m > 256 in some fold": [n for n in SIZES if n >= 17], "some H equals its neighbour's": [17, 31, 32, 33],
                           "2 max_hold - 1 > n": EDGE[2:]},
    ("cv_gap", "f17g5"): {"m*m > 256 in some fold": [n for n in SIZES if n >= 17]},
    ("cv_gap", "left"): {"m*m > 256 in some fold": [n for n in SIZES if n >= 17]},
    ("cv_gap", "right"): {"m*m > 256 in some fold": [n for n in SIZES if n >= 17]},
    ("cv_gap", "plateau"): {"some H equals its neighbour's": "all", "m*m > 256 in some fold": [n for n in SIZES if n >= 17],
                            "2 max_hold - 1 > n": EDGE[2:]},
    ("cv_gap", "short"): {"2 max_hold - 1 > n": "all", "some H equals its neighbour's": "all"},
}


def claimed(family, kind, n):
    """The reasons the case (family, kind, n) is in the table for."""
    out = [reason for reason, sizes in ANY_KIND.items() if n in sizes]
    for reason, sizes in REASONS.get((family, kind), {}).items():
        if sizes == "all" or n in sizes:
            out.append(reason)
    return out


def geometry(family, kind, n):
    """(fold_start, hold_lo, hold_hi, max_fold) of a case - for "loo" folds of one row; for "cv" the blocks are the folds."""
    if family == "loo":
        starts = np.arange(n + 1)
        return starts, starts[:-1], starts[1:], 1
    if family == "cv":
        make, _, bound = BLOCKED[kind]
        starts = make(n)
        return starts, starts[:-1], starts[1:], int(np.diff(starts).max()) if bound is None else bound
    starts, lo, hi = PURGED[kind][0](n)
    return starts, lo, hi, int((hi - lo).max())


_INPUTS = {}


def inputs(n):
    """x, y, noise by the recipe of tests/test_loo_gpu.py's `_case` (the kernel and the weights by the parity of n), the function
    (theta, noise) -> S and what every case on these rows shares: the longdouble and the float64 factorisation and one complex
    factorisation per kernel parameter (the complex step).  Computed once, never modified."""
    if n not in _INPUTS:
        name, weighted = kernel_of(n), n % 2 == 1
        kfun, theta = KERNELS[name]
        rng = np.random.default_rng(1000 * n + weighted)
        x = rng.uniform(0.0, 1.0, (n, 3))
        y = np.sin(5.0 * x[:, 0]) + np.cos(3.0 * x[:, 1]) + 0.5 * x[:, 2] + 0.2 * rng.standard_normal(n)
        noise = 0.05 / rng.uniform(0.5, 2.0, n) if weighted else np.full(n, 0.05)

        def S(th, d):   # (longdouble noise: the whole matrix in longdouble)
            xx = x.astype(np.longdouble) if np.asarray(d).dtype == np.longdouble else x
            return kfun(xx, th) + np.diag(d) + 1e-12 * np.eye(n)

        long = np.longdouble
        facs = {"long": ref.factor(S(theta.astype(long), noise.astype(long)), y.astype(long)), "double": ref.factor(S(theta, noise), y)}
        dK = []
        for j in range(theta.size):
            moved = theta.astype(complex)
            moved[j] += 1e-30j
            facs[j] = ref.factor(S(moved, noise), y)
            dK.append(kfun(x, moved).imag / 1e-30)
        _INPUTS[n] = dict(n=n, name=name, x=x, y=y, noise=noise, theta=theta, facs=facs, dK=dK)
    return _INPUTS[n]


def _form(family, inp, extents, rule, which, weights=True):
    starts, lo, hi = extents
    fac = inp["facs"][which]
    y = inp["y"].astype(np.longdouble) if which == "long" else inp["y"]
    if family == "loo":
        return ref.loo(None, y, rule, fac=fac, weights=weights)
    if family == "cv":
        return ref.blocked(None, y, starts, fac=fac, weights=weights)
    return ref.purged(None, y, starts, lo, hi, fac=fac, weights=weights)


_CASES = {}


def case(family, kind, n, rule="log"):
    """Inputs, geometry and the references of one case, computed once and shared (never modified): the longdouble yardstick ("value",
    "logdet", "mean", "var", "W", "half", "grads" - the gradients by the complex step) and the float64 evaluation of the same closed form
    under "double"."""
    key = (family, kind, n, rule)
    if key not in _CASES:
        inp = inputs(n)
        starts, lo, hi, bound = geometry(family, kind, n)
        out = dict(inp, family=family, kind=kind, rule=rule, starts=starts, lo=lo, hi=hi, bound=bound)
        for which in ("long", "double"):
            value, logdet, mean, var, W = _form(family, inp, (starts, lo, hi), rule, which)
            W = W.astype(float)
            got = dict(value=float(value), logdet=float(logdet), mean=mean.astype(float), var=var.astype(float), W=W, half=0.5 * np.diag(W),
                       grads=np.array([0.5 * np.sum(W * d) for d in inp["dK"]]))
            if which == "long":
                out.update(got)
            else:
                out["double"] = got
        theta = inp["theta"]
        out["grads"] = np.array([np.imag(_form(family, inp, (starts, lo, hi), rule, j, weights=False)[0]) / 1e-30 for j in range(theta.size)])
        _CASES[key] = out
    return _CASES[key]


def distance(got, want, scale=0.0):
    """Largest error over the largest entry of the yardstick (or `scale`, where that is larger: a mean is y minus a correction, and its
    rounding is that of y - from the prior, at n = 1, it is 0)."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    return float(np.max(np.abs(got - want)) / max(np.max(np.abs(want)), scale))


def over_tolerance(what, got, want):
    """Largest error over the parity tolerance of `what`."""
    rtol, atol = TOL[what]
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    return float(np.max(np.abs(got - want) / (atol + rtol * np.abs(want))))


# ---- one C ABI call with every buffer allocated here -------------------------------------------------------------------------------------
def _matrix(rows, cols, extra, dev, fill=SENTINEL):
    base = torch.full((rows, cols + extra), fill, dtype=torch.float64, device=dev)
    return base[:, :cols], base


def _vector(n, dev, fill=SENTINEL):
    base = torch.full((n + 8,), fill, dtype=torch.float64, device=dev)
    return base[:n], base


def raw_call(hip, c, mode, pad=0, incy=1, extents=None):  # noqa: F811
    """One call of the case's entry: mode "value", "grad" or "finish" (build + batched factorisation + the finish form), leading dimensions
    widened by `pad` (and to an even number), y strided by `incy`.  `extents`: (fold_start, hold_lo, hold_hi, bound) handed over as they
    are, unchecked, in place of the case's.  Every output starts as SENTINEL.  Returns the return code, the views and the whole buffers."""
    from gpar_amd import _lib
    from gpar_amd import hip as lib

    family, n, name = c["family"], c["n"], c["name"]
    ck = hip.compile(_library_kernel(name, KERNELS[name][1]), 3)
    dev = torch.device("cuda:0")
    cdll, nacc = _lib.load(), _lib.GRAD_NACC
    starts, lo, hi, bound = (c["starts"], c["lo"], c["hi"], c["bound"]) if extents is None else extents
    up = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=dev)   # noqa: E731
    arrays = (up(starts), up(lo), up(hi))
    nfolds = len(starts) - 1
    if family == "loo":
        extra, ws, wsk = (CODES[c["rule"]],), _lib.WS_LOO, 0
    elif family == "cv":
        extra, ws, wsk = (arrays[0].data_ptr(), nfolds, bound), _lib.WS_CV, bound
    else:
        extra, ws, wsk = (arrays[0].data_ptr(), arrays[1].data_ptr(), arrays[2].data_ptr(), nfolds, bound), _lib.WS_CV_GAP, bound
    x, _ = _matrix(n, 3, pad, dev)
    x.copy_(torch.tensor(c["x"]))
    ybuf = torch.zeros(n, incy, dtype=torch.float64, device=dev)
    ybuf[:, 0] = torch.tensor(c["y"])
    nz = torch.tensor(c["noise"], device=dev)
    bases = {}
    z, bases["z"] = _matrix(n, 3, pad, dev)
    zd, bases["zd"] = _matrix(n, 3, pad, dev, fill=0.0)
    A, bases["A"] = _matrix(n + 1, n + 1, pad + (n + 1) % 2, dev)
    X, bases["X"] = _matrix(n, n, pad + n % 2, dev)
    W, bases["W"] = _matrix(n, n, pad + n % 2, dev)
    grad = mode != "value"
    nblocks = max(1, min(((n + 63) // 64) * ((n + 63) // 64 + 1) // 2, 1024))
    nvec = int(cdll.gpar_workspace_doubles(ws, n, int(grad), wsk))
    assert nvec > 0
    vec = torch.empty(nvec, dtype=torch.float64, device=dev)
    work = torch.empty(nblocks * nacc, dtype=torch.float64, device=dev)
    alpha, bases["alpha"] = _vector(n, dev)
    out, bases["out"] = _vector(2 + nacc if grad else 2, dev)
    half, bases["half"] = _vector(n, dev)
    mean, bases["mean"] = _vector(n, dev)
    var, bases["var"] = _vector(n, dev)
    info = torch.zeros(2, dtype=torch.int32, device=dev)
    stream = lib.stream_ptr(dev)
    ld = lib._ld
    head = (ctypes.byref(ck.fspec), ctypes.byref(ck.kspec), x.data_ptr(), n, ld(x), ybuf.data_ptr(), incy)
    entry = {"loo": "gpar_loo_dense{}_score", "cv": "gpar_cv_dense{}", "cv_gap": "gpar_cv_gap_dense{}"}[family]
    entry = getattr(cdll, entry.format({"value": "", "grad": "_grad", "finish": "_grad_finish"}[mode]))
    if mode == "value":
        rc = entry(*head, nz.data_ptr(), 1e-12, z.data_ptr(), ld(z), A.data_ptr(), ld(A), X.data_ptr(), ld(X), W.data_ptr(), ld(W), vec.data_ptr(),
                   out.data_ptr(), mean.data_ptr(), var.data_ptr(), *extra, info.data_ptr(), 0, stream)
    elif mode == "grad":
        rc = entry(*head, nz.data_ptr(), 1e-12, z.data_ptr(), zd.data_ptr(), ld(z), A.data_ptr(), ld(A), X.data_ptr(), ld(X), W.data_ptr(), ld(W),
                   alpha.data_ptr(), vec.data_ptr(), work.data_ptr(), nblocks, out.data_ptr(), half.data_ptr(), mean.data_ptr(), var.data_ptr(),
                   *extra, info.data_ptr(), 0, stream)
    else:
        logdet = torch.zeros(1, dtype=torch.float64, device=dev)
        _lib.check(cdll.gpar_logpdf_dense_build(*head, nz.data_ptr(), 1e-12, z.data_ptr(), ld(z), A.data_ptr(), ld(A), logdet.data_ptr(), info.data_ptr(),
                                                stream), "build")
        _lib.check(cdll.gpar_potrf_batch(A.data_ptr(), 1, 0, n + 1, n, ld(A), logdet.data_ptr(), info.data_ptr(), 0, stream), "potrf_batch")
        rc = entry(*head, z.data_ptr(), zd.data_ptr(), ld(z), A.data_ptr(), ld(A), logdet.data_ptr(), info.data_ptr(), X.data_ptr(), ld(X), W.data_ptr(),
                   ld(W), alpha.data_ptr(), vec.data_ptr(), work.data_ptr(), nblocks, out.data_ptr(), half.data_ptr(), mean.data_ptr(), var.data_ptr(),
                   *extra, info[1:].data_ptr(), stream)
    torch.cuda.synchronize()
    views = dict(z=z, zd=zd, A=A, X=X, W=W, alpha=alpha, out=out, half=half, mean=mean, var=var)
    return dict(views, rc=rc, info=info.cpu().tolist(), ck=ck, bases=bases, mode=mode)


def padding_untouched(got):
    """Every padding column of the matrices and every word behind the last one of the vectors still holds what it went in with."""
    for key, base in got["bases"].items():
        view = got[key]
        fill = 0.0 if key == "zd" else SENTINEL
        tail = base[:, view.shape[1]:] if base.dim() == 2 else base[view.shape[0]:]
        assert bool((tail == fill).all()), key
    return True


def _own(label, what, got, c):
    """Check 3: the device's distance from longdouble against the float64 restatement's."""
    floor = c["n"] * 2.0 ** -52
    scale = float(np.max(np.abs(c["y"]))) if what == "mean" else 0.0
    theirs, ours = distance(c["double"][what], c[what], scale), distance(got, c[what], scale)
    ratio = ours / max(theirs, floor)
    print(f"cv_large parity | {label} | {what} | error / tolerance {over_tolerance(what, got, c[what]):.3g} | device / float64 distance {ratio:.3g}")
    assert ratio <= MARGIN, (label, what, ours, theirs)


def _printed(label, what, got, c):
    ratio = distance(got, c[what]) / max(distance(c["double"][what], c[what]), c["n"] * 2.0 ** -52)
    print(f"cv_large parity | {label} | {what} | error / tolerance {over_tolerance(what, got, c[what]):.3g} | device / float64 distance {ratio:.3g} (printed only)")


def check(hip, label, c, got):  # noqa: F811
    """Checks 1, 2, 3 and 5 of one call."""
    n, grad = c["n"], got["mode"] != "value"
    assert got["rc"] == 0 and got["info"] == [0, 0], (label, got["rc"], got["info"])
    out = got["out"].cpu().numpy()
    mean, var = got["mean"].cpu().numpy(), got["var"].cpu().numpy()
    for what, mine in (("value", out[0]), ("logdet", out[1]), ("mean", mean), ("var", var)):
        _own(label, what, mine, c)
        np.testing.assert_allclose(mine, c[what], rtol=TOL[what][0], atol=TOL[what][1], err_msg=f"{label} {what}")
    if grad:
        il = np.tril_indices(n)
        W = got["W"].cpu().numpy()
        sym = np.tril(W) + np.tril(W, -1).T
        half = got["half"].cpu().numpy()
        grads = _library_grads(c["name"], hip._grads_from_moments(got["ck"], out[2:], 0.5))
        for what, mine in (("W", sym), ("half", half), ("grads", grads)):
            _printed(label, what, mine, c)
        np.testing.assert_allclose(W[il], c["W"][il], rtol=1e-6, atol=1e-7, err_msg=f"{label} W")
        np.testing.assert_allclose(half, c["half"], rtol=1e-6, atol=1e-7, err_msg=f"{label} half diag W")
        np.testing.assert_allclose(half, 0.5 * np.diag(W), rtol=0, atol=0)
        np.testing.assert_allclose(grads, c["grads"], rtol=1e-6, atol=1e-7, err_msg=f"{label} gradients")
    assert padding_untouched(got)


def same_bits(a, b, n, keys=("out", "half", "mean", "var")):
    il = torch.tril_indices(n, n)
    for key in keys:
        assert torch.equal(a[key], b[key]), key
    assert torch.equal(a["W"][il[0], il[1]], b["W"][il[0], il[1]])


def three_entries(hip, label, c, pad=0, incy=1):  # noqa: F811
    """Value-only, one-call gradient (twice: the same bits) and finish form (the bits of the one-call form) of one case, each checked."""
    calls = {mode: raw_call(hip, c, mode, pad=pad, incy=incy) for mode in ("value", "grad", "finish")}
    for mode, got in calls.items():
        check(hip, f"{label} {mode}", c, got)
    again = raw_call(hip, c, "grad", pad=pad, incy=incy)
    same_bits(calls["grad"], again, c["n"])
    same_bits(calls["grad"], calls["finish"], c["n"])
    return calls


def _against(label, got, want, n):
    """One entry against another one's numbers under the parity rules."""
    a, b = got["out"].cpu().numpy(), want["out"].cpu().numpy()
    np.testing.assert_allclose(a[:2], b[:2], rtol=1e-10, err_msg=label)
    np.testing.assert_allclose(got["mean"].cpu().numpy(), want["mean"].cpu().numpy(), rtol=1e-8, atol=1e-10, err_msg=label)
    np.testing.assert_allclose(got["var"].cpu().numpy(), want["var"].cpu().numpy(), rtol=1e-8, atol=1e-10, err_msg=label)
    il = np.tril_indices(n)
    np.testing.assert_allclose(got["W"].cpu().numpy()[il], want["W"].cpu().numpy()[il], rtol=1e-6, atol=1e-7, err_msg=label)
    np.testing.assert_allclose(got["half"].cpu().numpy(), want["half"].cpu().numpy(), rtol=1e-6, atol=1e-7, err_msg=label)
    np.testing.assert_allclose(a[2:], b[2:], rtol=1e-6, atol=1e-7, err_msg=label)


# ---- leave-one-out -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rule", LOO_CASES, ids=lambda v: str(v))
def test_leave_one_out_three_entries_under_the_three_rules(hip, n, rule):  # noqa: F811
    c = case("loo", None, n, rule)
    three_entries(hip, f"loo n={n} {rule}", c)
    if n == 257:   # widened leading dimensions, strided observations
        three_entries(hip, f"loo n={n} {rule} padded", c, pad=5, incy=3)


# ---- blocked -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", BLOCKED_CASES, ids=lambda v: str(v))
def test_blocked_three_entries_over_the_fold_generators(hip, n, kind):  # noqa: F811
    c = case("cv", kind, n)
    calls = three_entries(hip, f"cv n={n} {kind}", c)
    if kind == "ones":   # folds of one row: the leave-one-out entry's numbers
        _against(f"cv n={n} ones against loo", calls["grad"], raw_call(hip, case("loo", None, n), "grad"), n)
    if kind == "loose":
        # The arithmetic of a fold does not depend on max_fold - it moves the second LDS tile and the rows of Rm alone -, so the value, the
        # means and the variances of `odd5` come back bit for bit, in both forms; W goes through the same kernels on the same numbers
        # too and is held to the parity rule the issue asks for.
        tight = case("cv", "odd5", n)
        assert c["bound"] == 64 and tight["bound"] == 5 and np.array_equal(c["starts"], tight["starts"])
        for mode in ("value", "grad"):
            want = raw_call(hip, tight, mode)
            assert np.array_equal(calls[mode]["out"].cpu().numpy()[:2], want["out"].cpu().numpy()[:2]), mode
            assert np.array_equal(calls[mode]["mean"].cpu().numpy(), want["mean"].cpu().numpy()), mode
            assert np.array_equal(calls[mode]["var"].cpu().numpy(), want["var"].cpu().numpy()), mode
        _against(f"cv n={n} loose against odd5", calls["grad"], want, n)


# ---- purged --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", PURGED_CASES, ids=lambda v: str(v))
def test_purged_three_entries_over_the_extents(hip, n, kind):  # noqa: F811
    c = case("cv_gap", kind, n)
    calls = three_entries(hip, f"cv_gap n={n} {kind}", c)
    if kind == "f1g0":   # folds of one row, nothing purged: the leave-one-out entry's numbers
        _against(f"cv_gap n={n} f1g0 against loo", calls["grad"], raw_call(hip, case("loo", None, n), "grad"), n)
    if kind == "f64g0":   # blocks equal to the folds: the blocked entry's numbers
        _against(f"cv_gap n={n} f64g0 against cv", calls["grad"], raw_call(hip, case("cv", "full", n), "grad"), n)
