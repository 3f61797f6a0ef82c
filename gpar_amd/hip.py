"""Thin torch-tensor front end of the C ABI: tensors in, raw device pointers across the boundary.

PyTorch is used only as the device-memory allocator and stream provider; every numerical operation here is a
call into libgpar_hip.so on the tensor's `data_ptr()`.  All matrices are float64, row-major with unit inner
stride (`stride(1) == 1`); the leading dimension is `stride(0)`.
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from .heldout import (Folds, Loo, Origins, Purged, Window, fold_offsets, hold_extents, horizon_weight_array, origin_array,  # noqa: F401
                      origins_array, upload_folds, upload_hold, upload_origin, upload_origins, upload_window, window_arrays)

__all__ = [
    "stream_ptr",
    "alloc_matrix",
    "featurize",
    "gram",
    "gram_diag",
    "periodogram",
    "rff_apply",
    "gram_apply_groups",
    "pivoted_chol",
    "chol_drop_leading",
    "chol_append_",
    "potrf_",
    "trsm_rlt_",
    "trsm_rln_",
    "gemm",
    "dot",
    "gemv_t",
    "rownorm2",
    "pack_lower",
    "unpack_lower_",
    "randn",
    "sample_stats",
    "trmv_lower",
    "gram_grad",
    "gram_grad_cross",
    "gram_grad_rows",
    "gram_input_grad",
    "chol_inverse",
]


def _check_mat(a, name):
    if a.dtype != torch.float64 or not a.is_cuda:
        raise TypeError(f"{name} must be a float64 tensor on the GPU (got {a.dtype} on {a.device})")
    if a.dim() == 2:
        if a.shape[1] > 1 and a.stride(1) != 1:
            raise ValueError(f"{name} must have unit inner stride")
    elif a.dim() != 1:
        raise ValueError(f"{name} must be a vector or a matrix")


def _ld(a):
    if a.dim() == 1:
        return 1
    # a single-row matrix may report any stride(0); make it safe for the kernels' index math
    return max(int(a.stride(0)), int(a.shape[1]), 1) if a.shape[0] > 1 else max(int(a.shape[1]), 1)


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def alloc_matrix(rows, cols, device, zero=False):
    """rows x cols view into a buffer whose leading dimension is padded to a multiple of 16 doubles (128-byte
    rows: every row start is aligned for the 16-byte vector paths and full-line stores)."""
    ld = max(16, (cols + 15) // 16 * 16)
    buf = (torch.zeros if zero else torch.empty)((max(rows, 1), ld), dtype=torch.float64, device=device)
    return buf[:rows, :cols]


def featurize(ck, x):
    """z = features(x) for a CompiledKernel `ck`; x: n x width."""
    _check_mat(x, "x")
    lib = _lib.load()
    n = x.shape[0]
    z = alloc_matrix(n, max(ck.dz, 1), x.device)
    if ck.dz == 0:
        z.zero_()
        return z
    _lib.check(
        lib.gpar_featurize(ctypes.byref(ck.fspec), x.data_ptr(), n, _ld(x), z.data_ptr(), _ld(z), stream_ptr(x.device)),
        "gpar_featurize",
    )
    return z


def _dense_layer_args(x, y, noise_diag):
    """(n, device, flat y, pointer of the noise diagonal or None) of one dense layer, checked (the noise vector is returned too: the
    caller keeps it alive across the call)."""
    _check_mat(x, "x")
    n = x.shape[0]
    y = y.reshape(-1)
    if y.numel() != n or y.dtype != torch.float64 or not y.is_cuda:
        raise ValueError("y must hold one fp64 device value per row of x")
    if noise_diag is not None:
        noise_diag = noise_diag.reshape(-1).contiguous()
        if noise_diag.numel() != n:
            raise ValueError("noise_diag must hold one value per row of x")
    return n, x.device, y, noise_diag


def _potrf_flags(lookahead, fused):
    return (0 if lookahead else _lib.POTRF_NO_LOOKAHEAD) | (0 if fused else _lib.POTRF_UNFUSED)


def logpdf_dense(ck, x, y, noise_diag, jitter, lookahead=True, fused=True):
    """log N(y; 0, k(x, x) + diag(noise_diag) + jitter I) in one library call (gpar_logpdf_dense): returns
    (value, logdet, info) as one-element device tensors and the (n + 1) x (n + 1) factor buffer."""
    lib = _lib.load()
    n, dev, y, noise_diag = _dense_layer_args(x, y, noise_diag)
    z = alloc_matrix(n, max(ck.dz, 1), dev)
    A = alloc_matrix(n + 1, n + 1, dev)
    words = torch.empty(2, dtype=torch.float64, device=dev)   # value, logdet
    info = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(
        lib.gpar_logpdf_dense(
            ctypes.byref(ck.fspec), ctypes.byref(ck.kspec), x.data_ptr(), n, _ld(x), y.data_ptr(), int(y.stride(0)),
            None if noise_diag is None else noise_diag.data_ptr(), float(jitter), z.data_ptr(), _ld(z), A.data_ptr(), _ld(A),
            words[1:].data_ptr(), info.data_ptr(), words.data_ptr(), _potrf_flags(lookahead, fused), stream_ptr(dev),
        ),
        "gpar_logpdf_dense",
    )
    return words[0], words[1:], info, A


def score_code(score):
    """GPAR_SCORE_* of a scoring rule's name ("log", "crps", "se"); anything else is a ValueError."""
    if score not in _lib.SCORES:
        raise ValueError('score must be "log", "crps" or "se"')
    return _lib.SCORES[score]


def held_out_trailing(scheme, n, dev, values, score):
    """What a scheme's entries take between the variances and the info word: the scheme's uploaded arrays by their pointers and its
    counts as they are (`scheme.device`), the K unweighted `values` where it scores K horizons, the scoring rule where it takes one."""
    args = tuple(a.data_ptr() if isinstance(a, torch.Tensor) else a for a in scheme.device(n, dev))
    if scheme.horizons:
        args += (values.data_ptr(),)
    return args + ((score_code(score),) if scheme.takes_score else ())


def held_out_call(lib, scheme, grad, ck, p, n, jitter, nblocks, trailing, flags, stream):
    """The ONE place a dense layer's objective entry is called - `scheme` None: gpar_logpdf_dense_grad; otherwise `scheme.entry(grad)` -
    and its argument list assembled, from the table `p` of pointers and leading dimensions (x ldx y incy noise z ldz A lda out info; mean
    var vec with a scheme; zd X ldxw W ldw alpha work half with `grad`; X ldxw T ldt for a value form on K^-1), `trailing`
    (`held_out_trailing`), the factorisation `flags` (not passed where nothing is factored whole) and the raw `stream`."""
    name = "gpar_logpdf_dense_grad" if scheme is None else scheme.entry(grad)
    factored = scheme is None or scheme.factored
    head = (ctypes.byref(ck.fspec), ctypes.byref(ck.kspec), p["x"], n, p["ldx"], p["y"], p["incy"], p["noise"], jitter, p["z"])
    vec = () if scheme is None else (p["vec"],)
    tail = (*(() if scheme is None else (p["mean"], p["var"], *trailing)), p["info"], *((flags,) if factored else ()), stream)
    if grad:
        mats = (p["X"], p["ldxw"], p["W"], p["ldw"], p["alpha"]) if factored else (p["W"], p["ldw"])
        args = (*head, p["zd"], p["ldz"], p["A"], p["lda"], *mats, *vec, p["work"], nblocks, p["out"], p["half"], *tail)
    else:
        mats = (p["X"], p["ldxw"], p["T"], p["ldt"]) if scheme.inverse else ()
        args = (*head, p["ldz"], p["A"], p["lda"], *mats, *vec, p["out"], *tail)
    _lib.check(getattr(lib, name)(*args), name)


def held_out_dense(scheme, ck, x, y, noise_diag, jitter, *, grad, periodic=False, score="log", lookahead=True, fused=True):
    """One dense layer's objective under a held-out scheme (`heldout`; None: the log marginal likelihood, `grad` alone) in one library
    call: all allocation and the one call for every family, the value form and - `grad` - the one that leaves the gradient's ingredients
    too.  `score`: the scoring rule of the families that take one.  Returns a dict: out = [value, logdet] and with `grad` the GRAD_NACC
    moment sums behind them; mean, var (n, or K x n for K horizons) and values (the K unweighted values, else None); info; with `grad`
    half = 1/2 diag(W), W (lower triangle) and A, the (n + 1) x (n + 1) factor buffer (a window factors nothing whole: no factor)."""
    lib = _lib.load()
    n, dev, y, noise_diag = _dense_layer_args(x, y, noise_diag)
    k = None if scheme is None else scheme.horizons
    factored = scheme is None or scheme.factored
    new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)   # noqa: E731
    dz, nacc = max(ck.dz, 1), _lib.GRAD_NACC
    z = alloc_matrix(n, dz, dev)
    A = alloc_matrix(n + 1, n + 1, dev)
    out = new(2 + nacc if grad else 2)
    values = new(k) if k else None
    trailing = () if scheme is None else held_out_trailing(scheme, n, dev, values, score)   # (uploads: beyond `fits()` the ValueError, first)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    if grad and not k:   # 1/2 diag W and - but for "mll" - the means and variances: the rows of one buffer
        half, mean, var = (*new(1, n), None, None) if scheme is None else new(3, n)
    else:                # the moments (K x n each for K horizons), 1/2 diag W apart from them
        half, (mean, var) = new(n) if grad else None, new(2, *((k, n) if k else (n,)))
    p = dict(x=x.data_ptr(), ldx=_ld(x), y=y.data_ptr(), incy=int(y.stride(0)), noise=None if noise_diag is None else noise_diag.data_ptr(),
             z=z.data_ptr(), ldz=_ld(z), A=A.data_ptr(), lda=_ld(A), out=out.data_ptr(), info=info.data_ptr())
    if scheme is not None:
        p.update(mean=mean.data_ptr(), var=var.data_ptr())
    W, nblocks = None, 0
    if grad:
        zd = alloc_matrix(n, dz, dev, zero=True) if periodic else None
        W = alloc_matrix(n, n, dev)
        nt = (n + 63) // 64
        nblocks = max(1, min(nt * (nt + 1) // 2, 1024))
        # gradient partials, alpha, the scheme's vector workspace (at an even offset: "ahead" keeps a matrix in it; a window has no alpha)
        nalpha = n + (n & 1) if factored else 0
        work = new(nblocks * nacc + nalpha + (0 if scheme is None else scheme.workspace(lib, n, 1)))
        p.update(zd=None if zd is None else zd.data_ptr(), W=W.data_ptr(), ldw=_ld(W), alpha=work[nblocks * nacc:].data_ptr(),
                 vec=work[nblocks * nacc + nalpha:].data_ptr(), work=work.data_ptr(), half=half.data_ptr())
    else:
        vec = new(scheme.workspace(lib, n, 0))
        p.update(vec=vec.data_ptr())
    if factored and (grad or scheme.inverse):   # K^-1; the value forms that work on it take a scratch matrix beside it
        X = alloc_matrix(n, n, dev)
        p.update(X=X.data_ptr(), ldxw=_ld(X))
        if not grad:
            T = alloc_matrix(n, n, dev)
            p.update(T=T.data_ptr(), ldt=_ld(T))
    held_out_call(lib, scheme, grad, ck, p, n, float(jitter), nblocks, trailing, _potrf_flags(lookahead, fused), stream_ptr(dev))
    return dict(out=out, values=values, half=half, mean=mean, var=var, info=info, A=A, W=W)


def logpdf_dense_grad(ck, x, y, noise_diag, jitter, periodic, lookahead=True, fused=True):
    """One dense layer's log marginal likelihood AND its gradient ingredients in one library call (gpar_logpdf_dense_grad).
    Returns (out, half_diag, info, A): out = [value, logdet, GRAD_NACC moment sums] (device), half_diag = 1/2 diag(W) (device, n),
    info word, the (n + 1) x (n + 1) factor buffer."""
    r = held_out_dense(None, ck, x, y, noise_diag, jitter, grad=True, periodic=periodic, lookahead=lookahead, fused=fused)
    return r["out"], r["half"], r["info"], r["A"]


def _value_form(scheme, ck, x, y, noise_diag, jitter, **kw):
    """(out, [the K values,] mean, var, info) of a scheme's value entry."""
    r = held_out_dense(scheme, ck, x, y, noise_diag, jitter, grad=False, **kw)
    return (r["out"], *((r["values"],) if scheme.horizons else ()), r["mean"], r["var"], r["info"])


def _grad_form(scheme, ck, x, y, noise_diag, jitter, periodic, **kw):
    """(out, [the K values,] half_diag, mean, var, info, [A,] W) of a scheme's gradient entry."""
    r = held_out_dense(scheme, ck, x, y, noise_diag, jitter, grad=True, periodic=periodic, **kw)
    return (r["out"], *((r["values"],) if scheme.horizons else ()), r["half"], r["mean"], r["var"], r["info"],
            *((r["A"],) if scheme.factored else ()), r["W"])


def loo_dense(ck, x, y, noise_diag, jitter, lookahead=True, fused=True, score="log"):
    """Leave-one-out value, means and variances of one dense layer in one library call (gpar_loo_dense_score; no inverse is formed).
    `score`: "log", "crps" or "se" - the rule every held-out entry is scored by; the value is one to maximise under each.
    Returns (out, loo_mean, loo_var, info): out = [value, logdet] (device), the n predictive means and variances (device), info word."""
    return _value_form(Loo(), ck, x, y, noise_diag, jitter, lookahead=lookahead, fused=fused, score=score)


def loo_dense_grad(ck, x, y, noise_diag, jitter, periodic, lookahead=True, fused=True, score="log"):
    """One dense layer's leave-one-out value AND its gradient ingredients in one library call (gpar_loo_dense_grad_score).  Returns
    (out, half_diag, loo_mean, loo_var, info, A, W): out = [value, logdet, GRAD_NACC moment sums] (device), half_diag = 1/2 diag(W),
    the n predictive means and variances, info word, the (n + 1) x (n + 1) factor buffer, the weights W (lower triangle)."""
    return _grad_form(Loo(), ck, x, y, noise_diag, jitter, periodic, lookahead=lookahead, fused=fused, score=score)


def cv_dense(ck, x, y, noise_diag, jitter, fold_start, lookahead=True, fused=True):
    """Blocked cross-validation value, means and marginal variances of one dense layer in one library call (gpar_cv_dense).
    `fold_start`: the nfolds + 1 row offsets of the contiguous folds (host sequence, the triple `upload_folds` returns, or a `Folds`).
    Returns (out, cv_mean, cv_var, info): out = [value, logdet] (device), the n predictive means and variances (device), info word."""
    return _value_form(Folds.of(fold_start, x.shape[0]), ck, x, y, noise_diag, jitter, lookahead=lookahead, fused=fused)


def cv_dense_grad(ck, x, y, noise_diag, jitter, periodic, fold_start, lookahead=True, fused=True):
    """One dense layer's blocked cross-validation value AND its gradient ingredients in one library call (gpar_cv_dense_grad).
    `fold_start` as for `cv_dense`.  Returns (out, half_diag, cv_mean, cv_var, info, A, W), laid out as `loo_dense_grad` returns them."""
    return _grad_form(Folds.of(fold_start, x.shape[0]), ck, x, y, noise_diag, jitter, periodic, lookahead=lookahead, fused=fused)


def cv_gap_dense(ck, x, y, noise_diag, jitter, fold_start, hold, lookahead=True, fused=True):
    """Purged blocked cross-validation value, means and marginal variances of one dense layer in one library call (gpar_cv_gap_dense).
    `fold_start`: the offsets of the scored folds; `hold`: the pair (hold_lo, hold_hi) of the blocks the folds are not predicted from
    (`hold_extents`); or `fold_start` the five-tuple `upload_hold` returns (or a `Purged`) and `hold` None.  Returns what `cv_dense` returns."""
    return _value_form(Purged.of(fold_start, hold, x.shape[0]), ck, x, y, noise_diag, jitter, lookahead=lookahead, fused=fused)


def cv_gap_dense_grad(ck, x, y, noise_diag, jitter, periodic, fold_start, hold, lookahead=True, fused=True):
    """One dense layer's purged blocked cross-validation value AND its gradient ingredients in one library call (gpar_cv_gap_dense_grad).
    `fold_start`, `hold` as for `cv_gap_dense`.  Returns (out, half_diag, cv_mean, cv_var, info, A, W), laid out as `loo_dense_grad` returns them."""
    return _grad_form(Purged.of(fold_start, hold, x.shape[0]), ck, x, y, noise_diag, jitter, periodic, lookahead=lookahead, fused=fused)


def ahead_dense(ck, x, y, noise_diag, jitter, origin, lookahead=True, fused=True, score="log"):
    """Rolling-origin forecast value, means and variances of one dense layer in one library call (gpar_ahead_dense_score): row r predicted from
    rows 0 ... origin[r] - 1, origin[r] = -1 not scored (NaN in its mean and variance).  `origin`: a host sequence of n ints, the device
    tensor `upload_origin` returns, or an `Origins`.  Returns (out, mean, var, info): out = [value, logdet] (device), means and variances
    (device), info."""
    return _value_form(Origins.of(origin, x.shape[0]), ck, x, y, noise_diag, jitter, lookahead=lookahead, fused=fused, score=score)


def ahead_dense_grad(ck, x, y, noise_diag, jitter, periodic, origin, lookahead=True, fused=True, score="log"):
    """One dense layer's rolling-origin forecast value AND its gradient ingredients in one library call (gpar_ahead_dense_grad_score).  `origin`
    and `score` as for `ahead_dense`.  Returns (out, half_diag, mean, var, info, A, W), laid out as `loo_dense_grad` returns them."""
    return _grad_form(Origins.of(origin, x.shape[0]), ck, x, y, noise_diag, jitter, periodic, lookahead=lookahead, fused=fused, score=score)


def ahead_multi_dense(ck, x, y, noise_diag, jitter, origins, weights=None, lookahead=True, fused=True, score="log"):
    """Rolling-origin forecast values, means and variances of one dense layer at K horizons in one library call (gpar_ahead_multi_dense):
    `origins` a K x n host array, the device tensor `upload_origins` returns or an `Origins`, `weights` K positive numbers (None: all 1).
    Returns (out, values, mean, var, info): out = [weighted value, logdet] (device), the K unweighted values (device), K x n means and
    variances."""
    scheme = Origins.of(origins, x.shape[0], weights, multi=True)
    return _value_form(scheme, ck, x, y, noise_diag, jitter, lookahead=lookahead, fused=fused, score=score)


def ahead_multi_dense_grad(ck, x, y, noise_diag, jitter, periodic, origins, weights=None, lookahead=True, fused=True, score="log"):
    """One dense layer's weighted multi-horizon rolling-origin value AND its gradient ingredients in one library call
    (gpar_ahead_multi_dense_grad); `origins`, `weights` and `score` as for `ahead_multi_dense`.  Returns (out, values, half_diag, mean, var,
    info, A, W): out = [weighted value, logdet, GRAD_NACC moment sums], the K unweighted values, 1/2 diag(W), K x n means and variances,
    info word, the (n + 1) x (n + 1) factor buffer, the weights W (lower triangle)."""
    scheme = Origins.of(origins, x.shape[0], weights, multi=True)
    return _grad_form(scheme, ck, x, y, noise_diag, jitter, periodic, lookahead=lookahead, fused=fused, score=score)


def ahead_window_dense(ck, x, y, noise_diag, jitter, lo, origin, score="log"):
    """Sliding-window forecast value, means and variances of one dense layer in one library call (gpar_ahead_window_dense): row r predicted
    from rows lo[r] ... origin[r] - 1 alone, origin[r] = -1 not scored (NaN in its mean and variance).  `lo`, `origin`: host sequences of n
    ints or the device tensors `upload_window` returns (or `lo` a `Window`).  Returns (out, mean, var, info): out = [value, 0] (device;
    nothing is factored whole, so there is no log-determinant), means and variances (device), info word."""
    return _value_form(Window.of(lo, origin, x.shape[0]), ck, x, y, noise_diag, jitter, score=score)


def ahead_window_dense_grad(ck, x, y, noise_diag, jitter, periodic, lo, origin, score="log"):
    """One dense layer's sliding-window forecast value AND its gradient ingredients in one library call (gpar_ahead_window_dense_grad); `lo`,
    `origin` and `score` as for `ahead_window_dense`.  Returns (out, half_diag, mean, var, info, W): out = [value, 0, GRAD_NACC moment sums],
    1/2 diag(W), means and variances, info word, the weights W (lower triangle).  No factor of the whole matrix is formed or returned."""
    return _grad_form(Window.of(lo, origin, x.shape[0]), ck, x, y, noise_diag, jitter, periodic, score=score)


def factor_dense_batch(items, jitter, fused=True):
    """Augmented matrices [[k_b(x_b, x_b) + diag(noise_b) + jitter I, .], [y_b^T, 0]] of layers b that share their number of rows,
    built per layer (gpar_logpdf_dense_build) into one buffer and factored in lock-step (gpar_potrf_batch).
    `items`: (compiled kernel, x, y, noise_diag or None) per layer.  Returns (A, logdet, info): A is the (batch (n + 1)) x (n + 1)
    buffer - block b holds L_b, (L_b^-1 y_b)^T in its last row and -|L_b^-1 y_b|^2 in its corner - logdet / info `batch` words."""
    lib = _lib.load()
    batch = len(items)
    x0 = items[0][1]
    n, dev = x0.shape[0], x0.device
    A = alloc_matrix(batch * (n + 1), n + 1, dev)   # matrix b = rows b (n + 1) ... of one buffer
    lda = _ld(A)
    stride = (n + 1) * lda          # lda is a multiple of 16: every matrix starts 128-byte aligned
    logdet = torch.empty(batch, dtype=torch.float64, device=dev)
    info = torch.empty(batch, dtype=torch.int32, device=dev)
    st = stream_ptr(dev)
    keep = []
    for b, (ck, x, y, noise_diag) in enumerate(items):
        _check_mat(x, "x")
        y = y.reshape(-1)
        if x.shape[0] != n or y.numel() != n or y.dtype != torch.float64 or not y.is_cuda:
            raise ValueError("every layer of a batch must hold one fp64 device value per row, and the same number of rows")
        nptr = None
        if noise_diag is not None:
            noise_diag = noise_diag.reshape(-1).contiguous()
            if noise_diag.numel() != n:
                raise ValueError("noise_diag must hold one value per row of x")
            nptr = noise_diag.data_ptr()
        z = alloc_matrix(n, max(ck.dz, 1), dev)
        keep.append((z, y, noise_diag))
        _lib.check(
            lib.gpar_logpdf_dense_build(
                ctypes.byref(ck.fspec), ctypes.byref(ck.kspec), x.data_ptr(), n, _ld(x), y.data_ptr(), int(y.stride(0)), nptr, float(jitter),
                z.data_ptr(), _ld(z), A.data_ptr() + 8 * b * stride, lda, logdet.data_ptr() + 8 * b, info.data_ptr() + 4 * b, st,
            ),
            "gpar_logpdf_dense_build",
        )
    flags = 0 if fused else _lib.POTRF_UNFUSED
    _lib.check(lib.gpar_potrf_batch(A.data_ptr(), batch, stride, n + 1, n, lda, logdet.data_ptr(), info.data_ptr(), flags, st), "gpar_potrf_batch")
    return A, logdet, info


def logpdf_dense_batch(items, jitter, fused=True):
    """log N(y_b; 0, k_b(x_b, x_b) + diag(noise_b) + jitter I) for layers b that share their number of rows and do not feed one
    another: factor_dense_batch, then one gpar_logpdf_dense_finish.  Returns (values, info): `batch` device words each."""
    lib = _lib.load()
    A, logdet, info = factor_dense_batch(items, jitter, fused=fused)
    batch = len(items)
    n = A.shape[1] - 1
    values = torch.empty(batch, dtype=torch.float64, device=A.device)
    _lib.check(lib.gpar_logpdf_dense_finish(A.data_ptr(), batch, (n + 1) * _ld(A), n, _ld(A), logdet.data_ptr(), values.data_ptr(),
                                            stream_ptr(A.device)), "gpar_logpdf_dense_finish")
    return values, info


def logpdf_lockstep(layers, x, y, w, jitter, fused=True):
    """The log marginal likelihoods of layers that share their rows and do not feed one another, and their sum, in ONE library
    call (gpar_logpdf_lockstep).  `layers`: (compiled kernel, noise variance, column of y / w) per layer; x: n x width, the widest
    design matrix ([inputs, y_0 .. y_(p-2)] for a GPAR) - every layer's feature map selects its own columns; y, w: n x p device
    matrices (w None: unit weights).  Returns (values, total, info): `batch` words, one word, `batch` words, all on the device."""
    lib = _lib.load()
    _check_mat(x, "x")
    _check_mat(y, "y")
    batch = len(layers)
    n, dev = x.shape[0], x.device
    if y.dim() != 2 or y.shape[0] != n or (w is not None and (w.shape != y.shape or w.dtype != torch.float64 or not w.is_cuda)):
        raise ValueError("y (and w) must be n x p fp64 device matrices")
    if w is not None and w.stride(1) != 1:
        w = w.contiguous()
    arr = (_lib.Layer * batch)()
    dz = 1
    for b, (ck, noise, col) in enumerate(layers):
        if not 0 <= col < y.shape[1]:
            raise ValueError("observed column out of range")
        arr[b].fs = ctypes.pointer(ck.fspec)
        arr[b].ks = ctypes.pointer(ck.kspec)
        arr[b].noise = float(noise)
        arr[b].y_col = int(col)
        dz = max(dz, ck.dz)
    A = alloc_matrix(batch * (n + 1), n + 1, dev)
    lda = _ld(A)
    z = alloc_matrix(batch * max(n, 1), dz, dev)
    nd = torch.empty(batch * max(n, 1), dtype=torch.float64, device=dev) if w is not None else None
    words = torch.empty(2 * batch + 1, dtype=torch.float64, device=dev)   # logdet[batch], value[batch], total
    info = torch.empty(batch, dtype=torch.int32, device=dev)
    _lib.check(
        lib.gpar_logpdf_lockstep(
            arr, batch, x.data_ptr(), n, _ld(x), y.data_ptr(), _ld(y), None if w is None else w.data_ptr(), 0 if w is None else _ld(w),
            float(jitter), z.data_ptr(), _ld(z), None if nd is None else nd.data_ptr(), A.data_ptr(), lda, (n + 1) * lda,
            words.data_ptr(), info.data_ptr(), words[batch:].data_ptr(), words[2 * batch:].data_ptr(), 0 if fused else _lib.POTRF_UNFUSED,
            stream_ptr(dev),
        ),
        "gpar_logpdf_lockstep",
    )
    return words[batch:2 * batch], words[2 * batch], info


def gram(ck, z1, z2=None, out=None, lower=False, diag_add=None, diag_const=0.0, row_scale=None):
    """K = k(z1, z2) (z2 None: symmetric, optionally lower-only, + diag_add + diag_const on the diagonal); with `row_scale`
    (n1 weights) row a is multiplied by row_scale[a]."""
    lib = _lib.load()
    sym = z2 is None
    if sym:
        z2 = z1
    _check_mat(z1, "z1")
    _check_mat(z2, "z2")
    n1, n2 = z1.shape[0], z2.shape[0]
    if out is None:
        out = alloc_matrix(n1, n2, z1.device)
    _check_mat(out, "out")
    flags = _lib.GRAM_LOWER if (lower and sym) else 0
    dptr = None
    if diag_add is not None:
        if not sym:
            raise ValueError("diag_add requires the symmetric Gram")
        _check_mat(diag_add, "diag_add")
        diag_add = diag_add.contiguous()
        dptr = diag_add.data_ptr()
    rptr = None
    if row_scale is not None:
        if row_scale.dim() != 1 or row_scale.numel() != n1 or row_scale.dtype != torch.float64:
            raise ValueError("row_scale must be a vector of n1 fp64 weights")
        row_scale = row_scale.contiguous()
        rptr = row_scale.data_ptr()
    _lib.check(
        lib.gpar_gram(
            ctypes.byref(ck.kspec), z1.data_ptr(), n1, _ld(z1), z2.data_ptr(), n2, _ld(z2), ck.dz,
            out.data_ptr(), _ld(out), flags, dptr, float(diag_const), rptr, stream_ptr(z1.device),
        ),
        "gpar_gram",
    )
    return out


def gram_batch_(ck, z_all, batch, out, lower=False, diag_add=None, diag_const=0.0):
    """out block b ((batch n) x n, stacked by rows) <- k(z_b, z_b) + diag(diag_add) + diag_const I for the `batch` input sets
    stacked by rows in z_all: one launch (gpar_gram_batch)."""
    lib = _lib.load()
    _check_mat(z_all, "z_all")
    _check_mat(out, "out")
    n = out.shape[1]
    if z_all.shape[0] != batch * n or out.shape[0] != batch * n:
        raise ValueError("shapes of a batched Gram matrix do not match")
    dptr = None
    if diag_add is not None:
        diag_add = diag_add.reshape(-1).contiguous()
        if diag_add.numel() != n:
            raise ValueError("diag_add must hold one value per row")
        dptr = diag_add.data_ptr()
    _lib.check(
        lib.gpar_gram_batch(ctypes.byref(ck.kspec), z_all.data_ptr(), n, _ld(z_all), n * _ld(z_all), ck.dz, out.data_ptr(), _ld(out),
                            n * _ld(out), _lib.GRAM_LOWER if lower else 0, dptr, float(diag_const), batch, stream_ptr(out.device)),
        "gpar_gram_batch",
    )
    return out


def gram_diag(ck, z):
    lib = _lib.load()
    _check_mat(z, "z")
    out = torch.empty(z.shape[0], dtype=torch.float64, device=z.device)
    _lib.check(
        lib.gpar_gram_diag(ctypes.byref(ck.kspec), z.data_ptr(), z.shape[0], _ld(z), ck.dz, out.data_ptr(), stream_ptr(z.device)),
        "gpar_gram_diag",
    )
    return out


def _comp_array(ck, comp):
    """The grouping of a compiled kernel's terms as the host int array the library reads (one entry per term)."""
    comp = [int(c) for c in comp]
    if len(comp) != int(ck.kspec.nterms):
        raise ValueError(f"the grouping holds {len(comp)} entries for {int(ck.kspec.nterms)} kernel terms")
    return (ctypes.c_int * max(len(comp), 1))(*comp)


def gram_terms(ck, comp, ncomp, z1, z2=None, out=None):
    """k_g(z1, z2) for the components of the grouping `comp` (per term of `ck` a component 0 .. ncomp - 1, or -1 for none), stacked by
    rows - component g in rows g n1 .. (g + 1) n1 of a (ncomp n1) x n2 matrix (`out`, or a new one) -, built in one pass over the pairs
    (gpar_gram_terms)."""
    lib = _lib.load()
    if z2 is None:
        z2 = z1
    _check_mat(z1, "z1")
    _check_mat(z2, "z2")
    n1, n2 = z1.shape[0], z2.shape[0]
    stacked = out if out is not None else alloc_matrix(ncomp * n1, n2, z1.device)
    _check_mat(stacked, "out")
    if stacked.shape[0] != ncomp * n1 or stacked.shape[1] != n2:
        raise ValueError("out must be (ncomp n1) x n2")
    _lib.check(
        lib.gpar_gram_terms(ctypes.byref(ck.kspec), _comp_array(ck, comp), int(ncomp), z1.data_ptr(), n1, _ld(z1), z2.data_ptr(), n2, _ld(z2),
                            ck.dz, stacked.data_ptr(), _ld(stacked), n1 * _ld(stacked), stream_ptr(z1.device)),
        "gpar_gram_terms",
    )
    return stacked


def gram_terms_diag(ck, comp, ncomp, z):
    """out[g][a] = k_g(z[a], z[a]): ncomp x n (gpar_gram_terms_diag)."""
    lib = _lib.load()
    _check_mat(z, "z")
    n = z.shape[0]
    out = torch.empty(ncomp, n, dtype=torch.float64, device=z.device)
    _lib.check(
        lib.gpar_gram_terms_diag(ctypes.byref(ck.kspec), _comp_array(ck, comp), int(ncomp), z.data_ptr(), n, _ld(z), ck.dz, out.data_ptr(),
                                 max(n, 1), stream_ptr(z.device)),
        "gpar_gram_terms_diag",
    )
    return out


def posterior_terms(ck, comp, ncomp, zs, z, alpha, L, variance=True, ws_doubles=None):
    """(mean, var), each ncomp x n*: the posterior moments of every component of the grouping `comp` at the test features `zs`, for the
    conditioned dense layer with training features `z`, alpha = K^-1 y and factor `L` - one library call (gpar_posterior_terms).  `var` is
    None without `variance`.  `ws_doubles`: the workspace to bring instead of the recommended one (a small one makes the variance pass
    take several chunks of test rows)."""
    lib = _lib.load()
    _check_mat(zs, "zs")
    _check_mat(z, "z")
    _check_mat(L, "L")
    ns, n = zs.shape[0], z.shape[0]
    alpha = alpha.reshape(-1).contiguous()
    if alpha.numel() != n or alpha.dtype != torch.float64 or not alpha.is_cuda:
        raise ValueError("alpha must hold one fp64 device value per training row")
    if L.shape[0] != n or L.shape[1] != n:
        raise ValueError("L must be the n x n factor of the training covariance")
    if ws_doubles is None:
        ws_doubles = lib.gpar_workspace_doubles(_lib.WS_POSTERIOR_TERMS, n, ns, int(ncomp))
    if ws_doubles < 0:
        raise ValueError(f"no workspace size for n={n}, n*={ns}, ncomp={ncomp}")
    ws = torch.empty(max(int(ws_doubles), 2), dtype=torch.float64, device=zs.device)
    mean = torch.empty(ncomp, ns, dtype=torch.float64, device=zs.device)
    var = torch.empty(ncomp, ns, dtype=torch.float64, device=zs.device) if variance else None
    _lib.check(
        lib.gpar_posterior_terms(ctypes.byref(ck.kspec), _comp_array(ck, comp), int(ncomp), zs.data_ptr(), ns, _ld(zs), z.data_ptr(), n, _ld(z),
                                 ck.dz, alpha.data_ptr(), L.data_ptr(), _ld(L), mean.data_ptr(), max(ns, 1),
                                 None if var is None else var.data_ptr(), max(ns, 1), ws.data_ptr(), int(ws_doubles), stream_ptr(zs.device)),
        "gpar_posterior_terms",
    )
    return mean, var


def feature_directions(ck, xs, U):
    """J (ndir x n* x dz): the feature-space image of the design-space directions `U` (n* x width, or ndir x n* x width) at the design
    rows `xs` under the feature map of the compiled kernel `ck`:
        J[c][a][q] = U[c][a][col[q]] * d embed_q / d x (xs[a][col[q]]) * inv_scale[q],
    d embed / d x = 1 (identity), freq cos(freq x) (sin dim), -freq sin(freq x) (cos dim) - what gpar_posterior_deriv takes for J.  torch
    on the device of `xs`: the feature map's few numbers go over as kernel arguments' data, nothing comes back."""
    fs, dz = ck.fspec, int(ck.dz)
    U3 = U if U.dim() == 3 else U[None]
    if xs.dim() != 2 or U3.shape[1] != xs.shape[0] or U3.shape[2] != xs.shape[1] or xs.shape[1] != ck.width:
        raise ValueError(f"directions must be n* x width (or ndir x n* x width) over design rows of width {ck.width}")
    if dz == 0:
        return torch.zeros(U3.shape[0], xs.shape[0], 0, dtype=torch.float64, device=xs.device)
    col = torch.tensor([int(fs.col[q]) for q in range(dz)], dtype=torch.long).to(xs.device, non_blocking=True)
    spec = torch.tensor([[float(fs.inv_scale[q]) for q in range(dz)], [float(fs.freq[q]) for q in range(dz)],
                         [float(fs.embed[q]) for q in range(dz)]], dtype=torch.float64).to(xs.device, non_blocking=True)
    inv_scale, freq, embed = spec[0], spec[1], spec[2]
    phase = xs.index_select(1, col) * freq
    slope = torch.where(embed == float(_lib.EMBED_SIN), freq * torch.cos(phase),
                        torch.where(embed == float(_lib.EMBED_COS), -freq * torch.sin(phase), torch.ones_like(phase)))
    return (U3.index_select(2, col) * (slope * inv_scale)[None]).contiguous()


def posterior_deriv(ck, zs, J, z, alpha, L, variance=True, ws_doubles=None):
    """(dmean, dvar), each ndir x n*: mean and latent variance of the directional derivatives of the conditioned dense layer with training
    features `z`, alpha = K^-1 y and factor `L`, at the test features `zs` along the feature-space directions `J` (ndir x n* x dz,
    `feature_directions`) - one library call (gpar_posterior_deriv).  `dvar` is None without `variance`.  `ws_doubles`: the workspace to
    bring instead of the recommended one (a small one means fewer splits of the mean pass and several chunks of test rows)."""
    lib = _lib.load()
    _check_mat(zs, "zs")
    _check_mat(z, "z")
    _check_mat(L, "L")
    ns, n = zs.shape[0], z.shape[0]
    if J.dim() != 3 or J.shape[1] != ns or J.shape[2] != ck.dz or J.dtype != torch.float64 or not J.is_cuda:
        raise ValueError("J must be an ndir x n* x dz fp64 device tensor")
    J = J.contiguous()
    ndir = int(J.shape[0])
    alpha = alpha.reshape(-1).contiguous()
    if alpha.numel() != n or alpha.dtype != torch.float64 or not alpha.is_cuda:
        raise ValueError("alpha must hold one fp64 device value per training row")
    if L.shape[0] != n or L.shape[1] != n:
        raise ValueError("L must be the n x n factor of the training covariance")
    if ws_doubles is None:
        ws_doubles = lib.gpar_workspace_doubles(_lib.WS_POSTERIOR_DERIV, n, ns, ndir)
    if ws_doubles < 0:
        raise ValueError(f"no workspace size for n={n}, n*={ns}, ndir={ndir}")
    ws = torch.empty(max(int(ws_doubles), 2), dtype=torch.float64, device=zs.device)
    mean = torch.empty(ndir, ns, dtype=torch.float64, device=zs.device)
    var = torch.empty(ndir, ns, dtype=torch.float64, device=zs.device) if variance else None
    _lib.check(
        lib.gpar_posterior_deriv(ctypes.byref(ck.kspec), zs.data_ptr(), ns, _ld(zs), J.data_ptr(), max(ck.dz, 1), ns * max(ck.dz, 1), ndir,
                                 z.data_ptr(), n, _ld(z), ck.dz, alpha.data_ptr(), L.data_ptr(), _ld(L), mean.data_ptr(), max(ns, 1),
                                 None if var is None else var.data_ptr(), max(ns, 1), ws.data_ptr(), int(ws_doubles), stream_ptr(zs.device)),
        "gpar_posterior_deriv",
    )
    return mean, var


def periodogram(t, y, omega, freq, t0):
    """power (p x F): the generalised Lomb-Scargle periodogram of the p columns of y (n x p; weights omega, 0 = unobserved) at the time
    stamps t (n) and frequencies freq (F), phases counted from the host number t0 (gpar_periodogram; semantics: include/gpar_hip.h)."""
    lib = _lib.load()
    for a, name in ((t, "t"), (y, "y"), (omega, "omega"), (freq, "freq")):
        _check_mat(a, name)
    t, freq = t.reshape(-1).contiguous(), freq.reshape(-1).contiguous()
    if y.dim() != 2 or tuple(omega.shape) != tuple(y.shape) or y.shape[0] != t.numel():
        raise ValueError("y and omega must be n x p, one row per time stamp")
    n, p, nf = int(y.shape[0]), int(y.shape[1]), int(freq.numel())
    power = torch.zeros(p, nf, dtype=torch.float64, device=y.device)
    _lib.check(
        lib.gpar_periodogram(t.data_ptr(), n, float(t0), y.data_ptr(), _ld(y), omega.data_ptr(), _ld(omega), p, freq.data_ptr(), nf,
                             power.data_ptr(), max(nf, 1), stream_ptr(y.device)),
        "gpar_periodogram",
    )
    return power


def rff_apply(z, dz, shift, omega, thc, ths, group_rows=0):
    """The random Fourier prior of pathwise sampling at the feature rows z (gpar_rff_apply; semantics: include/gpar_hip.h):
    sum_j thc[j, c] cos(2 pi omega_j . (z_r - shift)) + ths[j, c] sin(...).  group_rows > 0: z holds S = thc.shape[1] groups of group_rows
    rows, row r uses column r // group_rows, a vector of z.shape[0] values comes back; group_rows = 0: every row meets every column,
    rows x S."""
    lib = _lib.load()
    for a, name in ((z, "z"), (shift, "shift"), (omega, "omega"), (thc, "thc"), (ths, "ths")):
        _check_mat(a, name)
    rows, nfreq, count = int(z.shape[0]), int(omega.shape[0]), int(thc.shape[1])
    shift, thc, ths = shift.reshape(-1).contiguous(), thc.contiguous(), ths.contiguous()   # (one leading dimension for both weight matrices)
    if tuple(ths.shape) != tuple(thc.shape) or thc.shape[0] != nfreq or shift.numel() < dz or (nfreq and omega.shape[1] < dz) or (dz and z.shape[1] < dz):
        raise ValueError("rff_apply: omega must be F x dz, thc and ths F x S, shift dz long, z rows x dz")
    out = torch.empty(rows, dtype=torch.float64, device=z.device) if group_rows else torch.empty(rows, max(count, 1), dtype=torch.float64, device=z.device)
    _lib.check(
        lib.gpar_rff_apply(z.data_ptr(), rows, _ld(z), int(dz), shift.data_ptr(), omega.data_ptr(), _ld(omega), nfreq, thc.data_ptr(),
                           ths.data_ptr(), max(count, 1), count, int(group_rows), out.data_ptr(), max(count, 1),
                           stream_ptr(z.device)),
        "gpar_rff_apply",
    )
    return out if group_rows else out[:, :count]


def gram_apply_groups(ck, zs, z, vt, group_rows=0, ws_doubles=None):
    """sum_a k(zs_r, z_a) vt[c, a] without the rows x n matrix (gpar_gram_apply_groups): vt is S x n.  group_rows > 0: zs holds S groups of
    group_rows rows, row r uses vt[r // group_rows], a vector comes back; group_rows = 0: every row meets every vector, rows x S.
    `ws_doubles`: the workspace to bring instead of the recommended one (a small one allows fewer splits of the training rows)."""
    lib = _lib.load()
    for a, name in ((zs, "zs"), (z, "z"), (vt, "vt")):
        _check_mat(a, name)
    rows, n, count = int(zs.shape[0]), int(z.shape[0]), int(vt.shape[0])
    if vt.dim() != 2 or vt.shape[1] != n:
        raise ValueError("vt must be S x n: one vector per row")
    ncols = 1 if group_rows else count
    if ws_doubles is None:
        ws_doubles = lib.gpar_workspace_doubles(_lib.WS_GRAM_APPLY, n, rows, max(ncols, 1))
    ws = torch.empty(max(int(ws_doubles), 2), dtype=torch.float64, device=zs.device)
    out = torch.empty(rows, dtype=torch.float64, device=zs.device) if group_rows else torch.empty(rows, max(count, 1), dtype=torch.float64, device=zs.device)
    _lib.check(
        lib.gpar_gram_apply_groups(ctypes.byref(ck.kspec), zs.data_ptr(), rows, _ld(zs), z.data_ptr(), n, _ld(z), ck.dz, vt.data_ptr(), _ld(vt),
                                   count, int(group_rows), out.data_ptr(), max(count, 1), ws.data_ptr(), int(ws_doubles), stream_ptr(zs.device)),
        "gpar_gram_apply_groups",
    )
    return out if group_rows else out[:, :count]


def pivoted_chol(ck, z, max_rank, tol_trace, floor):
    """Greedy (partially pivoted) Cholesky of k(z, z) on the features z (gpar_pivoted_chol; semantics: include/gpar_hip.h).  Returns
    device tensors and never synchronises: (Lt max_rank x n - the factor transposed, rows from the rank on zero -, piv int32 max_rank
    with -1 beyond the rank, trace max_rank + 1, rank and info as one-element int32 tensors, the final residual diagonal d)."""
    lib = _lib.load()
    _check_mat(z, "z")
    n, dev, max_rank = z.shape[0], z.device, int(max_rank)
    if n < 1 or not 1 <= max_rank <= _lib.PIVCHOL_MAX_RANK:
        raise ValueError(f"pivoted_chol takes at least one row and 1 to {_lib.PIVCHOL_MAX_RANK} steps")
    Lt = alloc_matrix(max_rank, n, dev)
    piv = torch.empty(max_rank, dtype=torch.int32, device=dev)
    trace = torch.empty(max_rank + 1, dtype=torch.float64, device=dev)
    words = torch.empty(2, dtype=torch.int32, device=dev)   # rank, info
    ws = torch.empty(lib.gpar_workspace_doubles(_lib.WS_PIVOTED_CHOL, n, 0, 0), dtype=torch.float64, device=dev)
    _lib.check(
        lib.gpar_pivoted_chol(ctypes.byref(ck.kspec), z.data_ptr(), n, _ld(z), ck.dz, max_rank, float(tol_trace), float(floor), Lt.data_ptr(),
                              _ld(Lt), piv.data_ptr(), trace.data_ptr(), words.data_ptr(), words[1:].data_ptr(), ws.data_ptr(), stream_ptr(dev)),
        "gpar_pivoted_chol",
    )
    return Lt, piv, trace, words[0:1], words[1:2], ws[:n]


def chol_drop_leading(A, k):
    """The augmented factor of the trailing n - k observations from the (n + 1) x (n + 1) augmented factor `A` of all n, by a rank-k
    Cholesky update (gpar_chol_drop_leading; semantics: include/gpar_hip.h).  Out of place; returns (out (n - k + 1) x (n - k + 1),
    logdet, info) - device tensors, nothing synchronises."""
    lib = _lib.load()
    _check_mat(A, "A")
    n, k, dev = A.shape[0] - 1, int(k), A.device
    if A.shape[1] != n + 1 or not 1 <= k < n or k > _lib.CHOL_UPDATE_MAX_RANK:
        raise ValueError(f"chol_drop_leading takes a square augmented factor and 1 <= k < n, k <= {_lib.CHOL_UPDATE_MAX_RANK}")
    out = alloc_matrix(n - k + 1, n - k + 1, dev)
    ws = torch.empty(lib.gpar_workspace_doubles(_lib.WS_CHOL_UPDATE, n, k, 0), dtype=torch.float64, device=dev)
    logdet = torch.empty(1, dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(
        lib.gpar_chol_drop_leading(A.data_ptr(), n, k, _ld(A), out.data_ptr(), _ld(out), ws.data_ptr(), logdet.data_ptr(), info.data_ptr(),
                                   stream_ptr(dev)),
        "gpar_chol_drop_leading",
    )
    return out, logdet, info


def chol_append_(A, n0, k, logdet, lookahead=True, fused=True):
    """In place: the (n0 + k + 1) x (n0 + k + 1) matrix A, laid out as gpar_chol_append wants it (the old factor, the raw new Gram rows,
    the row [z_old, y_new, .]), becomes the augmented factor of the n0 + k observations; `logdet` (one device word holding the old
    log-determinant) is accumulated.  Returns (logdet, info)."""
    lib = _lib.load()
    _check_mat(A, "A")
    if A.shape[0] != n0 + k + 1 or A.shape[1] != n0 + k + 1 or k < 1:
        raise ValueError("A must be (n0 + k + 1) x (n0 + k + 1) with k >= 1")
    info = torch.zeros(1, dtype=torch.int32, device=A.device)
    _lib.check(
        lib.gpar_chol_append(A.data_ptr(), int(n0), int(k), _ld(A), logdet.data_ptr(), info.data_ptr(), _potrf_flags(lookahead, fused),
                             stream_ptr(A.device)),
        "gpar_chol_append",
    )
    return logdet, info


def potrf_(A, nf=None, logdet=None, info=None, lookahead=True, fused=True):
    """In-place (partial) Cholesky of the lower triangle of the square matrix A; returns (logdet, info) device
    scalars (logdet accumulates, info is sticky: pass fresh zeros).  `lookahead=False`: the caller has several
    factorisations in flight itself (see gpar_potrf_ex)."""
    lib = _lib.load()
    _check_mat(A, "A")
    N = A.shape[0]
    if A.shape[1] != N:
        raise ValueError("A must be square")
    nf = N if nf is None else int(nf)
    if logdet is None:
        logdet = torch.zeros(1, dtype=torch.float64, device=A.device)
    if info is None:
        info = torch.zeros(1, dtype=torch.int32, device=A.device)
    flags = (0 if lookahead else _lib.POTRF_NO_LOOKAHEAD) | (0 if fused else _lib.POTRF_UNFUSED)
    _lib.check(
        lib.gpar_potrf_ex(A.data_ptr(), N, nf, _ld(A), logdet.data_ptr(), info.data_ptr(), flags, stream_ptr(A.device)), "gpar_potrf_ex"
    )
    return logdet, info


def potrf_batch_(A, batch, nf=None, fused=True):
    """In-place (partial) Cholesky of `batch` square N x N matrices stacked by rows in A ((batch N) x N, one leading
    dimension), factored in lock-step (gpar_potrf_batch); returns (logdet, info): `batch` device words each."""
    lib = _lib.load()
    _check_mat(A, "A")
    N = A.shape[1]
    if A.shape[0] != batch * N:
        raise ValueError("A must hold batch square matrices stacked by rows")
    nf = N if nf is None else int(nf)
    logdet = torch.zeros(batch, dtype=torch.float64, device=A.device)
    info = torch.zeros(batch, dtype=torch.int32, device=A.device)
    _lib.check(
        lib.gpar_potrf_batch(A.data_ptr(), batch, N * _ld(A), N, nf, _ld(A), logdet.data_ptr(), info.data_ptr(),
                             0 if fused else _lib.POTRF_UNFUSED, stream_ptr(A.device)),
        "gpar_potrf_batch",
    )
    return logdet, info


def trsm_rlt_(L, B, when=None):
    """B <- B L^-T (rows of B solved by forward substitution).  `when` = (flag, sense): predicated on the device word flag[0] - the
    solve happens iff (flag[0] != 0) == sense (gpar_trsm_rlt_if); B is left untouched otherwise."""
    lib = _lib.load()
    _check_mat(L, "L")
    _check_mat(B, "B")
    n = L.shape[0]
    if B.shape[1] != n:
        raise ValueError("B must have as many columns as L has rows")
    if when is not None:
        flag, sense = when
        if flag.dtype != torch.int32 or not flag.is_cuda:
            raise TypeError("the predicate of a solve is an int32 device word")
        _lib.check(lib.gpar_trsm_rlt_if(L.data_ptr(), n, _ld(L), B.data_ptr(), B.shape[0], _ld(B), flag.data_ptr(), int(bool(sense)),
                                        stream_ptr(B.device)), "gpar_trsm_rlt_if")
        return B
    _lib.check(lib.gpar_trsm_rlt(L.data_ptr(), n, _ld(L), B.data_ptr(), B.shape[0], _ld(B), stream_ptr(B.device)), "gpar_trsm_rlt")
    return B


def vfe_factor(G, c, ys, kdiag, d, diag_add, with_trace, lookahead=True, fused=True):
    """The factor of A = I-shifted G with the row c appended, and the inducing-point bound from it (gpar_vfe_assemble, gpar_potrf,
    gpar_vfe_value): returns (A buffer (M + 1) x (M + 1), logdet word, info word, bound as a 0-d device tensor)."""
    lib = _lib.load()
    _check_mat(G, "G")
    M, n, dev = G.shape[0], ys.numel(), G.device
    c, ys, kdiag, d = (t.reshape(-1).contiguous() for t in (c, ys, kdiag, d))
    A = alloc_matrix(M + 1, M + 1, dev)
    words = torch.empty(258, dtype=torch.float64, device=dev)   # logdet, bound, then 64 x 4 partial sums
    info = torch.empty(1, dtype=torch.int32, device=dev)
    st = stream_ptr(dev)
    _lib.check(lib.gpar_vfe_assemble(G.data_ptr(), M, _ld(G), c.data_ptr(), ys.data_ptr(), kdiag.data_ptr(), d.data_ptr(), n, float(diag_add),
                                     A.data_ptr(), _ld(A), words[2:].data_ptr(), words.data_ptr(), info.data_ptr(), st), "gpar_vfe_assemble")
    flags = (0 if lookahead else _lib.POTRF_NO_LOOKAHEAD) | (0 if fused else _lib.POTRF_UNFUSED)
    _lib.check(lib.gpar_potrf_ex(A.data_ptr(), M + 1, M, _ld(A), words.data_ptr(), info.data_ptr(), flags, st), "gpar_potrf_ex")
    _lib.check(lib.gpar_vfe_value(words[2:].data_ptr(), words.data_ptr(), A.data_ptr(), _ld(A), M, n, int(bool(with_trace)), words[1:].data_ptr(), st),
               "gpar_vfe_value")
    return A, words[0:1], info, words[1]


def chol_spread(L, limit):
    """(spread, flag) device words of a Cholesky factor: (max L_jj / min L_jj)^2 and whether it exceeds `limit` (gpar_chol_spread)."""
    lib = _lib.load()
    _check_mat(L, "L")
    spread = torch.empty(1, dtype=torch.float64, device=L.device)
    flag = torch.empty(1, dtype=torch.int32, device=L.device)
    _lib.check(lib.gpar_chol_spread(L.data_ptr(), L.shape[0], _ld(L), float(limit), spread.data_ptr(), flag.data_ptr(), stream_ptr(L.device)),
               "gpar_chol_spread")
    return spread, flag


def trsm_rln_(L, B):
    """B <- B L^-1 (rows of B solved by backward substitution)."""
    lib = _lib.load()
    _check_mat(L, "L")
    _check_mat(B, "B")
    n = L.shape[0]
    if B.shape[1] != n:
        raise ValueError("B must have as many columns as L has rows")
    _lib.check(lib.gpar_trsm_rln(L.data_ptr(), n, _ld(L), B.data_ptr(), B.shape[0], _ld(B), stream_ptr(B.device)), "gpar_trsm_rln")
    return B


def gemm(A, B, ta=False, tb=False, alpha=1.0, beta=0.0, out=None, c_lower=False, a_lower=False, k_from_row=False, k_to_col=False):
    """out <- alpha op(A) op(B) + beta out;  ta: A stored k x m;  tb: B stored n x k.  `k_from_row` / `k_to_col`: op(A) is
    upper triangular (stored zeros left of its diagonal) / op(B) is upper triangular (stored zeros below it): the K loop
    skips the blocks that are zero."""
    lib = _lib.load()
    _check_mat(A, "A")
    _check_mat(B, "B")
    m, k = (A.shape[1], A.shape[0]) if ta else (A.shape[0], A.shape[1])
    n, kb = (B.shape[0], B.shape[1]) if tb else (B.shape[1], B.shape[0])
    if k != kb:
        raise ValueError(f"inner dimensions differ: {k} vs {kb}")
    if out is None:
        if (n == 1 and tb and not ta and beta == 0.0 and not (c_lower or a_lower or k_from_row or k_to_col) and B.dim() == 2 and m > 0
                and os.environ.get("GPAR_GEMV", "1") != "0"):
            # one column: a matrix-vector product (gpar_gemv: one wave per row) instead of 128-wide tiles with one live column
            y = torch.empty(m, 1, dtype=torch.float64, device=A.device)
            _lib.check(lib.gpar_gemv(A.data_ptr(), m, k, _ld(A), B.data_ptr(), 1, float(alpha), y.data_ptr(), 1, stream_ptr(A.device)), "gpar_gemv")
            return y
        out = alloc_matrix(m, n, A.device)
        if beta != 0.0:
            raise ValueError("beta != 0 needs an `out`")
    _check_mat(out, "out")
    flags = ((_lib.GEMM_C_LOWER if c_lower else 0) | (_lib.GEMM_A_LOWER if a_lower else 0) | (_lib.GEMM_K_FROM_ROW if k_from_row else 0)
             | (_lib.GEMM_K_TO_COL if k_to_col else 0))
    # few output tiles but a very long K: cut K into slices so that the launch fills the chip's 512 workgroup slots (two
    # 73.7 KB workgroups per CU) in one round; deterministic two-pass sum.  (The workspace comes from torch's stream-aware
    # caching allocator: no hipMalloc after the first call of a given size.)
    tm, tn = (m + 127) // 128, (n + 127) // 128
    tiles = (min(tm, tn) * (min(tm, tn) + 1) // 2 + (tm - min(tm, tn)) * min(tm, tn)) if c_lower else tm * tn
    if not (a_lower or k_from_row or k_to_col) and k >= 8192 and tiles <= 128:
        splits = max(2, min(64, 512 // max(tiles, 1), k // 1024))
        work = torch.empty(lib.gpar_workspace_doubles(_lib.WS_GEMM_SPLITK, m, n, splits), dtype=torch.float64, device=A.device)
        _lib.check(
            lib.gpar_gemm_splitk(
                int(ta), int(tb), m, n, k, float(alpha), A.data_ptr(), _ld(A), B.data_ptr(), _ld(B), float(beta),
                out.data_ptr(), _ld(out), flags, splits, work.data_ptr(), stream_ptr(A.device),
            ),
            "gpar_gemm_splitk",
        )
        return out
    _lib.check(
        lib.gpar_gemm(
            int(ta), int(tb), m, n, k, float(alpha), A.data_ptr(), _ld(A), B.data_ptr(), _ld(B), float(beta),
            out.data_ptr(), _ld(out), flags, stream_ptr(A.device),
        ),
        "gpar_gemm",
    )
    return out


def dot(x, incx, y, incy, n, out=None, accumulate=False):
    lib = _lib.load()
    if out is None:
        out = torch.zeros(1, dtype=torch.float64, device=x.device)
    _lib.check(
        lib.gpar_dot(x.data_ptr(), int(incx), y.data_ptr(), int(incy), int(n), out.data_ptr(), int(accumulate), stream_ptr(x.device)),
        "gpar_dot",
    )
    return out


def gemv_t(A, v):
    """A^T v for a tall matrix A (rows x cols) and a vector v (rows): new vector of `cols` entries."""
    lib = _lib.load()
    _check_mat(A, "A")
    rows, cols = A.shape
    v = v.reshape(-1).contiguous()
    if v.numel() != rows or v.dtype != torch.float64:
        raise ValueError("v must hold one fp64 weight per row of A")
    out = torch.empty(cols, dtype=torch.float64, device=A.device)
    work = torch.empty(max(1, lib.gpar_workspace_doubles(_lib.WS_GEMV_T, rows, cols, 0)), dtype=torch.float64, device=A.device)
    _lib.check(lib.gpar_gemv_t(A.data_ptr(), rows, cols, _ld(A), v.data_ptr(), out.data_ptr(), work.data_ptr(), stream_ptr(A.device)),
               "gpar_gemv_t")
    return out


def rownorm2(A):
    """Squared Euclidean norms of the rows of A: new vector."""
    lib = _lib.load()
    _check_mat(A, "A")
    out = torch.empty(A.shape[0], dtype=torch.float64, device=A.device)
    _lib.check(lib.gpar_rownorm2(A.data_ptr(), A.shape[0], A.shape[1], _ld(A), out.data_ptr(), stream_ptr(A.device)), "gpar_rownorm2")
    return out


def pack_lower(A, out=None):
    """Lower triangle (diagonal included) of the square matrix A as a contiguous vector of n (n + 1) / 2 doubles."""
    lib = _lib.load()
    _check_mat(A, "A")
    n = A.shape[0]
    if out is None:
        out = torch.empty(n * (n + 1) // 2, dtype=torch.float64, device=A.device)
    _lib.check(lib.gpar_pack_lower(A.data_ptr(), n, _ld(A), out.data_ptr(), stream_ptr(A.device)), "gpar_pack_lower")
    return out


def unpack_lower_(packed, A):
    """Inverse of pack_lower into the lower triangle of A (the strict upper triangle is left alone)."""
    lib = _lib.load()
    _check_mat(A, "A")
    n = A.shape[0]
    if packed.numel() < n * (n + 1) // 2 or not packed.is_contiguous():
        raise ValueError("packed buffer too small or not contiguous")
    _lib.check(lib.gpar_unpack_lower(packed.data_ptr(), n, A.data_ptr(), _ld(A), stream_ptr(A.device)), "gpar_unpack_lower")
    return A


def randn(seed, offset, rows, cols, device):
    lib = _lib.load()
    out = alloc_matrix(rows, cols, device)
    _lib.check(
        lib.gpar_randn(int(seed) & (2**64 - 1), int(offset) & (2**64 - 1), out.data_ptr(), rows, cols, _ld(out), stream_ptr(device)),
        "gpar_randn",
    )
    return out


def gemm_batch_(A, B, out, batch, ta=False, tb=False, alpha=1.0, beta=0.0, c_lower=False):
    """out_b <- alpha op(A_b) op(B_b) + beta out_b for `batch` problems of one shape whose operands are stacked by rows in A, B
    and out (block b = rows [b R, (b + 1) R) with R = rows / batch): one launch (gpar_gemm_batch)."""
    lib = _lib.load()
    for name, t in (("A", A), ("B", B), ("out", out)):
        _check_mat(t, name)
        if t.shape[0] % batch:
            raise ValueError(f"{name}: rows must be a multiple of the batch size")
    ra, rb, rc = A.shape[0] // batch, B.shape[0] // batch, out.shape[0] // batch
    m, k = (A.shape[1], ra) if ta else (ra, A.shape[1])
    n, kb = (rb, B.shape[1]) if tb else (B.shape[1], rb)
    if k != kb or rc != m or out.shape[1] != n:
        raise ValueError("shapes of a batched product do not match")
    _lib.check(
        lib.gpar_gemm_batch(int(ta), int(tb), m, n, k, float(alpha), A.data_ptr(), _ld(A), ra * _ld(A), B.data_ptr(), _ld(B), rb * _ld(B),
                            float(beta), out.data_ptr(), _ld(out), rc * _ld(out), _lib.GEMM_C_LOWER if c_lower else 0, batch,
                            stream_ptr(out.device)),
        "gpar_gemm_batch",
    )
    return out


def trmv_lower(L, x):
    """L x for the lower triangle of the square matrix L and one column x (n x 1, any row stride); new n x 1 tensor."""
    lib = _lib.load()
    _check_mat(L, "L")
    n = L.shape[0]
    if x.dim() != 2 or x.shape[0] != n or x.shape[1] != 1 or x.dtype != torch.float64:
        raise ValueError("x must be an n x 1 fp64 matrix")
    y = torch.empty(n, 1, dtype=torch.float64, device=L.device)
    _lib.check(lib.gpar_trmv_lower(L.data_ptr(), n, _ld(L), x.data_ptr(), int(x.stride(0)), y.data_ptr(), 1, stream_ptr(L.device)),
               "gpar_trmv_lower")
    return y


def trmv_lower_batch_(Ls, batch, X, out, add=None):
    """Column b of `out` (n x batch) <- L_b X[:, b] (+ add[b n : (b + 1) n]) for the `batch` lower-triangular n x n matrices
    stacked by rows in Ls; X: n x batch (any strides), add: (batch n) x 1 or None.  One launch."""
    lib = _lib.load()
    _check_mat(Ls, "Ls")
    n = Ls.shape[1]
    if Ls.shape[0] != batch * n or X.shape != (n, batch) or out.shape != (n, batch) or X.dtype != torch.float64 or out.dtype != torch.float64:
        raise ValueError("shapes of a batched triangular product do not match")
    aptr, inca, stride_add = None, 0, 0
    if add is not None:
        if add.numel() != batch * n or add.dtype != torch.float64:
            raise ValueError("add must hold one value per row and matrix")
        add = add.reshape(batch * n, -1)
        aptr, inca, stride_add = add.data_ptr(), int(add.stride(0)), n * int(add.stride(0))
    _lib.check(
        lib.gpar_trmv_lower_batch(Ls.data_ptr(), batch, n * _ld(Ls), n, _ld(Ls), X.data_ptr(), int(X.stride(0)), int(X.stride(1)), aptr, inca,
                                  stride_add, out.data_ptr(), int(out.stride(0)), int(out.stride(1)), stream_ptr(Ls.device)),
        "gpar_trmv_lower_batch",
    )
    return out


def percentile_index(num, q):
    """(k, g) such that numpy's default ("linear", Hyndman & Fan 7) percentile q of `num` sorted values v is
    lerp(v[k], v[k + 1], g), with virtual index h = (num - 1) * (q / 100), k = floor(h), g = h - k - the expression
    numpy >= 2.0 evaluates, so the device result is bit-identical to np.percentile there."""
    virtual = (num - 1) * (float(q) / 100.0)
    k = int(math.floor(virtual))
    g = virtual - k
    if k < 0:
        k, g = 0, 0.0
    if k >= num - 1:
        k, g = num - 1, 0.0
    return k, g


def sample_stats(samples, q_lo=None, q_hi=None):
    """samples: contiguous (S, ...) fp64 device tensor.  Returns (mean, lo, hi) over axis 0 (lo / hi None unless both
    percentiles are given) - np.mean / np.percentile(method="linear") of the reference's predict, on the device."""
    if samples.dtype != torch.float64 or not samples.is_contiguous() or samples.dim() < 2:
        raise ValueError("samples must be a contiguous fp64 tensor of shape (S, ...)")
    lib = _lib.load()
    S = samples.shape[0]
    count = samples[0].numel()
    mean = torch.empty(samples.shape[1:], dtype=torch.float64, device=samples.device)
    want = q_lo is not None and q_hi is not None
    lo = torch.empty_like(mean) if want else None
    hi = torch.empty_like(mean) if want else None
    (k0, g0), (k1, g1) = (percentile_index(S, q_lo), percentile_index(S, q_hi)) if want else ((0, 0.0), (0, 0.0))
    _lib.check(
        lib.gpar_sample_stats(samples.data_ptr(), int(S), int(count), int(count), k0, g0, k1, g1, mean.data_ptr(),
                              lo.data_ptr() if want else None, hi.data_ptr() if want else None, stream_ptr(samples.device)),
        "gpar_sample_stats",
    )
    return mean, lo, hi


def featurize_dfreq(ck, x):
    """zd = d features / d freq (zero for non-periodic features)."""
    _check_mat(x, "x")
    lib = _lib.load()
    n = x.shape[0]
    zd = alloc_matrix(n, max(ck.dz, 1), x.device, zero=True)
    if ck.dz:
        _lib.check(
            lib.gpar_featurize_dfreq(ctypes.byref(ck.fspec), x.data_ptr(), n, _ld(x), zd.data_ptr(), _ld(zd), stream_ptr(x.device)),
            "gpar_featurize_dfreq",
        )
    return zd


def gram_grad(ck, z, zd, W, nblocks=None):
    """Raw gradient moment sums (length GRAD_NACC, device tensor) of 1/2 sum W dK/dtheta; see csrc/gram.h."""
    lib = _lib.load()
    _check_mat(z, "z")
    _check_mat(W, "W")
    n = z.shape[0]
    nt = (n + 63) // 64
    ntiles = nt * (nt + 1) // 2
    if nblocks is None:
        nblocks = max(1, min(ntiles, 1024))
    work = torch.empty(nblocks * _lib.GRAD_NACC, dtype=torch.float64, device=z.device)
    out = torch.empty(_lib.GRAD_NACC, dtype=torch.float64, device=z.device)
    zdp = None
    if zd is not None:
        _check_mat(zd, "zd")
        if _ld(zd) != _ld(z):
            raise ValueError("z and zd must share a leading dimension")
        zdp = zd.data_ptr()
    _lib.check(
        lib.gpar_gram_grad(
            ctypes.byref(ck.kspec), z.data_ptr(), zdp, n, _ld(z), ck.dz, W.data_ptr(), _ld(W), work.data_ptr(), nblocks,
            out.data_ptr(), stream_ptr(z.device),
        ),
        "gpar_gram_grad",
    )
    return out


GRAD_SYM, GRAD_RECT, GRAD_DIAG = 0, 1, 2


def gram_grad_cross(ck, z1, zd1, z2, zd2, W, mode, nblocks=None):
    """Raw moment sums (length GRAD_NACC, device tensor) of sum W dK/dtheta for the weight shapes of the VFE bound:
    GRAD_SYM (z2 is z1, W symmetric, lower triangle read), GRAD_RECT (W: n1 x n2), GRAD_DIAG (z2 is z1, W: n1 weights of
    the pairs (a, a)).  Full sums: no factor 1/2."""
    lib = _lib.load()
    _check_mat(z1, "z1")
    _check_mat(z2, "z2")
    n1, n2 = z1.shape[0], z2.shape[0]
    nt1, nt2 = (n1 + 63) // 64, (n2 + 63) // 64
    ntiles = nt1 * (nt1 + 1) // 2 if mode == GRAD_SYM else (nt1 * nt2 if mode == GRAD_RECT else nt1)
    if nblocks is None:
        nblocks = max(1, min(ntiles, 1024))
    if mode == GRAD_DIAG:
        if W.dim() != 1 or not W.is_contiguous() or W.numel() != n1:
            raise ValueError("GRAD_DIAG takes a contiguous vector of n1 weights")
        ldw = 1
    else:
        _check_mat(W, "W")
        ldw = _ld(W)
    work = torch.empty(nblocks * _lib.GRAD_NACC, dtype=torch.float64, device=z1.device)
    out = torch.empty(_lib.GRAD_NACC, dtype=torch.float64, device=z1.device)
    for a, b in ((zd1, z1), (zd2, z2)):
        if a is not None and _ld(a) != _ld(b):
            raise ValueError("features and their frequency derivatives must share a leading dimension")
    _lib.check(
        lib.gpar_gram_grad_cross(
            ctypes.byref(ck.kspec), z1.data_ptr(), None if zd1 is None else zd1.data_ptr(), n1, _ld(z1), z2.data_ptr(),
            None if zd2 is None else zd2.data_ptr(), n2, _ld(z2), ck.dz, W.data_ptr(), ldw, int(mode), work.data_ptr(), nblocks,
            out.data_ptr(), stream_ptr(z1.device),
        ),
        "gpar_gram_grad_cross",
    )
    return out


def gram_grad_rows(ck, z1, z2, v, zd1=None, zd2=None, ws_doubles=None):
    """Raw moment sums PER ROW of z1 (n1 x GRAD_NACC, device tensor): row a holds sum_b v[b] (moment of the pair (z1_a, z2_b)), what
    `gram_grad_cross(GRAD_RECT)` returns for z1 = z1[a], W = v^T - one library call (gpar_gram_grad_rows), no n1 x n2 matrix.  zd1 / zd2:
    both or neither (the period sums).  `ws_doubles`: the workspace to bring instead of the recommended one (a small one means fewer
    splits of the rows of z2; from n1 * GRAD_NACC)."""
    lib = _lib.load()
    _check_mat(z1, "z1")
    _check_mat(z2, "z2")
    n1, n2 = int(z1.shape[0]), int(z2.shape[0])
    v = v.reshape(-1).contiguous()
    if v.numel() != n2 or v.dtype != torch.float64 or not v.is_cuda:
        raise ValueError("v must hold one fp64 device weight per row of z2")
    for a, b in ((zd1, z1), (zd2, z2)):
        if a is not None:
            _check_mat(a, "zd")
            if _ld(a) != _ld(b) or a.shape[0] != b.shape[0]:
                raise ValueError("features and their frequency derivatives must share rows and a leading dimension")
    if ws_doubles is None:
        ws_doubles = lib.gpar_workspace_doubles(_lib.WS_GRAM_GRAD_ROWS, n2, n1, 0)
    ws = torch.empty(max(int(ws_doubles), 2), dtype=torch.float64, device=z1.device)
    out = torch.empty(n1, _lib.GRAD_NACC, dtype=torch.float64, device=z1.device)
    rc = lib.gpar_gram_grad_rows(ctypes.byref(ck.kspec), z1.data_ptr(), None if zd1 is None else zd1.data_ptr(), n1, _ld(z1), z2.data_ptr(),
                                 None if zd2 is None else zd2.data_ptr(), n2, _ld(z2), ck.dz, v.data_ptr(), out.data_ptr(), _lib.GRAD_NACC,
                                 ws.data_ptr(), int(ws_doubles), stream_ptr(z1.device))
    if rc == -1010:   # GPAR_ARG_ERROR(10): say what a caller of hyper_jacobian / predict_moments_hyper can act on
        raise _lib.HipLibraryError(
            f"gpar_gram_grad_rows failed with status {rc}: the feature tiles and slot accumulators of this kernel structure "
            f"({ck.dz} feature dims{', with period sums' if zd1 is not None else ''}) need more than the kernel's 160 KiB of LDS "
            "(include/gpar_hip.h has the arithmetic).  Per-row gradient sums - hyper_jacobian, predict_moments_hyper - are not available "
            "for a layer this wide; the other posterior passes are."
        )
    _lib.check(rc, "gpar_gram_grad_rows")
    return out


def gram_input_grad(ck, z1, z2, W, mode):
    """out[a][q] = sum_b W(a, b) d k(z1_a, z2_b) / d z1_a[q] (feature space; n1 x dz).  mode GRAD_RECT (W: n1 x n2) or
    GRAD_SYM (z2 is z1, W symmetric, lower triangle read)."""
    lib = _lib.load()
    _check_mat(z1, "z1")
    _check_mat(z2, "z2")
    _check_mat(W, "W")
    n1, n2 = z1.shape[0], z2.shape[0]
    out = alloc_matrix(n1, max(ck.dz, 1), z1.device, zero=True)
    if ck.dz == 0 or n1 == 0:
        return out
    row_blocks = (n1 + 63) // 64
    col_tiles = max(1, (n2 + 63) // 64)
    nsplit = max(1, min(col_tiles, 512 // max(row_blocks, 1)))
    work = torch.empty(max(1, lib.gpar_workspace_doubles(_lib.WS_INPUT_GRAD, n1, ck.dz, nsplit)), dtype=torch.float64, device=z1.device)
    _lib.check(
        lib.gpar_gram_input_grad(ctypes.byref(ck.kspec), z1.data_ptr(), n1, _ld(z1), z2.data_ptr(), n2, _ld(z2), ck.dz, W.data_ptr(),
                                 _ld(W), int(mode), nsplit, work.data_ptr(), out.data_ptr(), _ld(out), stream_ptr(z1.device)),
        "gpar_gram_input_grad",
    )
    return out


def chol_inverse(L, with_x=False):
    """Lower triangle of (L L^T)^-1 (new matrix) from the Cholesky factor L; triangular-aware (2 n^3 / 3 flops).  `with_x`: also the
    workspace the call leaves behind, X = L^-T in its upper triangle (the strict lower triangle is scratch)."""
    lib = _lib.load()
    _check_mat(L, "L")
    n = L.shape[0]
    X = alloc_matrix(n, n, L.device)
    Kinv = alloc_matrix(n, n, L.device)
    _lib.check(
        lib.gpar_chol_inverse(L.data_ptr(), n, _ld(L), X.data_ptr(), _ld(X), Kinv.data_ptr(), _ld(Kinv), stream_ptr(L.device)),
        "gpar_chol_inverse",
    )
    return (Kinv, X) if with_x else Kinv


def trmv_upper(U, x):
    """U x for an upper-triangular U (the strict lower triangle is not read) and a single vector x (any shape with n entries, unit or
    row stride): new contiguous vector of n entries (gpar_trmv_upper)."""
    lib = _lib.load()
    _check_mat(U, "U")
    n = U.shape[0]
    x = x.reshape(-1)
    if x.numel() != n or x.dtype != torch.float64 or not x.is_cuda:
        raise ValueError("x must hold one fp64 device value per row of U")
    out = torch.empty(n, dtype=torch.float64, device=U.device)
    _lib.check(lib.gpar_trmv_upper(U.data_ptr(), n, _ld(U), x.data_ptr(), int(x.stride(0)), out.data_ptr(), 1, stream_ptr(U.device)),
               "gpar_trmv_upper")
    return out
