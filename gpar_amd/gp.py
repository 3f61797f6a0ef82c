"""GP layer objects: the stheno subset GPAR drives, computed on the MI355X through the engine seam.

The reference treats a layer as `(GP, noise)` and uses exactly these operations on it
(/root/reference/gpar/model.py): `f(x, noise)` -> finite-dimensional distribution (:264,270,287,289),
`Obs(fdd, y)` / `PseudoObs(f(x_ind), fdd, y)` (:286-289), `f.measure.logpdf(obs)` (:226), `f | obs` (:170,232,298),
`.mean(x)` (:299,301), `fdd.sample()` (:235,264,270) and, in its tests, `fdd.logpdf(y)` and `f | (fdd, y)`.
This module provides those names with the same call signatures; the arithmetic is

  exact GP (Rasmussen & Williams alg. 2.1), evaluated with ONE partial Cholesky of an augmented matrix

        [ K + D + eps I      .  ]   factor the first n columns     [ L          . ]
        [ r^T                0  ]   ------------------------>      [ (L^-1 r)^T   -|L^-1 r|^2 ]

    which yields log|K|, the quadratic form and L in a single device pipeline (include/gpar_hip.h:
    gpar_potrf); posterior moments at new inputs are V = K_*x L^-T (TRSM), mean = V (L^-1 r),
    cov = K_** - V V^T (SYRK);

  inducing points (Titsias 2009, VFE; stheno's PseudoObs default):  L_z = chol(K_zz), B^T = K_xz L_z^-T,
    A = I + B D^-1 B^T, bound = -1/2 [ sum_j (k_jj - |B_:j|^2)/d_j + sum_j log(2 pi d_j) + log|A| + r^T D^-1 r - |L_A^-1 B D^-1 r|^2 ].

A process is either the prior (zero mean, kernel k) or a posterior `g | obs`, whose mean and kernel are those of the
process the observations were made of, corrected by the observations:

    dense obs   mean + V_a (L^-1 r),        k(a, b) - V_a V_b^T,                 V_a = k(a, X) L^-T
    sparse obs  mean + k(a, Z) v,           k(a, b) - P_a P_b^T + Q_a Q_b^T,     P_a = k(a, Z) L_z^-T, Q_a = P_a L_A^-T

so observations of a posterior (a posterior log-density; conditioning twice) work for every combination of dense and
inducing-point observations by recursion over the chain (`GP._moments_into / _cross / _diag / _mean_at`); the common
cases - observations of the prior, dense observations of a dense posterior - keep their one-factorisation fast paths.

All heavy steps are engine primitives (HIP kernels); torch is used here only for O(n) vector plumbing.
"""
import contextlib
import os
import math

import numpy as np
import torch

from ._lib import CHOL_UPDATE_MAX_RANK, GPAR_MAX_TERMS
from .engine import get_engine, joining
from .heldout import (Folds, Loo, Origins, Purged, Window, fold_offsets, hold_extents, horizon_weight_array, origin_array, origins_array,
                      window_arrays)
from .kernels import Kernel

__all__ = ["Measure", "GP", "FDD", "Obs", "PseudoObs", "PseudoObsVFE", "PseudoObsFITC", "PseudoObsDTC", "SparseObs", "greedy_inducing"]

_LOG_2PI = math.log(2.0 * math.pi)


def one_call_grad_rows():
    """Layers with at most this many rows evaluate their training objective and its gradient through ONE library call
    (gpar_logpdf_dense_grad; GPAR_ONE_CALL_GRAD_ROWS, 0 = never): the same launches, without ~30 host-side steps and two of the
    three synchronisations around them.  Above, the host's share of an evaluation is negligible and the two-step form lets the
    factor be reused."""
    return int(os.environ.get("GPAR_ONE_CALL_GRAD_ROWS", "4096"))


def fused_terms():
    """GPAR_FUSED_TERMS=0: the decomposition by kernel component (`Obs.components`) through the composed route - one sub-kernel, Gram
    matrix and solve per component - on every engine; default: one library call (gpar_posterior_terms) where the engine has it."""
    return os.environ.get("GPAR_FUSED_TERMS", "1") != "0"


def fused_pathwise():
    """GPAR_FUSED_PATHWISE=0: pathwise sampling (`Obs.pathwise_sample_batch`) through the composed route - `pathwise.feature_map`, torch
    cos / sin, `eng.gram` + `eng.gemm` in chunks - on every engine; default: the two library calls (gpar_rff_apply,
    gpar_gram_apply_groups) where the engine has them."""
    return os.environ.get("GPAR_FUSED_PATHWISE", "1") != "0"


def _as_matrix(eng, x):
    """Engine tensor of rank 2 (`B.uprank`: a vector becomes a column)."""
    t = eng.tensor(x)
    if t.dim() == 0:
        t = t.reshape(1, 1)
    elif t.dim() == 1:
        t = t[:, None]
    return t


def _noise_vector(eng, noise, n):
    """None | scalar | length-n vector -> device vector of length n (or None)."""
    if noise is None:
        return None
    t = eng.tensor(noise)
    if t.dim() == 0 or t.numel() == 1:
        return t.reshape(1).expand(n).contiguous()
    t = t.reshape(-1)
    if t.numel() != n:
        raise ValueError(f"noise has {t.numel()} entries for {n} inputs")
    return t.contiguous()


def _zeros(n, like):
    return torch.zeros(n, 1, dtype=torch.float64, device=like.device)


class _Pts:
    """A set of inputs together with the compiled kernel and their features under it (shared by every process of one
    conditioning chain: conditioning changes the mean and the kernel's correction terms, not the base kernel)."""

    __slots__ = ("x", "ck", "z", "n")

    def __init__(self, eng, kernel, x):
        self.x = x
        self.n = int(x.shape[0])
        self.ck = eng.compile(kernel, x.shape[1])
        self.z = eng.features(self.ck, x)


class _Factor:
    """Cholesky of an n x n SPD matrix together with the solve against one right-hand side, from one partial
    factorisation of the (n + 1) x (n + 1) augmented matrix.  `fill(block)` must write the lower triangle of the
    SPD matrix into `block` (an n x n view) and return the vector to subtract from `rhs` (or None)."""

    def __init__(self, eng, n, fill, rhs):
        self.eng, self.n = eng, n
        A = eng.new_matrix(n + 1, n + 1)
        logdet = torch.zeros(1, dtype=torch.float64, device=A.device)
        scale = 1.0
        while n > 0:
            shift = fill(A[:n, :n], scale)
            row = rhs.reshape(-1)
            A[n, :n] = row if shift is None else row - shift.reshape(-1)
            A[n, n].zero_()  # (NOT `A[n, n] = 0.0`: a Python scalar assigned by index goes through a CPU tensor, a
            #                   synchronous host-to-device copy queued behind everything on the stream - a hidden host sync)
            logdet, info = eng.potrf_(A, nf=n)
            if not _retrying(eng, info, scale):
                break
            scale *= 10.0  # lab's Cholesky retry: jitter x 10 (B.cholesky_retry_factor)
        if n == 0:
            A[n, n].zero_()
        self.A = A
        self.L = A[:n, :n]
        self.zrow = A[n : n + 1, :n]  # (L^-1 rhs)^T, 1 x n
        self.logdet = logdet
        self.quad = -A[n, n]  # |L^-1 rhs|^2 (device scalar)
        self._alpha = None

    @classmethod
    def from_batch(cls, eng, n, A, logdet):
        """The factor of one layer out of a lock-step batch (HipEngine.factor_dense_batch): `A` its (n + 1) x (n + 1) block,
        `logdet` its word."""
        self = cls.__new__(cls)
        self.eng, self.n = eng, n
        self.A = A
        self.L = A[:n, :n]
        self.zrow = A[n : n + 1, :n]
        self.logdet = logdet
        self.quad = -A[n, n]
        self._alpha = None
        return self

    @classmethod
    def placeholder(cls, eng, n):
        """Buffers of a factor that another process computes (parallel.sharded_condition receives into `A`)."""
        self = cls.__new__(cls)
        self.eng, self.n = eng, n
        self.A = eng.new_matrix(n + 1, n + 1)
        self.L = self.A[:n, :n]
        self.zrow = self.A[n : n + 1, :n]
        self.logdet = None  # not exchanged: a received factor serves posterior means / samples, not logpdf
        self.quad = None
        self._alpha = None
        return self

    def logpdf(self):
        """-1/2 (log|S| + n log 2 pi + rhs^T S^-1 rhs) as a 0-d tensor: on the CPU (synchronises), or left on the
        device while the engine is deferring checks (the caller then reads the sum of many layers once)."""
        val = (-0.5 * (self.logdet[0] + self.n * _LOG_2PI + self.quad)).detach()
        return val if getattr(self.eng, "_deferred", None) is not None else val.cpu()

    def alpha(self):
        """S^-1 rhs as a row (1 x n): alpha^T = z^T L^-1."""
        if self._alpha is None:
            a = self.zrow.clone()
            if self.n > 0:
                self.eng.trsm_rln_(self.L, a)
            self._alpha = a
        return self._alpha


def _retrying(eng, info, scale):
    """Record / check the verdict of a factorisation.  True: it failed and lab's retry rule (engine.cholesky_retry_factor)
    allows another attempt with ten times the jitter."""
    from .engine import NotPositiveDefiniteError

    limit = getattr(eng, "cholesky_retry_factor", 1.0)
    if limit <= 1.0:
        eng.check_info(info)  # possibly deferred: no host sync
        return False
    try:
        eng._raise_for(info)  # synchronises: a retry needs the verdict now
    except NotPositiveDefiniteError:
        if scale * 10.0 > limit:
            raise
        return True
    return False


@contextlib.contextmanager
def _on_side(stream):
    """Run the block on `stream` after everything enqueued on the current stream so far."""
    stream.wait_stream(torch.cuda.current_stream(stream.device))
    with torch.cuda.stream(stream):
        yield


def _join_side(stream, *tensors):
    """The current stream waits for `stream`; tensors allocated there are handed over to the current stream."""
    main = torch.cuda.current_stream(stream.device)
    main.wait_stream(stream)
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            t.record_stream(main)


def _needs_grad(v):
    return isinstance(v, torch.Tensor) and v.requires_grad


def kernel_parameters(kernel):
    """(kind, term index, factor index, tensor) for every kernel parameter that is a torch tensor requiring grad."""
    out = []
    for ti, term in enumerate(kernel.terms):
        if _needs_grad(term.coef):
            out.append(("coef", ti, None, term.coef))
        for fi, f in enumerate(term.factors):
            for kind in ("scales", "periods", "alpha"):
                v = getattr(f, kind)
                if _needs_grad(v):
                    out.append((kind, ti, fi, v))
    return out


def _param_grads(params, shapes, grads, scale):
    """Gradient dictionary of an engine pass (coef / per-factor scales, periods, alpha) -> one tensor per kernel parameter."""
    outs = []
    for (kind, ti, fi, tensor), shape in zip(params, shapes):
        if kind == "coef":
            val = np.asarray(grads["coef"][ti])
        else:
            val = np.asarray(grads["factors"][ti][fi][kind], dtype=np.float64)
        numel = int(np.prod(shape)) if shape else 1
        if val.size != numel:
            val = val.sum()  # a scalar parameter broadcast over several features
        outs.append(torch.as_tensor(np.asarray(val, dtype=np.float64) * scale, dtype=tensor.dtype).reshape(shape).to(tensor.device))
    return outs


def _add_grads(a, b):
    """Sum of two engine gradient dictionaries of the same kernel."""
    if a is None:
        return b
    out = {"coef": [x + y for x, y in zip(a["coef"], b["coef"])], "factors": []}
    for fa, fb in zip(a["factors"], b["factors"]):
        out["factors"].append([{k: (None if ga[k] is None else np.asarray(ga[k]) + np.asarray(gb[k])) for k in ga} for ga, gb in zip(fa, fb)])
    return out


def _shaped_noise_grad(noise_grad, shape, device):
    numel = int(np.prod(shape)) if shape else 1
    out = noise_grad.sum().reshape(shape) if numel == 1 else noise_grad.reshape(shape)
    return out.to(device)


class _LogMarginal(torch.autograd.Function):
    """log N(y; 0, K_theta(X) + D) - or, for inducing-point observations, the VFE / DTC bound - as a differentiable
    function of the kernel parameters, the noise vector and (when they are themselves functions of hyper-parameters: fed
    forward posterior means, or inducing inputs being optimised) the inputs X and inducing inputs Z.

    Forward is the fused Gram + augmented Cholesky on the device.  Backward is analytic:
    with W = alpha alpha^T - K^-1,  d/dtheta = 1/2 sum_ab W_ab dK_ab/dtheta and d/dX = 1/2 d/dX sum_ab W_ab k(x_a, x_b);
    K^-1 comes from L (TRSM on the identity + SYRK), the kernel-parameter sums from one fused pass over W, the input
    gradients from a second one (csrc/gram.h).  torch then chains these through whatever produced the arguments (bound
    transforms, noise / w, `_update_inputs`' concatenations, `_PosteriorMean`).
    """

    @staticmethod
    def forward(ctx, obs, noise, X, Z, *tensors):
        ctx.obs = obs
        ctx.noise_shape = None if noise is None else tuple(noise.shape)
        ctx.shapes = [tuple(t.shape) for t in tensors]
        return obs._value()

    @staticmethod
    def backward(ctx, g):
        obs = ctx.obs
        noise_grad, grads = obs.gradients()
        gval = float(g)
        out_noise = None
        if ctx.noise_shape is not None:
            out_noise = _shaped_noise_grad(noise_grad * gval, ctx.noise_shape, obs._noise_device)
        gX = gZ = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            gX, gZ = obs.input_gradients(ctx.needs_input_grad[2], ctx.needs_input_grad[3])
            gX = None if gX is None else gX * gval
            gZ = None if gZ is None else gZ * gval
        # the weights of the backward pass (n x n for dense observations: 2 GB at n = 16384) are not needed again
        for name in ("_W", "_weights"):
            if hasattr(obs, name):
                delattr(obs, name)
        return (None, out_noise, gX, gZ, *_param_grads(obs._params, ctx.shapes, grads, gval))


class _HeldOutValue(torch.autograd.Function):
    """A cross-validation value of dense observations of a prior process as a differentiable function of the kernel parameters and the
    noise vector, under a held-out `scheme` (`heldout`): leave-one-out, sum_i log N(y_i; mean_-i, var_-i) (Rasmussen & Williams 5.4.2),
    the blocked value sum_F log N(y_F; mean_-F, cov_-F) over contiguous folds F, or a forecast score over rolling origins.  Forward:
    `Obs._held_out_eval`; `score` is the rule the held-out entries are scored by (`_score_rows`).  Backward: the same weighted-sum pass as `_LogMarginal`, on other weights - d/dtheta = 1/2 sum_ab W_ab
    dK_ab/dtheta with W = alpha u^T + u alpha^T - 2 K^-1 C K^-1, C diagonal or block-diagonal (`Obs._held_out_gradients`).  The inputs are
    not differentiated."""

    @staticmethod
    def forward(ctx, obs, scheme, score, noise, *tensors):
        ctx.obs = obs
        ctx.noise_shape = None if noise is None else tuple(noise.shape)
        ctx.shapes = [tuple(t.shape) for t in tensors]
        return obs._held_out_eval(scheme, want_grad=True, score=score)

    @staticmethod
    def backward(ctx, g):
        obs = ctx.obs
        noise_grad, grads = obs._held_out_gradients()
        gval = float(g)
        out_noise = None
        if ctx.noise_shape is not None:
            out_noise = _shaped_noise_grad(noise_grad * gval, ctx.noise_shape, obs._noise_device)
        return (None, None, None, out_noise, *_param_grads(obs._params, ctx.shapes, grads, gval))


SCORES = ("log", "crps", "se")


def check_score(score):
    """The scoring rules of `loo` and `ahead`: "log" (the Gaussian log density), "crps" (minus the continuous ranked probability score)
    and "se" (minus the squared error); every value is one to maximise."""
    if score not in SCORES:
        raise ValueError('score must be "log", "crps" or "se"')
    return score


def _score_rows(score, e, v):
    """(term, q, s) of held-out entries with errors e = y - mean and variances v under a scoring rule: what an entry adds to the value,
    q = -dterm/de and s = -dterm/dv, the two sensitivities the gradient chains of `loo` and `ahead` run on (csrc/score.h has the
    table).  With z = e / sqrt v: the CRPS of a Gaussian is sqrt v [z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt pi] (Gneiting & Raftery 2007)."""
    if score == "crps":
        sd = torch.sqrt(v)
        z = e / sd
        two_pdf = math.sqrt(2.0 / math.pi) * torch.exp(-0.5 * (z * z))
        q = torch.erf(z * math.sqrt(0.5))
        return -sd * (z * q + (two_pdf - 1.0 / math.sqrt(math.pi))), q, (two_pdf - 1.0 / math.sqrt(math.pi)) / (2.0 * sd)
    if score == "se":
        return -(e * e), 2.0 * e, torch.zeros_like(e)
    q = e / v
    return -0.5 * (_LOG_2PI + torch.log(v) + e * q), q, 0.5 * (1.0 / v - q * q)


def _fold_groups(starts, device):
    """Folds of equal size share batched block algebra: [(size m, k x m index tensor of the rows of the k folds of that size)]."""
    sizes, first = np.diff(starts), starts[:-1]
    return [(int(m), torch.as_tensor(first[sizes == m][:, None] + np.arange(m)[None, :], dtype=torch.long, device=device))
            for m in np.unique(sizes)]


# The block algebra of the two cross-validation values from K^-1 and alpha, where no library call takes the evaluation: (value - under
# the log score without its -n/2 log 2 pi -, the errors y - mean, b, variances, a function filling S with K^-1 R for the gradient's
# product S S^T = K^-1 C K^-1, C = R R^T).
def _loo_algebra(Kinv, alpha, score="log"):
    """Leave-one-out: the diagonal, in closed form.  With e = alpha / d, v = 1 / d and the rule's (q, s): b = q v, C = diag(q e v + s v^2);
    under the log score b = e, C = diag(1/2 (v + e^2))."""
    d = torch.diagonal(Kinv)
    e = alpha / d
    if score == "log":
        b = e

        def fill(S):
            S.copy_(Kinv * torch.sqrt(0.5 * (1.0 / d + b * b))[None, :])

        return torch.sum(0.5 * torch.log(d) - 0.5 * alpha * b), e, b, 1.0 / d, fill
    v = 1.0 / d
    term, q, s = _score_rows(score, e, v)

    def fill(S):
        S.copy_(Kinv * torch.sqrt(q * e * v + s * (v * v))[None, :])

    return torch.sum(term), e, q * v, v, fill


def _cv_algebra(eng, Kinv, alpha, starts):
    """Folds of any size: batched Cholesky over the folds of equal size.  b_F = D_F^-1 alpha_F, C = blockdiag(1/2 (D_F^-1 + b_F b_F^T))."""
    n = alpha.numel()
    b, var = torch.empty_like(alpha), torch.empty_like(alpha)
    value = torch.zeros((), dtype=torch.float64, device=alpha.device)
    blocks = []
    for m, idx in _fold_groups(starts, alpha.device):
        D = Kinv[idx[:, :, None], idx[:, None, :]]   # k x m x m
        G, info = torch.linalg.cholesky_ex(D)
        eng.check_info(info.max().reshape(1).to(torch.int32))   # (one word: the largest failing pivot of the group, 0 if none)
        Dinv = torch.cholesky_inverse(G)
        a_f = alpha[idx]
        b_f = torch.matmul(Dinv, a_f[:, :, None])[:, :, 0]
        b[idx], var[idx] = b_f, torch.diagonal(Dinv, dim1=1, dim2=2)
        value = value + torch.sum(torch.log(torch.diagonal(G, dim1=1, dim2=2))) - 0.5 * torch.sum(a_f * b_f)
        blocks.append((idx, Dinv, b_f))

    def fill(S):
        for idx, Dinv, b_f in blocks:   # S[:, F] = K^-1[:, F] R_F
            R = torch.linalg.cholesky(0.5 * (Dinv + b_f[:, :, None] * b_f[:, None, :]))
            cols = torch.matmul(Kinv[:, idx].permute(1, 0, 2), R)   # k x n x m
            S[:, idx.reshape(-1)] = cols.permute(1, 0, 2).reshape(n, -1)

    return value, b, b, var, fill


class _DenseC:
    """What `_cv_gap_algebra` hands the gradient in the place of a function filling S: C itself, which is indefinite - no S S^T."""

    def __init__(self, C):
        self.C = C


def _cv_gap_algebra(eng, Kinv, alpha, purged):
    """Purged folds with blocks of any size: batched algebra over the folds of equal (|F|, |G left|, |G right|).  Per fold, with the block
    P_HH ordered (G, F) and factored, P_HH = L L^T, N = L^-1, w = N alpha_H: the leading pivots factor P_GG and the trailing ones the
    Schur complement Dt, so value term = sum_F log L_ii - 1/2 |w_F|^2; e = N^T w = P_HH^-1 alpha_H holds y_F - mean on F; the predictive
    covariance is N_FF^T N_FF; b_H = N_F^T w_F, g = e - b_H = N_G^T w_G and C_H = 1/2 (N_F^T N_F + e e^T - g g^T).  The
    blocks of neighbouring folds overlap: b and C are summed group by group, the folds of a group chosen with disjoint blocks, so that
    every sum has a fixed order."""
    n, dev = alpha.numel(), alpha.device
    starts, lo, hi = purged.starts, purged.lo, purged.hi
    first, end = starts[:-1], starts[1:]
    err, var, b = torch.empty_like(alpha), torch.empty_like(alpha), torch.zeros_like(alpha)
    C = torch.zeros(n, n, dtype=torch.float64, device=dev)
    value = torch.zeros((), dtype=torch.float64, device=dev)
    colour, reach = np.zeros(first.size, dtype=np.int64), []   # (greedy: the first colour whose last block ends before this one begins)
    for f in range(first.size):
        c = next((c for c, h in enumerate(reach) if h <= lo[f]), len(reach))
        reach[c:c + 1] = [hi[f]]
        colour[f] = c
    shape = np.stack([end - first, first - lo, hi - end, colour], axis=1)
    for m, gl, gr, c in np.unique(shape, axis=0):
        fs = np.nonzero(np.all(shape == [m, gl, gr, c], axis=1))[0]
        g = int(gl + gr)
        rows = np.concatenate([lo[fs, None] + np.arange(gl), end[fs, None] + np.arange(gr), first[fs, None] + np.arange(m)], axis=1)
        idx = torch.as_tensor(rows, dtype=torch.long, device=dev)   # k x |H|, in the block's order
        L, info = torch.linalg.cholesky_ex(Kinv[idx[:, :, None], idx[:, None, :]])
        eng.check_info(info.max().reshape(1).to(torch.int32))
        N = torch.linalg.solve_triangular(L, torch.eye(g + int(m), dtype=torch.float64, device=dev).expand_as(L), upper=False)
        w = torch.matmul(N, alpha[idx][:, :, None])
        NF = N[:, g:, :]
        b_h = torch.matmul(NF.transpose(1, 2), w[:, g:])[:, :, 0]
        g_h = torch.matmul(N[:, :g, :].transpose(1, 2), w[:, :g])[:, :, 0]
        e_h = b_h + g_h
        F = idx[:, g:]
        err[F], var[F] = e_h[:, g:], torch.sum(NF[:, :, g:] ** 2, dim=1)
        value = value + torch.sum(torch.log(torch.diagonal(L, dim1=1, dim2=2)[:, g:])) - 0.5 * torch.sum(w[:, g:] ** 2)
        b[idx] = b[idx] + b_h
        at = (idx[:, :, None], idx[:, None, :])
        C[at] = C[at] + 0.5 * (torch.matmul(NF.transpose(1, 2), NF) + e_h[:, :, None] * e_h[:, None, :] - g_h[:, :, None] * g_h[:, None, :])
    return value, err, b, var, _DenseC(C)


def _rank_two_weights(eng, Kinv, alpha, b, fill):
    """W = alpha u^T + u alpha^T - 2 K^-1 C K^-1 on its lower triangle, u = K^-1 b, from what `_loo_algebra`, `_cv_algebra` or
    `_cv_gap_algebra` returned: S with C = R R^T, K^-1 C K^-1 = S S^T - or C itself -, then the rank-two update."""
    n = alpha.numel()
    u = eng.gemv_t(Kinv, b).reshape(-1)   # K^-1 b (K^-1 is symmetric)
    S = eng.new_matrix(n, n)
    W = eng.new_matrix(n, n)
    if isinstance(fill, _DenseC):   # purged folds: C is indefinite and banded, not block-diagonal R R^T:  K^-1 C K^-1 as K^-1 (C K^-1)
        P, Cm = eng.new_matrix(n, n), eng.new_matrix(n, n)
        P.copy_(Kinv)
        Cm.copy_(fill.C)
        eng.gemm(Cm, P, out=S)
        eng.gemm(P, S, alpha=-2.0, out=W, c_lower=True)
        del P, Cm
    else:
        fill(S)
        eng.gemm(S, S, tb=True, alpha=-2.0, out=W, c_lower=True)
    left, right = eng.new_matrix(2, n), eng.new_matrix(2, n)
    left.copy_(torch.stack([alpha, u]))
    right.copy_(torch.stack([u, alpha]))
    eng.gemm(left, right, ta=True, alpha=1.0, beta=1.0, out=W, c_lower=True)
    return W


def _ahead_algebra(eng, L, a, origin, score="log"):
    """Rolling-origin forecasts from the factor L and a = L^-1 y, where no library call takes the evaluation: (value, e = y - mean, v with
    NaN on unscored rows, a function returning the weights W on their lower triangle from K^-1).  Row r is predicted from rows
    0 ... origin[r] - 1: e_r = sum_{c = origin[r] .. r} L_rc a_c, v_r = sum L_rc^2; `score` turns (e_r, v_r) into the value term and
    the sensitivities q_r, s_r (`_score_rows`).  The weights follow the reverse mode of the Cholesky
    factorisation: W = L^-T (P + P^T) L^-1 = K^-1 [L (P + P^T) L^T] K^-1, P = Phi(L^T B - abar a^T), in products both engines have."""
    n, dev = a.numel(), a.device
    o = torch.as_tensor(origin, device=dev)
    scored = o >= 0
    cols = torch.arange(n, device=dev)
    band = scored[:, None] & (cols[None, :] >= o[:, None]) & (cols[None, :] <= cols[:, None])
    Lb = torch.where(band, torch.tril(L), torch.zeros((), dtype=torch.float64, device=dev))
    e = torch.sum(Lb * a[None, :], dim=1)
    v = torch.where(scored, torch.sum(Lb * Lb, dim=1), torch.ones((), dtype=torch.float64, device=dev))
    term, q, s_rows = _score_rows(score, e, v)
    value = torch.sum(torch.where(scored, term, torch.zeros((), dtype=torch.float64, device=dev)))
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)

    def weights(Kinv):
        s = torch.where(scored, s_rows, torch.zeros((), dtype=torch.float64, device=dev))
        B = eng.new_matrix(n, n)
        B.copy_(torch.where(band, -q[:, None] * a[None, :] - 2.0 * s[:, None] * Lb, torch.zeros((), dtype=torch.float64, device=dev)))
        abar = -torch.sum(Lb * q[:, None], dim=0)
        Lt = eng.new_matrix(n, n)
        Lt.copy_(torch.tril(L))
        raw = torch.tril(eng.gemm(Lt, B, ta=True) - abar[:, None] * a[None, :])
        S = eng.new_matrix(n, n)
        S.copy_(raw + torch.tril(raw, -1).T)            # P + P^T (Phi halves the diagonal, the sum restores it)
        G = eng.gemm(eng.gemm(Lt, S), Lt, tb=True)       # L (P + P^T) L^T
        W = eng.new_matrix(n, n)
        eng.gemm(eng.gemm(Kinv, G), Kinv, out=W, c_lower=True)
        return W

    return value, e, torch.where(scored, v, nan), scored, weights


def _ahead_window_algebra(eng, K, y, lo, origin, score="log"):
    """Sliding-window forecasts from the covariance K = k + D + eps I itself (symmetric, whole), where no library call takes the evaluation:
    (value, e = y - mean, v with NaN on unscored rows, scored, a function returning the weights W).  Per scored row r the block J = (lo[r]
    ... origin[r] - 1, r) is gathered and factored, K_JJ = G G^T with r last: z = G^-1 y_J, e_r = G_rr z_r, v_r = G_rr^2; `score` turns them
    into the value term and the sensitivities q_r, s_r (`_score_rows`); c = G_rr G^-T e_r = [-K_SS^-1 k_Sr; 1], p = [K_SS^-1 y_S; 0] and
    the row adds W^r = -2 s_r c c^T + q_r (p c^T + c p^T) on J.  Rows with windows of equal length share batched Cholesky algebra, as
    `_fold_groups` groups folds; the blocks of neighbouring rows overlap, so W is summed group by group, the rows of a group chosen
    with disjoint blocks - every sum has a fixed order (as `_cv_gap_algebra` sums C).  Windows of any length."""
    n, dev = y.numel(), y.device
    lo, origin = np.asarray(lo, dtype=np.int64), np.asarray(origin, dtype=np.int64)
    rows = np.nonzero(origin >= 0)[0]
    scored = torch.as_tensor(origin >= 0, device=dev)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    e, v = torch.zeros(n, dtype=torch.float64, device=dev), torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    value = torch.zeros((), dtype=torch.float64, device=dev)
    colour, reach = np.zeros(rows.size, dtype=np.int64), []   # (greedy: the first colour whose last block ends before this one begins)
    for k, r in enumerate(rows):
        c = next((c for c, h in enumerate(reach) if h < lo[r]), len(reach))
        reach[c:c + 1] = [r]
        colour[k] = c
    shape = np.stack([origin[rows] - lo[rows], colour], axis=1) if rows.size else np.zeros((0, 2), dtype=np.int64)
    parts = []
    for m, c in np.unique(shape, axis=0):
        rs = rows[np.all(shape == [m, c], axis=1)]
        m = int(m)
        idx = torch.as_tensor(np.concatenate([lo[rs, None] + np.arange(m), rs[:, None]], axis=1), dtype=torch.long, device=dev)   # k x (m + 1)
        G, info = torch.linalg.cholesky_ex(K[idx[:, :, None], idx[:, None, :]])
        eng.check_info(info.max().reshape(1).to(torch.int32))   # (one word: the largest failing pivot of the group, 0 if none)
        z = torch.linalg.solve_triangular(G, y[idx][:, :, None], upper=False)[:, :, 0]
        g = G[:, m, m]
        at = torch.as_tensor(rs, dtype=torch.long, device=dev)
        e_g, v_g = g * z[:, m], g * g
        term, q, s = _score_rows(score, e_g, v_g)
        e[at], v[at] = e_g, v_g
        value = value + torch.sum(term)
        parts.append((idx, G, z, g, q, s, m))

    def weights():
        W = torch.zeros(n, n, dtype=torch.float64, device=dev)
        for idx, G, z, g, q, s, m in parts:
            unit = torch.zeros(idx.shape[0], m + 1, 1, dtype=torch.float64, device=dev)
            unit[:, m, 0] = g
            c = torch.linalg.solve_triangular(G.transpose(1, 2), unit, upper=True)[:, :, 0]
            p = torch.zeros_like(c)
            if m:
                p[:, :m] = torch.linalg.solve_triangular(G[:, :m, :m].transpose(1, 2), z[:, :m, None], upper=True)[:, :, 0]
            pc = p[:, :, None] * c[:, None, :]
            block = -2.0 * s[:, None, None] * (c[:, :, None] * c[:, None, :]) + q[:, None, None] * (pc + pc.transpose(1, 2))
            at = (idx[:, :, None], idx[:, None, :])
            W[at] = W[at] + block
        out = eng.new_matrix(n, n)
        out.copy_(W)
        return out

    return value, e, torch.where(scored, v, nan), scored, weights


class _PosteriorMean(torch.autograd.Function):
    """Posterior mean of `f | obs` at x* as a differentiable function of the kernel parameters, the noise, the training
    inputs X, the inducing inputs Z and x* itself: the column `_update_inputs` feeds to the next layer
    (reference gpar/model.py:291-322, differentiated by torch autograd there when fit(fix=False) trains layers jointly).
    Backward: `Obs.mean_gradients` / `PseudoObs.mean_gradients` (weighted kernel-derivative passes on the device)."""

    @staticmethod
    def forward(ctx, obs, xs_value, xs, noise, X, Z, *tensors):
        ctx.obs, ctx.xs = obs, xs_value
        ctx.noise_shape = None if noise is None else tuple(noise.shape)
        ctx.noise_device = None if noise is None else noise.device
        ctx.shapes = [tuple(t.shape) for t in tensors]
        ctx.params = kernel_parameters(obs.base.kernel)
        return obs.mean_at(obs.base._pts(xs_value))

    @staticmethod
    def backward(ctx, g):
        obs = ctx.obs
        need = ctx.needs_input_grad
        out = obs.mean_gradients(ctx.xs, g.detach().reshape(-1), want_xs=need[2], want_x=need[4], want_z=need[5])
        g_noise = None if ctx.noise_shape is None else _shaped_noise_grad(out["noise"], ctx.noise_shape, ctx.noise_device)
        return (None, None, out.get("xs"), g_noise, out.get("x"), out.get("z"), *_param_grads(ctx.params, ctx.shapes, out["params"], 1.0))


class Measure:
    """Stand-in for stheno's `Measure`: only `logpdf` is used by GPAR (model.py:226)."""

    def logpdf(self, *args):
        if len(args) == 1:
            return args[0].logpdf()
        fdd, y = args
        return fdd.logpdf(y)


class GP:
    """Gaussian process with a `gpar_amd.kernels.Kernel`: the zero-mean prior, or (after `f | obs`) a posterior."""

    def __init__(self, kernel, measure=None, engine=None, _obs=None):
        if not isinstance(kernel, Kernel):
            raise TypeError("kernel must be a gpar_amd.kernels.Kernel")
        self.kernel = kernel
        self.measure = measure if measure is not None else Measure()
        self._engine = engine
        self._obs = _obs  # None: prior process

    @property
    def engine(self):
        return self._engine if self._engine is not None else get_engine()

    @property
    def is_posterior(self):
        return self._obs is not None

    def __call__(self, x, noise=None):
        return FDD(self, x, noise)

    def __or__(self, obs):
        if isinstance(obs, tuple):
            obs = Obs(*obs)
        if not isinstance(obs, (Obs, PseudoObs)):
            raise TypeError("can only condition on Obs / PseudoObs or a (fdd, y) tuple")
        if obs.base.kernel is not self.kernel:
            raise ValueError("observations belong to a different process")
        if obs.base is not self:
            if not (obs.base.is_posterior or self.is_posterior):
                obs = obs.rebased(self)  # another handle of the same prior
            else:
                raise ValueError("observations must be made of the process that is being conditioned")
        if self.is_posterior and isinstance(obs, Obs) and isinstance(self._obs, Obs) and not self._obs.base.is_posterior:
            # dense on dense: one factorisation of the stacked observations of the prior
            return GP(self.kernel, measure=Measure(), engine=self._engine, _obs=self._obs.merged_with(obs))
        return GP(self.kernel, measure=Measure(), engine=self._engine, _obs=obs)

    # ---- process primitives (recursive over the conditioning chain) ---------------------------------
    def _pts(self, x):
        eng = self.engine
        return _Pts(eng, self.kernel, _as_matrix(eng, x))

    def _mean_at(self, p):
        if not self.is_posterior or p.n == 0:
            return _zeros(p.n, p.x)
        return self._obs.mean_at(p)

    def _cross(self, pa, pb, row_scale=None):
        """k(a, b) as a new na x nb matrix (rows optionally scaled)."""
        if not self.is_posterior:
            return self.engine.gram(pa.ck, pa.z, pb.z, row_scale=row_scale)
        K = self._obs.cross(pa, pb)
        if row_scale is not None:
            K.mul_(row_scale[:, None])
        return K

    def _diag(self, p):
        """k(a, a) for every row of p (vector)."""
        if not self.is_posterior:
            return self.engine.gram_diag(p.ck, p.z)
        return self._obs.diag(p)

    def _moments_into(self, p, block, diag_add=None, jitter=0.0):
        """Lower triangle of k(p, p) + diag(diag_add) + jitter I into `block`; returns the mean at p (n x 1)."""
        if not self.is_posterior:
            self.engine.gram(p.ck, p.z, lower=True, diag_add=diag_add, diag_const=jitter, out=block)
            return _zeros(p.n, p.x)
        return self._obs.moments_into(p, block, diag_add, jitter)

    # ---- public ------------------------------------------------------------------------------------
    def mean(self, x):
        eng = self.engine
        xm = _as_matrix(eng, x)
        if self.is_posterior and torch.is_grad_enabled() and not self._obs.base.is_posterior and xm.shape[0] > 0 and self._obs.fdd.n > 0:
            obs = self._obs
            params = kernel_parameters(self.kernel)
            noise = obs.fdd.noise_arg if _needs_grad(obs.fdd.noise_arg) else None
            X = obs.fdd.x if obs.fdd.x.requires_grad else None
            Z = obs.u.x if isinstance(obs, PseudoObs) and obs.u.x.requires_grad else None
            xs = xm if xm.requires_grad else None
            if params or noise is not None or X is not None or Z is not None or xs is not None:
                return _PosteriorMean.apply(obs, xm.detach(), xs, noise, X, Z, *[p[3] for p in params])
        return self._mean_at(self._pts(xm))

    def marginal_moments(self, x, noise=None):
        """(mean, variance) of f(x) (+ noise) point by point - no n* x n* covariance is formed."""
        p = self._pts(x)
        var = self._diag(p)
        nv = _noise_vector(self.engine, noise, p.n)
        if nv is not None:
            var = var + nv
        return self._mean_at(p), var

    def component_moments(self, x, comp, ncomp, variance=True):
        """(mean, var), each ncomp x n*, of the components of the kernel under the grouping `comp` at x (`Obs.components`), for a process
        conditioned on dense observations of its prior.  Inducing points: ValueError."""
        if isinstance(self._obs, PseudoObs):
            raise ValueError("a decomposition by kernel component needs dense observations: inducing points are not supported")
        if not self.is_posterior:
            raise ValueError("a decomposition by kernel component needs a conditioned process")
        return self._obs.components(self._pts(x), comp, ncomp, variance)

    def derivative_moments(self, x, U, variance=True):
        """(dmean, dvar), each ndir x n*, of the directional derivatives of the process at x along the design-space directions U
        (`Obs.derivatives`), for a process conditioned on dense observations of its prior.  Inducing points: ValueError."""
        if isinstance(self._obs, PseudoObs):
            raise ValueError("posterior derivatives need dense observations: inducing points are not supported")
        if not self.is_posterior:
            raise ValueError("posterior derivatives need a conditioned process")
        return self._obs.derivatives(self._pts(x), U, variance)

    def sample_batch(self, xs, noise=None):
        """One draw of f (+ noise) at each input set in `xs` (a list of n* x D matrices, e.g. the per-sample design
        matrices of ancestral sampling): returns an n* x len(xs) matrix.  For a dense posterior the expensive step -
        V_s = K(x_s, X) L^-T for every s - is ONE stacked triangular solve instead of len(xs) separate ones."""
        if self.is_posterior and (self._obs.fast_dense or getattr(self._obs, "fast_sparse", False)):
            return self._obs.posterior_sample_batch(xs, noise)
        return torch.cat([self(x_s, noise).sample() for x_s in xs], dim=1)

    def marginal_sample_batch(self, xs, noise=None):
        """As `sample_batch`, but every point is drawn from its own marginal N(mean_j, var_j + noise_j) instead of the
        joint law of the n* points: per-point predictive statistics are unchanged, the draws of one sample are
        independent across points.  Needs no n* x n* covariance and no factorisation of one."""
        eng = self.engine
        S = len(xs)
        ns = int(xs[0].shape[0])
        if self.is_posterior and (self._obs.fast_dense or getattr(self._obs, "fast_sparse", False)):
            mean, var = self._obs.posterior_marginals_batch(xs)
        else:
            moments = [self.marginal_moments(x_s) for x_s in xs]
            mean = torch.cat([m for m, _ in moments], dim=1)
            var = torch.stack([v for _, v in moments], dim=1)
        nv = _noise_vector(eng, noise, ns)
        if nv is not None:
            var = var + nv[:, None]
        # eps as the joint sampler's jitter; a variance rounded below zero is clamped
        return mean + torch.sqrt(torch.clamp(var + eng.epsilon, min=0.0)) * eng.randn(ns, S)

    def mean_batch(self, xs):
        if self.is_posterior and (self._obs.fast_dense or getattr(self._obs, "fast_sparse", False)) and len(xs) > 1:
            return self._obs.posterior_mean_batch(xs)
        return [self.mean(x_s) for x_s in xs]

    # convenience used by tests / examples
    def marginals(self, x):
        return self(x).marginals()


class Stacked:
    """`count` input sets of `rows` points each, stacked by rows in ONE matrix: what ancestral sampling hands from layer to layer
    (each sample's design matrix differs in its last columns).  Behaves like the list of its blocks; the batched posterior
    routines take the matrix as it is (one featurize / cross-Gram launch) instead of concatenating a list again."""

    def __init__(self, matrix, count, shared_cols=0):
        self.matrix, self.count = matrix, int(count)
        self.rows = int(matrix.shape[0]) // max(self.count, 1)
        self.shared_cols = int(shared_cols)   # the leading columns that are the same in every set (Stacked.repeat: all of x)

    @classmethod
    def repeat(cls, x, count):
        return cls(x.repeat(count, 1), count, shared_cols=int(x.shape[1]))

    def __len__(self):
        return self.count

    def __getitem__(self, s):
        if isinstance(s, slice):
            a, b, step = s.indices(self.count)
            if step != 1:
                raise IndexError("contiguous slices only")
            return Stacked(self.matrix[a * self.rows : b * self.rows], max(b - a, 0), self.shared_cols)
        if s < 0:
            s += self.count
        return self.matrix[s * self.rows : (s + 1) * self.rows]

    def __iter__(self):
        return (self[s] for s in range(self.count))

    def with_columns(self, cols):
        """A new stack with `cols` appended to every set: rows x count (column s goes to set s) or already stacked
        ((count rows) x k)."""
        if cols.shape[0] == self.rows and cols.shape[0] != self.matrix.shape[0]:
            cols = cols.T.reshape(-1, 1)
        return Stacked(torch.cat([self.matrix, cols], dim=1), self.count, self.shared_cols)


class FDD:
    """`f(x, noise)`: the process at the rows of x, plus independent noise (scalar or per-row vector)."""

    def __init__(self, p, x, noise=None):
        self.p = p
        self.eng = p.engine
        self.x = _as_matrix(self.eng, x)
        self.n = self.x.shape[0]
        self.noise = _noise_vector(self.eng, noise, self.n)
        self.noise_arg = noise  # kept for the autograd path (may carry a graph)
        self._pts = None

    def pts(self):
        """Inputs + compiled kernel + features (cached)."""
        if self._pts is None:
            self._pts = _Pts(self.eng, self.p.kernel, self.x)
        return self._pts

    def features(self):
        p = self.pts()
        return p.ck, p.z

    # ---- moments ---------------------------------------------------------------------------------
    def mean(self):
        return self.p._mean_at(self.pts())

    def _fill_cov(self, block, jitter):
        """Write the lower triangle of cov(f(x)) + diag(noise) + jitter I into `block`; returns the mean (n x 1)."""
        return self.p._moments_into(self.pts(), block, self.noise, jitter)

    def var(self):
        """Dense covariance (including noise), symmetric; for tests and small problems."""
        block = self.eng.new_matrix(self.n, self.n)
        self._fill_cov(block, 0.0)
        low = torch.tril(block)
        return low + torch.tril(low, -1).T

    def marginals(self):
        mean, var = self.p.marginal_moments(self.x, self.noise)
        return mean.reshape(-1), var

    # ---- logpdf / sample ---------------------------------------------------------------------------
    def _factor(self, y):
        eng = self.eng
        y = _as_matrix(eng, y)
        if y.shape[0] != self.n:
            raise ValueError(f"{y.shape[0]} observations for {self.n} inputs")
        return _Factor(eng, self.n, lambda block, scale: self._fill_cov(block, eng.epsilon * scale), y)

    def logpdf(self, y):
        return self._factor(y).logpdf()

    def sample(self, num=1):
        """num draws, one per column: mean + chol(cov + eps I) randn."""
        eng = self.eng
        n = self.n
        if n == 0:
            return torch.zeros(0, num, dtype=torch.float64, device=self.x.device)
        S = eng.new_matrix(n, n)
        scale = 1.0
        while True:
            mean = self._fill_cov(S, eng.epsilon * scale)
            _, info = eng.potrf_(S)
            if not _retrying(eng, info, scale):
                break
            scale *= 10.0
        zr = eng.randn(n, num)
        out = eng.trmv_lower(S, zr) if num == 1 else eng.gemm(S, zr, a_lower=True)
        return out + mean


class Obs:
    """Exact observations `y = f(x) + noise` (stheno `Obs(fdd, y)`) of the process `fdd.p` (prior or posterior)."""

    def __init__(self, fdd, y):
        self.fdd = fdd
        self.eng = fdd.eng
        self.base = fdd.p
        self.y = _as_matrix(self.eng, y)
        if self.y.shape[0] != fdd.n:
            raise ValueError(f"{self.y.shape[0]} observations for {fdd.n} inputs")
        self._fac = None

    @property
    def fast_dense(self):
        """Dense observations of the prior: the stacked / batched posterior routines below apply."""
        return not self.base.is_posterior

    def prior_gp(self):
        p = self.base
        while p.is_posterior:
            p = p._obs.base
        return p

    def rebased(self, gp):
        return Obs(FDD(gp, self.fdd.x, self.fdd.noise_arg), self.y)

    # log marginal likelihood of y under the process the fdd belongs to (prior or posterior)
    def logpdf(self):
        if not self.base.is_posterior and torch.is_grad_enabled():
            params = kernel_parameters(self.base.kernel)
            noise = self.fdd.noise_arg if _needs_grad(self.fdd.noise_arg) else None
            X = self.fdd.x if self.fdd.x.requires_grad else None
            if params or noise is not None or X is not None:
                self._params = params
                self._noise_device = None if noise is None else noise.device
                # value and gradient ingredients in ONE library call when nothing but kernel parameters and noise is differentiated
                self._fuse_grad = X is None and self._fusable_grad()
                return _LogMarginal.apply(self, noise, X, None, *[p[3] for p in params])
        if self._value_only():
            # one library call: features, Gram, observations, factorisation, value (the factor is not kept)
            eng = self.eng
            ck = eng.compile(self.base.kernel, self.fdd.x.shape[1])
            value, info = eng.logpdf_dense(ck, self.fdd.x, self.y, self.fdd.noise, eng.epsilon)
            eng.check_info(info)
            return value.detach()
        return self.factor().logpdf()

    def _value_only(self):
        """The caller wants the number and nothing else (`transient`, set by GPAR.logpdf for layers that feed nobody), of a
        prior process, with checks deferred (the value stays on the device) and no retry ladder to climb."""
        eng = self.eng
        return (getattr(self, "transient", False) and self._fac is None and not self.base.is_posterior and self.fdd.n > 0
                and hasattr(eng, "logpdf_dense") and getattr(eng, "_deferred", None) is not None
                and getattr(eng, "cholesky_retry_factor", 1.0) <= 1.0 and isinstance(self.y, torch.Tensor) and self.y.is_cuda)

    def _fusable_grad(self):
        """The objective-and-gradient entry point applies: dense observations of a prior process, nothing factored yet, checks
        deferred (the value stays on the device), no retry ladder, small enough for the caller's side to matter."""
        eng = self.eng
        return (self._fac is None and not self.base.is_posterior and 0 < self.fdd.n <= one_call_grad_rows() and hasattr(eng, "logpdf_dense_grad")
                and getattr(eng, "_deferred", None) is not None and getattr(eng, "cholesky_retry_factor", 1.0) <= 1.0
                and isinstance(self.y, torch.Tensor) and self.y.is_cuda)

    def _value(self):
        fuse, self._fuse_grad = getattr(self, "_fuse_grad", False), False   # (decided per call by logpdf(): never sticky)
        if fuse and self._fac is None:
            eng = self.eng
            ck = eng.compile(self.base.kernel, self.fdd.x.shape[1])
            value, info, self._fused_gradients, (A, logdet) = eng.logpdf_dense_grad(ck, self.fdd.x.detach(), self.y, self.fdd.noise, eng.epsilon)
            eng.check_info(info)
            # the call leaves the factor behind: a posterior mean / conditioning on these observations (fit(fix=False), replace,
            # imputation) takes it from here instead of factoring the same matrix again
            self._fac = _Factor.from_batch(eng, self.fdd.n, A, logdet)
            return value.detach()
        return self.factor().logpdf()

    def gradients(self):
        """(1/2 diag(W) as a device vector, kernel-parameter gradients) with W = alpha alpha^T - (K + D)^-1."""
        fused = getattr(self, "_fused_gradients", None)
        if fused is not None:
            self._fused_gradients = None
            return fused()
        eng, fac = self.eng, self.factor()
        if hasattr(eng, "chol_inverse_x") and fac.n > 0:
            # alpha = (K + D)^-1 y = X (L^-1 y) with X = L^-T, which the inverse has just formed: a triangular matrix-vector product at
            # memory speed instead of a backward substitution (the launches of gpar_logpdf_dense_grad, same bits)
            W, X = eng.chol_inverse_x(fac.L)  # (K + D)^-1, lower triangle; L^-T, upper triangle
            a = eng.trmv_upper(X, fac.zrow)
            del X
        else:
            W = eng.chol_inverse(fac.L)  # (K + D)^-1, lower triangle
            a = fac.alpha()
        eng.gemm(a, a, ta=True, alpha=1.0, beta=-1.0, out=W, c_lower=True)
        ck, _ = self.fdd.features()
        grads = eng.kernel_grads(ck, self.fdd.x.detach(), W)
        self._W = W
        return 0.5 * torch.diagonal(W).clone(), grads

    # ---- leave-one-out and blocked cross-validation ----------------------------------------------------------
    def loo(self, score="log"):
        """(value, mean, var): the leave-one-out predictive means and variances of the observations - of y_i given all the others,
        mean_-i = y_i - alpha_i / d_i and var_-i = 1 / d_i with alpha = S^-1 (y - m), d = diag S^-1, S = cov(f(X)) + D + eps I - and
        value = sum_i log N(y_i; mean_-i, var_-i), a 0-d tensor that carries a gradient with respect to the kernel parameters and the
        noise where they require one (observations of a prior process; Rasmussen & Williams 5.4.2).  `score`: the rule each held-out
        entry is scored by - "log" as above, "crps": value = -sum_i CRPS(N(mean_-i, var_-i), y_i), "se": value = -sum_i (y_i - mean_-i)^2
        (minus PRESS); mean and var are the same under every rule, and the value is always one to maximise."""
        return self._held_out(Loo(), "leave-one-out", check_score(score))

    def cv(self, fold_start, hold=None):
        """(value, mean, var) of blocked (leave-fold-out) cross-validation over contiguous folds of the observations, given by their
        nfolds + 1 ascending row offsets (0 ... n).  With P = S^-1, alpha = P (y - m) and per fold D_F = P[F, F], b_F = D_F^-1 alpha_F:
        y_F given all other observations ~ N(y_F - b_F, D_F^-1); mean and var hold y_F - b_F and the marginal variances diag D_F^-1, and
        value = sum_F log N(y_F; y_F - b_F, D_F^-1), the JOINT fold densities - a 0-d tensor that carries a gradient with respect to
        the kernel parameters and the noise where they require one (observations of a prior process).  Folds of one row give `loo`;
        one fold of every row gives `logpdf`.  `hold`: purged (hv-block) cross-validation, the observations in the order given (the time
        order) - the pair (hold_lo, hold_hi), one int per fold: fold f is predicted from the rows OUTSIDE hold_lo[f] ... hold_hi[f] - 1, a
        block that contains the fold (`hip.hold_extents`); its other rows are neither scored nor conditioned on.  With G = H without F the
        formulas above hold for Dt = P_FF - P_FG P_GG^-1 P_GF and at = alpha_F - P_FG P_GG^-1 alpha_G in the place of D_F and alpha_F.
        None: the blocks are the folds themselves, today's route.  (`fold_start` may be a `heldout.Folds` or `Purged` made earlier: its
        uploaded arrays are shared.)"""
        if isinstance(fold_start, Folds):
            return self._held_out(fold_start, "cross-validation")
        if hold is None:
            return self._held_out(Folds(fold_offsets(fold_start, self.fdd.n)), "cross-validation")
        return self._held_out(Purged(*hold_extents(fold_start, hold, self.fdd.n)), "cross-validation")

    def ahead(self, origin, score="log", weights=None, lo=None):
        """(value, mean, var) of rolling-origin forecasts, the observations in the order given (the time order): row r is predicted from
        rows 0 ... origin[r] - 1 (origin[r] in 0 ... r; 0: from the prior), origin[r] = -1 leaves it unscored (NaN in mean and var).  mean
        and var are the predictive moments of the noisy observation and value = sum_scored log N(y_r; mean_r, var_r) - a 0-d tensor that
        carries a gradient with respect to the kernel parameters and the noise where they require one (observations of a prior process).
        All of it comes from the ONE factorisation `logpdf` computes; origin[r] = r for every row gives `logpdf`.  `score` as for `loo`:
        "crps" and "se" sum minus the CRPS / minus the squared error of the scored rows instead.

        A K x n `origin` scores K horizons from the one factorisation: mean and var are K x n, value = sum_k weights[k] value_k (`weights`:
        K positive finite numbers, default all 1; with a 1-D origin: ValueError) and the K unweighted value_k are left, detached, in
        `self._held_out_values`.  One library call where `logpdf` would take one and K <= `_lib.AHEAD_MAX_HORIZONS`; otherwise composed of
        `_ahead_algebra`'s terms and weights W, summed over the horizons - any K.

        `lo` (n ints, with a 1-D origin): a sliding window - row r is predicted from rows lo[r] ... origin[r] - 1 ALONE (0 <= lo[r] <=
        origin[r]; lo[r] = origin[r]: from the prior; neither array may decrease over the scored rows).  Nothing n x n is factored: every
        scored row conditions on its own block of the covariance.  One library call where `logpdf` would take one and no window exceeds
        `_lib.AHEAD_WINDOW_MAX` rows; otherwise composed of the Gram matrix and batched block algebra (`_ahead_window_algebra`) - any
        length.  lo = 0 everywhere gives the values above (by other arithmetic).  None: today's evaluation, untouched.  (`origin` may be
        a `heldout.Origins` or `Window` made earlier: its uploaded arrays are shared.)"""
        check_score(score)
        if self.base.is_posterior:
            raise NotImplementedError("rolling-origin forecasts are those of a prior process")
        if isinstance(origin, (Origins, Window)):
            return self._held_out(origin, "rolling-origin forecast" if origin.factored else "sliding-window forecast", score)
        if lo is not None:
            if np.ndim(origin.cpu() if isinstance(origin, torch.Tensor) else origin) != 1 or weights is not None:
                raise ValueError("a window belongs to one horizon: lo and origin hold one integer per row each, without weights")
            return self._held_out(Window(*window_arrays(lo, origin, self.fdd.n)), "sliding-window forecast", score)
        shaped = origin.cpu() if isinstance(origin, torch.Tensor) else origin
        if np.ndim(shaped) == 2:
            origins = origins_array(shaped, self.fdd.n)
            return self._held_out(Origins(origins, horizon_weight_array(weights, origins.shape[0])), "rolling-origin forecast", score)
        if weights is not None:
            raise ValueError("weights belong to a K x n origin array: one horizon has nothing to weigh against")
        return self._held_out(Origins(origin_array(origin, self.fdd.n)), "rolling-origin forecast", score)

    def ahead_gradients(self):
        """(1/2 diag(W) as a device vector, kernel-parameter gradients) of the rolling-origin value, with W = L^-T (P + P^T) L^-1,
        P = Phi(L^T B - abar a^T) (`_ahead_algebra`)."""
        return self._held_out_gradients()

    def _held_out(self, scheme, what, score="log"):
        """`loo`, `cv` and `ahead`: through `_HeldOutValue` where a kernel parameter or the noise needs a gradient.  They share one set
        of pending-gradient state on the observations (`_fused_held_out_gradients`, `_held_out_parts`): a second evaluation with gradients
        on the same `Obs` replaces what the first left, so run each value's backward pass before evaluating the next."""
        if torch.is_grad_enabled():
            params = kernel_parameters(self.base.kernel)
            noise = self.fdd.noise_arg if _needs_grad(self.fdd.noise_arg) else None
            if params or noise is not None:
                if self.base.is_posterior or self.fdd.x.requires_grad:
                    raise NotImplementedError(f"the {what} gradient covers kernel parameters and noise of a prior process")
                self._params = params
                self._noise_device = None if noise is None else noise.device
                value = _HeldOutValue.apply(self, scheme, score, noise, *[p[3] for p in params])
                return value, self._held_out_mean, self._held_out_var
        value = self._held_out_eval(scheme, score=score)
        return value, self._held_out_mean, self._held_out_var

    def _held_out_eval(self, scheme, want_grad=False, score="log"):
        """The value under `scheme` (detached; the means and variances are left in `_held_out_mean` / `_held_out_var`, K x n for K horizons,
        whose K unweighted values are left in `_held_out_values`).  One library call - the engine's method named after the scheme's family,
        looked up now - where the engine has it, `_value_only` / `_fusable_grad` would let `logpdf` take one and `scheme.fits()`; otherwise
        composed of engine primitives and the scheme's block algebra, without those limits.  `score`: the scoring rule of `loo` and `ahead`
        (blocked cross-validation scores a fold's joint density: "log" alone)."""
        eng, n = self.eng, self.fdd.n
        dev = self.y.device
        self._fused_held_out_gradients = self._held_out_parts = self._held_out_values = None   # (what an earlier evaluation left pending)
        K = scheme.horizons
        if n == 0:
            self._held_out_mean = self._held_out_var = torch.zeros((K, 0) if K else (0,), dtype=torch.float64, device=dev)
            if K:
                self._held_out_values = torch.zeros(K, dtype=torch.float64, device=dev)
            return torch.zeros((), dtype=torch.float64, device=dev)
        name = scheme.family + ("_dense_grad" if want_grad else "_dense")
        if scheme.fits() and hasattr(eng, name) and (self._fusable_grad() if want_grad else self._value_only()):
            ck = eng.compile(self.base.kernel, self.fdd.x.shape[1])
            rule = {} if score == "log" else {"score": score}   # (an engine's one-call forms take the rule by keyword)
            value, info, *rest = getattr(eng, name)(ck, self.fdd.x.detach() if want_grad else self.fdd.x, self.y, self.fdd.noise, eng.epsilon,
                                                    *scheme.args, **rule)
            eng.check_info(info)
            if want_grad:
                self._fused_held_out_gradients = rest.pop(0)
                if scheme.factored:   # (the call leaves the factor behind, as logpdf_dense_grad does)
                    self._fac = _Factor.from_batch(eng, n, *rest.pop(0))
            self._held_out_mean, self._held_out_var, *values = rest
            if K:
                self._held_out_values, = values
            return value.detach()
        compose = self._composed_inverse if scheme.inverse else self._composed_ahead if scheme.factored else self._composed_window
        value, self._held_out_mean, self._held_out_var, pending = compose(scheme, score)
        self._held_out_parts = pending if want_grad else None   # (a function returning the weights W on their lower triangle)
        return value.detach() if getattr(eng, "_deferred", None) is not None else value.detach().cpu()

    def _composed_inverse(self, scheme, score):
        """Leave-one-out and folds, purged or not, of any size: K^-1 and alpha, then the scheme's block algebra (`_loo_algebra`,
        `_cv_algebra`, `_cv_gap_algebra`).  (value, means, variances, a function returning W)."""
        eng, fac = self.eng, self.factor()
        low = torch.tril(eng.chol_inverse(fac.L))   # (only the lower triangle is defined)
        Kinv = low + torch.tril(low, -1).T
        alpha = fac.alpha().reshape(-1).detach()
        if scheme.family == "loo":
            value, e, b, var, fill = _loo_algebra(Kinv, alpha, score)
        elif scheme.family == "cv":
            value, e, b, var, fill = _cv_algebra(eng, Kinv, alpha, scheme.starts)
        else:
            value, e, b, var, fill = _cv_gap_algebra(eng, Kinv, alpha, scheme)
        if score == "log":
            value = value - 0.5 * self.fdd.n * _LOG_2PI
        return value, self.y.reshape(-1).detach() - e, var, lambda: _rank_two_weights(eng, Kinv, alpha, b, fill)

    def _composed_ahead(self, scheme, score):
        """Rolling origins at one horizon or K of them (any K): `_ahead_algebra`'s terms and weights per horizon from the one factor, summed
        with the horizons' weights.  (value, means, variances, a function returning W); the K unweighted values go to `_held_out_values`."""
        eng, n, fac = self.eng, self.fdd.n, self.factor()
        L, a, y = fac.L.detach(), fac.zrow.reshape(-1).detach(), self.y.reshape(-1).detach()
        w = scheme.weights   # (None: one horizon, nothing to weigh)
        total, means, variances, values, parts = None, [], [], [], []
        for k, origin in enumerate(scheme.origin if scheme.horizons else scheme.origin[None]):
            value, e, var, scored, weights = _ahead_algebra(eng, L, a, origin, score)
            means.append(torch.where(scored, y - e, var))
            variances.append(var)
            values.append(value.detach())
            parts.append(weights)
            term = value if w is None else float(w[k]) * value
            total = term if total is None else total + term

        def pending():   # K^-1, then the horizons' W - not of the rank-two form; linear in the horizons' (q, s): their weighted sum
            low = torch.tril(eng.chol_inverse(fac.L))
            Kinv = eng.new_matrix(n, n)
            Kinv.copy_(low + torch.tril(low, -1).T)
            W = parts[0](Kinv)
            if w is not None:
                W.mul_(float(w[0]))
                for k in range(1, len(parts)):
                    W.add_(parts[k](Kinv), alpha=float(w[k]))
            return W

        if not scheme.horizons:
            return total, means[0], variances[0], pending
        self._held_out_values = torch.stack(values)
        return total, torch.stack(means), torch.stack(variances), pending

    def _composed_window(self, scheme, score):
        """A sliding window of any length: `_ahead_window_algebra` on the covariance itself - no factor is formed or kept, no K^-1 anywhere.
        (value, means, variances, a function returning W from the rows' blocks)."""
        eng, n = self.eng, self.fdd.n
        block = eng.new_matrix(n, n)
        with torch.no_grad():
            self.fdd._fill_cov(block, eng.epsilon)   # (a prior process: the mean is zero)
            low = torch.tril(block)
            y = self.y.reshape(-1).detach()
            value, e, var, scored, weights = _ahead_window_algebra(eng, low + torch.tril(low, -1).T, y, scheme.lo, scheme.origin, score)
        return value, torch.where(scored, y - e, var), var, weights

    def _held_out_gradients(self):
        """(1/2 diag(W) as a device vector, kernel-parameter gradients) of the value `_held_out_eval(want_grad=True)` has just formed: from
        the fused call's sums, or from the weights W the composed route left pending."""
        fused = getattr(self, "_fused_held_out_gradients", None)
        if fused is not None:
            self._fused_held_out_gradients = None
            return fused()
        pending, self._held_out_parts = self._held_out_parts, None
        W = pending()
        ck, _ = self.fdd.features()
        grads = self.eng.kernel_grads(ck, self.fdd.x.detach(), W)
        return 0.5 * torch.diagonal(W).clone(), grads

    def loo_gradients(self):
        """(1/2 diag(W) as a device vector, kernel-parameter gradients) of the leave-one-out value, with
        W = alpha u^T + u alpha^T - 2 K^-1 C K^-1,  b = alpha / d,  C = diag(1/2 (1 / d + b^2)),  u = K^-1 b."""
        return self._held_out_gradients()

    def cv_gradients(self):
        """(1/2 diag(W) as a device vector, kernel-parameter gradients) of the blocked cross-validation value, with
        W = alpha u^T + u alpha^T - 2 K^-1 C K^-1,  C = blockdiag(1/2 (D_F^-1 + b_F b_F^T)) = blockdiag(R_F R_F^T),  u = K^-1 b."""
        return self._held_out_gradients()

    def input_gradients(self, want_x, want_z):
        """d logpdf / d X = 1/2 d/dX sum_ab W_ab k(x_a, x_b) (both arguments of k move)."""
        ck, _ = self.fdd.features()
        gX = 0.5 * self.eng.kernel_input_grads(ck, self.fdd.x.detach(), None, self._W, sym=True) if want_x else None
        return gX, None

    def mean_gradients(self, xs, g, want_xs=True, want_x=True, want_z=False):
        """Gradients of  g^T mean(xs),  mean(xs) = K(xs, X) alpha, alpha = S^-1 y, S = K(X, X) + D:
             d = sum_ab (g_a alpha_b) dK(xs_a, X_b) - sum_bc (beta_b alpha_c) dS_bc,      beta = S^-1 K(X, xs) g."""
        eng, fac = self.eng, self.factor()
        ck, z = self.fdd.features()
        X = self.fdd.x.detach()
        n = self.fdd.n
        alpha = fac.alpha().reshape(-1)  # n
        pxs = self.base._pts(xs)
        Ks = eng.gram(ck, pxs.z, z)  # n* x n
        beta = eng.gemv_t(Ks, g).reshape(1, n).clone()
        eng.trsm_rlt_(fac.L, beta)
        eng.trsm_rln_(fac.L, beta)
        beta = beta.reshape(-1)
        W_rect = eng.new_matrix(xs.shape[0], n)
        W_rect.copy_(g[:, None] * alpha[None, :])
        W_sym = eng.new_matrix(n, n)
        W_sym.copy_(-0.5 * (beta[:, None] * alpha[None, :] + alpha[:, None] * beta[None, :]))
        params = _add_grads(eng.kernel_grads_weighted(ck, xs, X, W_rect), eng.kernel_grads_weighted(ck, X, None, W_sym, sym=True))
        out = {"params": params, "noise": -beta * alpha}
        if want_xs:
            out["xs"] = eng.kernel_input_grads(ck, xs, X, W_rect)
        if want_x:
            Wt = eng.new_matrix(n, xs.shape[0])
            Wt.copy_(W_rect.T)
            out["x"] = eng.kernel_input_grads(ck, X, xs, Wt) + eng.kernel_input_grads(ck, X, None, W_sym, sym=True)
        return out

    def adopt_factor(self):
        """Install an empty factor whose buffer the caller fills (a factor computed by another rank)."""
        self._fac = _Factor.placeholder(self.eng, self.fdd.n)
        return self._fac

    def _streamable(self, what):
        if self.base.is_posterior or self.fdd.n == 0:
            raise ValueError(f"{what} needs dense observations of a prior process")
        if getattr(self.eng, "cholesky_retry_factor", 1.0) > 1.0:
            raise ValueError(f"{what} keeps the jitter of the factor it extends: not available with a Cholesky retry ladder")

    def extended(self, x_new, y_new, noise_new=None):
        """Observations of the same prior process with k more rows appended - a new `Obs` over [x; x_new], [y; y_new] whose factor
        is this one's, extended: only the k x (n + k) new rows of the Gram matrix are built (one rectangular `gram`), solved against
        L and factored (`chol_append_`: gpar_chol_append, O(k n^2)); nothing the factor already encodes is computed again.
        [(f | obs) built again on more data, reference gpar/model.py:286-301]"""
        self._streamable("extended")
        eng, fac, n0 = self.eng, self.factor(), self.fdd.n
        x_new, y_new = _as_matrix(eng, x_new), _as_matrix(eng, y_new)
        k = int(x_new.shape[0])
        if y_new.shape[0] != k or x_new.shape[1] != self.fdd.x.shape[1]:
            raise ValueError("x_new and y_new must hold the same number of rows, x_new as wide as the observed inputs")
        if k == 0:
            return self
        nv_new = _noise_vector(eng, noise_new, k)
        old = self.fdd.noise
        if old is None and nv_new is None:
            noise = None
        else:
            dev = self.fdd.x.device
            noise = torch.cat([old if old is not None else torch.zeros(n0, dtype=torch.float64, device=dev),
                               nv_new if nv_new is not None else torch.zeros(k, dtype=torch.float64, device=dev)])
        fdd = FDD(self.base, torch.cat([self.fdd.x, x_new], dim=0), noise)
        out = Obs(fdd, torch.cat([self.y, y_new], dim=0))
        ck, z = fdd.features()
        n = n0 + k
        A = eng.new_matrix(n + 1, n + 1)
        A[:n0, :n0] = fac.L
        eng.gram(ck, z[n0:], z, out=A[n0:n, :n])
        shift = torch.full((k,), eng.epsilon, dtype=torch.float64, device=A.device)
        torch.diagonal(A[n0:n, n0:n]).add_(shift if nv_new is None else shift + nv_new)
        A[n, :n0] = fac.zrow.reshape(-1)
        A[n, n0:n] = y_new.reshape(-1)
        logdet, info = chol_append_(eng, A, n0, k, fac.logdet.clone())
        eng.check_info(info)
        out._fac = _Factor.from_batch(eng, n, A, logdet)
        return out

    def without_leading(self, k):
        """Observations of the same prior process without their k leading rows - a new `Obs` over x[k:], y[k:] whose factor is this
        one's, updated: L22' L22'^T = L22 L22^T + L21 L21^T, a rank-k Cholesky UPDATE (`chol_drop_leading`: gpar_chol_drop_leading,
        O(k n^2), unconditionally stable), with L^-1 y carried along as one more row.
        [(f | obs) built again on less data, reference gpar/model.py:286-301]"""
        self._streamable("without_leading")
        k = int(k)
        n = self.fdd.n
        if not 0 <= k < n:
            raise ValueError(f"k={k}: between 0 and n - 1 = {n - 1} leading observations can be forgotten")
        if k == 0:
            return self
        eng, fac = self.eng, self.factor()
        noise = None if self.fdd.noise is None else self.fdd.noise[k:]
        out = Obs(FDD(self.base, self.fdd.x[k:], noise), self.y[k:])
        A, logdet, info = chol_drop_leading(eng, fac.A, k)
        eng.check_info(info)
        out._fac = _Factor.from_batch(eng, n - k, A, logdet)
        return out

    def _batchable(self):
        """This observation's factor may come out of a lock-step batch: a prior process (zero mean: the right-hand side is y
        itself), nothing factored yet, checks deferred, no retry ladder to climb."""
        eng = self.eng
        return (self._fac is None and not self.base.is_posterior and self.fdd.n > 0 and hasattr(eng, "factor_dense_batch")
                and getattr(eng, "_deferred", None) is not None and getattr(eng, "cholesky_retry_factor", 1.0) <= 1.0
                and isinstance(self.y, torch.Tensor) and self.y.is_cuda)

    def factor(self):
        """Cholesky of cov(f(X)) + D + eps I under the observed process and L^-1 (y - mean(X))."""
        if self._fac is None:
            self._fac = self.fdd._factor(self.y)
        return self._fac

    def merged_with(self, other):
        """Observations of the prior equivalent to conditioning on `self` and then on `other` (both dense)."""
        prior = self.prior_gp()
        a, b = self.fdd, other.fdd
        na = a.noise if a.noise is not None else torch.zeros(a.n, dtype=torch.float64, device=a.x.device)
        nb = b.noise if b.noise is not None else torch.zeros(b.n, dtype=torch.float64, device=b.x.device)
        x = torch.cat([a.x, b.x], dim=0)
        return Obs(FDD(prior, x, torch.cat([na, nb])), torch.cat([self.y, other.y], dim=0))

    # ---- the posterior's corrections (any base process) -----------------------------------------------
    def _V(self, p):
        """V = k_base(p, X) L^-T  (n_p x n)."""
        V = self.base._cross(p, self.fdd.pts())
        self.eng.trsm_rlt_(self.factor().L, V)
        return V

    def mean_at(self, p):
        base_mean = self.base._mean_at(p)
        if self.fdd.n == 0:
            return base_mean
        Ks = self.base._cross(p, self.fdd.pts())
        corr = self.eng.gemm(Ks, self.factor().alpha(), tb=True)
        return corr if not self.base.is_posterior else base_mean + corr

    def cross(self, pa, pb):
        K = self.base._cross(pa, pb)
        if self.fdd.n:
            self.eng.gemm(self._V(pa), self._V(pb), tb=True, alpha=-1.0, beta=1.0, out=K)
        return K

    def diag(self, p):
        d = self.base._diag(p)
        return d - self.eng.rownorm2(self._V(p)) if self.fdd.n else d

    def moments_into(self, p, block, diag_add, jitter):
        eng = self.eng
        mean = self.base._moments_into(p, block, diag_add, jitter)
        if self.fdd.n == 0:
            return mean
        V = self._V(p)
        eng.gemm(V, V, tb=True, alpha=-1.0, beta=1.0, out=block, c_lower=True)
        corr = eng.gemm(V, self.factor().zrow, tb=True)
        return corr if not self.base.is_posterior else mean + corr

    # ---- decomposition by kernel component (dense observations of the prior) -----------------------------
    def components(self, p, comp, ncomp, variance=True):
        """(mean, var), each ncomp x n*: the posterior moments at the points `p` of the components k_g = sum_{comp[t] = g} c_t k_t of the
        kernel k = sum_t c_t k_t - `comp` holds, per term of the kernel, its component 0 .. ncomp - 1 or -1 for none:
            mean_g = k_g(x*, X) alpha,        var_g = k_g(x*, x*) - |L^-1 k_g(X, x*)|^2        (latent: the noise belongs to no component)
        with alpha = K^-1 y and L the factor conditioning holds (Rasmussen & Williams 5.4.3).  `var` is None without `variance`.  One
        library call where the engine has it (`posterior_terms`; GPAR_FUSED_TERMS=0 turns it off), otherwise composed of what every
        engine has: the sub-kernel of each component, its Gram matrix and diagonal, the triangular solve."""
        if self.base.is_posterior:
            raise ValueError("a decomposition by kernel component needs dense observations of a prior process")
        comp = [int(c) for c in comp]
        ncomp = int(ncomp)
        if len(comp) != len(self.base.kernel.terms):
            raise ValueError(f"the grouping holds {len(comp)} entries for {len(self.base.kernel.terms)} kernel terms")
        if not 1 <= ncomp <= GPAR_MAX_TERMS or any(not -1 <= c < ncomp for c in comp):
            raise ValueError(f"components are numbered 0 .. ncomp - 1 (-1: none) with 1 <= ncomp <= {GPAR_MAX_TERMS}")
        eng, fac = self.eng, self.factor()
        if self.fdd.n > 0 and p.n > 0 and fused_terms() and hasattr(eng, "posterior_terms"):
            _, z = self.fdd.features()
            return eng.posterior_terms(p.ck, comp, ncomp, p.z, z, fac.alpha(), fac.L, variance=variance)
        return self._components_composed(p, comp, ncomp, variance)

    # ---- posterior derivatives (dense observations of the prior) -----------------------------------------
    def derivatives(self, p, U, variance=True):
        """(dmean, dvar), each ndir x n*: mean and latent variance of the directional derivatives of the posterior at the points `p` along
        the design-space directions `U` (n* x width: one direction per row; or ndir x n* x width) - the derivative of a Gaussian process
        is a Gaussian process (Rasmussen & Williams 9.4):
            dmean = u . grad_x k(x*, X) alpha,        dvar = u^T [grad_x grad_x'^T k](x*, x*) u - |L^-1 (u . grad_x k(x*, X))^T|^2
        with alpha = K^-1 y and L the factor conditioning holds.  One library call (`posterior_deriv`: no n* x n matrix for the means, one
        triangular solve for all variances); an engine without it raises NotImplementedError.  `dvar` is None without `variance`.
        ValueError: observations of a posterior process, a Matern 1/2 factor (its process is not differentiable)."""
        if self.base.is_posterior:
            raise ValueError("posterior derivatives need dense observations of a prior process")
        if any(f.type == "matern12" for t in self.base.kernel.terms for f in t.factors):
            raise ValueError("a Matern 1/2 process is not differentiable: no posterior derivatives")
        eng = self.eng
        if not hasattr(eng, "posterior_deriv"):
            raise NotImplementedError(f"{type(eng).__name__} has no posterior_deriv: posterior derivatives are a device kernel "
                                      "(gpar_posterior_deriv); run them on the HIP engine")
        U = eng.tensor(U)
        if U.dim() == 2:
            U = U[None]
        if U.dim() != 3 or tuple(U.shape[1:]) != tuple(p.x.shape) or not 1 <= U.shape[0] <= GPAR_MAX_TERMS:
            raise ValueError(f"directions must be n* x width or ndir x n* x width with 1 <= ndir <= {GPAR_MAX_TERMS}, one row per point")
        if p.n == 0:
            empty = torch.zeros(U.shape[0], 0, dtype=torch.float64, device=p.x.device)
            return empty, (empty.clone() if variance else None)
        fac = self.factor()
        _, z = self.fdd.features()
        J = eng.feature_directions(p.ck, p.x, U)
        return eng.posterior_deriv(p.ck, p.z, J, z, fac.alpha(), fac.L, variance=variance)

    # ---- sensitivity of the posterior mean to the hyperparameters (dense observations of the prior) ---------
    def mean_sensitivity(self, p, M, noise_col, noise_value):
        """The n* x P Jacobian of the latent posterior mean at the points `p` with respect to the layer's P trainable variables in the
        optimiser's unconstrained coordinates (those `fastfit.DenseLayerObjective.fg` differentiates in):
            J[a, theta] = sum_b alpha_b d k(z*_a, z_b) / d theta - k*_a^T K^-1 (dK / d theta) alpha,        alpha = K^-1 y.
        `M` (P x GRAD_NACC) and `noise_col` (P) are that objective's chain rule as a matrix (`chain_matrix`): raw moment sums ->
        variables, and the noise variance -> variables; `noise_value` the noise variance itself (dK / d noise = diag(noise_i) / noise,
        the inverse weights).  Computed as R* = gram_grad_rows(z*, Z, alpha) and R = gram_grad_rows(Z, Z, alpha) = (dK / d raw) alpha
        column by column - one fused pass each, rows unreduced -, T = K^-1 R for the slot columns M uses by the two triangular solves
        with the factor conditioning holds, the second term by `gram_apply_groups`, then the chain rule.  No n* x n matrix is written.
        The noise does not appear in k: only the second term contributes.  An engine without `gram_grad_rows` raises
        NotImplementedError.  ValueError: observations of a posterior process."""
        if self.base.is_posterior:
            raise ValueError("the sensitivity of the posterior mean needs dense observations of a prior process")
        eng = self.eng
        if not hasattr(eng, "gram_grad_rows"):
            raise NotImplementedError(f"{type(eng).__name__} has no gram_grad_rows: per-row gradient sums are a device kernel "
                                      "(gpar_gram_grad_rows); run them on the HIP engine")
        M = np.asarray(M, dtype=np.float64)
        noise_col = np.asarray(noise_col, dtype=np.float64).reshape(-1)
        P, n = M.shape[0], self.fdd.n
        dev = p.x.device
        if p.n == 0 or n == 0 or P == 0:
            return torch.zeros(p.n, P, dtype=torch.float64, device=dev)
        fac, pts = self.factor(), self.fdd.pts()
        ck, z = pts.ck, pts.z
        alpha = fac.alpha().reshape(-1).contiguous()
        zd = zds = None
        if eng._periodic(ck):
            zd, zds = eng.featurize_dfreq(ck, pts.x), eng.featurize_dfreq(p.ck, p.x)
        used = [int(s) for s in np.flatnonzero(np.any(M != 0.0, axis=0))]
        with_noise = bool(np.any(noise_col != 0.0))
        at = torch.tensor(used, dtype=torch.long).to(dev)
        Rs = eng.gram_grad_rows(p.ck, p.z, z, alpha, zd1=zds, zd2=zd).index_select(1, at)   # n* x U
        R = eng.gram_grad_rows(ck, z, z, alpha, zd1=zd, zd2=zd).index_select(1, at)         # n x U: (dK / d raw) alpha
        rows = [R.T]
        if with_noise:
            rows.append((alpha * (self.fdd.noise / float(noise_value)))[None])
        Tt = torch.cat(rows, dim=0).contiguous()   # (U [+ 1]) x n: rows b^T -> b^T K^-1 = b^T L^-T L^-1
        if Tt.shape[0] == 0:
            return torch.zeros(p.n, P, dtype=torch.float64, device=dev)
        eng.trsm_rlt_(fac.L, Tt)
        eng.trsm_rln_(fac.L, Tt)
        second = eng.gram_apply_groups(p.ck, p.z, z, Tt)   # n* x (U [+ 1]): k*^T K^-1 (dK / d .) alpha
        Mt = torch.from_numpy(np.ascontiguousarray(M[:, used].T)).to(dev)   # U x P
        J = (Rs - second[:, :len(used)]) @ Mt if used else torch.zeros(p.n, P, dtype=torch.float64, device=dev)
        if with_noise:
            J = J - second[:, len(used):] * torch.from_numpy(noise_col).to(dev)[None]
        return J

    def _components_composed(self, p, comp, ncomp, variance):
        eng, fac, n = self.eng, self.factor(), self.fdd.n
        kernel, width = self.base.kernel, self.fdd.x.shape[1]
        mean = torch.zeros(ncomp, p.n, dtype=torch.float64, device=p.x.device)
        var = torch.zeros(ncomp, p.n, dtype=torch.float64, device=p.x.device) if variance else None
        for g in range(ncomp):
            terms = [t for t, c in zip(kernel.terms, comp) if c == g]
            if not terms or p.n == 0:
                continue   # (a component without a term is zero)
            ck = eng.compile(Kernel(terms), width)
            zs = eng.features(ck, p.x)
            if variance:
                var[g] = eng.gram_diag(ck, zs)
            if n == 0:
                continue
            Ks = eng.gram(ck, zs, eng.features(ck, self.fdd.x))
            mean[g] = eng.gemm(Ks, fac.alpha(), tb=True).reshape(-1)
            if variance:
                eng.trsm_rlt_(fac.L, Ks)
                var[g] -= eng.rownorm2(Ks)
        return mean, var

    # ---- batched routines for dense observations of the prior (`fast_dense`) ----------------------------
    def posterior_mean_batch(self, xs):
        """Posterior means at several input sets with one stacked cross-Gram product."""
        eng, fac = self.eng, self.factor()
        ck, z = self.fdd.features()
        sizes = [int(x_s.shape[0]) for x_s in xs]
        if self.fdd.n == 0:
            return [torch.zeros(k, 1, dtype=torch.float64, device=z.device) for k in sizes]
        B = eng.new_matrix(sum(sizes), self.fdd.n)
        stacked = xs.matrix if isinstance(xs, Stacked) else torch.cat([_as_matrix(eng, x_s) for x_s in xs], dim=0)
        eng.gram(ck, eng.features(ck, _as_matrix(eng, stacked)), z, out=B)   # one launch each
        means = eng.gemm(B, fac.alpha(), tb=True)
        return list(torch.split(means, sizes, dim=0))

    def _stacked_features(self, xs):
        """Features of several input sets of one size in ONE launch: (the stacked matrix, its per-set row views)."""
        eng = self.eng
        ck, _ = self.fdd.features()
        ns = int(xs[0].shape[0])
        stacked = xs.matrix if isinstance(xs, Stacked) else torch.cat([_as_matrix(eng, x_s) for x_s in xs], dim=0)
        z_all = eng.features(ck, _as_matrix(eng, stacked))
        return z_all, [z_all[k * ns : (k + 1) * ns] for k in range(len(xs))]

    def _stacked_V(self, z_all):
        """Rows [k ns, (k + 1) ns): V_k = K(x_k, X) L^-T for every feature set stacked in z_all - ONE cross-Gram launch, ONE
        triangular solve."""
        eng, fac = self.eng, self.factor()
        ck, z = self.fdd.features()
        B = eng.new_matrix(z_all.shape[0], self.fdd.n)
        eng.gram(ck, z_all, z, out=B)
        eng.trsm_rlt_(fac.L, B)
        return B

    def _chunk(self, ns):
        """Samples per chunk: the stacked right-hand side (S n* x n doubles) and the stacked per-sample covariances
        (S n* x n*) are each bounded to ~16 GB of the 288 GB HBM; at most 16384 samples at a time (the batched launches
        carry the sample index in a grid dimension, limit 65535)."""
        return max(1, min(16384, int(16e9 // max(1, ns * max(self.fdd.n, ns, 1) * 8))))

    def posterior_marginals_batch(self, xs):
        """(means, variances), each n* x S: column s holds the posterior mean / marginal variance (no noise) at xs[s]."""
        eng, fac = self.eng, self.factor()
        ck, z = self.fdd.features()
        n, S = self.fdd.n, len(xs)
        ns = int(xs[0].shape[0])
        mean = torch.zeros(ns, S, dtype=torch.float64, device=z.device)
        var = torch.empty(ns, S, dtype=torch.float64, device=z.device)
        chunk = self._chunk(ns)
        for s0 in range(0, S, chunk):
            s1 = min(S, s0 + chunk)
            z_all, zss = self._stacked_features(xs[s0:s1])
            kd = eng.gram_diag(ck, z_all).reshape(s1 - s0, ns).T
            if n > 0:
                B = self._stacked_V(z_all)
                mean[:, s0:s1] = eng.gemm(B, fac.zrow, tb=True).reshape(s1 - s0, ns).T
                kd = kd - eng.rownorm2(B).reshape(s1 - s0, ns).T
            var[:, s0:s1] = kd
        return mean, var

    def _sample_batch_linear_tail(self, xs, noise_vec, zr, out):
        """posterior_sample_batch when the columns that differ between the sets only enter the kernel through linear factors
        standing alone in their terms (kernels.linear_tail) - GPAR's DEFAULT output dependence (reference
        gpar/regression.py:141-146, 276-278: `linear=True, nonlinear=False`).  Then, with c_s the weighted features of those columns
        at set s and Z_c the same at the training inputs,
            K(x_s, X)   = K0(x, X) + c_s Z_c^T                       (K0: those features zeroed - the same for every s)
            V_s         = K(x_s, X) L^-T = V0 + c_s U^T,              U = L^-1 Z_c      (n x q, q = number of such features)
            mean_s      = V0 r + c_s (U^T r),                          r = L^-1 y
            cov_s       = [K0(x, x) + D - V0 V0^T] + c_s E_s^T + E_s c_s^T,    E_s = c_s (I - U^T U) / 2 - V0 U
        so the S stacked n* x n solves and the S rank-n downdates of the general routine become ONE of each plus a rank-2q update
        per set; what stays per set is the n* x n* factorisation (lock-step) and the draw.  Same law, same random numbers, same
        samples up to rounding.  Returns False (nothing done) when the structure or the sizes do not qualify."""
        from .kernels import linear_tail

        eng, fac = self.eng, self.factor()
        if os.environ.get("GPAR_LINEAR_TAIL", "1") == "0" or not isinstance(xs, Stacked) or xs.shared_cols <= 0:
            return False
        ck, z = self.fdd.features()
        n, S, ns = self.fdd.n, len(xs), xs.rows
        if n == 0 or S < 2 or not hasattr(eng, "potrf_batch_") or ns > eng.batch_rows() or getattr(eng._tls, "safe", False):
            return False
        tail = linear_tail(ck, xs.shared_cols)
        if tail is None:
            return False
        idx, weight = tail
        q = len(idx)
        dev = z.device
        sel = torch.as_tensor(idx, dtype=torch.long, device=dev)
        wts = torch.as_tensor(weight, dtype=torch.float64, device=dev)
        # shared part: the first set with the varying features zeroed
        z0 = eng.features(ck, _as_matrix(eng, xs[0])).clone()
        z0.index_fill_(1, sel, 0.0)
        V0 = eng.new_matrix(ns, n)
        eng.gram(ck, z0, z, out=V0)
        eng.trsm_rlt_(fac.L, V0)
        Ut = eng.new_matrix(q, n)                      # U^T = Z_c^T L^-T
        Ut.copy_((z.index_select(1, sel) * wts).T)
        eng.trsm_rlt_(fac.L, Ut)
        base = eng.new_matrix(ns, ns)
        eng.gram(ck, z0, lower=True, diag_add=noise_vec, diag_const=eng.epsilon, out=base)
        eng.gemm(V0, V0, tb=True, alpha=-1.0, beta=1.0, out=base, c_lower=True)
        H = eng.gemm(V0, Ut, tb=True)                  # V0 U: n* x q
        T = eng.gemm(Ut, Ut, tb=True)                  # U^T U: q x q
        mean0 = eng.gemm(V0, fac.zrow, tb=True)        # n* x 1
        beta = eng.gemm(Ut, fac.zrow, tb=True)         # q x 1
        half = 0.5 * (torch.eye(q, dtype=torch.float64, device=dev) - T)
        half = 0.5 * (half + half.T)                   # (symmetric to the last bit: c E^T + E c^T then is, too)
        chunk = max(1, min(16384, int(16e9 // max(1, ns * ns * 8))))
        for s0 in range(0, S, chunk):
            s1 = min(S, s0 + chunk)
            K = s1 - s0
            z_all = eng.features(ck, _as_matrix(eng, xs[s0:s1].matrix))
            C = eng.new_matrix(K * ns, q)
            C.copy_(z_all.index_select(1, sel) * wts)  # (K n*) x q
            E = eng.gemm(C, half) - H.repeat(K, 1)
            means = mean0.repeat(K, 1) + eng.gemm(C, beta)
            left = eng.new_matrix(K * ns, 2 * q)
            right = eng.new_matrix(K * ns, 2 * q)
            left[:, :q], left[:, q:] = C, E
            right[:, :q], right[:, q:] = E, C
            covs = eng.new_matrix(K * ns, ns)
            covs.unflatten(0, (K, ns)).copy_(base.unsqueeze(0))   # (a view: the rows of `covs` are padded)
            eng.gemm_batch_(left, right, covs, K, tb=True, alpha=1.0, beta=1.0, c_lower=True)
            _, info = eng.potrf_batch_(covs, K)
            eng.check_info(info)
            eng.trmv_lower_batch_(covs, K, zr[:, s0:s1], out[:, s0:s1], add=means)
        return True

    def posterior_sample_batch(self, xs, noise):
        eng, fac = self.eng, self.factor()
        ck, z = self.fdd.features()
        n, S = self.fdd.n, len(xs)
        ns = int(xs[0].shape[0])
        out = torch.empty(ns, S, dtype=torch.float64, device=z.device)
        if ns == 0:
            return out
        noise_vec = _noise_vector(eng, noise, ns)
        zr = eng.randn(ns, S)
        if self._sample_batch_linear_tail(xs, noise_vec, zr, out):
            return out
        chunk = self._chunk(ns)
        for s0 in range(0, S, chunk):
            s1 = min(S, s0 + chunk)
            z_all, zss = self._stacked_features(xs[s0:s1])
            B = means = None
            if n > 0:
                B = self._stacked_V(z_all)  # every V_s = K(x_s, X) L^-T in one solve
                means = eng.gemm(B, fac.zrow, tb=True)
            # the per-sample blocks (Gram, SYRK downdate, an n* x n* factorisation, one matvec) are independent and of one
            # shape.  Up to HipEngine.batch_rows() points they go through ONE batched downdate and ONE lock-step
            # factorisation (gpar_gemm_batch, gpar_potrf_batch: a small factorisation is a latency-bound chain, `count` of
            # them in step cost little more than one) ...
            K = s1 - s0
            if K > 1 and hasattr(eng, "potrf_batch_") and ns <= eng.batch_rows() and not getattr(eng._tls, "safe", False):
                covs = eng.new_matrix(K * ns, ns)
                eng.gram_batch_(ck, z_all, K, covs, lower=True, diag_add=noise_vec, diag_const=eng.epsilon)
                if n > 0:
                    eng.gemm_batch_(B, B, covs, K, tb=True, alpha=-1.0, beta=1.0, c_lower=True)
                _, info = eng.potrf_batch_(covs, K)
                eng.check_info(info)
                eng.trmv_lower_batch_(covs, K, zr[:, s0:s1], out[:, s0:s1], add=means)   # mean_s + chol(cov_s) z_s, all s
                continue
            # ... larger ones are dealt over a few streams and checked once at the end
            pipe = eng.pipeline(min(4, s1 - s0)) if s1 - s0 > 1 else None
            with eng.defer_checks(), joining(pipe):  # streams are joined BEFORE the deferred info words are read
                for k, zs in enumerate(zss):
                    with (pipe.stage(k, B, zr, out, zs, noise_vec, means) if pipe is not None else contextlib.nullcontext()):
                        cov = eng.new_matrix(ns, ns)
                        eng.gram(ck, zs, lower=True, diag_add=noise_vec, diag_const=eng.epsilon, out=cov)
                        mean = None
                        if n > 0:
                            V = B[k * ns : (k + 1) * ns]
                            eng.gemm(V, V, tb=True, alpha=-1.0, beta=1.0, out=cov, c_lower=True)
                            mean = means[k * ns : (k + 1) * ns]
                        _, info = eng.potrf_(cov)
                        eng.check_info(info)
                        draw = eng.trmv_lower(cov, zr[:, s0 + k : s0 + k + 1])
                        out[:, s0 + k : s0 + k + 1] = draw if mean is None else draw + mean
        return out

    # ---- pathwise sampling (Matheron's rule; dense observations of the prior) ----------------------------------------
    def _pathwise_prior(self, basis, zf, theta, group_rows, fused):
        """The prior draws Phi(z) theta at the feature rows zf: rows x S (group_rows = 0: every row meets every column) or a vector
        (rows in groups of group_rows, group g uses column g).  Fused: the Fourier part in one library call, the few exact features by
        torch; composed: Phi in chunks of rows by torch."""
        eng, F = self.eng, basis.num_frequencies
        rows, S = int(zf.shape[0]), int(theta.shape[1])

        def apply(phi, tht, r0):
            if not group_rows:
                return phi @ tht
            col = torch.arange(r0, r0 + phi.shape[0], device=phi.device) // group_rows
            return (phi * tht.index_select(1, col).T).sum(dim=1)

        if fused:
            omega, amp, shift, _, _, _ = basis.on(zf)
            out = eng.rff_apply(zf, basis.dz, shift, omega, theta[:F] * amp[:, None], theta[F : 2 * F] * amp[:, None], group_rows=group_rows)
            if basis.num_weights > 2 * F:
                out = out + apply(basis.exact_phi(zf), theta[2 * F :], 0)
            return out
        out = torch.empty((rows,) if group_rows else (rows, S), dtype=torch.float64, device=zf.device)
        step = max(1, int(2 ** 27 // max(1, basis.num_weights)))   # (Phi of a chunk: at most 1 GiB)
        for r0 in range(0, rows, step):
            out[r0 : r0 + step] = apply(basis.phi(zf[r0 : r0 + step]), theta, r0)
        return out

    def pathwise_sample_batch(self, xs, noise, basis, S, draws=None):
        """S posterior draws by pathwise conditioning (Wilson et al., ICML 2020), n* x S:

            f*_s(.) = f_s(.) + k(., X) (K + D + eps I)^-1 (y - f_s(X) - e_s),      f_s = Phi theta_s,  e_s ~ N(0, D)

        with Phi the `pathwise.Basis` of this layer's kernel (shared by the S draws, which are independent given it), D the observation
        noise and (K + D + eps I) the factor conditioning holds (eps: the engine's jitter).  `xs`: a `Stacked` of S design matrices
        (group s is draw s's) or one matrix all draws share.  `noise`: added to the draws as N(0, noise) when not None.  Per draw what
        remains is an n-vector solve, a fused cross-Gram-times-vector over n* n pairs and a fused feature evaluation over n* F pairs: no
        n* x n* matrix exists, and the fused route writes no n* x n matrix either.  `draws`: (theta, e, xi) standard normals to use
        instead of the engine's (num_weights x S, n x S, n* x S) - for tests.  A posterior base process: ValueError."""
        from .pathwise import feature_map

        if self.base.is_posterior:
            raise ValueError("pathwise sampling needs dense observations of a prior process")
        eng, fac, n = self.eng, self.factor(), self.fdd.n
        ck, z = self.fdd.features()
        grouped = isinstance(xs, Stacked)
        if grouped and len(xs) != S:
            raise ValueError(f"{len(xs)} stacked design matrices for {S} draws")
        xmat = _as_matrix(eng, xs.matrix if grouped else xs)
        ns = xs.rows if grouped else int(xmat.shape[0])
        group_rows = ns if grouped else 0
        if ns == 0 or S == 0:
            return torch.empty(ns, S, dtype=torch.float64, device=xmat.device)
        fused = fused_pathwise() and hasattr(eng, "rff_apply") and hasattr(eng, "gram_apply_groups")
        zs = eng.features(ck, xmat)   # what the Gram passes read (the oracle engine: the design matrix itself)
        zf_train, zf_test = (z, zs) if fused else (feature_map(ck.kernel, self.fdd.x), feature_map(ck.kernel, xmat))
        if basis.shift is None:
            basis = basis.with_shift(zf_train)
        theta, e, xi = draws if draws is not None else (None, None, None)
        theta = eng.randn(basis.num_weights, S) if theta is None else eng.tensor(theta)
        out = self._pathwise_prior(basis, zf_test, theta, group_rows, fused)
        if n > 0:
            R = self.y - self._pathwise_prior(basis, zf_train, theta, 0, fused)
            if self.fdd.noise is not None:
                R = R - torch.sqrt(self.fdd.noise)[:, None] * (eng.randn(n, S) if e is None else eng.tensor(e))
            Vt = eng.new_matrix(S, n)   # v_s^T = R_s^T L^-T L^-1, row s
            Vt.copy_(R.T)
            eng.trsm_rlt_(fac.L, Vt)
            eng.trsm_rln_(fac.L, Vt)
            if fused:
                out = out + eng.gram_apply_groups(ck, zs, z, Vt, group_rows=group_rows)
            elif grouped:
                chunk = self._chunk(ns)
                for s0 in range(0, S, chunk):
                    s1 = min(S, s0 + chunk)
                    Ks = eng.gram(ck, zs[s0 * ns : s1 * ns], z)
                    for k in range(s1 - s0):
                        out[(s0 + k) * ns : (s0 + k + 1) * ns] += eng.gemm(Ks[k * ns : (k + 1) * ns], Vt[s0 + k : s0 + k + 1], tb=True).reshape(-1)
            else:
                step = max(1, int(2e9 // (8 * n)))
                for r0 in range(0, ns, step):
                    out[r0 : r0 + step] += eng.gemm(eng.gram(ck, zs[r0 : r0 + step], z), Vt, tb=True)
        if grouped:
            out = out.reshape(S, ns).T
        nv = _noise_vector(eng, noise, ns)
        if nv is not None:
            out = out + torch.sqrt(nv)[:, None] * (eng.randn(ns, S) if xi is None else eng.tensor(xi))
        return out


class _LazyV:
    """v = L_z^-T A^-1 c of an inducing-point observation, computed at first use on the stream of that use.  The producing
    stream and an event behind the solve are kept: a later consumer on ANOTHER stream (a posterior shared between worker streams)
    waits for that event instead of reading v unordered."""

    def __init__(self, eng, facA, Lz):
        self.eng, self.facA, self.Lz, self.value = eng, facA, Lz, None
        self._stream = self._ready = None

    def get(self):
        if self.value is None:
            v = self.facA.alpha().clone()  # (A^-1 c)^T, 1 x M
            self.eng.trsm_rln_(self.Lz, v)
            self.value = v
            if v.is_cuda:
                self._stream = torch.cuda.current_stream(v.device)
                self._ready = torch.cuda.Event()
                self._ready.record(self._stream)
        elif self._ready is not None:
            here = torch.cuda.current_stream(self.value.device)
            if here != self._stream:
                here.wait_event(self._ready)
                self.value.record_stream(here)
        return self.value


class PseudoObs:
    """Inducing-point observations (stheno `PseudoObs(f(x_ind), f(x, noise), y)`) of the process `fdd.p` (prior or
    posterior).  `method` selects the approximation, as stheno's `PseudoObsVFE` (the default, Titsias 2009) /
    `PseudoObsFITC` / `PseudoObsDTC` do:
        VFE   log N(y; m, Q + D) - 1/2 tr D^-1 (K - Q)
        DTC   log N(y; m, Q + D)
        FITC  log N(y; m, Q + D + diag(K - Q))        (the posterior then uses D + diag(K - Q) as well)
    with Q = K_xz K_zz^-1 K_zx."""

    fast_dense = False
    method = "vfe"

    def __init__(self, u, fdd, y):
        if isinstance(u, tuple):
            raise TypeError("pass a single FDD of inducing points")
        self.u = u
        self.fdd = fdd
        self.eng = fdd.eng
        self.base = fdd.p
        self.y = _as_matrix(self.eng, y)
        if u.p is not fdd.p and (u.p.kernel is not fdd.p.kernel or u.p.is_posterior or fdd.p.is_posterior):
            raise ValueError("inducing points and observations must belong to the same process")
        if fdd.noise is None:
            raise ValueError("inducing-point observations need observation noise")
        self._state = None

    def prior_gp(self):
        p = self.base
        while p.is_posterior:
            p = p._obs.base
        return p

    def rebased(self, gp):
        return type(self)(FDD(gp, self.u.x), FDD(gp, self.fdd.x, self.fdd.noise_arg), self.y)

    def _compute(self):
        if self._state is not None:
            return self._state
        eng, base = self.eng, self.base
        n, M = self.fdd.n, self.u.n
        px, pz = self.fdd.pts(), self.u.pts()
        d = self.fdd.noise
        # Which ORDER forms A - I = L_z^-1 K_zx D^-1 K_xz L_z^-T is decided on the device, from the pivot spread of L_z
        # (HipEngine.vfe_spread_limit): the n x M solve against L_z first (backward stable whatever cond(K_zz); M^2 n
        # flops), or the product first and the M x M result solved from both sides (2 M^3 flops; loses ~cond(K_zz) digits).
        # The gradient pass and FITC need the solved cross-Gram itself: they always take the first.
        limit = 0.0
        if self.method != "fitc" and not getattr(self, "_force_solve", False) and hasattr(eng, "vfe_spread_limit"):
            limit = eng.vfe_spread_limit(n, M)
        # L_z = chol(K_zz + eps I): a latency-bound chain of panel kernels on an M x M matrix (0.3 ms at M = 1024) that nothing
        # below needs before the triangular solve - on a side stream it runs beside the n x M cross-Gram build
        side = eng.side_stream() if hasattr(eng, "side_stream") and not base.is_posterior and n * M >= (1 << 22) else None
        Lz = eng.new_matrix(M, M)   # (allocated on the caller's stream: its lifetime follows that stream, whatever happens on the side)
        ill = None
        if side is not None:
            # Lz belongs to the caller's stream's pool but is written on the side stream: tell the allocator, so that an exception
            # between here and the join (out of memory in the n x M cross-Gram below, say) cannot hand the block to a new tensor
            # while the side stream's factorisation is still writing it
            Lz.record_stream(side)
        try:
            with (_on_side(side) if side is not None else contextlib.nullcontext()):
                mean_z = base._moments_into(pz, Lz, None, eng.epsilon)
                del mean_z  # the bound only involves the mean at the observed inputs
                _, info = eng.potrf_(Lz)
                if limit > 0.0:
                    _, ill = eng.chol_spread(Lz, limit)   # device word: 1 = K_zz too ill-conditioned for the product-first order
        except BaseException:
            if side is not None:   # whatever went wrong, the caller's stream is ordered after the side stream again
                torch.cuda.current_stream(side.device).wait_stream(side)
            raise
        pending_join = side is not None

        def joined():   # the factor is needed from here on (and its info word may only be read once it has been written)
            nonlocal pending_join
            if pending_join:
                _join_side(side, info, ill)
                pending_join = False
            eng.check_info(info)

        kdiag = base._diag(px)
        if self.method == "fitc":
            # the effective noise needs q_aa = |B_:a|^2 before anything can be scaled by it: one more pass over n x M
            Bs = base._cross(px, pz)
            joined()
            eng.trsm_rlt_(Lz, Bs)
            excess = kdiag - eng.rownorm2(Bs)  # k_aa - q_aa >= 0 up to rounding
            d = d + torch.clamp(excess, min=0.0)
            rs = torch.rsqrt(d)
            Bs.mul_(rs[:, None])
        else:
            rs = torch.rsqrt(d)
            # Bs = D^-1/2 K_xz L_z^-T (n x M): the row scaling rides along in the Gram kernel
            Bs = base._cross(px, pz, row_scale=rs)
            joined()
            if ill is None:
                eng.trsm_rlt_(Lz, Bs)
            else:
                eng.trsm_rlt_(Lz, Bs, when=(ill, True))   # (product-first order: Bs stays D^-1/2 K_xz)
        resid = self.y if not base.is_posterior else self.y - base._mean_at(px)
        ys = resid.reshape(-1) * rs
        # A - I = Bs^T Bs: ONE product over the n data points (K = n is cut into slices so that the whole chip works);
        # c = Bs^T ys is a matrix-vector pass; the trace term needs no pass of its own:
        #   sum_a (k_aa - |B_:a|^2) / d_a = sum_a k_aa / d_a - tr(A - I)
        # (the matrix-vector pass is bound by memory, the product by the matrix cores: side by side on two streams)
        side2 = eng.side_stream() if hasattr(eng, "side_stream") and n * M >= (1 << 22) else None
        if side2 is not None:
            with _on_side(side2):
                c = eng.gemv_t(Bs, ys).reshape(1, M)
            G = eng.gemm(Bs, Bs, ta=True, c_lower=True)
            _join_side(side2, c)
        else:
            G = eng.gemm(Bs, Bs, ta=True, c_lower=True)
            c = eng.gemv_t(Bs, ys).reshape(1, M)
        if ill is not None:
            # product-first order (skipped on the device when K_zz is ill-conditioned): [S; c^T] <- [S; c^T] L_z^-T, then the
            # transposed M x M block once more - L_z^-1 S L_z^-T and L_z^-1 c.  S enters symmetrised, so that the transposition
            # is the identity when the solves are skipped.
            W = eng.new_matrix(M + 1, M)
            low = torch.tril(G)
            W[:M].copy_(low + torch.tril(low, -1).T)
            W[M:].copy_(c)
            eng.trsm_rlt_(Lz, W, when=(ill, False))
            c = W[M:].clone()
            G = eng.new_matrix(M, M)
            G.copy_(W[:M].T)
            eng.trsm_rlt_(Lz, G, when=(ill, False))
        if hasattr(eng, "vfe_factor") and getattr(eng, "cholesky_retry_factor", 1.0) <= 1.0 and os.environ.get("GPAR_VFE_FUSED_SCALARS", "1") != "0":
            # the scalar side - four sums, the assembly of [[I + G, .], [c^T, 0]], the bound from its pieces - in three launches
            # around the factorisation instead of ~25 tensor operations (0.15 ms per layer at C4)
            Abuf, logdetA, infoA, elbo = eng.vfe_factor(G, c, ys, kdiag, d, self.method == "vfe")
            eng.check_info(infoA)
            facA = _Factor.from_batch(eng, M, Abuf, logdetA)
        else:
            yDy = torch.sum(ys * ys)
            trace_term = torch.sum(kdiag / d) - torch.sum(torch.diagonal(G)) if self.method == "vfe" else 0.0

            def fill(block, scale):
                block.copy_(G)
                # (first attempt: A as it is - its diagonal is >= 1; a retry of lab's ladder adds the grown part of the jitter,
                # so that every rung factors a different matrix)
                block.diagonal().add_(1.0 + (scale - 1.0) * eng.epsilon)

            facA = _Factor(eng, M, fill, c)
            elbo = -0.5 * (trace_term + torch.sum(torch.log(d)) + n * _LOG_2PI + facA.logdet[0] + yDy - facA.quad)
        # v = L_z^-T A^-1 c, so that the mean correction at x* is K_*z v: two single-row backward solves (0.17 ms at M = 1024) that
        # only a posterior MEAN needs - the value of the bound does not (the last layer of a log marginal likelihood never asks)
        deferring = getattr(eng, "_deferred", None) is not None
        self._state = {"Lz": Lz, "La": facA.L, "v": _LazyV(eng, facA, Lz), "elbo": elbo.detach() if deferring else elbo.detach().cpu(),
                       "Bs": Bs, "G": G, "facA": facA, "kdiag": kdiag, "ys": ys, "d": d, "solved": ill is None,
                       "moves": (excess > 0).to(d.dtype) if self.method == "fitc" else None}
        return self._state

    def _value(self):
        return self._compute()["elbo"]

    def _solved_state(self):
        """The state with Bs = D^-1/2 K_xz L_z^-T in it (what the gradient pass differentiates): computed again, cross-Gram solve
        first, should a value-only evaluation have left the order to the device."""
        st = self._compute()
        if not st["solved"]:
            self._state, self._force_solve = None, True
            st = self._compute()
        return st

    def logpdf(self):
        """The VFE bound; differentiable with respect to kernel parameters and noise when they carry a graph."""
        if not self.base.is_posterior and torch.is_grad_enabled():
            params = kernel_parameters(self.base.kernel)
            noise = self.fdd.noise_arg if _needs_grad(self.fdd.noise_arg) else None
            X = self.fdd.x if self.fdd.x.requires_grad else None
            Z = self.u.x if self.u.x.requires_grad else None
            if params or noise is not None or X is not None or Z is not None:
                self._params = params
                self._noise_device = None if noise is None else noise.device
                self._force_solve = True   # (the gradient pass needs the solved cross-Gram)
                return _LogMarginal.apply(self, noise, X, Z, *[p[3] for p in params])
        return self._value()

    elbo = logpdf

    def gradients(self):
        """(dF/dd as a device vector, kernel-parameter gradients) of the VFE bound F (Titsias 2009, eq. 9).

        With S = Q + D, Q = K_fu K_uu^-1 K_uf, G = alpha alpha^T - S^-1 (alpha = S^-1 y) and P = K_uu^-1 K_uf:
            dF = sum_aj [W_fu]_aj dK_fu[a, j] + sum_ij [W_uu]_ij dK_uu[i, j] - 1/2 sum_a dk_aa / d_a + sum_a g_a dd_a,
            W_fu = (G + D^-1) P^T,   W_uu = -1/2 P (G + D^-1) P^T,   g_a = 1/2 (G_aa + (k_aa - q_aa) / d_a^2).
        Nothing n x n is formed: with B = L_z^-1 K_uf, A = I + B D^-1 B^T (both available from the forward pass),
            G + D^-1 = alpha alpha^T + D^-1 B^T A^-1 B D^-1,
            W_fu = [alpha beta^T + D^-1 B^T (I - A^-1)] L_z^-1,   beta = B alpha,
            W_uu = -1/2 L_z^-T (beta beta^T + A - 2 I + A^-1) L_z^-1,
            (S^-1)_aa = 1/d_a - |L_A^-1 B_:a|^2 / d_a^2.
        The forward pass keeps Bs = D^-1/2 B^T, so B^T = D^1/2 Bs throughout.  The three weighted sums over kernel
        derivatives are one fused device pass each (`kernel_grads_vfe`)."""
        vfe, fitc = self.method == "vfe", self.method == "fitc"
        eng = self.eng
        st = self._solved_state()
        n, M = self.fdd.n, self.u.n
        d = st["d"]  # the observation noise; FITC: the effective noise d + k_aa - q_aa
        rs = torch.rsqrt(d)
        Bs, facA, Lz, G = st["Bs"], st["facA"], st["Lz"], st["G"]
        a = facA.alpha()  # (A^-1 B D^-1 y)^T, 1 x M
        alpha = (st["ys"] - eng.gemm(Bs, a, tb=True).reshape(-1)) * rs  # S^-1 y
        beta = eng.gemv_t(Bs, alpha / rs).reshape(1, M)  # (B alpha)^T
        Ainv = eng.chol_inverse(facA.L)  # lower triangle of A^-1
        Ainv_full = torch.tril(Ainv) + torch.tril(Ainv, -1).T
        # W_fu
        T = eng.new_matrix(n, M)
        if vfe:
            T.copy_(Bs)
        else:
            T.zero_()  # DTC: no trace term, W_fu = G P^T = [alpha beta^T - D^-1 B^T A^-1] L_z^-1
        eng.gemm(Bs, Ainv_full, alpha=-1.0, beta=1.0, out=T)  # Bs (I - A^-1)   [DTC: -Bs A^-1]
        T.mul_(rs[:, None])  # D^-1 B^T (I - A^-1)
        T.add_(alpha[:, None] * beta)
        # per-point terms: |L_A^-1 B_:a|^2 / d_a^2 = |Es_a|^2 / d_a with Es = Bs L_A^-T, and q_aa / d_a^2 = |Bs_a|^2 / d_a
        E = eng.new_matrix(n, M)
        E.copy_(Bs)
        eng.trsm_rlt_(facA.L, E)
        if vfe:
            noise_grad = 0.5 * (alpha * alpha - 1.0 / d + (eng.rownorm2(E) - eng.rownorm2(Bs)) / d + st["kdiag"] / (d * d))
            wdiag = -0.5 / d
        else:
            noise_grad = 0.5 * (alpha * alpha - 1.0 / d + eng.rownorm2(E) / d)
            wdiag = torch.zeros_like(d)
        del E
        S = eng.new_matrix(M, M)
        S.copy_(beta.reshape(M, 1) * beta + Ainv_full)
        if vfe:
            S.add_(torch.tril(G) + torch.tril(G, -1).T)  # B D^-1 B^T = A - I (the trace term's share)
        S.diagonal().sub_(1.0)
        if fitc:
            # FITC is the DTC objective at the effective noise e_a = d_a + k_aa - q_aa, q_aa = K_az K_zz^-1 K_za, which moves with
            # the kernel: with g_a = dF / de_a (the DTC noise gradient above), sum_a g_a de_a adds
            #   g_a dk_aa                      -> wdiag = g,
            #   -2 g_a [K_az K_zz^-1] dK_za    -> W_fu -= 2 diag(g) B^T L_z^-1          (B^T = D^1/2 Bs),
            #   +g_a [P dK_zz P^T]_aa          -> W_uu += P diag(g) P^T, i.e. S -= 2 B diag(g) B^T
            # (points whose k_aa - q_aa was clamped at zero do not move).
            chain = noise_grad * st["moves"]
            wdiag = chain
            T.sub_((2.0 * chain / rs)[:, None] * Bs)
            eng.gemm(Bs * (chain * d)[:, None], Bs, ta=True, alpha=-2.0, beta=1.0, out=S)
        eng.trsm_rln_(Lz, T)  # ... L_z^-1
        # W_uu
        eng.trsm_rln_(Lz, S)  # S L_z^-1
        St = eng.new_matrix(M, M)
        St.copy_(S.T)
        eng.trsm_rln_(Lz, St)  # L_z^-T S L_z^-1 (symmetric)
        Wuu = eng.new_matrix(M, M)
        Wuu.copy_(-0.25 * (St + St.T))
        ck = self.fdd.pts().ck
        grads = eng.kernel_grads_vfe(ck, self.fdd.x.detach(), self.u.x.detach(), T, Wuu, wdiag)
        self._weights = (T, Wuu, wdiag)
        return noise_grad, grads

    def input_gradients(self, want_x, want_z):
        """dF / dX and dF / dZ from the same three weight arrays as the parameter gradients:
        F' = sum W_fu dK(X, Z) + sum W_uu dK(Z, Z) + sum wdiag dk(x, x)."""
        eng = self.eng
        T, Wuu, wdiag = self._weights
        ck = self.fdd.pts().ck
        X, Z = self.fdd.x.detach(), self.u.x.detach()
        gX = gZ = None
        if want_x:
            gX = eng.kernel_input_grads(ck, X, Z, T) + eng.kernel_diag_input_grads(ck, X, wdiag)
        if want_z:
            Tt = eng.new_matrix(Z.shape[0], X.shape[0])
            Tt.copy_(T.T)
            gZ = eng.kernel_input_grads(ck, Z, X, Tt) + eng.kernel_input_grads(ck, Z, None, Wuu, sym=True)
        return gX, gZ

    def mean_gradients(self, xs, g, want_xs=True, want_x=True, want_z=True):
        """Gradients of  g^T mean(xs),  mean(xs) = K(xs, Z) v,  v = Sigma^-1 K_zx D^-1 y,  Sigma = K_zz + K_zx D^-1 K_xz.
        With h = Sigma^-1 K(Z, xs) g, p = K_xz v (the mean at X) and q = K_xz h:
            d = sum (g v^T) dK(xs, Z) + sum W_fu dK(X, Z) + sum W_uu dK(Z, Z) - sum_a q_a (y_a - p_a) / d_a^2 dd_a,
            W_fu = ((y - p) / d) h^T - (q / d) v^T,     W_uu = -1/2 (h v^T + v h^T).
        FITC: d is the effective noise e_a = d_a + k_aa - q_aa; the term sum_a n_a de_a (n_a = the noise gradient above) adds
        n_a dk_aa - 2 n_a [K_az K_zz^-1] dK_za + n_a [P dK_zz P^T]_aa to the three weighted sums, as in `gradients`."""
        eng, st = self.eng, self._compute()
        ck = self.fdd.pts().ck
        X, Z = self.fdd.x.detach(), self.u.x.detach()
        n, M = self.fdd.n, self.u.n
        d = st["d"]  # FITC: the effective noise (its own dependence on the kernel is chained in below)
        v = st["v"].get().reshape(-1)
        pxs = self.base._pts(xs)
        Ksz = eng.gram(ck, pxs.z, self.u.pts().z)  # n* x M
        Kxz = eng.gram(ck, self.fdd.pts().z, self.u.pts().z)  # n x M
        h = eng.gemv_t(Ksz, g).reshape(1, M).clone()
        eng.trsm_rlt_(st["Lz"], h)
        eng.trsm_rlt_(st["La"], h)
        eng.trsm_rln_(st["La"], h)
        eng.trsm_rln_(st["Lz"], h)
        h = h.reshape(-1)
        p_ = eng.gemm(Kxz, v.reshape(1, M), tb=True).reshape(-1)
        q_ = eng.gemm(Kxz, h.reshape(1, M), tb=True).reshape(-1)
        resid = self.y.reshape(-1).detach() - p_
        W_sz = eng.new_matrix(xs.shape[0], M)
        W_sz.copy_(g[:, None] * v[None, :])
        W_fu = eng.new_matrix(n, M)
        W_fu.copy_((resid / d)[:, None] * h[None, :] - (q_ / d)[:, None] * v[None, :])
        W_uu = eng.new_matrix(M, M)
        W_uu.copy_(-0.5 * (h[:, None] * v[None, :] + v[:, None] * h[None, :]))
        noise_grad = -q_ * resid / (d * d)
        chain = None
        if self.method == "fitc":
            chain = noise_grad * st["moves"]
            Pt = eng.new_matrix(n, M)
            Pt.copy_(st["Bs"] * torch.sqrt(d)[:, None])
            eng.trsm_rln_(st["Lz"], Pt)  # K_xz K_zz^-1
            W_fu.sub_(2.0 * chain[:, None] * Pt)
            eng.gemm(Pt * chain[:, None], Pt, ta=True, alpha=1.0, beta=1.0, out=W_uu)
            del Pt
        params = _add_grads(eng.kernel_grads_weighted(ck, xs, Z, W_sz), eng.kernel_grads_weighted(ck, X, Z, W_fu))
        params = _add_grads(params, eng.kernel_grads_weighted(ck, Z, None, W_uu, sym=True))
        if chain is not None:
            params = _add_grads(params, eng.kernel_grads_diag(ck, X, chain))
        out = {"params": params, "noise": noise_grad}
        if want_xs:
            out["xs"] = eng.kernel_input_grads(ck, xs, Z, W_sz)
        if want_x:
            out["x"] = eng.kernel_input_grads(ck, X, Z, W_fu)
            if chain is not None:
                out["x"] = out["x"] + eng.kernel_diag_input_grads(ck, X, chain)
        if want_z:
            A_ = eng.new_matrix(M, xs.shape[0])
            A_.copy_(W_sz.T)
            B_ = eng.new_matrix(M, n)
            B_.copy_(W_fu.T)
            out["z"] = (eng.kernel_input_grads(ck, Z, xs, A_) + eng.kernel_input_grads(ck, Z, X, B_)
                        + eng.kernel_input_grads(ck, Z, None, W_uu, sym=True))
        return out

    # ---- the posterior's corrections (any base process) -----------------------------------------------
    def _P(self, p):
        """(k_base(p, Z), P = k_base(p, Z) L_z^-T) as two n_p x M matrices."""
        Kz = self.base._cross(p, self.u.pts())
        P = Kz.clone()
        self.eng.trsm_rlt_(self._compute()["Lz"], P)
        return Kz, P

    def mean_at(self, p):
        st = self._compute()
        Kz = self.base._cross(p, self.u.pts())
        corr = self.eng.gemm(Kz, st["v"].get(), tb=True)
        return corr if not self.base.is_posterior else self.base._mean_at(p) + corr

    # kept for callers that use the stheno-like name
    def posterior_mean(self, x):
        return self.mean_at(self.base._pts(x))

    def cross(self, pa, pb):
        eng, st = self.eng, self._compute()
        K = self.base._cross(pa, pb)
        _, Pa = self._P(pa)
        _, Pb = self._P(pb)
        eng.gemm(Pa, Pb, tb=True, alpha=-1.0, beta=1.0, out=K)
        eng.trsm_rlt_(st["La"], Pa)
        eng.trsm_rlt_(st["La"], Pb)
        eng.gemm(Pa, Pb, tb=True, alpha=1.0, beta=1.0, out=K)
        return K

    def diag(self, p):
        eng, st = self.eng, self._compute()
        _, P = self._P(p)
        out = self.base._diag(p) - eng.rownorm2(P)
        eng.trsm_rlt_(st["La"], P)
        return out + eng.rownorm2(P)

    # ---- batched sampling (ancestral sampling hands every layer S input sets of one size: GPAR.sample_many) ----------------
    @property
    def fast_sparse(self):
        """The batched routines below are written for inducing-point observations of a PRIOR process (what GPAR builds)."""
        return not self.base.is_posterior

    def _stacked_P(self, xs):
        """For the input sets stacked by rows: (features, K(x_s, Z), P_s = K(x_s, Z) L_z^-T), ONE launch each."""
        eng, st = self.eng, self._compute()
        ck, zu = self.u.features()
        stacked = xs.matrix if isinstance(xs, Stacked) else torch.cat([_as_matrix(eng, x_s) for x_s in xs], dim=0)
        z_all = eng.features(ck, _as_matrix(eng, stacked))
        Kz = eng.new_matrix(z_all.shape[0], self.u.n)
        eng.gram(ck, z_all, zu, out=Kz)
        P = Kz.clone()
        eng.trsm_rlt_(st["Lz"], P)
        return ck, z_all, Kz, P

    def _sparse_chunk(self, ns):
        return max(1, min(16384, int(16e9 // max(1, ns * max(self.u.n, ns, 1) * 8))))

    def posterior_mean_batch(self, xs):
        """Posterior means K(x_s, Z) v at several input sets with one stacked cross-Gram product."""
        eng, st = self.eng, self._compute()
        ck, zu = self.u.features()
        sizes = [int(x_s.shape[0]) for x_s in xs]
        stacked = xs.matrix if isinstance(xs, Stacked) else torch.cat([_as_matrix(eng, x_s) for x_s in xs], dim=0)
        Kz = eng.new_matrix(sum(sizes), self.u.n)
        eng.gram(ck, eng.features(ck, _as_matrix(eng, stacked)), zu, out=Kz)
        return list(torch.split(eng.gemm(Kz, st["v"].get(), tb=True), sizes, dim=0))

    def posterior_marginals_batch(self, xs):
        """(means, variances), each n* x S (no noise):  k_aa - |P_a|^2 + |P_a L_A^-T|^2  per point."""
        eng, st = self.eng, self._compute()
        S, ns = len(xs), int(xs[0].shape[0])
        dev = self.y.device
        mean = torch.zeros(ns, S, dtype=torch.float64, device=dev)
        var = torch.empty(ns, S, dtype=torch.float64, device=dev)
        chunk = self._sparse_chunk(ns)
        for s0 in range(0, S, chunk):
            s1 = min(S, s0 + chunk)
            ck, z_all, Kz, P = self._stacked_P(xs[s0:s1])
            mean[:, s0:s1] = eng.gemm(Kz, st["v"].get(), tb=True).reshape(s1 - s0, ns).T
            kd = eng.gram_diag(ck, z_all) - eng.rownorm2(P)
            eng.trsm_rlt_(st["La"], P)
            var[:, s0:s1] = (kd + eng.rownorm2(P)).reshape(s1 - s0, ns).T
        return mean, var

    def posterior_sample_batch(self, xs, noise):
        """One joint draw at each input set: mean_s + chol(K_ss - P_s P_s^T + R_s R_s^T + noise + eps I) z_s with P_s = K(x_s, Z) L_z^-T,
        R_s = P_s L_A^-T - the stacked cross-Gram, both triangular solves, the per-sample Gram builds, the two rank-M corrections
        and the n* x n* factorisations each ONE (batched / lock-step) launch sequence for all samples, as the dense posterior's
        sampler does it.  (Until round 3 every sample went through `f(x_s).sample()` on its own: `predict` with 50 samples at
        n* = 1000, M = 300 took 85 ms - four times the DENSE posterior's 21 ms.)"""
        eng, st = self.eng, self._compute()
        S, ns = len(xs), int(xs[0].shape[0])
        out = torch.empty(ns, S, dtype=torch.float64, device=self.y.device)
        if ns == 0:
            return out
        noise_vec = _noise_vector(eng, noise, ns)
        zr = eng.randn(ns, S)
        chunk = self._sparse_chunk(ns)
        for s0 in range(0, S, chunk):
            s1 = min(S, s0 + chunk)
            K = s1 - s0
            ck, z_all, Kz, P = self._stacked_P(xs[s0:s1])
            means = eng.gemm(Kz, st["v"].get(), tb=True)
            batched = K > 1 and hasattr(eng, "potrf_batch_") and ns <= eng.batch_rows() and not getattr(eng._tls, "safe", False)
            if batched:
                covs = eng.new_matrix(K * ns, ns)
                eng.gram_batch_(ck, z_all, K, covs, lower=True, diag_add=noise_vec, diag_const=eng.epsilon)
                eng.gemm_batch_(P, P, covs, K, tb=True, alpha=-1.0, beta=1.0, c_lower=True)
                eng.trsm_rlt_(st["La"], P)
                eng.gemm_batch_(P, P, covs, K, tb=True, alpha=1.0, beta=1.0, c_lower=True)
                _, info = eng.potrf_batch_(covs, K)
                eng.check_info(info)
                eng.trmv_lower_batch_(covs, K, zr[:, s0:s1], out[:, s0:s1], add=means)
                continue
            R = P.clone()
            eng.trsm_rlt_(st["La"], R)
            for k in range(K):
                rows = slice(k * ns, (k + 1) * ns)
                cov = eng.new_matrix(ns, ns)
                eng.gram(ck, z_all[rows], lower=True, diag_add=noise_vec, diag_const=eng.epsilon, out=cov)
                eng.gemm(P[rows], P[rows], tb=True, alpha=-1.0, beta=1.0, out=cov, c_lower=True)
                eng.gemm(R[rows], R[rows], tb=True, alpha=1.0, beta=1.0, out=cov, c_lower=True)
                _, info = eng.potrf_(cov)
                eng.check_info(info)
                out[:, s0 + k : s0 + k + 1] = eng.trmv_lower(cov, zr[:, s0 + k : s0 + k + 1]) + means[rows]
        return out

    def moments_into(self, p, block, diag_add, jitter):
        eng, st = self.eng, self._compute()
        mean = self.base._moments_into(p, block, diag_add, jitter)
        Kz, P = self._P(p)
        corr = eng.gemm(Kz, st["v"].get(), tb=True)
        eng.gemm(P, P, tb=True, alpha=-1.0, beta=1.0, out=block, c_lower=True)
        eng.trsm_rlt_(st["La"], P)  # Q = P L_A^-T
        eng.gemm(P, P, tb=True, alpha=1.0, beta=1.0, out=block, c_lower=True)
        return corr if not self.base.is_posterior else mean + corr


class PseudoObsFITC(PseudoObs):
    method = "fitc"


class PseudoObsDTC(PseudoObs):
    method = "dtc"


PseudoObsVFE = PseudoObs
SparseObs = PseudoObs


def fused_updates():
    """GPAR_CHOL_UPDATE=0 (read at every call): `chol_drop_leading` / `chol_append_` take the route composed of the engine's primitives
    on every engine - the yardstick of the library calls."""
    return os.environ.get("GPAR_CHOL_UPDATE", "1") != "0"


def _chol_drop_leading_composed(eng, A, k):
    """The augmented factor of the observations k .. n - 1 from that of all n, from primitives every engine has: with B = [L21, L22] (the
    rows k .. n - 1 of L), S22 = B B^T = L21 L21^T + L22 L22^T and y2 = B z by `gemm`, then the partial factorisation of the augmented
    [[S22, .], [y2^T, 0]] by `potrf_` - O(n^3 / 3), where the library's rank-k update costs O(k n^2)."""
    n = int(A.shape[0]) - 1
    m = n - k
    B = eng.new_matrix(m, n)
    B.copy_(torch.tril(A[k:n, :n], diagonal=k))   # (the strict upper triangle of a factor buffer is scratch)
    out = eng.new_matrix(m + 1, m + 1)
    eng.gemm(B, B, tb=True, out=out[:m, :m], c_lower=True)
    out[m:m + 1, :m] = eng.gemm(A[n:n + 1, :n], B, tb=True)
    out[m, m].zero_()
    logdet, info = eng.potrf_(out, nf=m)
    return out, logdet, info


def chol_drop_leading(eng, A, k):
    """(out, logdet, info): `HipEngine.chol_drop_leading` where the engine has it (and `fused_updates()`), otherwise composed."""
    if hasattr(eng, "chol_drop_leading") and fused_updates() and k <= CHOL_UPDATE_MAX_RANK:
        return eng.chol_drop_leading(A, k)
    return _chol_drop_leading_composed(eng, A, k)


def _chol_append_composed(eng, A, n0, k, logdet):
    """gpar_chol_append from primitives every engine has, on the same layout: the k new rows solved against L (`trsm_rlt_`), the trailing
    (k + 1) x (k + 1) block downdated by the k + 1 bottom rows (`gemm`), and factored (`potrf_`, nf = k)."""
    A[n0 + k, n0 + k].zero_()
    tail = A[n0:, n0:]
    if n0 > 0:
        eng.trsm_rlt_(A[:n0, :n0], A[n0:n0 + k, :n0])
        bottom = A[n0:, :n0]
        eng.gemm(bottom, bottom, tb=True, alpha=-1.0, beta=1.0, out=tail, c_lower=True)
    more, info = eng.potrf_(tail, nf=k)
    return logdet + more, info


def chol_append_(eng, A, n0, k, logdet):
    """(logdet, info) with A factored in place: `HipEngine.chol_append_` where the engine has it (and `fused_updates()`), otherwise composed."""
    if hasattr(eng, "chol_append_") and fused_updates():
        return eng.chol_append_(A, n0, k, logdet)
    return _chol_append_composed(eng, A, n0, k, logdet)


def _pivoted_cholesky_composed(eng, ck, z, max_rank, tol, floor):
    """The greedy pivoted Cholesky of k(z, z) from primitives every engine has - `gram_diag`, `gram` against the pivot's single row,
    torch for the update and the argmax, ONE device-to-host read per pivot (the row, its residual and the trace together) - with the
    semantics of gpar_pivoted_chol (include/gpar_hip.h): ties go to the smallest row, a NaN ranks above every number (+inf included),
    the same three stop rules, zero rows and -1 pivots beyond the rank.  The route of engines without `pivoted_cholesky`, and the
    yardstick of the fused call."""
    n = int(z.shape[0])
    d = eng.gram_diag(ck, z).reshape(-1).clone()
    dev = d.device
    Lt = torch.zeros(max_rank, n, dtype=torch.float64, device=dev)
    rows = torch.arange(n, device=dev)
    piv, trace = [-1] * max_rank, [0.0] * (max_rank + 1)
    rank, info = max_rank, 0
    for j in range(max_rank + 1):
        nan = torch.isnan(d)
        top = torch.where(nan, torch.full_like(d, -math.inf), d).max()
        p = torch.where(torch.where(nan.any(), nan, d == top), rows, n).min()
        p, dp, tr = torch.stack([p.to(torch.float64), d[p], d.sum()]).tolist()   # (the step's one synchronisation)
        p = int(p)
        trace[j] = tr
        if j == max_rank:
            break
        if dp <= floor or tr <= tol * trace[0] or not math.isfinite(dp):
            rank, info = j, (0 if math.isfinite(dp) else p + 1)
            break
        c = eng.gram(ck, z, z[p:p + 1]).reshape(-1) - Lt[:j, p] @ Lt[:j]
        root = math.sqrt(dp)
        col = c / root
        col[p] = root
        Lt[j] = col
        d = d - col * col
        d[p] = 0.0
        piv[j] = p
    eng.check_info(torch.tensor([info], dtype=torch.int32))
    return (Lt, torch.tensor(piv, dtype=torch.int32, device=dev), torch.tensor(trace, dtype=torch.float64, device=dev),
            torch.tensor([rank], dtype=torch.int32, device=dev))


def greedy_inducing(eng, ck, x, num, tol=0.0, floor=None):
    """Greedy selection of up to `num` inducing points among the rows of the design matrix `x` under the compiled kernel `ck`: the
    partially pivoted Cholesky factorisation of k(x, x) that always takes the row of largest conditional variance next (Fine &
    Scheinberg 2001; the initialisation Burt et al. 2019 recommend for sparse variational GPs).  O(n num^2), deterministic, and it stops
    early when the largest residual variance is at most `floor` (None: the engine's jitter, which K_zz receives anyway) or the
    residual trace tr(K - Q) - the quantity the VFE bound penalises - has fallen to `tol` times its start.
    Returns engine tensors (Lt, piv, trace, rank): the factor transposed (num x n, K ~ Lt^T Lt, zero rows from the rank on), the chosen
    rows in order (int32, -1 beyond the rank), the residual trace before every step (num + 1 values; trace[rank] is the final one)
    and the rank as a one-element tensor.  Engines with `pivoted_cholesky` take it (one library call, no synchronisation); others run
    the same algorithm composed of their primitives."""
    z = eng.features(ck, _as_matrix(eng, x))
    num = int(num)
    if not 1 <= num <= int(z.shape[0]):
        raise ValueError(f"num={num}: between 1 and the number of rows ({int(z.shape[0])}) inducing points can be selected")
    floor = eng.epsilon if floor is None else float(floor)
    if hasattr(eng, "pivoted_cholesky"):
        return eng.pivoted_cholesky(ck, z, num, tol=tol, floor=floor)
    return _pivoted_cholesky_composed(eng, ck, z, num, float(tol), floor)
