"""Layer-parallel GPAR over the GPUs of one node: one process per GPU, `torch.distributed` (backend "nccl" = RCCL
over xGMI on the MI355X box, "gloo" in the CPU tests).

The p autoregressive layers are the units of work: layer i is owned by rank i mod G.  What has to travel between
ranks is decided by the model, exactly as in /root/reference/gpar/model.py:291-322:

  * `replace=False`, nothing to impute, no inducing points: layer i's design matrix is `[x, observed y_<i]`, which
    every rank already holds -> layers are independent, the data path has NO collective; only the p scalar
    log-likelihoods are summed (one 8-byte all-reduce).
  * otherwise (posterior means are fed forward): the owner of layer i computes the new input column (and the new
    inducing-input column) and broadcasts it — n x 8 bytes per layer, latency-bound — before layer i+1 can start.

With `markov=k` a forwarded column is read by the next k layers only (reference regression.py:49-59: the kernel of layer j
selects the last k outputs), so it is SENT to the owners of those layers alone (point-to-point) instead of broadcast; ranks
that never read a column hold NaN in its place (a violation would be loud).

The log marginal likelihood (`sharded_logpdf`) and the conditioning (`sharded_condition`) run the model's own layer loops
(`GPAR._logpdf`, `GPAR._condition`) with a `_Shard`: which layers this rank owns, and
how a forwarded column travels.  An evaluation that fails in a way `GPAR.logpdf` would retry in the engine's safe mode is retried
here too: every rank repeats it when any rank asks for it (`sharded_logpdf`: NaN in the all-reduce, then one more small one).

`fit(fix=True)` trains each layer on its owner (the optimiser only touches names "{i}/*", reference
regression.py:453-454) and then broadcasts the trained latent variables so every rank holds the same `Vars`.
`fit(fix=False)` (the joint objective, reference regression.py:447-456) shards the sum over layers the same way: every rank
evaluates its layers' terms and their gradients, one all-reduce adds values and gradient vectors (the slices "{i}/*" are
disjoint, the tied "0/input/scales" receives every layer's contribution), and ONE L-BFGS-B driver on rank 0 broadcasts the
iterates.  Where layer inputs are posterior means of earlier layers (`replace`, imputation, inducing points) training is
REPLICATED: every rank runs the serial `fit` (`sharded_fit` returns which of the three it did).
`predict` conditions layer-parallel (`sharded_condition`), splits the Monte-Carlo samples across ranks, all-gathers the
device-resident sample stacks once and reduces them with `gpar_sample_stats` (`sharded_predict`).
"""
import contextlib

import numpy as np
import torch
import torch.distributed as dist

from .engine import get_engine
from .model import host_masks, per_output

__all__ = ["world", "sharded_logpdf", "sharded_fit", "sharded_condition", "sharded_sample", "sharded_predict", "forward_plan"]


def world(group=None):
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


class _Shard:
    """Layer i is evaluated by rank i mod G; a column of posterior means it feeds forward goes to the ranks that read it
    (`needs`, from `forward_plan`) - what `GPAR._logpdf` / `GPAR._condition` ask of their `shard` argument."""

    def __init__(self, rank, size, group, needs=None):
        self.rank, self.size, self.group, self.needs = rank, size, group, needs

    def owns(self, i):
        return i % self.size == self.rank

    def forward(self, i, col, ind_col):
        mine = self.owns(i)
        if mine:
            col, ind_col = col.contiguous(), (None if ind_col is None else ind_col.contiguous())
        _forward(col, ind_col, mine, i % self.size, self.needs[i], self.rank, self.size, self.group)


def sharded_logpdf(gpar, x, y, w, group=None, timing=None):
    """`GPAR.logpdf(x, y, w)` with the layers divided over the ranks of `group`; every rank returns the total.
    `timing` (a dict, optional) accumulates under "busy_s" the wall-clock this rank spent on its own layers, i.e. up to
    the collective, and under "collective_s" the time in the 8-byte all-reduce - which includes the wait for the slowest rank (what
    makes a multi-GPU run interpretable without a second one: the slowest rank's busy time bounds the step, a fast rank's
    collective time is the imbalance).

    The retry of `GPAR.logpdf` (model._retry_unfused) is decided by all ranks together, as the forwarded columns of the dependent
    regimes are collectives inside the evaluation and a rank must not repeat it alone: a rank whose evaluation failed adds NaN to
    the all-reduce; only when the sum is not finite do the ranks exchange a second word - how many failed in a way that may be
    retried (model._retryable) and how many fatally.  After a retryable failure every rank repeats the evaluation once in the
    engine's safe mode; a failure in the repetition, or a fatal one, raises on every rank (the failing rank its own exception,
    the others a RuntimeError); a sum that is NaN without a failure is returned.  This covers failures reported when the
    evaluation's deferred checks are read, at its end - where the HIP engine reports them.  An exception raised in the middle of
    the layer loop, before a forward (the oracle engine raises at once), leaves the other ranks waiting in that forward."""
    import time

    from .model import _retryable

    t_start = time.perf_counter()
    rank, size = world(group)
    if size == 1:
        value = gpar.logpdf(x, y, w)
        if timing is not None:
            timing["busy_s"] = timing.get("busy_s", 0.0) + (time.perf_counter() - t_start)
        return value
    eng = get_engine()
    m = int(x.shape[1]) if len(x.shape) == 2 else 1
    shard = _Shard(rank, size, group, forward_plan(gpar, m, size))
    for attempt in range(2):
        failure = None
        try:
            with eng.safe_mode() if attempt else contextlib.nullcontext():
                local = gpar._logpdf(x, y, w, False, False, False, None, None, shard)
            buf = local.detach().to(device=eng.device, dtype=torch.float64).reshape(1).clone()
        except Exception as e:  # noqa: BLE001 - every rank must reach the all-reduce below
            failure = e
            buf = torch.full((1,), float("nan"), dtype=torch.float64, device=eng.device)
        t_busy = time.perf_counter()
        if timing is not None:
            timing["busy_s"] = timing.get("busy_s", 0.0) + (t_busy - t_start)
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
        total = buf[0].cpu()
        if timing is not None:   # (includes the wait for the slowest rank: busy + collective = the step on every rank)
            timing["collective_s"] = timing.get("collective_s", 0.0) + (time.perf_counter() - t_busy)
        if torch.isfinite(total):
            return total
        retry = failure is not None and attempt == 0 and _retryable(failure, gpar.layers, (x, y, w))
        flags = torch.tensor([float(retry), float(failure is not None and not retry)], dtype=torch.float64, device=eng.device)
        dist.all_reduce(flags, op=dist.ReduceOp.SUM, group=group)
        retries, fatal = (int(v) for v in flags.cpu().tolist())
        if fatal:
            if failure is not None:
                raise failure
            raise RuntimeError(f"sharded_logpdf failed on {retries + fatal} other rank(s) (their exception is raised there)")
        if not retries:
            return total   # a log-likelihood that is NaN on its own
        t_start = time.perf_counter()


def _columns_read(kernel, width):
    """Design-matrix columns a layer kernel reads (a factor without a selection reads all `width` of them)."""
    cols = set()
    for term in kernel.terms:
        for factor in term.factors:
            cols.update(range(width) if factor.cols is None else (int(c) for c in factor.cols))
    return cols


def forward_plan(gpar, m, size):
    """needs[i] = ranks that read output column i (design-matrix column m + i): the owners (j mod size) of the layers j > i whose
    kernel selects it - all later layers without `markov`, the next k with `markov=k` (reference regression.py:49-59).  The
    owner of layer j also evaluates layer j's posterior mean when it forwards column j, through the same kernel."""
    import os

    count = len(gpar.layers)
    if os.environ.get("GPAR_MARKOV_SENDS", "1") == "0":
        return [set(range(size)) for _ in range(count)]
    needs = [set() for _ in range(count)]
    for j, model in enumerate(gpar.layers):
        f, _ = model()
        for c in _columns_read(f.kernel, m + j):
            if m <= c < m + j:
                needs[c - m].add(j % size)
    return needs


def _forward(col, ind_col, mine, owner, receivers, rank, size, group):
    """The forwarded column (and its inducing-input counterpart) from `owner` to `receivers` (group ranks): one broadcast when
    every other rank reads it, point-to-point sends otherwise; ranks that do not read it get NaN."""
    others = set(range(size)) - {owner}
    targets = set(receivers) - {owner}
    if not targets:
        if not mine:
            col.fill_(float("nan"))
            if ind_col is not None:
                ind_col.fill_(float("nan"))
        return
    if targets == others:
        dist.broadcast(col, src=_global_rank(owner, group), group=group)
        if ind_col is not None:
            dist.broadcast(ind_col, src=_global_rank(owner, group), group=group)
        return
    # one message per receiver: [column; inducing column]
    packed = col.reshape(-1) if ind_col is None else torch.cat([col.reshape(-1), ind_col.reshape(-1)])
    if mine:
        packed = packed.contiguous()
        for work in [dist.isend(packed, dst=_global_rank(r, group), group=group) for r in sorted(targets)]:
            work.wait()
    elif rank in targets:
        buf = torch.empty_like(packed)
        dist.recv(buf, src=_global_rank(owner, group), group=group)
        col.copy_(buf[: col.numel()].reshape(col.shape))
        if ind_col is not None:
            ind_col.copy_(buf[col.numel():].reshape(ind_col.shape))
    else:
        col.fill_(float("nan"))
        if ind_col is not None:
            ind_col.fill_(float("nan"))


def _global_rank(group_rank, group):
    if group is None:
        return group_rank
    return dist.get_global_rank(group, group_rank)


def layers_train_independently(reg, y):
    """With `fix=True`, is the training of layer pi independent of the training of the other layers?  Its inputs must be
    data only (no `replace`, no inducing points, nothing to impute) and it must not share a hyper-parameter with
    another layer (`scale_tie` reads "0/input/scales", which only layer 0 trains)."""
    return inputs_are_data(reg, y) and not reg.model_config.get("scale_tie", False)


def inputs_are_data(reg, y):
    """Every layer's design matrix is [x, observed y_<i]: nothing a layer computes is fed to a later one (no `replace`, no
    inducing points, nothing to impute), so the terms of the log-likelihood are separate functions of the hyper-parameters."""
    return not (reg.replace or reg.sparse or (reg.impute and bool(torch.isnan(y).any())))


def _tag_host_nan(reg, y_dev):
    """The NaN pattern of the (host-resident) training outputs, attached for per_output: masks planned on the host (GPAR._prep)."""
    if y_dev.is_cuda and host_masks():
        y_dev._host_nan, y_dev._host_nan_version = torch.isnan(reg.y).numpy(), y_dev._version


def _refuse_auto_periods(reg):
    """`spectral_period="auto"` reads a periodogram off the device engine; the ranks of a sharded driver may run on engines without one
    and would have to agree on the picks: refused, with the way out."""
    if reg.model_config.get("spectral_period") == "auto":
        raise ValueError('spectral_period="auto" is not available in the sharded drivers (their ranks may have no periodogram): pick the '
                         "periods once (GPARRegressor.periodogram, spectral_peaks) and pass spectral_period=(...)")


def sharded_fit(reg, x, y, w=None, group=None, fix=True, **kw_args):
    """`GPARRegressor.fit(x, y, w, fix=fix)` over the ranks of `group`; every rank ends up with the same hyper-parameters.
    Returns what it did:
      "layer-parallel"  fix=True, inputs are data, no tied scales: layer pi trained on rank pi mod G, results broadcast;
      "joint-sharded"   fix=False, inputs are data: the reference's p successive joint optimisations (layers 0..pi together,
                        regression.py:447-456) with the sum over layers divided over the ranks - see `_minimise_sharded`;
      "replicated"      layer inputs are posterior means of earlier layers (or, with fix=True, scales are tied): the chain is
                        sequential, every rank runs the serial `fit`."""
    from .regression import _construct_gpar

    _refuse_auto_periods(reg)
    rank, size = world(group)
    eng = get_engine()
    reg.condition(x, y, w)
    x_dev, y_dev, w_dev = eng.tensor(reg.x), eng.tensor(reg.y), eng.tensor(reg.w)
    _tag_host_nan(reg, y_dev)
    if not inputs_are_data(reg, y_dev) or (fix and not layers_train_independently(reg, y_dev)):
        # inputs of layer pi depend on the trained layers < pi: the chain is sequential; train replicated
        reg.fit(x, y, w, fix=fix, **kw_args)
        return "replicated"
    # instantiate every variable on every rank (lazy creation, reference regression.py:92-180)
    with torch.no_grad():
        _construct_gpar(reg, reg.vs, reg.m, reg.p).logpdf(x_dev[:2], y_dev[:2], w_dev[:2])
    owned = [pi for pi in range(reg.p) if pi % size == rank]
    if not fix:
        y_cached = {k: list(per_output(y_dev, w_dev, keep=k)) for k in [True, False]}
        # the design matrix of an owned layer, [x, y_<pi] with its rows: data only, so it is formed once
        fixed = {}
        for pi in owned:
            gpar = _construct_gpar(reg, reg.vs, reg.m, pi + 1)
            fixed[pi] = gpar.logpdf(x_dev, y_cached, None, only_last_layer=True, outputs=list(range(pi)), return_inputs=True)

        def term(vs, pi):
            g = _construct_gpar(reg, vs, reg.m, pi + 1)
            return -g.logpdf(fixed[pi][0], y_cached, None, only_last_layer=True, outputs=[pi], x_ind=fixed[pi][1])

        for pi in range(reg.p):
            mine = [i for i in owned if i <= pi]

            def local_objective(vs, mine=mine):
                total = torch.zeros((), dtype=torch.float64)
                for i in mine:
                    total = total + term(vs, i)
                return total

            _minimise_sharded(local_objective, reg.vs, [f"{i}/*" for i in range(pi + 1)], group, **kw_args)
        return "joint-sharded"
    # this rank's layers through the regressor's own layer-wise training: the prepared objective (gpar_amd/fastfit.py) and the
    # worker streams where they apply, the general route otherwise - what the single-process `fit` runs for the same layers
    reg._train(owned, fix=True, **kw_args)
    if size > 1:
        for pi in range(reg.p):
            names = reg.vs.match([f"{pi}/*"])
            if not names:
                continue
            vec = torch.as_tensor(reg.vs.get_vector(names), dtype=torch.float64).to(eng.device)
            dist.broadcast(vec, src=_global_rank(pi % size, group), group=group)
            reg.vs.set_vector(vec.cpu().numpy(), names)
    return "layer-parallel"


def _minimise_sharded(local_objective, vs, patterns, group, iters=1000, f_calls=10000, trace=False):
    """L-BFGS-B over the variables matching `patterns` of an objective that is a SUM of per-rank terms: `local_objective(vs)`
    is this rank's share.  One evaluation = every rank evaluates its share and back-propagates, then ONE all-reduce adds
    [value, gradient] over the ranks (a variable only this rank's layers read gets zeros from the others; a tied variable gets
    every layer's contribution).  The optimiser itself runs on rank 0 only and broadcasts each iterate - [1, x] to evaluate,
    [0, x_opt] to finish - so the ranks cannot drift apart, whatever their arithmetic.  Returns the final objective value."""
    import logging

    import scipy.optimize

    from . import optimise
    from .engine import NotPositiveDefiniteError

    rank, size = world(group)
    eng = get_engine()
    names = vs.match(patterns)
    latents = vs.get_vars(*names)
    if not latents:
        raise ValueError("no variables to optimise")
    x0 = vs.get_vector(names)
    dim = x0.size

    def evaluate(xvec):
        optimise._evaluations += 1
        vs.set_vector(xvec, names)
        previous = [t.requires_grad for t in latents]
        for t in latents:
            t.requires_grad_(True)
            t.grad = None
        fatal = None
        try:
            value = local_objective(vs)
            if value.requires_grad:
                value.backward()
            grad = np.concatenate([(t.grad if t.grad is not None else torch.zeros_like(t)).detach().numpy().reshape(-1) for t in latents])
            val = float(value.detach())
        except (NotPositiveDefiniteError, ArithmeticError) as e:  # as varz: report NaN and let the line search back off
            logging.getLogger(__name__).warning("objective evaluation failed (%s); returning NaN", e)
            val, grad = np.nan, np.zeros(dim)
        except Exception as e:  # noqa: BLE001 - anything else (a hand-off timeout re-raised under autograd, out of memory, a failed
            # point-to-point transfer) must not leave the other ranks waiting in the all-reduce below: this rank takes part in it,
            # with a failure flag every rank sees, and all of them raise afterwards
            fatal = e
            val, grad = np.nan, np.zeros(dim)
        finally:
            for t, r in zip(latents, previous):
                t.requires_grad_(r)
                t.grad = None
        buf = torch.as_tensor(np.concatenate([[val], grad, [0.0 if fatal is None else 1.0]]), dtype=torch.float64).to(eng.device)
        if size > 1:
            dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
        out = buf.cpu().numpy()
        if out[-1] > 0.0:
            if fatal is not None:
                raise fatal
            raise RuntimeError(f"the joint objective failed on {int(out[-1])} other rank(s) (their exception is raised there)")
        val, grad = float(out[0]), out[1:-1].copy()
        if not np.isfinite(val):
            val, grad = np.nan, np.zeros(dim)   # some rank's share failed: a failed evaluation for everybody
        if trace and rank == 0:
            print(f"  objective {val:.6e}  |grad| {np.linalg.norm(grad):.3e}")
        return val, grad

    def announce(flag, xvec):
        ctrl = torch.as_tensor(np.concatenate([[flag], np.asarray(xvec, dtype=np.float64)]), dtype=torch.float64).to(eng.device)
        if size > 1:
            dist.broadcast(ctrl, src=_global_rank(0, group), group=group)
        return ctrl.cpu().numpy()

    if rank == 0:
        def fg(xvec):
            announce(1.0, xvec)
            return evaluate(xvec)

        x_opt, val, _ = scipy.optimize.fmin_l_bfgs_b(fg, x0, maxiter=iters, maxfun=f_calls)
        announce(0.0, x_opt)
        vs.set_vector(x_opt, names)
        return val
    val = np.nan   # (never returned as such: scipy's driver evaluates its starting point, so rank 0 announces at least one evaluation)
    while True:
        ctrl = announce(0.0, np.zeros(dim))
        if ctrl[0] == 0.0:
            vs.set_vector(ctrl[1:], names)
            return val
        val, _ = evaluate(ctrl[1:])


def sharded_condition(reg, group=None):
    """The conditioned GPAR of `reg` (as `gpar | (x, y, w)`), with the p training-data factorisations divided over the
    ranks when no layer feeds another: layer i is factored by rank i mod G (a rank's layers pipelined over its streams, or in
    lock-step), through `GPAR._condition` and its retry in safe mode, and the factor buffers - L and the row L^-1 y - are then
    all-gathered in packed lower-triangular form, G layers per collective; every rank ends up holding every factor, which is what
    sample-parallel prediction needs.  In the dependent regimes (imputation, `replace`, inducing points) every rank conditions
    locally, as the chain is sequential anyway."""
    from .model import _retry_unfused
    from .regression import _construct_gpar

    _refuse_auto_periods(reg)
    rank, size = world(group)
    eng = get_engine()
    gpar = _construct_gpar(reg, reg.vs, reg.m, reg.p)
    data = (reg.x, reg.y, reg.w)
    x, y, w = gpar._prep(*data)
    items = list(per_output(y, w, keep=gpar.impute))
    if size == 1 or not gpar._independent(items) or not gpar._same_rows(items):
        # (layers whose rows differ - `impute=False` with missing data - are independent too, but their factors do not share a
        # shape: they are conditioned locally rather than exchanged)
        return gpar | data
    shard = _Shard(rank, size, group)

    def condition():
        post = gpar._condition(data, shard)
        return post, [layer()[0]._obs.factor() for layer in post.layers]   # (the others' factors: the empty buffers installed)

    post, factors = _retry_unfused(condition, gpar.layers, data)
    _exchange_factors(eng, factors, rank, size, group)
    return post


def _exchange_factors(eng, factors, rank, size, group):
    """Layer i's factor (L and the row L^-1 y: the lower triangle of the (n + 1) x (n + 1) buffer; every layer has the same n)
    lives on rank i mod G.  Round k all-gathers layers k G .. k G + G - 1 in PACKED form - (n + 1)(n + 2) / 2 doubles each, half
    the bytes of the padded square buffers and one collective over all xGMI links per round instead of one broadcast (one root's
    links) per layer.  The caller has joined its streams, so the collective is ordered after the factorisations."""
    count = len(factors)
    for first in range(0, count, size):
        mine = first + rank
        N = factors[first].n + 1
        length = N * (N + 1) // 2
        send = torch.empty(length, dtype=torch.float64, device=eng.device)
        if mine < count:
            eng.pack_lower(factors[mine].A, send)
        else:
            send.zero_()  # this rank has no layer in the last, incomplete round
        recv = [torch.empty(length, dtype=torch.float64, device=eng.device) for _ in range(size)]
        dist.all_gather(recv, send, group=group)
        for r in range(size):
            i = first + r
            if i < count and r != rank:
                eng.unpack_lower_(recv[r], factors[i].A)


def _sharded_sample_stack(reg, x, w, num_samples, latent, group, marginal=False):
    """(S x n* x p device tensor holding every rank's draws, in rank order; the per-rank counts): the conditioning is
    layer-parallel (`sharded_condition`), each rank draws its share with its own Philox stream, and the device-resident stacks
    are all-gathered ONCE - no sample visits the host."""
    _refuse_auto_periods(reg)
    rank, size = world(group)
    eng = get_engine()
    counts = [num_samples // size + (1 if r < num_samples % size else 0) for r in range(size)]
    eng.seed(getattr(eng, "_seed", 0) * 1000003 + rank + 1)
    post = sharded_condition(reg, group) if size > 1 else None
    mine = reg._sample_device(x, w, None, True, max(counts[rank], 1), latent, conditioned=post, marginal=marginal)[: counts[rank]]
    rows = int(np.shape(x)[0])
    local = torch.zeros(max(counts), rows, reg.p, dtype=torch.float64, device=eng.device)
    if mine:
        local[: len(mine)] = torch.stack([s.to(eng.device) for s in mine])
    if size == 1:
        return local[: counts[0]], counts
    gathered = [torch.empty_like(local) for _ in range(size)]
    dist.all_gather(gathered, local, group=group)
    return torch.cat([gathered[r][: counts[r]] for r in range(size)], dim=0), counts


def _refuse_pathwise(sampler):
    """The sharded drivers keep the exact sampler: a pathwise basis would have to be agreed on by the ranks."""
    if sampler != "exact":
        raise ValueError(f'the sharded drivers keep the exact sampler (got sampler={sampler!r}): use GPARRegressor.predict / sample for '
                         'sampler="pathwise"')


def sharded_sample(reg, x, w=None, num_samples=100, latent=False, group=None, sampler="exact"):
    """Posterior samples split over ranks (`_sharded_sample_stack`).  Returns the full list of `num_samples` arrays on every
    rank (the reference's return type: host arrays, regression.py:564).  `sampler`: "exact" only (ValueError otherwise)."""
    _refuse_pathwise(sampler)
    stack, _ = _sharded_sample_stack(reg, x, w, num_samples, latent, group)
    host = stack.cpu().numpy()
    return [host[k] for k in range(host.shape[0])]


def sharded_predict(reg, x, w=None, num_samples=100, latent=False, credible_bounds=False, marginal=False, group=None, sampler="exact"):
    """`GPARRegressor.predict` with the samples drawn across the ranks and the Monte-Carlo reduction (mean, central 95 %
    bounds; reference regression.py:589-595) done on the device by `gpar_sample_stats` over the gathered stack - only the
    n* x p results cross to the host.  Every rank returns the same arrays.  `sampler`: "exact" only (ValueError otherwise)."""
    _refuse_pathwise(sampler)
    stack, _ = _sharded_sample_stack(reg, x, w, num_samples, latent, group, marginal=marginal)
    eng = get_engine()
    if num_samples == 1:
        # the reference hands np.mean a single (n*, p) array here, so axis 0 is the input axis (regression.py:589-595); kept
        one = stack[0].cpu().numpy()
        mean = np.mean(one, axis=0)
        return (mean, np.percentile(one, 2.5, axis=0), np.percentile(one, 100 - 2.5, axis=0)) if credible_bounds else mean
    if credible_bounds:
        mean, lower, upper = eng.sample_stats(stack.contiguous(), 2.5, 100 - 2.5)
        return mean.cpu().numpy(), lower.cpu().numpy(), upper.cpu().numpy()
    return eng.sample_stats(stack.contiguous())[0].cpu().numpy()
