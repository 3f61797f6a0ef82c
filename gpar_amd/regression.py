"""GPARRegressor: sklearn-style front end (drop-in for /root/reference/gpar/regression.py).

Same constructor keywords and defaults (reference regression.py:264-286), attributes (:288-326) and methods —
`get_variables`, `condition`, `fit`, `logpdf`, `sample`, `predict` — with the same argument meaning, return
types and exceptions.  What differs is underneath: the per-layer kernels are `gpar_amd.kernels` objects lowered
to one fused device kernel, and every Gram / Cholesky / solve runs in libgpar_hip.so on the MI355X.

Hyper-parameter names, initialisations and bounds follow reference regression.py:92-180 exactly (table in
SURVEY.md Appendix C), so `get_variables()` dictionaries are interchangeable.
"""
import collections
import fnmatch
import os
import warnings

import numpy as np
import torch

from ._lib import CHOL_UPDATE_MAX_RANK, GPAR_MAX_DIMS, GPAR_MAX_FACTORS, GPAR_MAX_TERMS
from .engine import get_engine
from .gp import GP, Measure, check_score, greedy_inducing
from .kernels import EQ, RQ, Cosine, Linear, Matern12, Matern32, Matern52, ZeroKernel
from .model import GPAR, check_gap, check_window, host_index, host_masks, per_output
from .optimise import minimise_l_bfgs_b
from .spectrum import Periodogram, periodogram_grid, periodogram_inputs, spectral_peaks
from .vars import Vars

__all__ = ["GPARRegressor", "Decomposition", "HyperPosterior", "Periodogram", "spectral_peaks", "log_transform", "squishing_transform"]


def _xp(x):
    return torch if isinstance(x, torch.Tensor) else np


#: Log transform for the data: (transform, inverse).
log_transform = (lambda x: _xp(x).log(x), lambda x: _xp(x).exp(x))

#: Squishing transform for the data: sign(x) log(1 + |x|) and its inverse.
squishing_transform = (
    lambda x: _xp(x).sign(x) * _xp(x).log(1 + _xp(x).abs(x)),
    lambda x: _xp(x).sign(x) * (_xp(x).exp(_xp(x).abs(x)) - 1),
)


def _vector_from_init(init, length):
    """Broadcast a scalar initialisation, or take the first `length` entries of a vector one
    (reference regression.py:31-46; known answers tests/test_regression.py:43-49)."""
    if np.size(init) == 1:
        return init * np.ones(length)
    squeezed = np.squeeze(init)
    if np.ndim(squeezed) != 1:
        raise ValueError(f"Incorrect shape {np.shape(init)} of hyperparameters.")
    if np.size(squeezed) < length:
        raise ValueError("Not enough hyperparameters specified.")
    return np.array(squeezed)[:length]


def _determine_indices(m, pi, markov):
    """Columns of the design matrix used by layer `pi`: the m inputs and the last `markov` previous outputs
    (all of them for markov=None).  (reference regression.py:49-59; table tests/test_regression.py:52-83)"""
    p_last = pi - 1
    p_start = 0 if markov is None else max(p_last - (markov - 1), 0)
    p_num = p_last - p_start + 1
    return list(range(m)), list(range(m + p_start, m + p_last + 1)), p_num


def _to_torch(x):
    if x is None or isinstance(x, torch.Tensor):
        return x
    return torch.tensor(np.asarray(x))


def _to_engine(x):
    """A transient input (not kept as an attribute) goes to the engine's device before any arithmetic: element-wise host
    operators on n x p arrays open OpenMP regions whose workers then spin (see _default_weights)."""
    from .engine import get_engine

    return x if x is None else get_engine().tensor(x if isinstance(x, torch.Tensor) else np.asarray(x))


def _uprank(x):
    if x.dim() == 0:
        return x.reshape(1, 1)
    if x.dim() == 1:
        return x[:, None]
    return x


#: `matern=` values of GPARRegressor -> the kernel that stands where the default model has EQ
_MATERN = {0.5: Matern12, 1.5: Matern32, 2.5: Matern52}


def _spectral_periods(spectral, spectral_period):
    """Initial period of each of the `spectral` components: a scalar T gives the harmonics T / (q + 1) - distinct starting points, so that
    the components do not stay copies of one another -, a vector of Q gives component q its entry."""
    if np.size(spectral_period) == 1:
        return [float(np.reshape(spectral_period, -1)[0]) / (q + 1) for q in range(spectral)]
    periods = np.asarray(spectral_period, dtype=np.float64).reshape(-1)
    if periods.size != spectral:
        raise ValueError(f"spectral_period holds {periods.size} periods for spectral={spectral} components")
    return [float(v) for v in periods]


def _layer_kernel_size(config, m, p):
    """(terms, factors, feature dims) of the widest layer kernel the configuration produces for m inputs and p outputs - the last layer,
    which sees the most previous outputs."""
    markov, q = config["markov"], config.get("spectral") or 0
    p_num = max(p - 1, 0) if markov is None else min(max(p - 1, 0), markov)
    per, inlin = bool(config["per"]), bool(config["input_linear"])
    lin, nonlin = bool(config["linear"]) and p_num > 0, bool(config["nonlinear"]) and p_num > 0
    terms = 1 + per + 2 * inlin + lin + nonlin + q
    factors = 1 + 2 * per + inlin + lin + nonlin + 2 * q
    dims = m + 3 * m * per + m * inlin + p_num * lin + p_num * nonlin + 2 * q * m
    return terms, factors, dims


def _check_layer_kernel_size(config, m, p):
    """ValueError if the widest layer kernel does not fit the device's kernel specification (include/gpar_hip.h)."""
    terms, factors, dims = _layer_kernel_size(config, m, p)
    what = f"spectral={config.get('spectral')}" + (f" with {m} inputs and {p} outputs" if m is not None and p > 2 else "")
    if terms > GPAR_MAX_TERMS:
        raise ValueError(f"{what}: the layer kernel would have {terms} terms; the device specification holds GPAR_MAX_TERMS = {GPAR_MAX_TERMS}")
    if factors > GPAR_MAX_FACTORS:
        raise ValueError(f"{what}: the layer kernel would have {factors} factors; the device specification holds GPAR_MAX_FACTORS = {GPAR_MAX_FACTORS}")
    if dims > GPAR_MAX_DIMS:
        raise ValueError(f"{what}: the layer kernel would have {dims} feature dims; the device specification holds GPAR_MAX_DIMS = {GPAR_MAX_DIMS}")


def _model_generator(vs, m, pi, scale, scale_tie, per, per_period, per_scale, per_decay, input_linear,
                     input_linear_scale, linear, linear_scale, nonlinear, nonlinear_scale, rq, markov, noise, matern=None,
                     spectral=None, spectral_period=1.0, spectral_scale=10.0):
    """Constructor of layer `pi`: kernel over the inputs + kernel over the selected previous outputs, and the
    observation-noise variance; hyper-parameters are created in `vs` on first use (reference regression.py:72-182)."""

    config = repr((m, pi, scale, scale_tie, per, per_period, per_scale, per_decay, input_linear, input_linear_scale, linear,
                   linear_scale, nonlinear, nonlinear_scale, rq, markov, noise) + (() if matern is None else (matern,))
                  + (() if spectral is None else (("spectral", spectral, spectral_period, spectral_scale),)))

    def model():
        return vs.memo(config, build)

    def build():
        m_inds, p_inds, p_num = _determine_indices(m, pi, markov)
        k_in, k_out = ZeroKernel(), ZeroKernel()

        def nonlinear_kernel(prefix):
            if matern is not None:   # (same variables as EQ: a Matern kernel has no parameter beyond its scales)
                return _MATERN[matern]()
            return RQ(vs.bnd(name=f"{prefix}/alpha", init=1e-2, lower=1e-3, upper=1e3)) if rq else EQ()

        # nonlinear kernel over the inputs
        var = vs.bnd(name=f"{pi}/input/var", init=1.0)
        scales = vs.bnd(name=f"{0 if scale_tie else pi}/input/scales", init=_vector_from_init(scale, m))
        # (every term is named after the variables it comes from: `GPARRegressor.decompose` reads the names off the compiled term order)
        k_in = k_in + (var * nonlinear_kernel(f"{pi}/input").stretch(scales)).labelled("input/nonlin")

        # locally periodic kernel over the inputs
        if per:
            var = vs.bnd(name=f"{pi}/input/per/var", init=1.0)
            scales = vs.bnd(name=f"{pi}/input/per/scales", init=_vector_from_init(per_scale, 2 * m))
            periods = vs.bnd(name=f"{pi}/input/per/pers", init=_vector_from_init(per_period, m))
            decays = vs.bnd(name=f"{pi}/input/per/decay", init=_vector_from_init(per_decay, m))
            k_in = k_in + (var * EQ().stretch(scales).periodic(periods) * EQ().stretch(decays)).labelled("input/per")

        # spectral mixture over the inputs (Wilson & Adams 2013): Q Gaussian-windowed cosines of a SUM over the inputs, periods learned.
        # The envelope stays EQ under `matern` / `rq` (as the locally periodic term's factors do); `scale_tie` does not tie these.
        if spectral is not None:
            for q, period in enumerate(_spectral_periods(spectral, spectral_period)):
                var = vs.bnd(name=f"{pi}/input/sm{q}/var", init=1.0 / spectral)
                scales = vs.bnd(name=f"{pi}/input/sm{q}/scales", init=_vector_from_init(spectral_scale, m))
                periods = vs.bnd(name=f"{pi}/input/sm{q}/pers", init=_vector_from_init(period, m))
                k_in = k_in + (var * EQ().stretch(scales) * Cosine().stretch(periods)).labelled(f"input/sm{q}")

        # linear kernel (plus constant) over the inputs
        if input_linear:
            scales = vs.bnd(name=f"{pi}/input/lin/scales", init=_vector_from_init(input_linear_scale, m))
            const = vs.get(name=f"{pi}/input/lin/const", init=1.0)
            k_in = k_in + (Linear().stretch(scales).labelled("input/lin") + (ZeroKernel() + const).labelled("input/const"))

        # linear dependencies on the previous outputs
        if linear and pi > 0:
            scales = vs.bnd(name=f"{pi}/output/lin/scales", init=_vector_from_init(linear_scale, p_num))
            k_out = k_out + Linear().stretch(scales).labelled("output/lin")

        # nonlinear dependencies on the previous outputs
        if nonlinear and pi > 0:
            var = vs.bnd(name=f"{pi}/output/nonlin/var", init=1.0)
            scales = vs.bnd(name=f"{pi}/output/nonlin/scales", init=_vector_from_init(nonlinear_scale, p_num))
            k_out = k_out + (var * nonlinear_kernel(f"{pi}/output/nonlin").stretch(scales)).labelled("output/nonlin")

        noise_variance = vs.bnd(name=f"{pi}/noise", init=_vector_from_init(noise, pi + 1)[pi], lower=1e-8)
        f = GP(k_in.select(m_inds) + k_out.select(p_inds), measure=Measure())
        return f, noise_variance

    return model


#: What `GPARRegressor.decompose` returns: per output a tuple of component names, a G_i x n* array of means, one of variances (or None
#: for `var`), and the p normalisation shifts.
Decomposition = collections.namedtuple("Decomposition", "names mean var offset")

# What `laplace` returns: `names` the trained variables layer by layer, `value` / `stderr` one array per name in natural units, `cov` the
# P x P covariance in the optimiser's unconstrained coordinates (block diagonal over layers), `flat` the dropped directions per layer;
# `slices` (per name) and `layers` (per layer) locate them among the P coordinates.
HyperPosterior = collections.namedtuple("HyperPosterior", "names value stderr cov flat slices layers")

FLAT_RELATIVE = 1e-10   # eigenvalues of a layer's Hessian at or below this fraction of the largest (or <= 0) are flat directions


def laplace_block(H, relative=FLAT_RELATIVE):
    """(Sigma, flat, support) of one layer from the Hessian H of its negative log marginal likelihood: the pseudo-inverse over the
    eigen-directions with eigenvalue > max(relative * lambda_max, 0) - the others are FLAT (not at a mode, or pinned at a bound), are left
    out and counted in `flat`; `support[i]` = the squared length of coordinate i within the kept directions (0: the variable lies wholly
    in flat directions and has no finite standard error)."""
    H = np.asarray(H, dtype=np.float64)
    if H.size == 0:
        return np.zeros((0, 0)), 0, np.zeros(0)
    lam, V = np.linalg.eigh(0.5 * (H + H.T))
    keep = lam > max(relative * lam.max(), 0.0)
    Vk = V[:, keep]
    return (Vk / lam[keep]) @ Vk.T, int((~keep).sum()), (Vk ** 2).sum(axis=1)


def block_diagonal(blocks):
    """The blocks on the diagonal of one matrix, in order."""
    sizes = [int(b.shape[0]) for b in blocks]
    out = np.zeros((sum(sizes), sum(sizes)))
    at = 0
    for b, s in zip(blocks, sizes):
        out[at:at + s, at:at + s] = b
        at += s
    return out


def _group_terms(labels, components):
    """(names, comp) of one layer whose kernel terms are named `labels`: the names of its components and, per term, the index of its
    component among them (-1: none).  `components` None: one component per term; a dict {name: patterns}: a term belongs to the
    component one of whose patterns its name matches (`fnmatch`, case-sensitive), to none where no pattern does - two components
    matching one term is a ValueError -, and a component without a term here is not among the names."""
    if components is None:
        return tuple(labels), list(range(len(labels)))
    owner = []
    for label in labels:
        hits = [name for name, patterns in components.items()
                if any(fnmatch.fnmatchcase(str(label), pat) for pat in ([patterns] if isinstance(patterns, str) else patterns))]
        if len(hits) > 1:
            raise ValueError(f"kernel term {label!r} is matched by the components {hits}: a term belongs to one component")
        owner.append(hits[0] if hits else None)
    names = tuple(name for name in components if name in owner)
    return names, [names.index(o) if o is not None else -1 for o in owner]


def update_drop_fraction():
    """`GPARRegressor.update` forgets up to this fraction of its rows by a rank-k update of the layers' factors and conditions again
    above it (GPAR_UPDATE_DROP_FRACTION, read at every call).  By flop count the update costs ~3 k n^2 vector flops against n^3 / 3 on
    the matrix cores, which predicts a crossover near k = n / 16.  MEASURED (tools/time_update.py, profiles/update_times.txt) the
    update loses at every size tried, k = 1 included - n = 1024 / 4096 / 16384, one row forgotten and one appended, then `predict`:
    2.5 / 8.8 / 38.3 ms against 1.2 / 3.6 / 35.0 ms for conditioning again - because its diagonal kernel is a chain of n k dependent
    sqrt / divide steps on one wave.  So the default is 0: rows are only forgotten by conditioning again (the kept factors still
    spare `predict` its own conditioning), rows are appended incrementally, and the rank-k route is opt-in through this switch."""
    return float(os.environ.get("GPAR_UPDATE_DROP_FRACTION", "0"))


def layer_config(reg, m, pi):
    """The keywords `_model_generator` builds layer `pi` of `reg` from: the regressor's `model_config`, and where periods were picked from
    a periodogram (`spectral_period="auto"`, `init_spectral`) the layer's own Q of them as its `spectral_period` - given where a user
    would have given them, so names, bounds, every other initial value and the rule that an existing variable is not overwritten are
    the constructor's."""
    config = reg.model_config
    picked = getattr(reg, "_spectral_auto", None)   # p x Q
    if picked is None:
        if config.get("spectral_period") == "auto":
            raise RuntimeError('spectral_period="auto" takes the initial periods from data: call fit, condition or init_spectral first')
        return config
    if m != 1 or pi >= picked.shape[0]:
        raise ValueError(f"the spectral periods were picked for one input and {picked.shape[0]} outputs; this model has {m} inputs and a layer {pi}")
    return {**config, "spectral_period": tuple(float(v) for v in picked[pi])}


def _construct_gpar(reg, vs, m, p):
    x_ind = reg.x_ind
    if x_ind is not None and getattr(reg, "_x_ind_trainable", False):
        # inducing inputs as a variable of the store (an addition: the reference keeps them fixed, todo.tasks:5)
        x_ind = vs.get(init=np.asarray(x_ind, dtype=np.float64), name="x_ind")
    gpar = GPAR(replace=reg.replace, impute=reg.impute, x_ind=x_ind, sparse_method=reg.sparse_method)
    if reg.model_config.get("spectral") is not None:   # (the feature dims grow with m and p, which the constructor did not know)
        _check_layer_kernel_size(reg.model_config, m, p)
    for pi in range(p):
        gpar = gpar.add_layer(_model_generator(vs, m, pi, **layer_config(reg, m, pi)))
    return gpar


def _default_weights(rows, cols):
    """The reference's default, a matrix of ones - made where it is used.  (A CPU `torch.ones` of 32768 elements or more
    opens an OpenMP parallel region; its worker threads - one per host core - then spin, and in a container with a CPU
    quota that throttles the process for tens of milliseconds: seen as one 60 ms evaluation in three at C4.)"""
    from .engine import get_engine

    return torch.ones(rows, cols, dtype=torch.float64, device=get_engine().device)


def _init_weights(w, y, attribute=False):
    if w is None:
        # (`condition` keeps the reference's attribute: a host tensor, made once)
        return torch.from_numpy(np.ones(tuple(y.shape), dtype=np.float64)) if attribute else _default_weights(*y.shape)
    return _uprank(_to_torch(w))


def _run_on_streams(eng, streams, shares, fn, on_exit=None):
    """fn(item) for every item of shares[k] on stream k, one host thread per stream; exceptions re-raised here.  `on_exit(k)`: called
    by thread k when it is done with its share, whatever happened (a lane of a lock-step rendezvous leaves it there)."""
    import threading

    main = torch.cuda.current_stream(eng.device)
    errors = []

    def work(k, stream, items):
        try:
            with torch.cuda.device(eng.device), torch.cuda.stream(stream):
                try:
                    for item in items:
                        fn(item)
                finally:
                    if on_exit is not None:
                        on_exit(k)
        except BaseException as exc:  # noqa: BLE001 - handed to the caller's thread
            errors.append(exc)

    threads = []
    for k, (stream, items) in enumerate(zip(streams, shares)):
        stream.wait_stream(main)
        threads.append(threading.Thread(target=work, args=(k, stream, items), daemon=True))
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for stream in streams:
        main.wait_stream(stream)
    if errors:
        raise errors[0]


def _check_horizon(horizon, start, n):
    """`horizon` (an int >= 1, or a non-empty list, tuple or 1-D integer array of distinct ints >= 1: several horizons scored in one pass,
    returned as a tuple) and `start` (an int in 0 ... n - 1) of `ahead` / `fit(objective="ahead")`."""
    several = isinstance(horizon, (list, tuple, np.ndarray))
    if several:
        if np.ndim(horizon) != 1 or len(horizon) == 0:
            raise ValueError("horizon must be an integer or a non-empty sequence of integers")
        if len(set(horizon)) != len(horizon):
            raise ValueError(f"horizon={tuple(horizon)}: the horizons must be distinct")
    for name, v in [("horizon", h) for h in (horizon if several else (horizon,))] + [("start", start)]:
        if not isinstance(v, (int, np.integer)) or isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{name} must be an integer")
    for h in horizon if several else (horizon,):
        if h < 1:
            raise ValueError(f"horizon={h}: forecasts look at least one row ahead")
    if not 0 <= start <= max(n - 1, 0):
        raise ValueError(f"start={start}: the first scored row must lie in 0 ... {max(n - 1, 0)}")
    return (tuple(int(h) for h in horizon) if several else int(horizon)), int(start)


def _check_horizon_weights(horizon_weights, horizon):
    """`horizon_weights` of `ahead` / `fit(objective="ahead")` for the checked `horizon`: None, or one positive finite number per horizon of
    a sequence (returned as a float64 array)."""
    if horizon_weights is None:
        return None
    if not isinstance(horizon, tuple):
        raise ValueError("horizon_weights belong to a sequence of horizons: one horizon has nothing to weigh against")
    from .hip import horizon_weight_array

    return horizon_weight_array(horizon_weights, len(horizon))


def _check_window(window, horizon, horizon_weights=None):
    """`window` of `ahead` / `fit(objective="ahead")` (None: the expanding origin): an int >= 1, beside ONE horizon."""
    if window is None:
        return None
    window = check_window(window)
    if isinstance(horizon, (list, tuple, np.ndarray)) or horizon_weights is not None:
        raise ValueError("window takes one horizon, not a sequence of horizons: the multi-horizon pass shares one factorisation of all rows, "
                         "which the windowed score never forms")
    return window


def _check_objective(objective, sparse, fix, folds=None, horizon=None, start=None, score="log", gap=None, horizon_weights=None, window=None):
    """The training objectives `fit` knows, and what the held-out ones need."""
    if objective not in ("mll", "loo", "cv", "ahead"):
        raise ValueError('objective must be "mll", "loo", "cv" or "ahead"')
    check_score(score)
    if score != "log" and objective in ("mll", "cv"):
        raise ValueError(f'score="{score}" belongs to objective="loo" or "ahead": '
                         + ("the marginal likelihood is a joint density of all rows" if objective == "mll" else "a fold is scored by its joint density")
                         + ", which has no per-row scoring rule")
    if objective != "ahead" and (horizon is not None or start is not None):
        raise ValueError('horizon and start belong to objective="ahead"')
    if objective != "ahead" and horizon_weights is not None:
        raise ValueError('horizon_weights belong to objective="ahead"')
    if window is not None:
        if objective != "ahead":
            raise ValueError('window belongs to objective="ahead"')
        _check_window(window, horizon, horizon_weights)
    if objective == "cv" and folds is None:
        raise ValueError('objective="cv" needs folds: a number of contiguous blocks or one integer label per row')
    if objective != "cv" and folds is not None:
        raise ValueError('folds belong to objective="cv"')
    if gap is not None:
        check_gap(gap)
        if objective != "cv":
            raise ValueError('gap belongs to objective="cv"')
    if objective != "mll" and sparse:
        raise ValueError(f'objective="{objective}" needs dense layers: not available with inducing points (x_ind)')
    if objective != "mll" and not fix:
        raise NotImplementedError(f'objective="{objective}" trains layers with fixed inputs (fix=True) only')


def _check_purge(gap, labels):
    """`gap` of `cv` / `fit(objective="cv")` (None: 0) against the fold labels: purged rows need every fold to be one run of rows."""
    gap = 0 if gap is None else check_gap(gap)
    if gap and np.any(np.diff(labels) < 0):
        raise ValueError("gap > 0 needs fold labels that do not decrease along the rows: a gap in time has no meaning for scattered folds")
    return gap


def _fold_labels(folds, n):
    """`folds` of `cv` / `fit(objective="cv")` as one integer label per row: an int k stands for k contiguous blocks of the rows as
    given, split as `np.array_split` splits them; a 1-D integer array of n labels is taken as it is."""
    if isinstance(folds, (int, np.integer)) and not isinstance(folds, bool):
        k = int(folds)
        if not 1 <= k <= n:
            raise ValueError(f"folds={k}: the number of blocks must lie between 1 and the number of rows ({n})")
        return np.concatenate([np.full(len(part), j, dtype=np.int64) for j, part in enumerate(np.array_split(np.arange(n), k))])
    labels = np.asarray(folds.cpu() if isinstance(folds, torch.Tensor) else folds)
    if labels.ndim != 1 or labels.size != n or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError(f"folds must be a number of blocks or a 1-D array of {n} integer labels, one per row")
    return labels.astype(np.int64)


def _surviving_rows(items, pi, n):
    """The rows of the conditioned data that reach layer `pi`: those the masks of the earlier layers (`model.per_output`) keep."""
    rows = np.arange(n)
    for _, _, mask in items[:pi]:
        rows = rows[host_index(mask)]
    return rows


class GPARRegressor:
    """GPAR regressor.  See the reference docstring (regression.py:200-262) for the meaning of every keyword;
    signature and defaults are identical."""

    #: `fit(fix=True)` trains dense layers through the prepared objective of gpar_amd/fastfit.py (same device launches, no
    #: autograd, no per-evaluation model objects); False keeps the general route for every layer (tests compare the two).
    fast_fit = True

    #: `logpdf` on device-resident outputs remembers their NaN pattern ON THE CALLER'S TENSOR (attribute `_gpar_nan`, with the tensor's
    #: version counter) so that a loop over the same outputs pays the device-to-host synchronisation once.  Writes torch cannot see
    #: - a raw-pointer kernel, another library, `.data` writes, a DLPack alias - do not move the counter: after one, `del y._gpar_nan`,
    #: or set this attribute False (per regressor, or on the class) and the pattern is read from the device at every call.
    nan_pattern_cache = True

    def __init__(self, replace=False, impute=True, scale=1.0, scale_tie=False, per=False, per_period=1.0,
                 per_scale=1.0, per_decay=10.0, input_linear=False, input_linear_scale=100.0, linear=True,
                 linear_scale=100.0, nonlinear=False, nonlinear_scale=1.0, rq=False, markov=None, noise=0.1,
                 x_ind=None, normalise_y=True, transform_y=(lambda x: x, lambda x: x), sparse_method="vfe", matern=None, spectral=None,
                 spectral_period=1.0, spectral_scale=10.0):
        self.replace = replace
        if sparse_method not in ("vfe", "fitc", "dtc"):
            raise ValueError('sparse_method must be "vfe", "fitc" or "dtc"')
        self.sparse_method = sparse_method  # an addition behind the reference's keywords: "vfe" | "fitc" | "dtc"
        self.impute = impute
        self.sparse = x_ind is not None
        self.x_ind = None if x_ind is None else _uprank(_to_torch(x_ind))
        self.model_config = {
            "scale": scale, "scale_tie": scale_tie, "per": per, "per_period": per_period, "per_scale": per_scale,
            "per_decay": per_decay, "input_linear": input_linear, "input_linear_scale": input_linear_scale,
            "linear": linear, "linear_scale": linear_scale, "nonlinear": nonlinear,
            "nonlinear_scale": nonlinear_scale, "rq": rq, "markov": markov, "noise": noise,
        }
        # an addition behind the reference's keywords: `matern` = 0.5 | 1.5 | 2.5 puts the Matern kernel of that smoothness where the
        # default model has EQ (the nonlinear input and output kernels; the locally periodic term keeps its EQ factors, as under rq)
        if matern is not None:
            if isinstance(matern, bool) or not isinstance(matern, (int, float, np.floating, np.integer)) or float(matern) not in _MATERN:
                raise ValueError("matern must be None, 0.5, 1.5 or 2.5")
            if rq:
                raise ValueError("matern and rq=True exclude one another")
            self.model_config["matern"] = float(matern)
        self.matern = None if matern is None else float(matern)
        # an addition as well: `spectral` = Q >= 1 adds, to every layer's kernel over the inputs, the spectral mixture
        # sum_q var_q EQ().stretch(l_q) * Cosine().stretch(T_q) - oscillating components whose periods are learned (`spectral_period`: a scalar
        # T starts them at the harmonics T / (q + 1), a vector of Q gives each its own; `spectral_scale`: the envelopes' length scales)
        if spectral is not None:
            if isinstance(spectral, (bool, np.bool_)) or not isinstance(spectral, (int, np.integer)) or spectral < 1:
                raise ValueError("spectral must be None or an integer >= 1 (the number of spectral-mixture components)")
            spectral = int(spectral)
            if isinstance(spectral_period, str):
                # "auto": the periods are picked from the generalised Lomb-Scargle periodogram of the data the model is first built on
                # (`init_spectral`; Wilson & Adams 2013 initialise from the empirical spectrum) - one input column, the device engine
                if spectral_period != "auto":
                    raise ValueError(f'spectral_period={spectral_period!r}: a number, {spectral} numbers or "auto"')
            else:
                spectral_period = float(spectral_period) if np.ndim(spectral_period) == 0 else tuple(float(v) for v in np.reshape(spectral_period, -1))
            spectral_scale = float(spectral_scale) if np.ndim(spectral_scale) == 0 else tuple(float(v) for v in np.reshape(spectral_scale, -1))
            if spectral_period != "auto":
                _spectral_periods(spectral, spectral_period)
            self.model_config.update(spectral=spectral, spectral_period=spectral_period, spectral_scale=spectral_scale)
            # terms and factors of the widest layer (one with previous outputs) are known now; its feature dims once m and p are
            _check_layer_kernel_size(self.model_config, 1, 2)
        elif isinstance(spectral_period, str):
            raise ValueError(f"spectral_period={spectral_period!r} belongs to spectral=Q")
        self.spectral = spectral
        self._spectral_auto = None   # p x Q periods picked from a periodogram, once there are any
        self.vs = Vars(dtype=torch.float64)
        self.is_conditioned = False
        self.x = self.y = self.w = None
        self.n = self.m = self.p = None
        self.normalise_y = normalise_y
        self._unnormalise_y, self._normalise_y = (lambda x: x), (lambda x: x)
        self._transform_y, self._untransform_y = transform_y
        self._stream_cache = None            # (key, conditioned GPAR) kept by `update`
        self.last_update_incremental_ = None  # did the last `update` take the incremental route?

    def get_variables(self):
        """Dictionary name -> value of every hyper-parameter instantiated so far."""
        return {name: self.vs[name].detach().numpy() for name in self.vs.names}

    def condition(self, x, y, w=None):
        """Store (and transform / normalise) the training data without training (reference regression.py:339-389)."""
        # The attributes are host tensors, as in the reference.  The element-wise passes over them (mask, mean, standard
        # deviation, normalisation) go through numpy, which runs them on the calling thread: a torch CPU operator on 32768 or
        # more elements opens an OpenMP region whose workers (one per core) spin afterwards, which in a container with a CPU
        # quota throttles the evaluations that follow (fit(iters=3) at n = 8192: 0.68 -> 0.60 s) - and changing torch's
        # global thread count around the call instead would be visible to other threads of the process.
        self._stream_cache = None
        self.x = _uprank(_to_torch(x)).detach().cpu()
        self.y = self._transform_y(_uprank(_to_torch(y))).detach().cpu()
        self.w = _init_weights(w, self.y, attribute=True)
        self.n, self.m = self.x.shape
        self.p = self.y.shape[1]
        if self.normalise_y:
            y_np = self.y.detach().cpu().numpy()   # (a device tensor handed to fit / condition comes to the host here)
            means = np.empty((1, self.p), dtype=y_np.dtype)
            stds = np.empty((1, self.p), dtype=y_np.dtype)
            for i in range(self.p):
                y_i = y_np[~np.isnan(y_np[:, i]), i]
                means[0, i] = np.mean(y_i)
                std = np.std(y_i)  # population std, as lab's B.std
                stds[0, i] = std if std > 0 else 1.0
            means_t, stds_t = torch.from_numpy(means), torch.from_numpy(stds)

            def normalise_y(y_):
                return (y_ - means_t.to(y_.device)) / stds_t.to(y_.device)

            def unnormalise_y(y_):
                return y_ * stds_t.to(y_.device) + means_t.to(y_.device)

            self._normalise_y, self._unnormalise_y = normalise_y, unnormalise_y
            self.y = torch.from_numpy((y_np - means) / stds)
        if self.model_config.get("spectral_period") == "auto" and (self._spectral_auto is None or self._spectral_auto.shape[0] < self.p):
            # the first data the model is built on: the periods every layer's components start at (later calls keep them)
            self._spectral_auto = self._pick_periods(self.x.numpy(), self.y.numpy(), self.w.numpy())
        self.is_conditioned = True

    def fit(self, x, y, w=None, greedy=False, fix=True, optimise_x_ind=False, objective="mll", folds=None, horizon=None, start=None,
            score="log", gap=None, horizon_weights=None, window=None, **kw_args):
        """Train layer by layer with L-BFGS-B on the negative log marginal likelihood; keyword arguments go to
        `minimise_l_bfgs_b` (`iters`, `f_calls`, `trace`).  (reference regression.py:391-459)

        `objective` (an addition): "mll", the log marginal likelihood, or "loo", the layer-wise leave-one-out predictive log-density
        (`loo`; Rasmussen & Williams 5.4.2) - more robust where the kernel family is misspecified.  "loo" needs dense layers with
        fixed inputs: ValueError with inducing points, NotImplementedError with `fix=False`.  "cv" is the blocked form for ordered data
        (`cv`): whole folds are held out and scored by their joint predictive density; it needs `folds` (as `cv` takes them), which
        no other objective accepts, and has the restrictions of "loo"; `gap` (an int >= 0, default 0, "cv" alone) purges that many rows
        on either side of a held-out fold from the rows it is predicted from (`cv`), for which the labels must not decrease.  "ahead" is the rolling-origin forecast score (`ahead`): every
        row predicted from the rows at least `horizon` (default 1) rows before it, rows before `start` (default 0) not scored - for
        models whose purpose is the forecast at that horizon; `horizon` / `start` belong to it alone; the restrictions of "loo".
        `horizon` may be a sequence of distinct ints >= 1: the layers are trained on sum_k horizon_weights[k] (the score at horizon k), every
        evaluation scoring all of them from one factorisation (`ahead`); `horizon_weights`: one positive finite number per horizon of
        such a sequence (default all 1) - ValueError with a single horizon or another objective.
        `window` (an int >= 1, "ahead" with ONE horizon alone: ValueError otherwise): the layers are trained on the sliding-window score
        (`ahead(window=)`), every row predicted from the `window` rows before its origin alone - the objective of a model that `update(...,
        drop=k)` keeps on a window of recent rows; no evaluation factors a layer's whole covariance.  None: the expanding origin, untouched.

        `score` (with "loo" and "ahead" alone: ValueError otherwise): the rule each held-out entry is scored by.  "log", the Gaussian
        log density; "crps", minus the continuous ranked probability score - linear in the error where the log score is quadratic over
        the variance, so a few outliers do not buy themselves out through the noise, and still strictly proper; "se", minus the
        squared error (PRESS / the rolling-origin MSE), which ignores the predictive variances altogether.

        `optimise_x_ind` (an addition, off by default; the reference's todo.tasks:5): the inducing inputs `x_ind` become the
        variable "x_ind" of `self.vs` and are trained along with every layer's hyper-parameters (the gradient with respect to
        inducing locations comes from the same device passes as the joint gradient of `fix=False`)."""
        _check_objective(objective, self.sparse, fix, folds, horizon, start, score, gap, horizon_weights, window)
        self.condition(x, y, w)
        if greedy:
            # (as the reference, regression.py:409-410 and its test tests/test_regression.py:241-243; the search itself is
            # `greedy_order` below - an addition, not a change of this call)
            raise NotImplementedError("Greedy search is not implemented yet.")
        if optimise_x_ind and not self.sparse:
            raise ValueError("optimise_x_ind needs inducing points (x_ind)")
        self._train(range(self.p), fix, optimise_x_ind, objective=objective, folds=folds, horizon=horizon, start=start, score=score,
                    **({} if gap is None else {"gap": gap}), **({} if horizon_weights is None else {"horizon_weights": horizon_weights}),
                    **({} if window is None else {"window": window}), **kw_args)

    def _train(self, layers, fix=True, optimise_x_ind=False, concurrent=True, objective="mll", folds=None, horizon=None, start=None, score="log",
               gap=None, horizon_weights=None, window=None, **kw_args):
        """Train the given layers of the conditioned model, one after the other (or, where they do not feed one another, on the
        engine's worker streams); returns {layer: final value of its objective}."""
        _check_objective(objective, self.sparse, fix, folds, horizon, start, score, gap, horizon_weights, window)
        loo, cv, ahead = objective == "loo", objective == "cv", objective == "ahead"
        labels = _fold_labels(folds, self.n) if cv else None
        gap = _check_purge(gap, labels) if cv else 0   # (0: blocked cross-validation as it was - the calls below are then today's)
        if ahead:
            horizon, start = _check_horizon(1 if horizon is None else horizon, 0 if start is None else start, self.n)
            horizon_weights = _check_horizon_weights(horizon_weights, horizon)
        several = {"weights": horizon_weights} if ahead and isinstance(horizon, tuple) else {}   # (a single horizon: the calls below are today's)
        windowed = {} if window is None else {"window": int(window)}   # (no window: no new argument reaches any call below)
        self._x_ind_trainable = bool(optimise_x_ind) or getattr(self, "_x_ind_trainable", False)
        layers = list(layers)
        finals = {}
        eng = get_engine()
        x_dev, y_dev, w_dev = eng.tensor(self.x), eng.tensor(self.y), eng.tensor(self.w)
        if host_masks():
            # self.y is a host tensor (condition): its NaN pattern costs nothing here, and per_output then plans the masks on the
            # host - index tensors, no synchronisation per layer and evaluation (on any engine: the CPU tests walk the same route)
            if y_dev is self.y:
                y_dev = y_dev.view(y_dev.shape)   # (never hang the plan on the regressor's own attribute)
            y_dev._host_nan, y_dev._host_nan_version = torch.isnan(self.y).numpy(), y_dev._version
        y_cached = {k: list(per_output(y_dev, w_dev, keep=k)) for k in [True, False]}
        self._prepare_kernels(self.m, self.p, self.n, training=True, inputs=not fix or bool(optimise_x_ind))

        def train_layer(pi, group=None, lane=None):
            if fix:
                gpar = _construct_gpar(self, self.vs, self.m, pi + 1)
                fixed_x, fixed_x_ind = gpar.logpdf(
                    x_dev, y_cached, None, only_last_layer=True, outputs=list(range(pi)), return_inputs=True
                )
            # (the fold labels of the rows that reach this layer: earlier layers' masks have dropped the others from fixed_x)
            layer_labels = labels[_surviving_rows(y_cached[bool(self.impute)], pi, self.n)] if cv else None
            # (rolling origins count rows of the data as given: the indices there of the rows that reach this layer)
            layer_rows = _surviving_rows(y_cached[bool(self.impute)], pi, self.n) if ahead or gap else None

            def neg_value(vs):
                gpar = _construct_gpar(self, vs, self.m, pi + 1)
                if fix:
                    x_ind_pi = fixed_x_ind
                    if optimise_x_ind:  # the m base columns are the variable; the columns appended by earlier layers stay fixed
                        x_ind_pi = torch.cat([eng.tensor(vs["x_ind"]), fixed_x_ind[:, self.m :]], dim=1)
                    if loo:
                        return -gpar.loo(fixed_x, y_cached, None, outputs=[pi], score=score)[0]
                    if cv and gap:   # (a gap counts rows of the data as given, as a horizon does: the labels of all rows, and which reach this layer)
                        return -gpar.cv(fixed_x, y_cached, None, labels, outputs=[pi], gap=gap, rows=layer_rows)[0]
                    if cv:
                        return -gpar.cv(fixed_x, y_cached, None, layer_labels, outputs=[pi])[0]
                    if ahead:
                        return -gpar.ahead(fixed_x, y_cached, None, horizon, start, outputs=[pi], rows=layer_rows, score=score, **several, **windowed)[0]
                    return -gpar.logpdf(fixed_x, y_cached, None, only_last_layer=True, outputs=[pi], x_ind=x_ind_pi)
                return -gpar.logpdf(x_dev, y_cached, None, only_last_layer=False)

            names = [f"{pi}/*"] if fix else [f"{i}/*" for i in range(pi + 1)]
            if optimise_x_ind:
                names = names + ["x_ind"]
            fast = None
            if fix and not optimise_x_ind and self.fast_fit:
                # a dense layer with fixed inputs: the objective prepared once, an evaluation = one library call + the chain rule
                # in numpy (gpar_amd/fastfit.py); None where that route does not apply
                from . import fastfit
                from .optimise import objective_and_gradient

                general = []

                def general_fg(x):   # (a failed factorisation goes through the general route's evaluation: unfused retry, NaN)
                    if not general:
                        general.append(objective_and_gradient(neg_value, self.vs, names, trace=kw_args.get("trace", False))[0])
                    return general[0](x)

                fast = fastfit.build(self, eng, self.vs, pi, names, fixed_x, y_cached[bool(self.impute)][pi], general_fg=general_fg,
                                     group=group, lane=lane, objective=objective, **({"folds": layer_labels} if cv and not gap else {}),
                                     **({"folds": labels, "purge": (gap, layer_rows)} if gap else {}),
                                     **({"ahead": (horizon, start, layer_rows, *several.values())} if ahead else {}), **({} if score == "log" else {"score": score}),
                                     **windowed)
            if group is not None and (fast is None or fast.group is None):
                group.leave(lane)   # (this lane trains through the general route from here on: the others must not wait for it)
            if fast is not None:
                finals[pi] = fast.minimise(**kw_args)
            else:
                finals[pi] = minimise_l_bfgs_b(neg_value, self.vs, names=names, **kw_args)
            if optimise_x_ind and "x_ind" in self.vs:
                self.x_ind = self.vs["x_ind"].detach().clone()

        from .parallel import layers_train_independently

        depth, prepared = None, False
        if fix and not optimise_x_ind and self.fast_fit and not self.sparse:
            from .gp import one_call_grad_rows

            prepared = 0 < self.n <= one_call_grad_rows()   # every layer goes through the prepared objective (fastfit.py)
            if prepared and os.environ.get("GPAR_FIT_THREADS") is None:
                # the prepared objective leaves ~0.1 ms of interpreter time per evaluation: four drivers no longer contend for it
                # (fit(iters=20), four layers, 2 -> 4 threads: n = 100 21 -> 15 ms, 400 35 -> 29, 1024 43 -> 30; profiles/r06_small_fit.txt)
                depth = 4
        streams = eng.worker_streams(depth=depth, rows=self.n) if hasattr(eng, "worker_streams") else []
        if concurrent and fix and len(layers) > 1 and len(streams) > 1 and layers_train_independently(self, y_dev):
            # Layers whose inputs are data and whose hyper-parameters are their own train independently of one another:
            # two host threads, each on its own stream, keep two L-BFGS-B drivers in flight so that one layer's
            # latency-bound stretches (panel chains, host-side optimiser steps) run under the other's GEMMs.  The result
            # is the serial one: every evaluation is the same deterministic device computation.
            with torch.no_grad():  # lazily created variables must all exist before the store is shared between threads
                _construct_gpar(self, self.vs, self.m, self.p).logpdf(x_dev[:2], y_dev[:2], w_dev[:2])
            lanes = min(len(streams), len(layers))
            shares = [layers[k::lanes] for k in range(lanes)]
            group = None
            if prepared and not loo and not cv and not ahead and lanes > 1 and all(isinstance(item[2], slice) for item in y_cached[bool(self.impute)]):
                # every layer goes through the prepared objective on the same number of rows: from ~1000 rows on their
                # factorisations are taken in lock-step, one gpar_potrf_batch per round of evaluations (fastfit.LockstepFactor)
                from . import fastfit

                lo, hi = fastfit.lockstep_rows()
                if lo <= self.n <= hi and hasattr(eng, "_grads_from_moments"):
                    group = fastfit.LockstepFactor(eng, self.n, lanes)
            if group is None:
                _run_on_streams(eng, streams[:lanes], shares, train_layer)
            else:
                tagged = [[(pi, k) for pi in share] for k, share in enumerate(shares)]
                _run_on_streams(eng, streams[:lanes], tagged, lambda item: train_layer(item[0], group, item[1]), on_exit=group.leave)
                self._lockstep_rounds = (group.rounds, group.batches)
        else:
            for pi in layers:
                train_layer(pi)
        return finals

    def greedy_order(self, x, y, w=None, **kw_args):
        """Greedy search for the ORDER of the outputs - the reference's open item (regression.py:400 `greedy`, :409-410
        NotImplementedError, todo.tasks:8; Requeima et al. 2019, section 5: "greedily select the output that maximises the
        log marginal likelihood conditioned on the already selected ones") as an ADDITION: `fit(greedy=True)` keeps raising.

        Position by position: every remaining output is trained as the next layer - inputs x and the outputs chosen so far,
        exactly the layer `fit(fix=True)` would train there, same initial values, same L-BFGS-B keyword arguments (`iters`,
        `f_calls`, `trace`) - and the one with the largest trained log marginal likelihood of that layer is kept.  That is
        p (p + 1) / 2 layer fits; the candidates of a position are independent of one another and are trained concurrently on the
        engine's worker streams where layers do not feed one another (complete data, no `replace`, no inducing points).

        Returns (order, values): `order[i]` is the column of y placed at position i, `values[i]` the log marginal likelihood of
        that layer after training (of the normalised outputs, as `fit` sees them).  With `objective="loo"` among the keyword arguments
        the candidates are trained on, and ranked by, the layer's leave-one-out value instead (`fit`); with `objective="cv", folds=...` by its
        blocked cross-validation value; with `objective="ahead", horizon=...` by its rolling-origin forecast score; `score="crps"` / `"se"`
        beside "loo" or "ahead" trains on and ranks by that rule's value (`fit`; `values` are to be maximised under every rule).  The trained hyper-parameters of the chosen
        chain are kept in `self.greedy_vs_` (layer i there belongs to output `order[i]`): `reg.vs = reg.greedy_vs_.copy();
        reg.fit(x, y[:, order], ...)` continues from them.  `self` is conditioned on (x, y, w) in the GIVEN order, as after
        `condition`."""
        from .vars import Vars

        if self.model_config.get("spectral_period") == "auto":
            raise ValueError('spectral_period="auto" picks layer i\'s periods from output i\'s periodogram, and greedy_order decides which '
                             "output layer i models: pick the periods yourself (periodogram, spectral_peaks) and pass spectral_period=(...)")
        self.condition(x, y, w)
        eng = get_engine()
        x_host, y_host, w_host = self.x, self.y, self.w
        order, values, remaining = [], [], list(range(self.p))
        chain_vs = Vars(dtype=torch.float64)
        config = dict(self.model_config)
        streams = eng.worker_streams(rows=self.n) if hasattr(eng, "worker_streams") else []
        independent = not self.replace and not self.sparse and not bool(torch.isnan(y_host).any())
        for k in range(self.p):
            results = {}

            def trial(c):
                cols = order + [c]
                reg = GPARRegressor(replace=self.replace, impute=self.impute, x_ind=self.x_ind, normalise_y=False,
                                    sparse_method=self.sparse_method, **config)
                reg.vs = chain_vs.copy(detach=True)
                reg.condition(x_host, y_host[:, cols], w_host[:, cols])
                final = reg._train([k], fix=True, concurrent=False, **kw_args)[k]
                results[c] = (-float(final), reg.vs)

            if independent and len(streams) > 1 and len(remaining) > 1:
                lanes = min(len(streams), len(remaining))
                _run_on_streams(eng, streams[:lanes], [remaining[j::lanes] for j in range(lanes)], trial)
            else:
                for c in remaining:
                    trial(c)
            # (ties - identical columns - go to the lower column index: the order of `remaining`; a trial whose optimisation ended on
            # a failed evaluation carries NaN, which would make the comparisons order-dependent: it ranks below every finite value)
            def rank(c):
                value = results[c][0]
                return (value if np.isfinite(value) else -np.inf, -c)

            if not any(np.isfinite(results[c][0]) for c in remaining):
                raise ArithmeticError(f"greedy_order: every candidate for position {k} ended on a failed evaluation")
            best = max(remaining, key=rank)
            order.append(best)
            values.append(results[best][0])
            chain_vs = results[best][1]
            remaining.remove(best)
        self.greedy_vs_ = chain_vs
        self.greedy_order_ = list(order)
        return order, values

    def select_inducing(self, x, num, tol=0.0, assign=False):
        """Greedy selection of inducing points among the rows of x (n x m) - an addition; the reference's constructor takes an array and
        nothing else.  The rows are picked by largest conditional variance under the first layer's kernel over the inputs, as the
        model builds it for output 0 at the current values of `self.vs` (variables that do not exist yet are created with their
        usual names, initial values and bounds, as `fit` would create them; after `fit`: the trained length scales): a partially
        pivoted Cholesky factorisation of k(x, x) (`gp.greedy_inducing`), O(n num^2) and deterministic.  It stops before `num` rows
        when the residual trace tr(K - K_xz K_zz^-1 K_zx) - what the VFE bound penalises - has fallen to `tol` times tr K, or when no
        remaining row has a conditional variance above the engine's jitter.
        Returns numpy arrays (x_ind, index, trace): the rank <= num selected rows of x in selection order, their row indices, and the
        residual trace before each step and after the last (rank + 1 values).  `assign=True` installs the rows as `self.x_ind` and
        makes the regressor sparse, as the constructor would have, dropping any conditioned state; otherwise nothing changes."""
        x_np = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)
        if x_np.ndim < 2:
            x_np = x_np.reshape(-1, 1)
        n, m = x_np.shape
        num = int(num)
        if num < 1 or num > n:
            raise ValueError(f"num={num}: between 1 and the number of rows ({n}) inducing points can be selected")
        if self.m is not None and m != self.m:
            raise ValueError(f"x has {m} columns, the model has {self.m} inputs")
        eng = get_engine()
        with torch.no_grad():
            kernel = _model_generator(self.vs, m, 0, **layer_config(self, m, 0))()[0].kernel
            with eng.defer_checks():
                _, piv, trace, rank = greedy_inducing(eng, eng.compile(kernel, m), eng.tensor(x_np), num, tol=tol)
        rank = int(rank.item())
        index = piv[:rank].cpu().numpy().astype(np.int64)
        x_ind = x_np[index]
        if assign:
            self.x_ind = _uprank(_to_torch(x_ind.copy()))
            self.sparse = True
            # (inducing inputs trained earlier - fit(optimise_x_ind=True) - live on as the variable "x_ind", which the model would
            # prefer to the attribute: the constructor's state has neither the variable nor the flag)
            self._x_ind_trainable = False
            if "x_ind" in self.vs:
                self.vs.remove("x_ind")
            self.is_conditioned = False
            self._stream_cache = None
            self.x = self.y = self.w = None
            self.n = self.m = self.p = None
            self._unnormalise_y, self._normalise_y = (lambda x: x), (lambda x: x)
        return x_ind, index, trace[: rank + 1].cpu().numpy()

    # ---- streaming conditioning ------------------------------------------------------------------------
    def _stream_key(self):
        """What the kept factors are a function of, besides the data: the store, its variables' names and a COPY of their values, and
        the inducing inputs."""
        names = self.vs.names
        return self.vs, tuple(names), self.vs.get_vector(names).copy(), (None if self.x_ind is None else self.x_ind.detach().clone())

    def _stream_posterior(self):
        """The conditioned model `update` keeps, if it still belongs to the current hyper-parameters and inducing inputs; otherwise the
        cache is dropped and None returned (the caller conditions as if `update` had never been called)."""
        cache = self._stream_cache
        if cache is None:
            return None
        (vs, names, vector, x_ind), gpar = cache
        now = self._stream_key()
        same = (vs is now[0] and names == now[1] and np.array_equal(vector, now[2])
                and ((x_ind is None and now[3] is None) or (x_ind is not None and now[3] is not None and x_ind.shape == now[3].shape
                                                            and torch.equal(x_ind, now[3]))))
        if not same:
            self._stream_cache = None
            return None
        return gpar

    def update(self, x_new=None, y_new=None, w=None, drop=0):
        """Move the window of data a conditioned regressor holds - an addition; the reference conditions again (regression.py:339-389).
        Forget the `drop` leading rows and append the rows (x_new, y_new, w): afterwards the regressor is exactly what
        `condition(concat(x[drop:], x_new), concat(y[drop:], y_new), concat(w[drop:], w))` would make it, EXCEPT that the output
        normalisation constants of the last `condition` / `fit` are kept: the new outputs are normalised with the means and standard
        deviations computed then (a stream must not re-standardise under a trained model).  `self.x / y / w / n` are updated.

        The first `update` conditions every layer once in the ordinary way and keeps the p conditioned layers - p factors of n^2
        doubles, held until the next `fit`, `condition`, `select_inducing(assign=True)` or change of a hyper-parameter.  `predict`,
        `sample(posterior=True)`, `predict_moments` and `logpdf(posterior=True)` use them instead of conditioning again, and later
        updates move them incrementally: per layer a rank-`drop` Cholesky update and a bordered extension by the new rows, O((drop + k)
        n^2) instead of the O(n^3 / 3) of a factorisation.  That route applies where every layer's design matrix is the data's own -
        dense layers, `replace=False`, no NaN among the stored or the new outputs - and while `drop` is at most
        `update_drop_fraction()` of n (0 by default: as measured, forgetting rows is cheaper by conditioning again); anything else is conditioned in full on the new window inside this call (same result, same
        frozen normalisation).  `last_update_incremental_` says which route ran.

        ValueError: `drop` outside 0 .. n, `drop == n` with nothing appended, x_new / y_new / w of the wrong width or without one
        another; RuntimeError: not conditioned."""
        if not self.is_conditioned:
            raise RuntimeError("Must condition or fit model before updating it.")
        drop = int(drop)
        k = 0
        if (x_new is None) != (y_new is None):
            raise ValueError("x_new and y_new come together")
        if x_new is not None:
            x_new = _uprank(_to_torch(x_new)).detach().cpu().to(torch.float64)
            y_new = _uprank(_to_torch(y_new)).detach().cpu().to(torch.float64)
            k = int(x_new.shape[0])
            if x_new.shape[1] != self.m or y_new.shape[1] != self.p or y_new.shape[0] != k:
                raise ValueError(f"x_new must be k x {self.m} and y_new k x {self.p}")
            w_new = _init_weights(w, y_new, attribute=True).detach().cpu().to(torch.float64)
            if tuple(w_new.shape) != tuple(y_new.shape):
                raise ValueError("w must have the shape of y_new")
            y_new = self._normalise_y(self._transform_y(y_new))   # the constants of the last condition / fit
        elif w is not None:
            raise ValueError("w belongs to the appended rows")
        if drop < 0 or drop > self.n or (drop == self.n and k == 0):
            raise ValueError(f"drop={drop}: between 0 and n = {self.n} leading rows can be forgotten, all of them only when rows are appended")
        if drop == 0 and k == 0:
            self.last_update_incremental_ = self._stream_posterior() is not None
            return self
        incremental = (not self.sparse and not self.replace and drop < self.n and drop <= update_drop_fraction() * self.n
                       and drop <= CHOL_UPDATE_MAX_RANK and not bool(torch.isnan(self.y).any())
                       and (k == 0 or not bool(torch.isnan(y_new).any())))
        gpar = None
        if incremental:
            gpar = self._stream_posterior()
            if gpar is None:   # the first update: an ordinary full conditioning on the data held so far
                gpar = _construct_gpar(self, self.vs, self.m, self.p) | (self.x, self.y, self.w)
            gpar = gpar.update(x_new, y_new, w_new if k else None, drop=drop)
        parts = lambda old, new: torch.cat([old[drop:], new], dim=0) if k else old[drop:].clone()
        self.x, self.y, self.w = parts(self.x, x_new), parts(self.y, y_new), parts(self.w, w_new if k else None)
        self.n = int(self.x.shape[0])
        if gpar is None:
            gpar = _construct_gpar(self, self.vs, self.m, self.p) | (self.x, self.y, self.w)
        self._stream_cache = (self._stream_key(), gpar)
        self.last_update_incremental_ = bool(incremental)
        return self

    # ---- periodogram and the initial periods of spectral-mixture layers --------------------------------------------------
    def _periodogram(self, t, y, omega, freq=None, oversample=5, nyquist=1.0):
        """`periodogram` for prepared arrays (`spectrum.periodogram_inputs`): every ValueError first, then the engine."""
        span = float(t.max() - t.min())
        n_obs = int((omega > 0).sum(axis=0).max())
        if freq is None:
            freq = periodogram_grid(span, n_obs, oversample, nyquist)
        else:
            freq = np.asarray(freq, dtype=np.float64).reshape(-1)
            if not span > 0:
                raise ValueError("the time stamps must span a positive range: a periodogram of one instant has no frequencies")
            if freq.size == 0 or not np.all(np.isfinite(freq)) or np.any(freq <= 0):
                raise ValueError("freq must hold positive, finite frequencies (cycles per unit of x)")
        eng = get_engine()
        if not hasattr(eng, "periodogram"):
            raise NotImplementedError(f"{type(eng).__name__} has no periodogram: the generalised Lomb-Scargle periodogram is a device kernel "
                                      "(HipEngine.periodogram, gpar_periodogram) and has no CPU fallback")
        power = eng.periodogram(t, y, omega, freq, t0=float(t.min()))
        return Periodogram(freq, power.cpu().numpy())

    def periodogram(self, x, y, w=None, freq=None, oversample=5, nyquist=1.0):
        """Generalised Lomb-Scargle periodogram (Zechmeister & Kuerster 2009: floating mean, weights) of every output - an addition, and
        where `spectral_period="auto"` takes its periods from.  x: n x 1 or 1-D, in any order (more than one input column: ValueError);
        y: n x p, NaN = missing, taken through `transform_y` as the model sees it (the power is invariant under affine maps of y, so the
        normalisation plays no part); w: the observation weights of `fit`.  Returns `Periodogram(freq, power)`: F frequencies in cycles
        per unit of x and the p x F powers in [0, 1] - the share of the output's weighted variance a sinusoid of that frequency explains;
        exactly 0 for an output with fewer than 3 observed rows or constant values.  `freq`: the frequencies to use, or None for the grid
        k / (oversample span), k = 1, 2, ... up to nyquist n_obs / (2 span), with span = max x - min x and n_obs the observed rows of the
        best-observed output (`spectrum.periodogram_grid`).  ValueError: span = 0, fewer than 3 rows.  One device call
        (`gpar_periodogram`); NotImplementedError on an engine without it."""
        y = np.asarray(self._transform_y(_uprank(_to_torch(y))).detach().cpu().numpy(), dtype=np.float64)
        x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
        w = w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w
        return self._periodogram(*periodogram_inputs(x, y, w), freq=freq, oversample=oversample, nyquist=nyquist)

    def _pick_periods(self, x, y, w, **grid):
        """p x Q periods, strongest first: 1 / `spectral_peaks` of each output's periodogram, inside the variables' bounds."""
        if self.spectral is None:
            raise ValueError("initial periods belong to spectral=Q")
        t, y, omega = periodogram_inputs(x, y, w)   # (more than one input column is refused here)
        pg = self._periodogram(t, y, omega, **grid)
        span = float(t.max() - t.min())
        return np.stack([np.clip(1.0 / spectral_peaks(pg.freq, row, self.spectral, span), 1e-4, 1e4) for row in pg.power])

    def init_spectral(self, x, y, w=None, **grid):
        """Pick the initial periods of the spectral-mixture components from the data's periodogram, now: layer i's `{i}/input/sm{q}/pers`
        become 1 / the q-th strongest peak (`spectral_peaks`) of output i's periodogram (`periodogram(x, y, w, **grid)`).  What
        `spectral_period="auto"` does at the first `fit` / `condition`, on demand and for any `spectral_period` - and where "auto" leaves a
        variable that already exists alone, this OVERWRITES it.  Returns the p x Q periods."""
        y_t = np.asarray(self._transform_y(_uprank(_to_torch(y))).detach().cpu().numpy(), dtype=np.float64)
        x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
        w = w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w
        periods = self._pick_periods(x, y_t, w, **grid)
        self._spectral_auto = periods
        self._stream_cache = None
        for pi in range(periods.shape[0]):
            for q in range(self.spectral):
                name = f"{pi}/input/sm{q}/pers"
                if name in self.vs:
                    self.vs.assign(name, _vector_from_init(periods[pi, q], 1))
        return periods.copy()

    def loo(self, x, y, w=None, score="log"):
        """Layer-wise leave-one-out cross-validation under the prior model (`GPAR.loo`): `(value, mean, var)`.  `value` is the sum
        over outputs and observed entries of log N(y_ij; mean_ij, var_ij), with the data handling of `logpdf(x, y, w)` (same
        transform and normalisation calls; a numpy scalar unless x or y was a torch tensor); `mean` and `var` are n x p numpy arrays
        of the predictive mean and variance of every observed y_ij given all other observations of output j (and the layer's inputs
        [x, y_<j] as `logpdf` builds them), in the space the model sees the outputs in, NaN where y is missing.  `score`: "log" as
        above; "crps": `value` is minus the summed continuous ranked probability score of those Gaussian predictives; "se": minus the
        summed squared error, -nansum((y - mean)^2) in the space the model sees the outputs in.  `value` is to be maximised under every
        rule and is in units of the normalised outputs, summed over the outputs; `mean` and `var` do not depend on the rule.  With
        inducing points there is no dense K^-1 to leave a point out of: ValueError."""
        check_score(score)
        if self.sparse:
            raise ValueError("leave-one-out cross-validation needs dense layers: not available with inducing points (x_ind)")
        any_torch = isinstance(x, torch.Tensor) or isinstance(y, torch.Tensor)
        x = _uprank(_to_engine(x))
        y = self._unnormalise_y(self._transform_y(_uprank(_to_engine(y))))  # (as logpdf)
        w = _init_weights(w, y)
        m, p = x.shape[1], y.shape[1]
        self._prepare_kernels(m, p, int(x.shape[0]))
        with torch.no_grad():
            value, pieces = _construct_gpar(self, self.vs, m, p).loo(x, y, w, score=score)
        mean = np.full((int(x.shape[0]), p), np.nan)
        var = np.full((int(x.shape[0]), p), np.nan)
        for i, (rows, mean_i, var_i, _) in enumerate(pieces):
            rows = rows.cpu().numpy()
            mean[rows, i], var[rows, i] = mean_i.cpu().numpy(), var_i.cpu().numpy()
        value = value.detach() if any_torch else value.detach().cpu().numpy()
        return value, mean, var

    def ahead(self, x, y, w=None, horizon=1, start=0, score="log", horizon_weights=None, window=None):
        """Rolling-origin forecast scoring under the prior model (`GPAR.ahead`): `(value, mean, var)` with the conventions of `loo`.
        The rows are taken in the order given (the time order); every observed y_rj with r >= `start` is predicted from the rows of
        output j observed at index <= r - `horizon` (and the layer's inputs [x, y_<j] as `logpdf` builds them) - the `horizon`-step-ahead
        forecast at every origin, from ONE factorisation per output instead of one conditioning per origin.  `value` is the sum of
        log N(y_rj; mean_rj, var_rj) over the scored entries, which by the chain rule over the outputs is the exact GPAR log score;
        `mean` and `var` are n x p numpy arrays of the predictive means and variances (of the noisy observation), NaN where y is missing
        or the row is not scored.  `horizon`: an int >= 1, counting rows as given (missing values make the bands ragged); a horizon >= n
        predicts every row from the prior.  `start`: an int in 0 ... n - 1.  `score` as for `loo`: "crps" / "se" sum minus the CRPS /
        minus the squared error of the scored forecasts.  Dense layers only: ValueError with inducing points.

        `horizon` a non-empty list, tuple or 1-D integer array of K distinct ints >= 1 (any order): all K horizons are scored from the one
        factorisation per output.  `mean` and `var` are then K x n x p (also for K = 1), `value` is sum_k horizon_weights[k] value_k with
        `horizon_weights` K positive finite numbers (default all 1; ValueError with an int `horizon`), and the K unweighted value_k,
        summed over the outputs, are left in `self.ahead_values_` (with an int `horizon`: the one value).

        `window` (an int >= 1, with an int `horizon`: ValueError beside a sequence): the sliding-window form of the evaluation - y_rj is
        predicted from the rows of output j observed at index r - horizon - window + 1 ... r - horizon ALONE, the forecast of a model kept
        on a window of recent rows (`update(..., drop=k)`); with no row observed there, from the prior.  `window` counts rows as given:
        missing values make the windows shorter, never longer.  window >= n gives the expanding score above; None is that evaluation
        itself."""
        check_score(score)
        if self.sparse:
            raise ValueError("rolling-origin forecast scoring needs dense layers: not available with inducing points (x_ind)")
        window = _check_window(window, horizon, horizon_weights)
        any_torch = isinstance(x, torch.Tensor) or isinstance(y, torch.Tensor)
        x = _uprank(_to_engine(x))
        y = self._unnormalise_y(self._transform_y(_uprank(_to_engine(y))))  # (as logpdf)
        w = _init_weights(w, y)
        m, p = x.shape[1], y.shape[1]
        horizon, start = _check_horizon(horizon, start, int(x.shape[0]))
        horizon_weights = _check_horizon_weights(horizon_weights, horizon)
        self._prepare_kernels(m, p, int(x.shape[0]))
        if isinstance(horizon, tuple):
            with torch.no_grad():
                value, pieces = _construct_gpar(self, self.vs, m, p).ahead(x, y, w, horizon, start, score=score, weights=horizon_weights)
            mean = np.full((len(horizon), int(x.shape[0]), p), np.nan)
            var = np.full((len(horizon), int(x.shape[0]), p), np.nan)
            values = np.zeros(len(horizon))
            for i, (rows, mean_i, var_i, values_i) in enumerate(pieces):
                rows = rows.cpu().numpy()
                mean[:, rows, i], var[:, rows, i] = mean_i.cpu().numpy(), var_i.cpu().numpy()
                values += values_i.cpu().numpy()
            self.ahead_values_ = values
            value = value.detach() if any_torch else value.detach().cpu().numpy()
            return value, mean, var
        with torch.no_grad():
            value, pieces = _construct_gpar(self, self.vs, m, p).ahead(x, y, w, horizon, start, score=score,
                                                                       **({} if window is None else {"window": window}))
        mean = np.full((int(x.shape[0]), p), np.nan)
        var = np.full((int(x.shape[0]), p), np.nan)
        for i, (rows, mean_i, var_i) in enumerate(pieces):
            rows = rows.cpu().numpy()
            mean[rows, i], var[rows, i] = mean_i.cpu().numpy(), var_i.cpu().numpy()
        self.ahead_values_ = np.array([float(value.detach())])
        value = value.detach() if any_torch else value.detach().cpu().numpy()
        return value, mean, var

    def cv(self, x, y, w=None, folds=None, score="log", gap=0):
        """Layer-wise blocked (leave-fold-out) cross-validation under the prior model (`GPAR.cv`): `(value, mean, var)` with the
        conventions of `loo`.  `folds`: an int k - k contiguous blocks of the rows as given, split as `np.array_split` splits them, the
        estimator for time series and other ordered data, where a single left-out point is predicted almost for free from its
        neighbours - or a 1-D integer array of n labels (any order; per output the labels are restricted to its observed rows, and a
        fold left empty vanishes).  `value` is the sum over outputs and folds of the JOINT log-density of the fold's observed entries
        given every other fold's; `mean` and `var` are n x p numpy arrays of the predictive means and marginal variances (the diagonals
        of the folds' predictive covariances), NaN where y is missing.  Folds of one row give `loo`; one fold gives `logpdf` for one
        output.  `score`: "log" alone - a fold is scored by its JOINT density, which has no per-row scoring rule ("crps" and "se"
        belong to `loo` and `ahead`: ValueError).  Dense layers only: ValueError with inducing points.

        `gap` (an int >= 0): purged, or hv-block, cross-validation (Burman, Chow & Nolan 1994; Racine 2000), the rows in the order given
        (the time order).  When a fold is held out, the `gap` rows before its first and after its last row are removed from the
        conditioning set as well, without being scored - the first and last rows of a held-out block otherwise keep a training row
        one step away.  The fold's span comes from the labels (missing values or not) and the gap counts rows as given, so per output
        missing values make the purge ragged; the first and last fold are purged on one side.  The labels must then not decrease
        along the rows (an int k never does): ValueError otherwise.  Every observed row is still scored exactly once; one fold gives
        `logpdf` whatever the gap, a gap >= n predicts every fold from the prior, and gap = 0 is the evaluation above, bit for bit."""
        if check_score(score) != "log":
            raise ValueError(f'score="{score}" belongs to loo and ahead: a fold is scored by its joint density, which has no per-row scoring rule')
        if self.sparse:
            raise ValueError("cross-validation needs dense layers: not available with inducing points (x_ind)")
        if folds is None:
            raise ValueError("cv needs folds: a number of contiguous blocks or one integer label per row")
        any_torch = isinstance(x, torch.Tensor) or isinstance(y, torch.Tensor)
        x = _uprank(_to_engine(x))
        y = self._unnormalise_y(self._transform_y(_uprank(_to_engine(y))))  # (as logpdf)
        w = _init_weights(w, y)
        m, p = x.shape[1], y.shape[1]
        labels = _fold_labels(folds, int(x.shape[0]))
        gap = _check_purge(check_gap(gap), labels)
        self._prepare_kernels(m, p, int(x.shape[0]))
        with torch.no_grad():
            value, pieces = _construct_gpar(self, self.vs, m, p).cv(x, y, w, labels, **({"gap": gap} if gap else {}))
        mean = np.full((int(x.shape[0]), p), np.nan)
        var = np.full((int(x.shape[0]), p), np.nan)
        for i, (rows, mean_i, var_i) in enumerate(pieces):
            rows = rows.cpu().numpy()
            mean[rows, i], var[rows, i] = mean_i.cpu().numpy(), var_i.cpu().numpy()
        value = value.detach() if any_torch else value.detach().cpu().numpy()
        return value, mean, var

    def _prepare_kernels(self, m, p, rows, training=False, inputs=False):
        """Have the engine compile the layers' run-time specialised device kernels up front and concurrently (HipEngine.prepare);
        the layer constructors instantiate their hyper-parameters on the way, as the first evaluation would."""
        eng = get_engine()
        cols = int(self.x_ind.shape[0]) if self.sparse else rows   # (inducing points: the launches are rows x M)
        if not hasattr(eng, "prepare") or rows * cols < (1 << 22) or os.environ.get("GPAR_JIT_PREPARE", "1") == "0":   # (prepare applies the thresholds)
            return
        with torch.no_grad():
            layers = _construct_gpar(self, self.vs, m, p).layers
            eng.prepare([(model()[0].kernel, m + pi) for pi, model in enumerate(layers)], rows, training=training, sparse=self.sparse,
                        inputs=inputs, cols=cols)

    def logpdf(self, x, y, w=None, sample_missing=False, posterior=False):
        """Log-density of observations under the prior (or, with `posterior`, the conditioned model).  Returns a
        numpy scalar unless x or y was a torch tensor (reference regression.py:461-506)."""
        any_torch = isinstance(x, torch.Tensor) or isinstance(y, torch.Tensor)
        y_given = y
        x = _uprank(_to_engine(x))
        y = self._unnormalise_y(self._transform_y(_uprank(_to_engine(y))))  # sic: reference regression.py:483
        if isinstance(y_given, torch.Tensor) and y_given.is_cuda and y.dim() == 2 and y.data_ptr() == y_given.data_ptr() and host_masks():
            # Device-resident outputs handed over as they are (no transform, no normalisation: `y` is an alias of the caller's
            # tensor): their NaN pattern decides every mask of the evaluation and costs a device-to-host synchronisation, which a
            # loop over the same outputs (an optimiser, a benchmark) would pay every time.  It is kept ON THE CALLER'S TENSOR OBJECT
            # together with the version counter it was taken at - it lives and dies with that object, nothing global holds the
            # tensor, and an in-place torch operation is seen.  (A write torch cannot see - a raw-pointer kernel, `.data`, a DLPack
            # alias - is not: `del y._gpar_nan` after one, or switch the cache off with `nan_pattern_cache = False`.)
            cached = getattr(y_given, "_gpar_nan", None) if self.nan_pattern_cache else None
            if cached is None or cached[0] != y_given._version or cached[1].shape != tuple(y.shape):
                cached = (y_given._version, torch.isnan(y).cpu().numpy())
                if self.nan_pattern_cache:
                    try:
                        y_given._gpar_nan = cached
                    except (AttributeError, RuntimeError):
                        pass
            y._host_nan, y._host_nan_version = cached[1], y._version
        w = _init_weights(w, y)
        m, p = x.shape[1], y.shape[1]
        if posterior and not self.is_conditioned:
            raise RuntimeError("Must condition or fit model before computing the logpdf under the posterior.")
        self._prepare_kernels(m, p, int(x.shape[0]))
        gpar = _construct_gpar(self, self.vs, m, p)
        if posterior:
            cached = self._stream_posterior() if getattr(self, "_stream_cache", None) is not None else None
            gpar = cached if cached is not None else gpar | (self.x, self.y, self.w)
        value = gpar.logpdf(x, y, w, only_last_layer=False, sample_missing=sample_missing)
        if not any_torch:
            value = value.detach().cpu().numpy()
        return value

    def _sample_device(self, x, w, p, posterior, num_samples, latent, conditioned=None, marginal=False, sampler="exact", features=2048):
        """The samples of `sample` as engine tensors (n* x p each), output transforms undone."""
        if sampler == "pathwise" and not posterior:
            raise ValueError('sampler="pathwise" conditions prior draws on the data: it needs posterior=True')
        x = _uprank(_to_engine(x))
        if posterior and not self.is_conditioned:
            raise RuntimeError("Must condition or fit model before sampling from the posterior.")
        elif not posterior and p is None:
            raise ValueError("Must specify number of outputs to sample.")
        if w is None:
            w = _default_weights(x.shape[0], self.p if posterior else p)
        else:
            w = _uprank(_to_torch(w))
        if posterior and conditioned is None and getattr(self, "_stream_cache", None) is not None:
            conditioned = self._stream_posterior()   # the factors `update` keeps, while they are valid
        if posterior and conditioned is not None:
            gpar = conditioned  # parallel.sharded_condition: factors computed across ranks
        elif posterior:
            gpar = _construct_gpar(self, self.vs, self.m, self.p)
            gpar = gpar | (self.x, self.y, self.w)
        else:
            gpar = _construct_gpar(self, self.vs, x.shape[1], p)
        return [self._untransform_y(self._unnormalise_y(s)).detach()
                for s in gpar.sample_many(x, w, num_samples, latent=latent, marginal=marginal, sampler=sampler, features=features)]

    def predict_moments(self, x, w=None, latent=False, _conditioned=None):
        """Predictive means and variances (two n* x p arrays) of the conditioned model at x in CLOSED FORM - for `replace=True`,
        where posterior means are fed forward and the predictive law of every output at every point is Gaussian.  These are
        the limits of `predict`'s Monte-Carlo mean and of the variance of its samples (central 95 % bounds: mean -+ 1.96 sd);
        no sampling, no n* x n* covariance.  An addition behind the reference's API (it only samples, regression.py:566-597);
        raises ValueError for `replace=False`, where sampled values are fed forward and no closed form exists."""
        if not self.is_conditioned:
            raise RuntimeError("Must condition or fit model before predicting.")
        if not self.replace:
            raise ValueError("closed-form predictive moments need replace=True")
        self._check_identity_transform()
        x = _uprank(_to_engine(x))
        w = _default_weights(x.shape[0], self.p) if w is None else _uprank(_to_torch(w))
        gpar = _conditioned
        if gpar is None and getattr(self, "_stream_cache", None) is not None:
            gpar = self._stream_posterior()
        if gpar is None:
            gpar = _construct_gpar(self, self.vs, self.m, self.p) | (self.x, self.y, self.w)
        with torch.no_grad():
            mean, var = gpar.moments(x, w, latent=latent)
            # un-normalisation is affine (y = y_n * std + mean): apply it to the mean, its slope squared to the variance
            zero = torch.zeros(1, self.p, dtype=mean.dtype, device=mean.device)
            one = torch.ones(1, self.p, dtype=mean.dtype, device=mean.device)
            shift = self._unnormalise_y(zero)
            slope = self._unnormalise_y(one) - shift
            mean = self._unnormalise_y(mean)
            var = var * slope ** 2
        return mean.cpu().numpy(), var.cpu().numpy()

    def _check_identity_transform(self):
        probe = torch.tensor([-1.5, 0.25, 3.0], dtype=torch.float64)
        if not torch.equal(self._untransform_y(probe), probe):
            raise ValueError("closed-form predictive moments need the identity output transform (a non-linear map of a Gaussian is not Gaussian)")

    def decompose(self, x, components=None, variance=True):
        """What each part of the trained kernel explains at x - an addition; the reference shows only the sum.  A layer's kernel is a
        sum of named terms - `input/nonlin`, `input/per`, `input/sm0` .. , `input/lin`, `input/const`, `output/lin`, `output/nonlin`,
        named after the variables they come from - and its latent posterior is the sum of one Gaussian process per term (Rasmussen &
        Williams 5.4.3): `decompose` returns their means and marginal variances, for time series the trend and the seasonal part, for
        GPAR how much of an output comes from the inputs and how much from the outputs before it.

        `components` None: one component per term.  A dict {name: [patterns]}: the terms whose name matches a pattern (`fnmatch`) form
        the component; terms no pattern matches are left out, a term matched by two components is a ValueError, a component without a
        term in a layer is absent from that layer's names.

        Returns `Decomposition(names, mean, var, offset)`: per output i a tuple of names, a G_i x n* array of means and one of variances
        (`var` is None without `variance`), in the units of y - means times the output's normalisation slope, variances times its
        square - and the p normalisation shifts `offset`.  The layers see [x, latent posterior means of the outputs before them] (the
        plug-in decomposition, `GPAR.decompose`): with `replace=True` and every term used, offset[i] + mean[i].sum(0) is
        `predict_moments(x, latent=True)[0][:, i]`.  RuntimeError: not conditioned; ValueError: a non-identity `transform_y`, inducing
        points."""
        if not self.is_conditioned:
            raise RuntimeError("Must condition or fit model before decomposing.")
        self._check_identity_transform()
        if self.sparse:
            raise ValueError("a decomposition by kernel component needs dense layers: inducing points are not supported")
        x = _uprank(_to_engine(x))
        gpar = self._stream_posterior() if getattr(self, "_stream_cache", None) is not None else None
        if gpar is None:
            gpar = _construct_gpar(self, self.vs, self.m, self.p) | (self.x, self.y, self.w)
        names, comps = [], []
        for model in gpar.layers:
            layer_names, comp = _group_terms([t.label for t in model()[0].kernel.terms], components)
            names.append(layer_names)
            comps.append((comp, len(layer_names)))
        with torch.no_grad():
            parts = gpar.decompose(x, comps, variance=variance)
            zero = torch.zeros(1, self.p, dtype=torch.float64, device=x.device)
            shift = self._unnormalise_y(zero)
            slope = self._unnormalise_y(torch.ones_like(zero)) - shift   # (un-normalisation is affine, as in predict_moments)
            mean = [(m * slope[0, i]).cpu().numpy() for i, (m, _) in enumerate(parts)]
            var = [(v * slope[0, i] ** 2).cpu().numpy() for i, (_, v) in enumerate(parts)] if variance else None
        return Decomposition(tuple(names), mean, var, shift.reshape(-1).cpu().numpy())

    def derivative(self, x, wrt=0, variance=True):
        """How fast every output changes with input column `wrt` at x, and how certain that is - an addition; the reference has no
        derivatives.  The derivative of a Gaussian process is a Gaussian process (Rasmussen & Williams 9.4): returns `(mean, var)`, two
        n* x p arrays in the units of y per unit of x - means times the output's normalisation slope, variances times its square; `var`
        is None without `variance`.  A slope is significant where |mean| exceeds about two sqrt(var).

        The layers are visited along the plug-in path of `decompose` (`GPAR.derivative`): layer i sees [x, latent posterior means of the
        outputs before it] and is differentiated along (e_wrt, the derivatives of those means), so mean[:, i] is the TOTAL derivative of
        output i's plug-in mean - with `replace=True` exactly d / d x_wrt of `predict_moments(x, latent=True)[0][:, i]` - and var[:, i]
        the latent variance of layer i's derivative along that direction, the earlier outputs' means held as given.  After `update()` the
        kept factors are used, as in `decompose`.  On the device one library call per layer (`gpar_posterior_deriv`); an engine without
        it raises NotImplementedError.  RuntimeError: not conditioned; ValueError: a non-identity `transform_y`, inducing points, `wrt`
        outside 0 .. m - 1, `matern=0.5` (not differentiable)."""
        if not self.is_conditioned:
            raise RuntimeError("Must condition or fit model before differentiating.")
        self._check_identity_transform()
        if self.sparse:
            raise ValueError("posterior derivatives need dense layers: inducing points are not supported")
        if self.model_config.get("matern") == 0.5:
            raise ValueError("matern=0.5: the Matern 1/2 process is not differentiable")
        wrt = int(wrt)
        if not 0 <= wrt < self.m:
            raise ValueError(f"wrt={wrt}: the model has inputs 0 .. {self.m - 1}")
        x = _uprank(_to_engine(x))
        gpar = self._stream_posterior() if getattr(self, "_stream_cache", None) is not None else None
        if gpar is None:
            gpar = _construct_gpar(self, self.vs, self.m, self.p) | (self.x, self.y, self.w)
        with torch.no_grad():
            mean, var = gpar.derivative(x, wrt, variance=variance)
            zero = torch.zeros(1, self.p, dtype=torch.float64, device=x.device)
            slope = self._unnormalise_y(torch.ones_like(zero)) - self._unnormalise_y(zero)   # (un-normalisation is affine, as in predict_moments)
            mean = (mean * slope).cpu().numpy()
            var = (var * slope ** 2).cpu().numpy() if variance else None
        return mean, var

    # ---- hyperparameter uncertainty: Laplace at the trained values, delta method for the forecast -------------------------------------
    def _layer_chains(self):
        """Every layer's chain rule as an object (`fastfit.LayerChain`): the layer's kernel over value holders and the layout of its
        variables.  Host work only - no data, no device buffer, any number of rows."""
        from . import fastfit

        if self.sparse:
            raise ValueError("hyperparameter uncertainty needs dense layers: inducing points are not supported")
        eng = get_engine()
        if not hasattr(eng, "gram_grad_rows"):
            raise NotImplementedError(f"{type(eng).__name__} has no gram_grad_rows: per-row gradient sums are a device kernel "
                                      "(gpar_gram_grad_rows); run them on the HIP engine")
        out = []
        for pi in range(self.p):
            chain = fastfit.layer_chain(self, eng, self.vs, pi, [f"{pi}/*"])
            if chain is None:
                raise ValueError(f"layer {pi}: a kernel parameter is not one variable of the store; its chain rule cannot be traced")
            out.append(chain)
        return out

    def _layer_objectives(self):
        """Per layer (chain, fg) on the conditioned data: the chain rule (`_layer_chains`; the prepared objective itself where there is
        one) and `fg(u)` -> (negative log marginal likelihood, gradient) in the optimiser's coordinates - the prepared objective of
        `fit(fix=True)` (fastfit.build) where it applies, above `one_call_grad_rows()` rows (or wherever else it does not) the general
        route's objective and back-propagated gradient, exactly what `fit` itself trains such a layer through."""
        from . import fastfit
        from .optimise import objective_and_gradient

        chains = self._layer_chains()
        eng = get_engine()
        x_dev, y_dev, w_dev = eng.tensor(self.x), eng.tensor(self.y), eng.tensor(self.w)
        if host_masks():
            if y_dev is self.y:
                y_dev = y_dev.view(y_dev.shape)
            y_dev._host_nan, y_dev._host_nan_version = torch.isnan(self.y).numpy(), y_dev._version
        y_cached = {k: list(per_output(y_dev, w_dev, keep=k)) for k in [True, False]}
        self._prepare_kernels(self.m, self.p, self.n, training=True, inputs=False)
        out = []
        for pi, chain in enumerate(chains):
            with torch.no_grad():
                gpar = _construct_gpar(self, self.vs, self.m, pi + 1)
                fixed_x, _ = gpar.logpdf(x_dev, y_cached, None, only_last_layer=True, outputs=list(range(pi)), return_inputs=True)
            obj = fastfit.build(self, eng, self.vs, pi, [f"{pi}/*"], fixed_x, y_cached[bool(self.impute)][pi]) if self.fast_fit else None
            if obj is not None and obj.names == chain.names:
                out.append((obj, obj.fg))
                continue

            def neg_value(vs, pi=pi, fixed_x=fixed_x):
                return -_construct_gpar(self, vs, self.m, pi + 1).logpdf(fixed_x, y_cached, None, only_last_layer=True, outputs=[pi])

            out.append((chain, objective_and_gradient(neg_value, self.vs, chain.names)[0]))
        return out

    def laplace(self, x, y, w=None):
        """How sure the trained values are - an addition; the reference's todo.tasks asks for an "overview of trained hyperparameters".
        The Laplace approximation at the current values, layer by layer (layers train independently under `fit(fix=True)`: no
        cross-layer blocks): H = the Hessian of the layer's negative log marginal likelihood on (x, y, w) in the optimiser's
        unconstrained coordinates (`fastfit.hessian_of`: a central difference of the analytic gradient, 2 P evaluations - of the
        prepared objective where `fit(fix=True)` trains the layer through it, of the general route's back-propagated gradient above
        `one_call_grad_rows()` rows),
        Sigma = its pseudo-inverse over the directions with eigenvalue > 1e-10 lambda_max.  The others are FLAT - the values are not at
        a mode there, or a variable is pinned at a bound -, are left out and counted; any flat direction issues ONE warning.

        Returns `HyperPosterior(names, value, stderr, cov, flat, slices, layers)`: the trained variables' names layer by layer, per name
        the value and the standard error in natural units (delta method through the variable's transform: |d value / d u| sqrt(cov_uu);
        inf for a variable lying wholly in flat directions), `cov` (P x P, block diagonal over layers, unconstrained coordinates),
        `flat` per layer; `slices[k]` / `layers[i]` locate name k / layer i among the P coordinates.  The data are conditioned on, as
        `fit` does.  RuntimeError: neither fitted nor conditioned; ValueError: inducing points; NotImplementedError: an engine without
        `gram_grad_rows` (the forecast's side of this needs it: `predict_moments_hyper`)."""
        if not self.is_conditioned:
            raise RuntimeError("Must condition or fit model before the Laplace approximation.")
        if self.sparse:
            raise ValueError("hyperparameter uncertainty needs dense layers: inducing points are not supported")
        self.condition(x, y, w)
        names, values, errors, slices, layers, blocks, flats = [], [], [], [], [], [], []
        at = 0
        from .fastfit import hessian_of

        for obj, fg in self._layer_objectives():
            u = self.vs.get_vector(obj.names)
            try:
                sigma, flat, support = laplace_block(hessian_of(fg, u))
            finally:
                self.vs.set_vector(u, obj.names)   # (the general route's evaluations write the store)
            value, slope = obj.natural(u)
            sd = np.where(support > 1e-12, np.abs(slope) * np.sqrt(np.maximum(np.diag(sigma), 0.0)), np.inf)
            for name, kind, lower, upper, sl, shape in obj.layout:
                names.append(name)
                values.append(value[sl].reshape(shape))
                errors.append(sd[sl].reshape(shape))
                slices.append(slice(at + sl.start, at + sl.stop))
            layers.append(slice(at, at + obj.size))
            at += obj.size
            blocks.append(sigma)
            flats.append(flat)
        if any(flats):
            warnings.warn(f"laplace: {sum(flats)} flat direction(s) of the training objective (per layer: {tuple(flats)}) - not at a mode, or a "
                          "variable pinned at a bound; they are left out of the covariance", stacklevel=2)
        return HyperPosterior(tuple(names), tuple(values), tuple(errors), block_diagonal(blocks), tuple(flats), tuple(slices), tuple(layers))

    def predict_moments_hyper(self, x, hp, w=None, latent=False):
        """What the uncertainty of the trained values does to the forecast - an addition.  Returns `(mean, var, var_hyper)`, three n* x p
        arrays: `mean` and `var` are `predict_moments(x, w, latent)` (that call), and, to first order (Laplace at the mode, delta method),
            var_hyper[:, i] = diag(J_i Sigma J_i^T)        in the units of y,
        J_i the TOTAL Jacobian of output i's plug-in latent mean over all layers' variables (`GPAR.hyper_jacobian`: per layer one fused
        device pass with the row index unreduced, `gpar_gram_grad_rows`, and the chain rule through the test-time inputs) and Sigma =
        `hp.cov` from `laplace`.  The first-order total variance is var + var_hyper; the sensitivity of `var` itself to the
        hyperparameters is second order and left out, and so is, under `replace=True`, the dependence of the replaced TRAINING inputs on
        earlier layers' variables (they are held as given, as `fit(fix=True)` holds them).  `matern=0.5` is served for a model with ONE output (the
        parameter gradient takes the r = 0 multiplier as 0, as in training); with more outputs it is refused up front (ValueError): a
        Matern 1/2 layer after the first has no input derivative for the chain rule.  Any number of rows: the chain rule is traced
        on the host (`fastfit.LayerChain`) and needs none of the training objective's buffers.  ValueError: inducing points, a non-identity
        `transform_y`, `replace=False` (`predict_moments`), an `hp` of another model; NotImplementedError: an engine without
        `gram_grad_rows`."""
        if not self.is_conditioned:
            raise RuntimeError("Must condition or fit model before predicting.")
        if self.sparse:
            raise ValueError("hyperparameter uncertainty needs dense layers: inducing points are not supported")
        self._check_identity_transform()
        if self.model_config.get("matern") == 0.5 and self.p > 1:
            raise ValueError("matern=0.5 with more than one output: a Matern 1/2 layer after the first has no input derivative for the "
                             "chain rule through the earlier outputs (its process is not differentiable)")
        eng = get_engine()
        if not hasattr(eng, "gram_grad_rows"):
            raise NotImplementedError(f"{type(eng).__name__} has no gram_grad_rows: per-row gradient sums are a device kernel "
                                      "(gpar_gram_grad_rows); run them on the HIP engine")
        mean, var = self.predict_moments(x, w, latent)
        objectives = self._layer_chains()
        cov = np.asarray(hp.cov, dtype=np.float64)
        if tuple(n for obj in objectives for n in obj.names) != tuple(hp.names) or cov.shape[0] != sum(obj.size for obj in objectives):
            raise ValueError("hp does not belong to this model: its names are not the trained variables of the layers")
        chains = [obj.chain_matrix(self.vs.get_vector(obj.names)) for obj in objectives]
        x = _uprank(_to_engine(x))
        gpar = self._stream_posterior() if getattr(self, "_stream_cache", None) is not None else None
        if gpar is None:
            gpar = _construct_gpar(self, self.vs, self.m, self.p) | (self.x, self.y, self.w)
        with torch.no_grad():
            jac = gpar.hyper_jacobian(x, chains)
            sigma = torch.from_numpy(cov).to(x.device)
            zero = torch.zeros(1, self.p, dtype=torch.float64, device=x.device)
            slope = self._unnormalise_y(torch.ones_like(zero)) - self._unnormalise_y(zero)
            extra = torch.stack([((J @ sigma) * J).sum(dim=1) for J in jac], dim=1) * slope ** 2
        return mean, var, extra.cpu().numpy()

    def sample(self, x, w=None, p=None, posterior=False, num_samples=1, latent=False, _conditioned=None, sampler="exact", features=2048):
        """Draw samples from the prior or the posterior at inputs x; a single ndarray for num_samples=1, otherwise
        a list (reference regression.py:508-564).  (`_conditioned`: an already conditioned GPAR, used by the
        multi-GPU path.)  `sampler`, `features`: as in `predict`; "pathwise" needs `posterior=True`."""
        samples = [s.cpu().numpy() for s in self._sample_device(x, w, p, posterior, num_samples, latent, _conditioned, sampler=sampler,
                                                                 features=features)]
        return samples[0] if num_samples == 1 else samples

    def predict(self, x, w=None, num_samples=100, latent=False, credible_bounds=False, marginal=False, sampler="exact", features=2048):
        """Monte-Carlo predictive mean (and central 95% marginal bounds) from posterior samples
        (reference regression.py:566-597).  The reduction over the sample axis runs on the device
        (`gpar_sample_stats`: sequential mean, numpy-"linear" percentiles); only the n* x p results cross PCIe.

        `marginal=True` (an addition, off by default; reference todo.tasks:5): the statistics returned here only involve
        per-point marginals, so within each layer the points may be drawn from their marginals N(mean_j, var_j)
        instead of jointly - same distribution of every returned number, no n* x n* covariance, SYRK downdate or
        factorisation per sample (`GPAR.sample_many`).

        `sampler="pathwise"` (an addition; the default "exact" is the path above, unchanged): the samples are drawn by pathwise
        conditioning (Matheron's rule; Wilson et al., ICML 2020) - a prior draw through a random Fourier basis of `features`
        frequencies per stationary kernel term, corrected by one exact update from the factor conditioning holds.  Joint draws over
        the n* points without any n* x n* matrix: the cost per sample and layer falls from n^2 n* to n n* + n* `features`, and n* is
        bounded by the output alone.  The prior part is an approximation that improves with `features` (DESIGN 3.23 tabulates it); the
        update is exact.  One basis per layer and call, seeded from the engine's seed.  ValueError: inducing points, `marginal=True`,
        a kernel term without a basis (a linear factor times another), an unknown sampler, `features < 1`."""
        samples = self._sample_device(x, w, None, True, num_samples, latent, marginal=marginal, sampler=sampler, features=features)
        if num_samples == 1:
            # the reference hands np.mean a single (n*, p) array here, so axis 0 is the input axis; keep that
            samples = samples[0].cpu().numpy()
            mean = np.mean(samples, axis=0)
            if credible_bounds:
                return mean, np.percentile(samples, 2.5, axis=0), np.percentile(samples, 100 - 2.5, axis=0)
            return mean
        stack = torch.stack(samples)
        if credible_bounds:
            mean, lower, upper = get_engine().sample_stats(stack, 2.5, 100 - 2.5)
            return mean.cpu().numpy(), lower.cpu().numpy(), upper.cpu().numpy()
        return get_engine().sample_stats(stack)[0].cpu().numpy()
