"""The held-out scoring schemes behind `loo()`, `cv()`, `ahead()` and `fit(objective=...)`, as host-side objects: one class per scheme,
carried from `gp.Obs` and `fastfit.build` through `HipEngine` to the one marshaller of the library calls (`hip.held_out_dense`).

A scheme holds its checked host arrays and answers what the layers above the C ABI need to know of it: which family of entries scores
it (`family`, `entry`), whether those take a scoring rule (`takes_score`), whether the whole matrix is factored (`factored`) and K^-1
formed by the value form (`inverse`), how many horizons it scores (`horizons`), the doubles of its vector workspace (`workspace`),
whether the fused call takes it (`fits`) and the uploaded arrays as the entry's trailing arguments (`device`, made once).  The array
checkers (`fold_offsets`, `hold_extents`, `origin_array`, `origins_array`, `horizon_weight_array`, `window_arrays`) are the one check
of each kind of array; the `upload_*` functions are what `device` runs.
"""
import ctypes

import numpy as np
import torch

from . import _lib

__all__ = ["Loo", "Folds", "Purged", "Origins", "Window", "scheme_of"]


def _host(a):
    return a.cpu() if isinstance(a, torch.Tensor) else a


def _on_device(a):
    return isinstance(a, torch.Tensor) and a.is_cuda


def fold_offsets(fold_start, n):
    """The nfolds + 1 row offsets of contiguous folds over n rows as a checked host array (int64): ascending strictly from 0 to n
    (no rows: the single offset 0).  The one check of fold offsets: `gp.Obs.cv` and `upload_folds` both go through it."""
    starts = np.asarray(_host(fold_start), dtype=np.int64).reshape(-1)
    if n == 0 and starts.size <= 1:
        return np.zeros(1, dtype=np.int64)
    if starts.size < 2 or starts[0] != 0 or starts[-1] != n or np.any(np.diff(starts) < 1):
        raise ValueError("fold_start must ascend strictly from 0 to the number of rows")
    return starts


def upload_folds(fold_start, n, device):
    """(device int32 array of the nfolds + 1 row offsets, nfolds, largest fold): what the fused cross-validation entries take, from
    offsets checked by `fold_offsets`; a fold larger than GPAR_CV_MAX_FOLD is a ValueError."""
    starts = fold_offsets(fold_start, n)
    sizes = np.diff(starts)
    if sizes.size == 0 or int(sizes.max()) > _lib.CV_MAX_FOLD:
        raise ValueError(f"the fused cross-validation takes 1 to {_lib.CV_MAX_FOLD} rows per fold")
    return torch.tensor(starts, dtype=torch.int32, device=device), int(sizes.size), int(sizes.max())


def hold_extents(fold_start, hold, n):
    """(offsets, hold_lo, hold_hi) of purged cross-validation as checked host arrays (int64): the offsets as `fold_offsets` checks them, and
    per fold the block [hold_lo[f], hold_hi[f]) it is not predicted from - inside 0 ... n, containing the fold, neither end decreasing from
    one fold to the next.  The one check of these extents: `gp.Obs.cv` and `upload_hold` both go through it."""
    starts = fold_offsets(fold_start, n)
    if not isinstance(hold, (tuple, list)) or len(hold) != 2:
        raise ValueError("hold must be the pair (hold_lo, hold_hi)")
    lo, hi = (np.asarray(_host(h)) for h in hold)
    nfolds = starts.size - 1
    for h in (lo, hi):
        if h.ndim != 1 or h.size != nfolds or (h.size and not np.issubdtype(h.dtype, np.integer)):
            raise ValueError("hold_lo and hold_hi must hold one integer per fold")
    lo, hi = lo.astype(np.int64), hi.astype(np.int64)
    if nfolds and (np.any(lo < 0) or np.any(hi > n) or np.any(lo > starts[:-1]) or np.any(hi < starts[1:]) or np.any(np.diff(lo) < 0)
                   or np.any(np.diff(hi) < 0)):
        raise ValueError("every block hold_lo[f] ... hold_hi[f] must lie in 0 ... n and contain its fold, neither end decreasing along the folds")
    return starts, lo, hi


def upload_hold(fold_start, hold, n, device):
    """(device int32 offsets, hold_lo, hold_hi, nfolds, largest block): what the fused purged cross-validation entries take, from extents
    checked by `hold_extents`; a block of more than GPAR_CV_MAX_FOLD rows is a ValueError."""
    starts, lo, hi = hold_extents(fold_start, hold, n)
    if lo.size == 0 or int((hi - lo).max()) > _lib.CV_MAX_FOLD:
        raise ValueError(f"the fused purged cross-validation takes 1 to {_lib.CV_MAX_FOLD} rows per fold, its purged rows included")
    up = lambda a: torch.tensor(a, dtype=torch.int32, device=device)   # noqa: E731
    return up(starts), up(lo), up(hi), int(lo.size), int((hi - lo).max())


def origin_array(origin, n):
    """The n origins of a rolling-origin evaluation as a checked host array (int64): -1 (not scored) or 0 ... r for row r.  The one check
    of origins: `gp.Obs.ahead` and `upload_origin` both go through it."""
    o = np.asarray(_host(origin))
    if o.ndim != 1 or o.size != n or (o.size and not np.issubdtype(o.dtype, np.integer)):
        raise ValueError("origin must hold one integer per row")
    o = o.astype(np.int64)
    if np.any(o < -1) or np.any(o > np.arange(n)):
        raise ValueError("origin[r] must be -1 (not scored) or lie in 0 ... r")
    return o


def upload_origin(origin, n, device):
    """Device int32 array of the n origins the fused rolling-origin entries take, checked by `origin_array`."""
    return torch.tensor(origin_array(origin, n), dtype=torch.int32, device=device)


def origins_array(origins, n):
    """The K x n origins of a multi-horizon rolling-origin evaluation as a checked host array (int64), every row as `origin_array` checks
    it.  The one check of such origins: `gp.Obs.ahead` and `upload_origins` both go through it."""
    o = np.asarray(_host(origins))
    if o.ndim != 2 or o.shape[0] < 1:
        raise ValueError("origins must hold one row of n integers per horizon")
    return np.stack([origin_array(row, n) for row in o])


def upload_origins(origins, n, device):
    """Device int32 array of the K x n origins the fused multi-horizon entries take, checked by `origins_array`; more than
    GPAR_AHEAD_MAX_HORIZONS rows are a ValueError."""
    o = origins_array(origins, n)
    if o.shape[0] > _lib.AHEAD_MAX_HORIZONS:
        raise ValueError(f"the fused multi-horizon entries take 1 to {_lib.AHEAD_MAX_HORIZONS} horizons")
    return torch.tensor(o, dtype=torch.int32, device=device)


def horizon_weight_array(weights, k):
    """The k weights of a multi-horizon evaluation as a checked host array (float64): positive and finite; None: all 1."""
    if weights is None:
        return np.ones(k)
    if isinstance(weights, (str, bytes)) or np.ndim(weights) != 1:
        raise ValueError(f"the horizons' weights must be {k} positive finite numbers")
    try:
        w = np.array([float(v) for v in weights], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"the horizons' weights must be {k} positive finite numbers") from None
    if w.size != k or not np.all(np.isfinite(w)) or np.any(w <= 0.0):
        raise ValueError(f"the horizons' weights must be {k} positive finite numbers")
    return w


def window_arrays(lo, origin, n):
    """(lo, origin) of a sliding-window forecast evaluation as checked host arrays (int64): origin as `origin_array` checks it, and on every
    scored row 0 <= lo[r] <= origin[r] - row r is predicted from rows lo[r] ... origin[r] - 1 -, neither array decreasing over the scored
    rows.  The one check of these arrays: `gp.Obs.ahead` and `upload_window` both go through it."""
    o = origin_array(origin, n)
    l = np.asarray(_host(lo))
    if l.ndim != 1 or l.size != n or (l.size and not np.issubdtype(l.dtype, np.integer)):
        raise ValueError("lo must hold one integer per row")
    l = l.astype(np.int64)
    scored = o >= 0
    if np.any(l[scored] < 0) or np.any(l[scored] > o[scored]):
        raise ValueError("lo[r] must lie in 0 ... origin[r] on every scored row")
    if np.any(np.diff(l[scored]) < 0) or np.any(np.diff(o[scored]) < 0):
        raise ValueError("lo and origin must not decrease over the scored rows: a window slides forward")
    return l, o


def upload_window(lo, origin, n, device):
    """(device int32 lo, device int32 origin): what the fused sliding-window entries take, from arrays checked by `window_arrays`; a window
    of more than GPAR_AHEAD_WINDOW_MAX rows is a ValueError."""
    l, o = window_arrays(lo, origin, n)
    if l.size and int((o - l)[o >= 0].max(initial=0)) > _lib.AHEAD_WINDOW_MAX:
        raise ValueError(f"the fused sliding-window entries take windows of at most {_lib.AHEAD_WINDOW_MAX} rows")
    return torch.tensor(l, dtype=torch.int32, device=device), torch.tensor(o, dtype=torch.int32, device=device)


class Loo:
    """Leave-one-out, and the base of the schemes: what is said here holds for every scheme that does not say otherwise."""

    family = "loo"        # the stem of the `hip` / `HipEngine` names: family + "_dense" (+ "_grad")
    suffix = "_score"     # ... and of the library's entries, with this behind them where the ABI has the score-taking form
    ws = _lib.WS_LOO      # the code `gpar_workspace_doubles` sizes the family's vector workspace by
    takes_score = True    # the entries take a scoring rule (blocked folds score a fold's joint density: "log" alone)
    factored = True       # the whole matrix is factored: X, alpha and the factorisation flags are passed, the factor comes back
    inverse = True        # the value form works on K^-1: it takes X and a scratch matrix
    horizons = None       # K: the moments are K x n and a K-vector of unweighted values exists
    param = 0             # the family's parameter of `gpar_workspace_doubles`
    args = ()             # what `Obs` hands the engine's named methods in the places of their scheme arguments

    def __init__(self):
        self._device = None

    def entry(self, grad):
        """The library entry that scores the scheme: the value form, or the one that returns the gradient's ingredients too."""
        return f"gpar_{self.family}_dense{'_grad' if grad else ''}{self.suffix}"

    def workspace(self, lib, n, grad):
        """Doubles of the family's vector workspace."""
        return int(lib.gpar_workspace_doubles(self.ws, n, int(grad), self.param))

    def fits(self):
        """The fused call takes the scheme (the host-side limit; the composed route has none)."""
        return True

    def _upload(self, n, dev):
        return ()

    def device(self, n, dev):
        """The uploaded arrays as the entry's trailing arguments, in its order: tensors, counts, the ctypes weight array.  Made once and
        kept (the scheme keeps the host array of weights alive with them); beyond `fits()` the upload's ValueError."""
        if self._device is None:
            self._device = self._upload(n, dev)
        return self._device


class Folds(Loo):
    """Contiguous folds by their nfolds + 1 row offsets (`fold_offsets`), or the triple `upload_folds` returned."""

    family, suffix, ws, takes_score = "cv", "", _lib.WS_CV, False

    def __init__(self, starts=None, uploaded=None):
        self.starts, self._device, self.args = starts, uploaded, (self,)
        self.param = int(uploaded[2]) if uploaded is not None else int(np.diff(starts).max(initial=0))   # (the largest fold)

    @classmethod
    def of(cls, fold_start, n):
        """The scheme of what `cv_dense[_grad]` take: itself, the triple `upload_folds` returns, or offsets (checked here)."""
        if isinstance(fold_start, cls):
            return fold_start
        return cls(uploaded=fold_start) if isinstance(fold_start, tuple) else cls(fold_offsets(fold_start, n))

    def fits(self):
        return self.param <= _lib.CV_MAX_FOLD

    def _upload(self, n, dev):
        return upload_folds(self.starts, n, dev)


class Purged(Folds):
    """Contiguous folds, each predicted from the rows outside a block that contains it (`hold_extents`), or the five-tuple `upload_hold`
    returned.  The fused calls hold a fold AND its purged rows in one tile."""

    family, ws = "cv_gap", _lib.WS_CV_GAP

    def __init__(self, starts=None, lo=None, hi=None, uploaded=None):
        self.starts, self.lo, self.hi, self._device, self.args = starts, lo, hi, uploaded, (self, None)
        self.param = int(uploaded[4]) if uploaded is not None else int((hi - lo).max(initial=0))   # (the largest block)

    @classmethod
    def of(cls, fold_start, hold, n):
        """The scheme of what `cv_gap_dense[_grad]` take: itself or the five-tuple `upload_hold` returns (`hold` None), or offsets and
        the pair (hold_lo, hold_hi) (checked here)."""
        if isinstance(fold_start, cls):
            return fold_start
        return cls(uploaded=fold_start) if hold is None else cls(*hold_extents(fold_start, hold, n))

    def _upload(self, n, dev):
        return upload_hold(self.starts, (self.lo, self.hi), n, dev)


class Origins(Loo):
    """Rolling origins, one per row (`origin_array`; or the device tensor `upload_origin` returned) - or K x n of them with K weights, K
    horizons scored from the one factorisation (`origins_array`, `horizon_weight_array`; or the device tensor `upload_origins` returned)."""

    family, ws, inverse = "ahead", _lib.WS_AHEAD, False

    def __init__(self, origin=None, weights=None, uploaded=None):
        self.origin, self.weights, self.args = origin, weights, (self,)
        self._device = None if uploaded is None else (uploaded,)
        shape = (origin if uploaded is None else uploaded).shape
        if len(shape) == 2:
            self.family, self.suffix, self.ws = "ahead_multi", "", _lib.WS_AHEAD_MULTI
            self.horizons = self.param = int(shape[0])
            if uploaded is not None:
                self._device = (uploaded, self.horizons, self._c_weights())

    @classmethod
    def of(cls, origin, n, weights=None, multi=False):
        """The scheme of what `ahead_dense[_grad]` and (`multi`) `ahead_multi_dense[_grad]` take: itself, the device tensor `upload_origin`
        / `upload_origins` returns, or host origins (checked here); with `multi` the K weights beside them (None: all 1)."""
        if isinstance(origin, cls):
            return origin
        if not multi:
            return cls(uploaded=origin) if _on_device(origin) else cls(origin_array(origin, n))
        if not _on_device(origin):
            origin = origins_array(origin, n)
            return cls(origin, horizon_weight_array(weights, origin.shape[0]))
        if origin.dim() != 2 or origin.shape[1] != n or origin.dtype != torch.int32 or not origin.is_contiguous():
            raise ValueError("device origins must be a contiguous K x n int32 tensor (upload_origins)")
        return cls(weights=horizon_weight_array(weights, int(origin.shape[0])), uploaded=origin)

    def _c_weights(self):
        return (ctypes.c_double * self.horizons)(*self.weights)

    def fits(self):
        return self.horizons is None or self.horizons <= _lib.AHEAD_MAX_HORIZONS

    def _upload(self, n, dev):
        if self.horizons is None:
            return (upload_origin(self.origin, n, dev),)
        return upload_origins(self.origin, n, dev), self.horizons, self._c_weights()


class Window(Loo):
    """Rolling origins with a window: row r predicted from rows lo[r] ... origin[r] - 1 alone (`window_arrays`; or the device pair
    `upload_window` returned).  Nothing is factored whole: no X, no alpha, no factorisation flags, no factor."""

    family, suffix, ws, factored, inverse = "ahead_window", "", _lib.WS_AHEAD_WINDOW, False, False

    def __init__(self, lo=None, origin=None, uploaded=None):
        self.lo, self.origin, self._device, self.args = lo, origin, uploaded, (self, None)
        scored = None if uploaded is not None else origin >= 0
        self.longest = 0 if scored is None or not scored.any() else int((origin - lo)[scored].max())

    @classmethod
    def of(cls, lo, origin, n):
        """The scheme of what `ahead_window_dense[_grad]` take: itself, the device pair `upload_window` returns, or host arrays (checked
        here)."""
        if isinstance(lo, cls):
            return lo
        if _on_device(lo) and _on_device(origin):
            for a in (lo, origin):
                if a.dim() != 1 or a.numel() != n or a.dtype != torch.int32 or not a.is_contiguous():
                    raise ValueError("device lo and origin must be contiguous int32 tensors of n entries (upload_window)")
            return cls(uploaded=(lo, origin))
        return cls(*window_arrays(lo, origin, n))

    def fits(self):
        return self.longest <= _lib.AHEAD_WINDOW_MAX

    def _upload(self, n, dev):
        return upload_window(self.lo, self.origin, n, dev)


def scheme_of(objective, fold_start=None, hold=None, origin=None, weights=None, lo=None):
    """The scheme of a training objective ("loo", "cv", "ahead"; None for "mll") from the keywords that select it - the one place that
    maps them: `fold_start` (with `hold`: purged) belongs to "cv", `origin` (K x n with `weights`; one array with `lo`: a window) to
    "ahead".  The arrays are taken as they are (int64); `device` checks them against the rows when it uploads them."""
    if objective not in ("mll", "loo", "cv", "ahead"):
        raise ValueError('objective must be "mll", "loo", "cv" or "ahead"')
    if (objective == "cv") != (fold_start is not None):
        raise ValueError('fold_start belongs to objective="cv"')
    if (objective == "ahead") != (origin is not None):
        raise ValueError('origin belongs to objective="ahead"')
    if hold is not None and objective != "cv":
        raise ValueError('hold belongs to objective="cv"')
    origin = None if origin is None else np.asarray(origin, dtype=np.int64)
    multi = origin is not None and origin.ndim == 2
    if weights is not None and not multi:
        raise ValueError("weights belong to a K x n origin array")
    if lo is not None and (origin is None or multi):
        raise ValueError("lo belongs to one array of origins")
    if objective == "cv":
        starts = np.asarray(fold_start, dtype=np.int64).reshape(-1)
        return Folds(starts) if hold is None else Purged(starts, *(np.asarray(h, dtype=np.int64).reshape(-1) for h in hold))
    if objective == "ahead":
        if multi:
            return Origins(origin, horizon_weight_array(weights, origin.shape[0]))
        origin = origin.reshape(-1)
        return Origins(origin) if lo is None else Window(np.asarray(lo, dtype=np.int64).reshape(-1), origin)
    return Loo() if objective == "loo" else None
