"""Time of the hyperparameter-uncertainty calls on the four-output six-term model of tools/time_derivative.py (smooth, locally periodic,
linear and constant terms over one input; linear and nonlinear terms over the previous outputs; replace=True) at n* = 2048 test rows and
n = 1024, 4096, 16384 training rows, IN ONE RUN:

  a  hyper      `predict_moments_hyper(xs, hp)` given `hp`: `predict_moments`, the layers' chain-rule matrices, per layer two
                gpar_gram_grad_rows passes, two triangular solves, one gpar_gram_apply_groups, the cross-layer chain rule, J Sigma J^T.
  b  laplace    `laplace(x, y)`: per layer 2 P evaluations of the analytic gradient - of the prepared objective up to
                `one_call_grad_rows()` rows (n = 1024, 4096), of the general route's back-propagated gradient above (n = 16384).
  c  composed   the Jacobian the way it could be had before: a central difference of `predict_moments(xs, latent=True)` over every
                variable, re-conditioning 2 P times.  At n = 16384 over the variables of layer 0 ONLY (the line says so: `composed_layers`).

The values are the initial ones (nothing is trained: the clock is on the calls, and the Hessian there need not be positive definite - the
flat-direction warning is silenced).  Host wall time around a device synchronise, milliseconds; the first round of (a) is a warm-up and
is not reported, (b) and (c) are run once after it.  One JSON line per n.

    python tools/time_laplace.py > profiles/laplace_times.txt"""
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from gpar_amd import GPARRegressor
from gpar_amd.engine import HipEngine, set_engine

eng = HipEngine(seed=1)
set_engine(eng)
NS, P, REPS, H = 2048, 4, 3, 1e-5
sizes = [int(v) for v in sys.argv[1:]] or [1024, 4096, 16384]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def composed(reg, xs, names):
    """d predict_moments(latent=True) means / d u by central differences: n* x p x len(names)."""
    u0 = reg.vs.get_vector(names)
    out = np.zeros((xs.shape[0], reg.p, u0.size))
    for k in range(u0.size):
        for sign in (1.0, -1.0):
            u = u0.copy()
            u[k] += sign * H
            reg.vs.set_vector(u, names)
            out[:, :, k] += sign * reg.predict_moments(xs, latent=True)[0] / (2 * H)
    reg.vs.set_vector(u0, names)
    return out


for n in sizes:
    rng = np.random.default_rng(n)
    x = np.sort(rng.uniform(0, 10, (n, 1)), axis=0)
    base = np.sin(2 * np.pi * x / 0.9) + 0.1 * x
    y = np.concatenate([base * (1 + 0.2 * i) + 0.3 * np.cos(x * (i + 1)) + 0.05 * rng.standard_normal((n, 1)) for i in range(P)], axis=1)
    xs = np.sort(rng.uniform(0, 10, (NS, 1)), axis=0)
    reg = GPARRegressor(normalise_y=False, replace=True, scale=0.5, per=True, per_period=0.9, input_linear=True, linear=True, nonlinear=True)
    reg.condition(x, y)
    out = {"n": n, "n_star": NS, "outputs": P}
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t_laplace, hp = timed(lambda: reg.laplace(x, y))
        out["variables"] = int(hp.cov.shape[0])
        out["laplace_ms"] = t_laplace
        ms = []
        for rep in range(REPS + 1):
            t, got = timed(lambda: reg.predict_moments_hyper(xs, hp, latent=True))
            if rep:
                ms.append(t)
        out["hyper"] = {"ms": ms, "ms_median": float(np.median(ms))}
        layers = 1 if n >= 16384 else P
        names = [name for name in hp.names if int(name.split("/")[0]) < layers]
        t_composed, jac = timed(lambda: composed(reg, xs, names))
        out["composed_layers"] = layers
        out["composed_variables"] = int(jac.shape[2])
        out["composed_ms"] = t_composed
        out["composed_ms_per_variable"] = t_composed / max(int(jac.shape[2]), 1)
    except (ValueError, NotImplementedError) as e:   # (a size the prepared objective does not take: said, not hidden)
        out["not_measured"] = str(e)
    print(json.dumps(out), flush=True)
    del reg
    torch.cuda.empty_cache()
