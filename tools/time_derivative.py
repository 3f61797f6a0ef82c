"""Time of one posterior derivative - `GPAR.derivative` on a conditioned four-output model (smooth, locally periodic, linear and constant
terms over one input; linear and nonlinear terms over the previous outputs), derivative with respect to the input at n* = 2048 test rows,
n = 1024, 4096, 16384 training rows - means only and means plus variances, through the fused library call (gpar_posterior_deriv), against
what was available before it, IN THE SAME RUN, the routes alternating:

  weights  the mean derivative by the input-gradient pass: per layer the n* x n weight matrix 1 alpha^T is WRITTEN and handed to
           `kernel_input_grads` (gpar_gram_input_grad), the result dotted with the direction; the same plug-in chain.  No variances.
  fd       a central difference of the closed-form moments: two `GPAR.moments(x +- h, latent=True)` calls (each forms means AND
           variances of f, none of the derivative).

The factors are computed before the clock starts (a first, untimed round): what is timed is the derivative, not the conditioning.  Host
wall time around a device synchronise, milliseconds; one JSON line per n.

    python tools/time_derivative.py > profiles/derivative_times.txt"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from gpar_amd import GPARRegressor
from gpar_amd.engine import HipEngine, set_engine
from gpar_amd.model import last
from gpar_amd.regression import _construct_gpar

eng = HipEngine(seed=1)
set_engine(eng)
NS, P, REPS, H = 2048, 4, 5, 1e-5
sizes = [int(v) for v in sys.argv[1:]] or [1024, 4096, 16384]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def by_weights(gpar, x):
    """The mean derivative with the written n* x n weights, layer by layer along the plug-in path."""
    U = torch.ones_like(x)
    out = []
    for is_last, model in last(gpar.layers):
        f, _ = model()
        obs = f._obs
        p = f._pts(x)
        alpha = obs.factor().alpha().reshape(-1)
        W = eng.new_matrix(p.n, obs.fdd.n)
        W.copy_(alpha[None, :].expand(p.n, -1))
        dmean = (U * eng.kernel_input_grads(p.ck, x, obs.fdd.x, W)).sum(dim=1)
        out.append(dmean.reshape(-1, 1))
        if not is_last:
            x = torch.cat([x, f.mean(x).reshape(-1, 1)], dim=1)
            U = torch.cat([U, dmean.reshape(-1, 1)], dim=1)
    return torch.cat(out, dim=1)


for n in sizes:
    rng = np.random.default_rng(n)
    x = np.sort(rng.uniform(0, 10, (n, 1)), axis=0)
    base = np.sin(2 * np.pi * x / 0.9) + 0.1 * x
    y = np.concatenate([base * (1 + 0.2 * i) + 0.3 * np.cos(x * (i + 1)) + 0.05 * rng.standard_normal((n, 1)) for i in range(P)], axis=1)
    xs = np.sort(rng.uniform(0, 10, (NS, 1)), axis=0)
    reg = GPARRegressor(normalise_y=False, replace=True, scale=0.5, per=True, per_period=0.9, input_linear=True, linear=True, nonlinear=True)
    with torch.no_grad():
        gpar = _construct_gpar(reg, reg.vs, 1, P) | (eng.tensor(x), eng.tensor(y), torch.ones(n, P, dtype=torch.float64, device=eng.device))
        xt = eng.tensor(xs)
        w = torch.ones(NS, P, dtype=torch.float64, device=eng.device)
        routes = {
            "fused_means_only": lambda: gpar.derivative(xt, 0, variance=False)[0],
            "fused_means_and_variances": lambda: gpar.derivative(xt, 0, variance=True)[0],
            "weights_means_only": lambda: by_weights(gpar, xt),
            "fd_two_moments_calls": lambda: (gpar.moments(xt + H, w, latent=True)[0] - gpar.moments(xt - H, w, latent=True)[0]) / (2 * H),
        }
        ms = {k: [] for k in routes}
        results = {}
        for rep in range(REPS + 1):   # (the first round factors the layers / loads the kernels and is not reported)
            for key, fn in routes.items():
                t, results[key] = timed(fn)
                if rep:
                    ms[key].append(t)
        out = {"n": n, "n_star": NS, "outputs": P, "reps": REPS}
        for key in routes:
            out[key] = {"ms": ms[key], "ms_median": float(np.median(ms[key]))}
        ref = results["fused_means_only"]
        scale = float(ref.abs().max())
        out["max_difference_relative_to_largest_derivative"] = {
            "weights": float((results["weights_means_only"] - ref).abs().max()) / scale,
            "fd": float((results["fd_two_moments_calls"] - ref).abs().max()) / scale,
        }
    print(json.dumps(out), flush=True)
    del gpar, results, routes
    torch.cuda.empty_cache()
