"""Time of `GPARRegressor.predict(num_samples=100)` with the exact sampler against `sampler="pathwise"` (features = 2048), nonlinear output
dependence (every sample has a design matrix of its own from the second layer on), on one MI355X in ONE run:

    n = 2000,  m = 2, p = 4, n* = 1000        exact and pathwise
    n = 16384, m = 4, p = 8, n* = 2048        exact and pathwise (the C3 bench shape)
    the first shape at n* = 65536             pathwise alone (the exact sampler has no route for an n* x n* covariance of that size)

Host wall time around the call, which ends with the results on the host; conditioning (the factorisations) is done before and is not
in the figures; the first call of every leg is not reported.  Not measured: kernel times by a profiler, other `features`.  One JSON line
per leg.

    python tools/time_pathwise.py > profiles/pathwise_times.txt"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from gpar_amd import GPARRegressor
from gpar_amd.engine import HipEngine, set_engine

set_engine(HipEngine(seed=1))
S, FEATURES = 100, 2048


def problem(n, m, p, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n, m))
    cols = []
    for i in range(p):
        base = np.sin(2 * np.pi * (x @ rng.uniform(0.5, 1.5, m)) + i)
        if cols:
            base = base + 0.5 * cols[-1] ** 2
        cols.append(base + 0.1 * rng.standard_normal(n))
    y = np.stack(cols, axis=1)
    return x, (y - y.mean(0)) / y.std(0)


def leg(reg, xs, sampler, reps):
    kw = dict(sampler="pathwise", features=FEATURES) if sampler == "pathwise" else {}
    reg.predict(xs, num_samples=S, **kw)   # (not reported: first use of the kernels at this shape)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reg.predict(xs, num_samples=S, **kw)
        times.append(time.perf_counter() - t0)
    return times


for n, m, p, ns, samplers, reps in ((2000, 2, 4, 1000, ("exact", "pathwise"), 3), (16384, 4, 8, 2048, ("exact", "pathwise"), 2),
                                    (2000, 2, 4, 65536, ("pathwise",), 2)):
    x, y = problem(n, m, p, seed=n)
    xs = np.random.default_rng(1).uniform(0, 1, (ns, m))
    reg = GPARRegressor(scale=0.5, linear=True, nonlinear=True, noise=0.1)
    reg.condition(x, y)
    for sampler in samplers:
        times = leg(reg, xs, sampler, reps)
        print(json.dumps({"n": n, "m": m, "p": p, "n_star": ns, "samples": S, "sampler": sampler, "features": FEATURES if sampler == "pathwise" else None,
                          "predict_s": times, "predict_s_median": float(np.median(times))}), flush=True)
