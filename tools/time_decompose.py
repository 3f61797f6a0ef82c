"""Time of one decomposition by kernel component - `GPAR.decompose` on a conditioned four-output model with six kernel terms (smooth,
locally periodic, linear and constant over the inputs; linear and nonlinear over the previous outputs; layer 0 has the first four), one
component per term - through the fused library call (gpar_posterior_terms) against the composed route (GPAR_FUSED_TERMS=0: one
sub-kernel, Gram matrix, product and solve per component), IN THE SAME RUN, the two alternating.  n = 1024, 4096, 16384 training rows,
n* = 2048 test rows; means only, and means plus variances.  The factors are computed before the clock starts (a first, untimed call):
what is timed is the decomposition, not the conditioning.  Host wall time around a device synchronise, milliseconds; one JSON line per n.

    python tools/time_decompose.py > profiles/decompose_times.txt"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from gpar_amd import GPARRegressor
from gpar_amd.engine import HipEngine, set_engine
from gpar_amd.regression import _construct_gpar, _group_terms

eng = HipEngine(seed=1)
set_engine(eng)
NS, P, REPS = 2048, 4, 5
sizes = [int(v) for v in sys.argv[1:]] or [1024, 4096, 16384]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for n in sizes:
    rng = np.random.default_rng(n)
    x = np.sort(rng.uniform(0, 10, (n, 1)), axis=0)
    base = np.sin(2 * np.pi * x / 0.9) + 0.1 * x
    y = np.concatenate([base * (1 + 0.2 * i) + 0.3 * np.cos(x * (i + 1)) + 0.05 * rng.standard_normal((n, 1)) for i in range(P)], axis=1)
    xs = np.sort(rng.uniform(0, 10, (NS, 1)), axis=0)
    reg = GPARRegressor(normalise_y=False, scale=0.5, per=True, per_period=0.9, input_linear=True, linear=True, nonlinear=True)
    with torch.no_grad():
        gpar = _construct_gpar(reg, reg.vs, 1, P) | (eng.tensor(x), eng.tensor(y), torch.ones(n, P, dtype=torch.float64, device=eng.device))
        comps = []
        for model in gpar.layers:
            names, comp = _group_terms([t.label for t in model()[0].kernel.terms], None)
            comps.append((comp, len(names)))
        xt = eng.tensor(xs)
        out = {"n": n, "n_star": NS, "outputs": P, "components_per_layer": [c[1] for c in comps], "reps": REPS}
        results = {}
        for variance in (False, True):
            ms = {"1": [], "0": []}
            for rep in range(REPS + 1):   # (the first round factors the layers / loads the kernels and is not reported)
                for switch in ("1", "0"):
                    os.environ["GPAR_FUSED_TERMS"] = switch
                    t = timed(lambda: results.__setitem__((switch, variance), gpar.decompose(xt, comps, variance=variance)))
                    if rep:
                        ms[switch].append(t)
            key = "means_and_variances" if variance else "means_only"
            out[key] = {"fused_ms": ms["1"], "composed_ms": ms["0"], "fused_ms_median": float(np.median(ms["1"])),
                        "composed_ms_median": float(np.median(ms["0"]))}
        # the two routes agree (largest difference over layers and components, relative to the largest value)
        diff = {}
        for variance, which in ((True, 0), (True, 1)):
            a, b = results[("1", variance)], results[("0", variance)]
            diff["mean" if which == 0 else "var"] = max(
                float((la[which] - lb[which]).abs().max() / lb[which].abs().max().clamp(min=1e-300)) for la, lb in zip(a, b))
        out["max_relative_difference"] = diff
    print(json.dumps(out), flush=True)
    del gpar, results
    torch.cuda.empty_cache()
