"""Cost of the spectral-mixture components against the default EQ structure at n = 4096, m = 1, one output: the Gram build of
the layer kernel (lower triangle, as `logpdf` builds it; event-timed back-to-back launches as in tools/time_gram_configs.py) and
a warm `fit(iters=10)` (wall time divided by the objective evaluations it made is not separated: the whole call is reported).
One JSON line per structure: default EQ, spectral=2, spectral=4.

    python tools/time_spectral.py > profiles/spectral_gram_configs.jsonl"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from gpar_amd import GPARRegressor, hip
from gpar_amd.engine import HipEngine, set_engine
from gpar_amd.kernels import compile_kernel
from gpar_amd.regression import _construct_gpar

eng = HipEngine(seed=1)
set_engine(eng)
n = 4096
rng = np.random.default_rng(0)
x = np.sort(rng.uniform(0, 10, (n, 1)), axis=0)
y = np.sin(2 * np.pi * x / 0.9) + 0.3 * np.sin(2 * np.pi * x / 0.31) + 0.05 * rng.standard_normal((n, 1))


def timeit(fn, reps=120):
    fn()
    torch.cuda.synchronize()
    time.sleep(0.2)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]
    return {"burst": float(np.mean(ms[1:6])), "sustained": float(np.mean(ms[-20:])), "best": float(min(ms)), "spread": float(np.std(ms[-20:]))}


for Q in (None, 2, 4):
    kw = dict(normalise_y=False, scale=0.5) if Q is None else dict(normalise_y=False, scale=0.5, spectral=Q, spectral_period=0.9)
    reg = GPARRegressor(**kw)
    with torch.no_grad():
        f, _ = _construct_gpar(reg, reg.vs, 1, 1).layers[0]()
    ck = compile_kernel(f.kernel, 1)
    xt = eng.tensor(x)
    z = hip.featurize(ck, xt)
    K = hip.alloc_matrix(n + 1, n + 1, eng.device)[:n, :n]
    d = torch.full((n,), 0.1, dtype=torch.float64, device=eng.device)
    gram = timeit(lambda: hip.gram(ck, z, None, out=K, lower=True, diag_add=d, diag_const=1e-12))
    fits = []
    for rep in range(3):   # the first call compiles / loads kernels and is not reported
        r = GPARRegressor(**kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.fit(x, y, iters=10)
        torch.cuda.synchronize()
        fits.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"n": n, "m": 1, "spectral": Q, "feature_dims": int(ck.dz), "terms": [[fa.type for fa in t.factors] for t in ck.kernel.terms],
                      "gram_ms": gram["sustained"], "gram_ms_burst": gram["burst"], "gram_ms_best": gram["best"], "gram_ms_spread": gram["spread"],
                      "fit_iters10_ms_first": fits[0], "fit_iters10_ms_warm": fits[1:]}), flush=True)
