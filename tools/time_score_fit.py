"""Wall time of fit(iters=20) for p layers of n rows with the leave-one-out objective and the rolling-origin forecast objective (horizons 1
and 16) under each scoring rule - "log", "crps", "se" - next to the log marginal likelihood, all in one process: median of five fits after
a warm-up fit per leg, with the objective-and-gradient evaluations one fit makes (L-BFGS-B takes another path under another rule: a ratio
of times is a ratio of kernel cost only where the evaluations agree; the time per evaluation is printed for that).
python tools/time_score_fit.py [n:p ...]   (a tree without the `score` keyword - an earlier commit on the module path - reports the "mll" and
"log" legs alone)"""
import inspect
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import synthetic
from gpar_amd import optimise
from gpar_amd.engine import HipEngine, set_engine
from gpar_amd.regression import GPARRegressor

KW = dict(scale=0.5, linear=True, nonlinear=True, noise=0.1)


def timed(call, repeats=6):
    ts, evals = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        before = optimise.evaluation_count()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
        evals.append(optimise.evaluation_count() - before)
    med = float(np.median(ts[1:]))
    return f"{med:.1f} ms (min {min(ts[1:]):.1f}, max {max(ts[1:]):.1f}; {evals[-1]} evaluations, {med / max(evals[-1], 1):.2f} ms each)"


def main():
    set_engine(HipEngine())
    cases = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:]] or [(1024, 4), (4096, 4)]
    rules = ("log", "crps", "se") if "score" in inspect.signature(GPARRegressor.fit).parameters else ("log",)
    for n, p in cases:
        x, y = synthetic(n, 2, p)
        print(f"n={n} p={p} fit(iters=20):", flush=True)
        print("  mll " + timed(lambda: GPARRegressor(**KW).fit(x, y, iters=20)), flush=True)
        for label, kw in (("loo", {"objective": "loo"}), ("ahead h=1", {"objective": "ahead", "horizon": 1}),
                          ("ahead h=16", {"objective": "ahead", "horizon": 16})):
            for rule in rules:
                extra = {} if rule == "log" else {"score": rule}
                print(f"  {label} {rule} " + timed(lambda: GPARRegressor(**KW).fit(x, y, iters=20, **kw, **extra)), flush=True)


if __name__ == "__main__":
    main()
