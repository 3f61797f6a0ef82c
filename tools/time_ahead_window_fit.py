"""Wall time of fit(iters=20) for p layers of n rows with the log marginal likelihood, the expanding rolling-origin objective at horizon 1
and the sliding-window objective at horizon 1 with windows of 16 and 64 rows, all in one process: median of five fits after a warm-up fit
per objective, the objective evaluations of a fit (summed over the layers) and the time per evaluation - the L-BFGS-B paths of the
objectives differ, so the fits do not make the same number of them; then one `ahead(window=)` call against one `ahead()` call (median of
five after a warm-up call).
python tools/time_ahead_window_fit.py [n:p ...]   (a tree without `window` - an earlier commit on the module path - reports "mll" and "ahead" alone)"""
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
WINDOWS = (16, 64)


def timed(call, repeats=6, per_evaluation=False):
    ts, evals = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        before = optimise.evaluation_count()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
        evals.append(optimise.evaluation_count() - before)
    text = f"{float(np.median(ts[1:])):.1f} ms (min {min(ts[1:]):.1f}, max {max(ts[1:]):.1f})"
    if per_evaluation:
        k = int(np.argsort(ts[1:])[len(ts[1:]) // 2]) + 1   # (the median fit's own count)
        text += f" [{evals[k]} evaluations, {ts[k] / max(evals[k], 1):.3f} ms each]"
    return text


def main():
    set_engine(HipEngine())
    cases = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:]] or [(1024, 4), (4096, 4)]
    has_window = "window" in inspect.signature(GPARRegressor.fit).parameters
    for n, p in cases:
        x, y = synthetic(n, 2, p)
        legs = [("mll", {}), ("ahead h=1", {"objective": "ahead", "horizon": 1})]
        if has_window:
            legs += [(f"window {w} h=1", {"objective": "ahead", "horizon": 1, "window": w}) for w in WINDOWS]
        print(f"n={n} p={p} fit(iters=20):", flush=True)
        for label, kw in legs:
            print(f"  {label}  " + timed(lambda: GPARRegressor(**KW).fit(x, y, iters=20, **kw), per_evaluation=True), flush=True)
        reg = GPARRegressor(**KW)
        line = [f"n={n} p={p} one call:", "ahead h=1 " + timed(lambda: reg.ahead(x, y, horizon=1))]
        if has_window:
            line += [f"window {w} h=1 " + timed(lambda: reg.ahead(x, y, horizon=1, window=w)) for w in WINDOWS]
        print("  ".join(line), flush=True)


if __name__ == "__main__":
    main()
