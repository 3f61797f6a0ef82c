"""Wall time of fit(iters=20) for p layers of n rows with the log marginal likelihood and with the rolling-origin forecast objective at
horizons 1, 16 and n, all in one process: median of five fits after a warm-up fit per objective; then one `ahead()` call against one
`logpdf()` call (median of five after a warm-up call).
python tools/time_ahead_fit.py [n:p ...]   (a tree without the objective - an earlier commit on the module path - reports "mll" alone)"""
import inspect
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import synthetic
from gpar_amd.engine import HipEngine, set_engine
from gpar_amd.regression import GPARRegressor

KW = dict(scale=0.5, linear=True, nonlinear=True, noise=0.1)


def timed(call, repeats=6):
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return f"{float(np.median(ts[1:])):.1f} ms (min {min(ts[1:]):.1f}, max {max(ts[1:]):.1f})"


def main():
    set_engine(HipEngine())
    cases = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:]] or [(1024, 4), (4096, 4)]
    has_ahead = "horizon" in inspect.signature(GPARRegressor.fit).parameters
    for n, p in cases:
        x, y = synthetic(n, 2, p)
        legs = [("mll", {})] + ([(f"ahead h={h}", {"objective": "ahead", "horizon": h}) for h in (1, 16, n)] if has_ahead else [])
        line = [f"n={n} p={p} fit(iters=20):"]
        for label, kw in legs:
            line.append(f"{label} " + timed(lambda: GPARRegressor(**KW).fit(x, y, iters=20, **kw)))
        print("  ".join(line), flush=True)
        reg = GPARRegressor(**KW)
        line = [f"n={n} p={p} one call:", "logpdf " + timed(lambda: reg.logpdf(x, y))]
        if has_ahead:
            line += [f"ahead h={h} " + timed(lambda: reg.ahead(x, y, horizon=h)) for h in (1, 16, n)]
        print("  ".join(line), flush=True)


if __name__ == "__main__":
    main()
