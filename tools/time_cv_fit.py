"""Wall time of fit(iters=20) for p layers of n rows with the log marginal likelihood, the leave-one-out and the blocked cross-validation
objective (contiguous folds of 16 rows), all in one process: median of five fits after a warm-up fit per objective.
python tools/time_cv_fit.py [n:p ...]   (a tree without one of the objectives - an earlier commit on the module path - reports the others)"""
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

FOLD = 16


def main():
    eng = HipEngine()
    set_engine(eng)
    cases = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:]] or [(1024, 4), (4096, 4)]
    params = inspect.signature(GPARRegressor.fit).parameters
    objectives = ["mll"] + (["loo"] if "objective" in params else []) + (["cv"] if "folds" in params else [])
    for n, p in cases:
        x, y = synthetic(n, 2, p)
        line = [f"n={n} p={p} fit(iters=20):"]
        for objective in objectives:
            kw = {"objective": objective} if objective != "mll" else {}
            if objective == "cv":
                kw["folds"] = np.arange(n) // FOLD
            ts = []
            for i in range(6):
                reg = GPARRegressor(scale=0.5, linear=True, nonlinear=True, noise=0.1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                reg.fit(x, y, iters=20, **kw)
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            line.append(f"{objective} {float(np.median(ts[1:])):.1f} ms (min {min(ts[1:]):.1f}, max {max(ts[1:]):.1f})")
        print("  ".join(line), flush=True)


if __name__ == "__main__":
    main()
