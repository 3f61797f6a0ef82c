"""Wall time of fit(iters=20) for p layers of n rows with the blocked cross-validation objective over folds of 16 rows, purged by
gap = 0 (`cv` as it was: the yardstick, measured in the same run), 4 and 24 rows: median of five fits after a warm-up fit per gap, with
the number of objective evaluations the prepared route made in the last fit and the time per evaluation beside it (fit times differ
mostly by the path L-BFGS-B takes); then one `cv(gap=)` call per gap (median of five after a warm-up call).
python tools/time_cv_gap_fit.py [n:p ...]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import synthetic
from gpar_amd import fastfit
from gpar_amd.engine import HipEngine, set_engine
from gpar_amd.regression import GPARRegressor

KW = dict(scale=0.5, linear=True, nonlinear=True, noise=0.1)
FOLD = 16
GAPS = (0, 4, 24)


def timed(call, repeats=6):
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])


def main():
    set_engine(HipEngine())
    cases = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:]] or [(1024, 4), (4096, 4)]
    built = []
    real_build = fastfit.build

    def build(*args, **kwargs):
        built.append(real_build(*args, **kwargs))
        return built[-1]

    fastfit.build = build
    for n, p in cases:
        x, y = synthetic(n, 2, p)
        folds = np.arange(n) // FOLD
        per_eval = {}
        for gap in GAPS:
            kw = {"gap": gap} if gap else {}   # (gap = 0 without the keyword: the call as it was)
            med, lo, hi = timed(lambda: (built.clear(), GPARRegressor(**KW).fit(x, y, iters=20, objective="cv", folds=folds, **kw)))
            evals = sum(b.evaluations for b in built if b is not None)
            per_eval[gap] = med / max(evals, 1)
            print(f"n={n} p={p} fit(iters=20) cv folds of {FOLD} gap={gap}: {med:.1f} ms (min {lo:.1f}, max {hi:.1f})  {evals} evaluations "
                  f"({sum(b is None for b in built)} layers off the prepared route)  {per_eval[gap]:.3f} ms per evaluation "
                  f"({per_eval[gap] / per_eval[0]:.2f} x gap=0)", flush=True)
        reg = GPARRegressor(**KW)
        line = [f"n={n} p={p} one call:"]
        base = None
        for gap in GAPS:
            kw = {"gap": gap} if gap else {}
            med, lo, hi = timed(lambda: reg.cv(x, y, folds=folds, **kw))
            base = med if base is None else base
            line.append(f"cv gap={gap} {med:.1f} ms (min {lo:.1f}, max {hi:.1f}; {med / base:.2f} x gap=0)")
        print("  ".join(line), flush=True)


if __name__ == "__main__":
    main()
