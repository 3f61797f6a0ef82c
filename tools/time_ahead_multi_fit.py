"""Wall time of fit(iters=20) for p layers of n rows with the log marginal likelihood, the rolling-origin forecast objective at the single
horizons 1, 4 and 16 and the three together in one pass (horizon=(1, 4, 16)) - per fit and per objective evaluation -, then one `ahead()`
call for each of them against one `logpdf()` call: median of five after a warm-up (min, max).

Every (n, leg) runs in a child process of its own under a time limit, one after the other, and the first child that fails or runs out of
time ends the run: nothing is started on the device after a failure.
python tools/time_ahead_multi_fit.py [n:p ...]   (a tree without the multi-horizon objective - an earlier commit on the module path - reports
the single horizons and "mll" alone: the parent-commit column)"""
import inspect
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KW = dict(scale=0.5, linear=True, nonlinear=True, noise=0.1)
LEGS = ["mll", "1", "4", "16", "1,4,16"]
LIMIT = 300   # seconds per child


def timed(call, repeats=6):
    import numpy as np
    import torch

    from gpar_amd import optimise

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
    if evals[-1]:
        text += f" = {float(np.median(ts[1:])) / evals[-1]:.3f} ms x {evals[-1]} evaluations"
    return text


def leg(n, p, name):
    from bench import synthetic
    from gpar_amd.engine import HipEngine, set_engine
    from gpar_amd.regression import GPARRegressor

    set_engine(HipEngine())
    x, y = synthetic(n, 2, p)
    if name == "mll":
        reg = GPARRegressor(**KW)
        print(f"n={n} p={p} mll: fit(iters=20) " + timed(lambda: GPARRegressor(**KW).fit(x, y, iters=20)) + "  logpdf() "
              + timed(lambda: reg.logpdf(x, y)), flush=True)
        return 0
    horizon = tuple(int(h) for h in name.split(",")) if "," in name else int(name)
    if isinstance(horizon, tuple) and "horizon_weights" not in inspect.signature(GPARRegressor.fit).parameters:
        print(f"n={n} p={p} ahead h=({name}): not in this tree", flush=True)
        return 0
    reg = GPARRegressor(**KW)
    print(f"n={n} p={p} ahead h={name}: fit(iters=20) " + timed(lambda: GPARRegressor(**KW).fit(x, y, iters=20, objective="ahead", horizon=horizon))
          + "  ahead() " + timed(lambda: reg.ahead(x, y, horizon=horizon)), flush=True)
    return 0


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--leg":
        return leg(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
    cases = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:]] or [(1024, 4), (4096, 4)]
    for n, p in cases:
        for name in LEGS:
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", str(n), str(p), name], timeout=LIMIT).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(f"n={n} p={p} leg {name} ended with status {rc}: stopping", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
