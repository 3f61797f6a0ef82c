"""Wall time per layer of one step of a sliding window - `update(drop=k, k new rows)` followed by `predict(num_samples=1)` - against the
route without kept factors: `condition` on the moved window followed by the same call; then the same for a GROWING window
(`update(k new rows)`, nothing forgotten), whose steps need no rank-k update.  One layer (p = 1), n rows, 64 test points; the
two routes alternate in one process, median of five steps after a warm-up step each; every step ends in a device synchronisation.
GPAR_UPDATE_DROP_FRACTION=1 holds `update` to its incremental route at every k, so that the crossover can be read off the table.
python tools/time_update.py [n:k ...]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPAR_UPDATE_DROP_FRACTION", "1")
import numpy as np
import torch

from bench import synthetic
from gpar_amd.engine import HipEngine, set_engine
from gpar_amd.regression import GPARRegressor

STEPS = 6


def main():
    set_engine(HipEngine())
    cases = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:]] or [(n, k) for n in (1024, 4096, 16384) for k in (1, 16, 64, 256)]
    for n, k in cases:
        x, y = synthetic(n + (STEPS + 1) * k + 64, 2, 1)
        x, y = np.asarray(x), np.asarray(y)
        xs = x[-64:]
        for drop, what in ((k, "slide"), (0, "grow")):
            step_times(n, k, drop, what, x, y, xs)


def step_times(n, k, drop, what, x, y, xs):
    kept = GPARRegressor(scale=0.5, linear=True, nonlinear=True, noise=0.1, normalise_y=False)
    kept.condition(x[:n], y[:n])
    kept.update(x[n:n + k], y[n:n + k], drop=drop)   # the first update conditions in full and keeps the factors
    again = GPARRegressor(scale=0.5, linear=True, nonlinear=True, noise=0.1, normalise_y=False)
    t_kept, t_again = [], []
    for step in range(1, STEPS + 1):
        lo, hi = (step * k if drop else -k), n + step * k
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kept.update(x[hi:hi + k], y[hi:hi + k], drop=drop)
        kept.predict(xs, num_samples=1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        again.condition(x[lo + k:hi + k], y[lo + k:hi + k])
        again.predict(xs, num_samples=1)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert kept.last_update_incremental_
        t_kept.append(1e3 * (t1 - t0))
        t_again.append(1e3 * (t2 - t1))
    a, b = float(np.median(t_kept[1:])), float(np.median(t_again[1:]))
    print(f"n={n} k={k} {what}: update+predict {a:.2f} ms (min {min(t_kept[1:]):.2f}, max {max(t_kept[1:]):.2f})  "
          f"condition+predict {b:.2f} ms (min {min(t_again[1:]):.2f}, max {max(t_again[1:]):.2f})  ratio {a / b:.2f}", flush=True)


if __name__ == "__main__":
    main()
