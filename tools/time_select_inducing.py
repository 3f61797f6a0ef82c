"""Wall time of the greedy inducing-point selection on one GPU: the fused call (gpar_pivoted_chol through HipEngine.pivoted_cholesky)
and the route composed of the engine's primitives (gp._pivoted_cholesky_composed: gpar_gram_diag, gpar_gram against the pivot's row,
torch for the update and the argmax, a host synchronisation per pivot), in one process.

    python tools/time_select_inducing.py [n:M ...] [--out FILE]        (default: 4096:256 65536:1024)

Inputs: m = 4 columns drawn uniformly from [0, 1) as bench.py draws them; kernel: the first layer of GPARRegressor(scale=0.5, linear=True,
nonlinear=True, noise=0.1) - C4's keywords.  Per size and route: one warm-up run, then five timed runs, each ending in a device
synchronisation; median (min, max).  The two routes' pivots are compared on the way.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpar_amd.engine import HipEngine, set_engine  # noqa: E402
from gpar_amd.gp import _pivoted_cholesky_composed  # noqa: E402
from gpar_amd.regression import GPARRegressor, _model_generator  # noqa: E402


def _time(fn, device, runs=5):
    fn()   # warm-up
    torch.cuda.synchronize(device)
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(device)
        times.append(1e3 * (time.perf_counter() - t0))
    return out, float(np.median(times)), min(times), max(times)


def main(argv):
    out_path = None
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
        argv = [a for i, a in enumerate(argv) if a != "--out" and (i == 0 or argv[i - 1] != "--out")]
    sizes = [tuple(int(v) for v in a.split(":")) for a in argv] or [(4096, 256), (65536, 1024)]
    eng = HipEngine()
    set_engine(eng)
    reg = GPARRegressor(scale=0.5, linear=True, nonlinear=True, noise=0.1)
    lines = ["tools/time_select_inducing.py on one MI355X: wall time of one selection, median of five runs after a warm-up (min, max); m = 4,",
             "uniform inputs, first-layer kernel of GPARRegressor(scale=0.5, linear=True, nonlinear=True, noise=0.1), tol = 0, floor = 1e-12."]
    for n, M in sizes:
        x = eng.tensor(np.random.default_rng(0).uniform(0, 1, (n, 4)))
        with torch.no_grad():
            ck = eng.compile(_model_generator(reg.vs, 4, 0, **reg.model_config)()[0].kernel, 4)
        z = eng.features(ck, x)
        with eng.defer_checks():
            fused, tf, tf_lo, tf_hi = _time(lambda: eng.pivoted_cholesky(ck, z, M), eng.device)
        composed, tc, tc_lo, tc_hi = _time(lambda: _pivoted_cholesky_composed(eng, ck, z, M, 0.0, eng.epsilon), eng.device)
        rank_f, rank_c = int(fused[3].item()), int(composed[3].item())
        same = int((fused[1] == composed[1]).sum().item())
        traffic = 8.0 * n * rank_f * rank_f / 2.0
        lines.append(f"n={n} M={M}:  fused {tf:.2f} ms (min {tf_lo:.2f}, max {tf_hi:.2f})  composed {tc:.1f} ms (min {tc_lo:.1f}, max {tc_hi:.1f})  "
                     f"rank {rank_f} / {rank_c}, {same} of {M} pivots equal, residual trace {float(fused[2][rank_f]):.4g} of {float(fused[2][0]):.4g}; "
                     f"factor traffic 8 n rank^2 / 2 = {traffic / 1e9:.2f} GB -> {traffic / 1e9 / tf:.2f} TB/s over the fused time")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
