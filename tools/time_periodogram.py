"""Time of one `GPARRegressor.periodogram` call - host arrays in, host arrays out, on the default grid (about 2.5 n frequencies) - at
n = 4096 and n = 16384 irregular rows, p = 4 outputs with a tenth of one output missing, against the numpy restatement of
tests/test_periodogram.py on the host IN THE SAME RUN (float64, torch's thread count - 16 where the tool was run - set for numpy's BLAS
as well; its sines and cosines are numpy's own, one thread).  Host wall time around the call, which ends with the copy of the powers to
the host; the first device call is not reported.  Not measured: the kernel alone by a profiler, other p.  One JSON line per n.

    python tools/time_periodogram.py > profiles/periodogram_times.txt"""
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from gpar_amd import GPARRegressor
from gpar_amd.engine import HipEngine, set_engine
from gpar_amd.spectrum import periodogram_inputs
from tests.test_periodogram import gls

set_engine(HipEngine(seed=1))
P, REPS = 4, 5
sizes = [int(v) for v in sys.argv[1:]] or [4096, 16384]
reg = GPARRegressor()
for n in sizes:
    rng = np.random.default_rng(n)
    x = np.sort(rng.uniform(0, 100, n))
    y = np.stack([np.sin(2 * np.pi * x / (0.9 + 0.4 * j)) + 0.3 * rng.standard_normal(n) for j in range(P)], axis=1)
    y[rng.uniform(size=n) < 0.1, P - 1] = np.nan
    reg.periodogram(x, y)   # (loads the library, creates the context)
    device_ms = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pg = reg.periodogram(x, y)
        device_ms.append((time.perf_counter() - t0) * 1e3)
    t, yy, omega = periodogram_inputs(x, y)
    t0 = time.perf_counter()
    # (in blocks of frequencies: the restatement holds a rows x frequencies matrix at a time)
    host = np.concatenate([gls(t, t.min(), yy, omega, pg.freq[k : k + 2048]) for k in range(0, pg.freq.size, 2048)], axis=1)
    host_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"n": n, "outputs": P, "frequencies": int(pg.freq.size), "reps": REPS, "device_call_ms": device_ms,
                      "device_call_ms_median": float(np.median(device_ms)), "numpy_restatement_ms": host_ms, "numpy_threads": torch.get_num_threads(),
                      "max_abs_difference": float(np.max(np.abs(host - pg.power)))}), flush=True)
