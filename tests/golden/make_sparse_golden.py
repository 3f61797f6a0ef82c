"""Writes tests/golden/sparse_cases.json: the inducing-point layer (gp.PseudoObs: VFE, FITC, DTC) pinned to 50-digit arithmetic.

Run by hand (`python tests/golden/make_sparse_golden.py`, a few minutes on eight cores), never by a test.  Per case the file holds the
inputs, cond(K_zz + eps I), and per method the truth of oracle/mp_ref.py rounded to float64 - bound, posterior mean and full covariance at
xs, derivatives of the bound - beside the YARDSTICK: the error of the fp64 numpy oracle against that truth on the same problem
(`gp_ref.Process.vfe_bound` / `condition_sparse` for values and moments, the oracle engine through gp.py for gradients), one max-abs
figure per quantity.  tests/test_sparse_precision_gpu.py holds the HIP engine to a multiple of it.  `engine_error` is the error of the
oracle ENGINE through gp.PseudoObs for every quantity (for the gradients it IS the yardstick): what tests/test_sparse_precision.py
reproduces to show that the file is not stale.

Shapes: the smallest at which the device routes change behaviour - below a 64-wide panel / tile, straddling it, straddling 128.  `dims`
counts the input columns; the design matrix carries one fed-forward output column more, because the kernel is the regressor's layer
kernel of layer 1, var * EQ(inputs) + Linear(previous output) (gpar_ref.layer_spec).  Every case comes with two inducing sets:
  well   a jittered grid spaced at more than a length scale: cond(K_zz + eps I) <= 1e6, where the oracle itself is good to <= 1e-11
         (asserted below) and the comparison has teeth;
  used   uniform random inducing inputs under length scales of half the box, as the workloads have them: cond ~ 1e9 or worse.
Conditions are met by choosing inputs, never by editing a bound."""
import json
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import gp_ref, gpar_ref, mp_ref  # noqa: E402
from oracle import kernels as ok  # noqa: E402
from tests import sparse_precision_support as sp  # noqa: E402

EPS = 1e-12
NS = 5   # posterior inputs


def _hypers(m, scale, kind, rng):
    h = {"1/input/var": float(rng.uniform(0.8, 1.6)), "1/input/scales": list(scale * rng.uniform(0.9, 1.1, m)),
         "1/output/lin/scales": [float(rng.uniform(2.0, 3.0))], "1/noise": 0.0}
    config = dict(linear=True, nonlinear=False)
    if kind == "matern52":
        config["matern"] = 2.5
    if kind == "spectral":
        config["spectral"] = 1
        h.update({"1/input/sm0/var": float(rng.uniform(0.3, 0.6)), "1/input/sm0/scales": list(1.5 * scale * rng.uniform(0.9, 1.1, m)),
                  "1/input/sm0/pers": list(4.0 * scale * rng.uniform(0.9, 1.1, m))})
    return gpar_ref.layer_spec(h, m, 1, config)[0]


def _grid(M, m, lo, hi, rng):
    side = int(np.ceil(M ** (1.0 / m)))
    axes = [np.linspace(lo, hi, side)] * m
    pts = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, m)[:M]
    return pts + rng.uniform(-0.05, 0.05, pts.shape) * (hi - lo) / max(side - 1, 1), (hi - lo) / max(side - 1, 1)


def make_inputs(name, n, M, m, kind, which, vector_noise, coincide, derivatives, seed):
    rng = np.random.default_rng(seed)
    coincide = coincide if which == "used" else 0   # (the well-conditioned sets stay free of outliers: they are the sharp half)
    lo, hi = (-2.0, 2.0) if n == 30 else (0.0, 1.0)
    if which == "well":
        zin, spacing = _grid(M, m, lo, hi, rng)
        scale = 0.75 * spacing
    else:
        zin = rng.uniform(lo, hi, (M, m))
        scale = 0.5 * (hi - lo)
    spec = _hypers(m, scale, kind, rng)
    feed = lambda k: rng.standard_normal((k, 1))
    z = np.concatenate([zin, feed(M)], axis=1)
    x = np.concatenate([rng.uniform(lo, hi, (n, m)), feed(n)], axis=1)
    z = np.round(z, 6)
    if coincide:
        # training inputs that ARE inducing inputs, with an outlying fed-forward value: k_aa - q_aa is eps-sized there (<= 1e-12) while
        # k_aa ~ 3e3 rounds at ~1e-12, so that the sign FITC's clamp sees is decided by rounding - some of these points clamp, some do not
        z[1:2 * coincide:2, -1] = 150.0 * rng.choice([-1.0, 1.0], coincide) * rng.uniform(0.8, 1.2, coincide)
        x[:coincide] = z[1:2 * coincide:2]
    xs = np.concatenate([rng.uniform(lo, hi, (NS, m)), feed(NS)], axis=1)
    y = np.sin(3.0 * x[:, 0] / (hi - lo) * 2.0) + 0.3 * x[:, -1] + 0.1 * rng.standard_normal(n)
    noise = rng.uniform(0.05, 0.2, n) if vector_noise else float(rng.uniform(0.05, 0.15))
    # six decimals: the inputs are whatever the file says (exactly, as float64), and the file stays small
    x, z, xs, y, noise = (np.round(a, 6) for a in (x, z, xs, y, noise))
    noise = noise if vector_noise else float(noise)
    wrt = []
    if derivatives:
        for ti, t in enumerate(spec["terms"]):
            wrt.append({"kind": "coef", "term": ti})
            for fi, f in enumerate(t["factors"]):
                wrt += [{"kind": "scales", "term": ti, "factor": fi, "index": k} for k in range(len(f["scales"]))]
        wrt.append({"kind": "noise"})
        if vector_noise:
            wrt += [{"kind": "noise", "index": int(a)} for a in rng.choice(n, 6, replace=False)]
        for kind_, rows in (("z", M), ("x", n)):
            picks = set()
            if kind_ == "x" and coincide:
                picks.add((0, 0))   # a coordinate of a clamped point
            while len(picks) < 6:
                picks.add((int(rng.integers(rows)), int(rng.integers(m + 1))))
            wrt += [{"kind": kind_, "row": r, "col": c} for r, c in sorted(picks)]
        for kind_, rows in (("zdir", M), ("xdir", n)):
            for _ in range(2):
                direction = rng.standard_normal((rows, m + 1))
                # (one decimal of a standard normal: the direction is whatever the file says, and the file stays small)
                wrt.append({"kind": kind_, "direction": [[float(v) for v in r] for r in np.round(direction, 1)]})
    cond = float(np.linalg.cond(ok.gram(spec, z, None, jitter=EPS)))
    as_list = lambda a: [[float(v) for v in r] for r in a]
    return {"name": name, "n": n, "M": M, "dims": m, "kernel": kind, "inducing": which, "eps": EPS, "cond_kzz": cond, "spec": spec,
            "x": as_list(x), "z": as_list(z), "xs": as_list(xs), "y": [float(v) for v in y],
            "noise": [float(v) for v in noise] if vector_noise else noise, "wrt": wrt}


def _truth(case):
    x, z, xs, y, noise = case["x"], case["z"], case["xs"], case["y"], case["noise"]
    bounds = mp_ref.sparse_bounds(case["spec"], x, y, noise, z, sp.METHODS, EPS)
    derivs = mp_ref.sparse_bound_derivatives(case["spec"], x, y, noise, z, case["wrt"], sp.METHODS, EPS) if case["wrt"] else None
    out = {}
    for method in sp.METHODS:
        mean, cov = mp_ref.sparse_posterior(case["spec"], x, y, noise, z, xs, method, EPS)
        out[method] = {"bound": float(bounds[method]), "mean": [float(v) for v in mean], "cov": [[float(v) for v in row] for row in cov]}
        if derivs is not None:
            out[method]["derivatives"] = [float(v) for v in derivs[method]]
    return out


def _yardstick(case):
    from oracle.engine import OracleEngine

    x, z, xs, y = (np.array(case[k]) for k in ("x", "z", "xs", "y"))
    noise = np.array(case["noise"])
    prior = gp_ref.Process.prior(case["spec"])
    eng = OracleEngine()
    out, engine, clamped = {}, {}, None
    for method in sp.METHODS:
        want = sp.truth(case, method)
        post = prior.condition_sparse(x, y, noise, z, eps=EPS, method=method)
        cov = post.k(xs, xs)
        got = {"bound": np.array([prior.vfe_bound(x, y, noise, z, eps=EPS, method=method)]), "mean": post.mean(xs), "cov": cov.reshape(-1)}
        got["marginal_var"] = np.diag(cov).copy()
        with sp.installed(eng):
            through = sp.evaluate(case, method, eng)
        if method == "fitc":
            clamped = through["_clamped"]
        got.update({k: v for k, v in through.items() if k.startswith("grad_")})
        short = lambda e: float(f"{e:.3g}")   # (an error is a magnitude: three digits of it)
        out[method] = {k: short(e) for k, (e, _) in sp.errors(got, want).items()}
        engine[method] = {k: short(e) for k, (e, _) in sp.errors(through, want).items()}
    return out, engine, clamped


def build(args):
    case = make_inputs(*args)
    case["truth"] = _truth(case)
    yard, engine, case["fitc_clamped_on_oracle"] = _yardstick(case)
    for method in sp.METHODS:
        case["truth"][method]["yardstick"] = yard[method]
        case["truth"][method]["engine_error"] = engine[method]
    print(f"[{case['name']}] cond {case['cond_kzz']:.2e}  clamped {case['fitc_clamped_on_oracle']}  "
          + "  ".join(f"{m}: bound {yard[m]['bound']:.1e} cov {yard[m]['cov']:.1e}" for m in sp.METHODS), flush=True)
    return case


#        n    M  dims kernel      vector noise  coincident  derivatives
SHAPES = [(30, 5, 1, "layer", True, 0, True),
          (65, 33, 2, "layer", True, 10, True),
          (65, 33, 2, "matern52", False, 0, True),
          (65, 33, 2, "spectral", False, 0, True),
          (130, 64, 2, "layer", False, 0, True),
          (129, 65, 1, "layer", False, 0, False)]


def main():
    jobs = []
    for i, (n, M, m, kind, vec, coincide, derivs) in enumerate(SHAPES):
        for j, which in enumerate(("well", "used")):
            jobs.append((f"n{n}-M{M}-d{m}-{kind}-{which}", n, M, m, kind, which, vec, coincide, derivs, 20261021 + 10 * i + j))
    jobs.sort(key=lambda a: -a[1] * a[2] ** 2 * (1 + 40 * a[8]))   # longest first
    with Pool(min(8, len(jobs))) as pool:
        cases = pool.map(build, jobs, chunksize=1)
    cases.sort(key=lambda c: (c["n"], c["kernel"], c["inducing"]))
    # the conditions the fixture has to meet - by the choice of inputs above
    for case in cases:
        if case["inducing"] != "well":
            continue
        assert case["cond_kzz"] <= 1e6, (case["name"], case["cond_kzz"])
        for method in sp.METHODS:
            t = case["truth"][method]
            for quantity, scale in (("bound", abs(t["bound"])), ("mean", np.max(np.abs(t["mean"]))), ("cov", np.max(np.abs(t["cov"])))):
                assert t["yardstick"][quantity] <= 1e-11 * scale, (case["name"], method, quantity, t["yardstick"][quantity], scale)
    assert any(0 < c["fitc_clamped_on_oracle"] < c["n"] for c in cases), "no FITC case with some points clamped and some not"
    path = sp.CASES
    with open(path, "w") as f:
        json.dump({"eps": EPS, "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    size = os.path.getsize(path)
    assert size < os.path.getsize(os.path.join(os.path.dirname(path), "gpar_cases.json")), size
    print(f"wrote {path}: {len(cases)} cases, {size} bytes")


if __name__ == "__main__":
    main()
