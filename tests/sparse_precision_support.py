"""What tests/golden/make_sparse_golden.py, tests/test_sparse_precision.py and tests/test_sparse_precision_gpu.py share: reading the
fixture, running one case through `gp.PseudoObs` on a given engine, and measuring the result against the stored 50-digit truth.

A "quantity" is a named vector (the bound, the posterior mean, the full posterior covariance, a group of gradient entries ...); its
error is the max-abs difference from the truth, its scale the max-abs truth value ("inducing-point path")."""
import contextlib
import json
import os

import numpy as np
import torch

CASES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_cases.json")
METHODS = ("vfe", "fitc", "dtc")
MARGIN = 8          # err_hip <= MARGIN * max(err_oracle, floor): the margin of tests/test_update_gpu.py
STALE = 4           # the oracle engine reproduces the stored yardstick within this factor
GRADIENT_GROUPS = {"coef": "grad_params", "scales": "grad_params", "periods": "grad_params", "alpha": "grad_params", "noise": "grad_noise",
                   "z": "grad_z", "x": "grad_x", "zdir": "grad_zdir", "xdir": "grad_xdir"}


def load_cases():
    with open(CASES) as f:
        return json.load(f)["cases"]


def floor(n, scale):
    """n roundings of the scale: below this an fp64 error is luck, not accuracy."""
    return n * 2.0 ** -53 * scale


@contextlib.contextmanager
def installed(eng):
    from gpar_amd.engine import set_engine

    previous = set_engine(eng)
    try:
        yield eng
    finally:
        set_engine(previous)


def kernel_from_spec(spec, grad=False):
    """The product kernel of an oracle kernel dict; with `grad`, every coefficient and every scale vector is a leaf tensor, returned in
    the order `gp.kernel_parameters` walks them: [(kind, term, factor, tensor)]."""
    from gpar_amd.kernels import Factor, Kernel, Term

    leaves, terms = [], []
    for ti, t in enumerate(spec["terms"]):
        coef = t["coef"]
        if grad:
            coef = torch.tensor(float(coef), dtype=torch.float64, requires_grad=True)
            leaves.append(("coef", ti, None, coef))
        fs = []
        for fi, f in enumerate(t["factors"]):
            scales = np.array(f["scales"], dtype=np.float64)
            if grad:
                scales = torch.tensor(scales, requires_grad=True)
                leaves.append(("scales", ti, fi, scales))
            fs.append(Factor(f["type"], tuple(f["cols"]), scales, None if f["periods"] is None else np.array(f["periods"]),
                             f["alpha"] if f["type"] == "rq" else None))
        terms.append(Term(coef, fs))
    return Kernel(terms), leaves


def _obs_class(method):
    from gpar_amd import gp

    return {"vfe": gp.PseudoObs, "fitc": gp.PseudoObsFITC, "dtc": gp.PseudoObsDTC}[method]


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def evaluate(case, method, eng, gradients=True, posterior=True):
    """{quantity: numpy vector} of one case and method through `gp.PseudoObs` on `eng` (which the caller has installed)."""
    from gpar_amd.gp import GP

    out = {}
    x, z, y, xs = (np.array(case[k], dtype=np.float64) for k in ("x", "z", "y", "xs"))
    noise = np.array(case["noise"], dtype=np.float64)
    cls = _obs_class(method)
    kernel, _ = kernel_from_spec(case["spec"])
    f = GP(kernel, engine=eng)
    with torch.no_grad():
        obs = cls(f(z), f(x, noise), y)
        out["bound"] = np.array([float(obs.logpdf())])
        if method == "fitc":
            out["_clamped"] = int((_np(obs._compute()["moves"]) == 0).sum())
        if posterior:
            post = f | obs
            out["mean"] = _np(post.mean(xs)).reshape(-1)
            out["cov"] = _np(post(xs).var()).reshape(-1)
            mean, var = post.marginal_moments(xs)
            out["marginal_mean"], out["marginal_var"] = _np(mean).reshape(-1), _np(var).reshape(-1)
            p = post._pts(xs)
            out["cross"] = _np(post._cross(p, p)).reshape(-1)
    if gradients and case.get("wrt"):
        gkernel, leaves = kernel_from_spec(case["spec"], grad=True)
        xt, zt = torch.tensor(x, requires_grad=True), torch.tensor(z, requires_grad=True)
        nt = torch.tensor(noise, requires_grad=True)
        g = GP(gkernel, engine=eng)
        value = cls(g(zt), g(xt, nt), y).logpdf()
        out["bound_with_graph"] = np.array([float(value.detach())])
        value.backward()
        groups = {}
        for entry in case["wrt"]:
            kind = entry["kind"]
            if kind == "coef":
                v = next(t for k, ti, fi, t in leaves if k == "coef" and ti == entry["term"]).grad
            elif kind == "scales":
                v = next(t for k, ti, fi, t in leaves if k == "scales" and ti == entry["term"] and fi == entry["factor"]).grad[entry["index"]]
            elif kind == "noise":
                v = nt.grad.sum() if entry.get("index") is None else nt.grad.reshape(-1)[entry["index"]]
            elif kind in ("x", "z"):
                v = (xt if kind == "x" else zt).grad[entry["row"], entry["col"]]
            else:
                v = ((xt if kind == "xdir" else zt).grad * torch.tensor(entry["direction"], dtype=torch.float64)).sum()
            groups.setdefault(GRADIENT_GROUPS[kind], []).append(float(v))
        out.update({k: np.array(v) for k, v in groups.items()})
    return out


def truth(case, method):
    """{quantity: numpy vector} of the stored 50-digit values (rounded to float64), the derivative entries grouped as `evaluate` does."""
    t = case["truth"][method]
    out = {"bound": np.array([t["bound"]]), "mean": np.array(t["mean"]), "cov": np.array(t["cov"]).reshape(-1)}
    out["marginal_mean"] = out["mean"]
    out["marginal_var"] = np.diag(np.array(t["cov"])).copy()
    out["cross"] = out["cov"]
    out["bound_with_graph"] = out["bound"]
    groups = {}
    for entry, v in zip(case.get("wrt") or [], t.get("derivatives") or []):
        groups.setdefault(GRADIENT_GROUPS[entry["kind"]], []).append(v)
    out.update({k: np.array(v) for k, v in groups.items()})
    return out


def yardstick(case, method):
    """The stored error of the fp64 oracle per quantity; quantities that are another route to the same numbers share theirs."""
    y = dict(case["truth"][method]["yardstick"])
    y.update(marginal_mean=y["mean"], cross=y["cov"], bound_with_graph=y["bound"], bound_unfused=y["bound"])
    return y


def errors(got, want):
    """{quantity: (max-abs error, max-abs truth)} over the quantities both hold."""
    return {k: (float(np.max(np.abs(got[k] - want[k]))), float(np.max(np.abs(want[k])))) for k in got if k in want}
