"""The inducing-point layer (gp.PseudoObs: VFE, FITC, DTC) against 50-digit arithmetic, CPU half.

  * the new functions of oracle/mp_ref.py against the older n x n `vfe_bound` and against each other (DTC + trace term = VFE; FITC with
    Z = X is the dense log-density up to the jitter; the mp central differences against a closed-form derivative);
  * the fixture tests/golden/sparse_cases.json: its shapes, its conditioning, the oracle's stored error on the well-conditioned sets;
  * the numpy oracle ENGINE through gp.PseudoObs - `_compute`, `gradients`, `input_gradients`, `cross`, `diag`, `moments_into`, the host
    algebra the HIP engine runs as well - against the stored truth: within 4 x the stored yardstick (the oracle's own error on the same
    problem, floored at n roundings of the scale).  A wrong term of relative size 1e-6 in that algebra fails here on the
    well-conditioned sets, where the yardstick is ~1e-13.
"""
import mpmath as mp
import numpy as np
import pytest

from oracle import mp_ref

from . import sparse_precision_support as sp

CASES = sp.load_cases()
_rows = lambda a: [[float(v) for v in r] for r in a]


def _small_problem(seed, n=22, M=6, vector_noise=True):
    from oracle import gpar_ref

    rng = np.random.default_rng(seed)
    hypers = {"1/input/var": 1.3, "1/input/scales": [0.7], "1/output/lin/scales": [2.5], "1/noise": 0.0}
    spec, _ = gpar_ref.layer_spec(hypers, 1, 1, dict(linear=True, nonlinear=False))
    x, z = rng.uniform(-2, 2, (n, 2)), rng.uniform(-2, 2, (M, 2))
    y = np.sin(x[:, 0]) + 0.3 * x[:, 1] + 0.1 * rng.standard_normal(n)
    noise = rng.uniform(0.05, 0.2, n) if vector_noise else 0.08
    return spec, x, y, noise, z


@pytest.mark.parametrize("seed,n,M", [(1, 22, 6), (2, 30, 12), (3, 9, 9)])
def test_m_by_m_form_equals_the_n_by_n_bound_to_40_digits(seed, n, M):
    spec, x, y, noise, z = _small_problem(seed, n, M)
    old = mp_ref.vfe_bound(spec, _rows(x), y, noise, _rows(z))
    new = mp_ref.sparse_bound(spec, _rows(x), y, noise, _rows(z), "vfe")
    assert abs((new - old) / old) < mp.mpf(10) ** -40


def test_methods_against_each_other_and_the_dense_log_density():
    spec, x, y, noise, z = _small_problem(4)
    rows = _rows(x)
    b = mp_ref.sparse_bounds(spec, rows, y, noise, _rows(z))
    # DTC + trace term = VFE, the trace term from the n x n definition
    Kzz, Kxz = mp_ref.gram(spec, _rows(z), None, None, 1e-12), mp_ref.gram(spec, rows, _rows(z))
    Q = Kxz * mp_ref._solve(Kzz, Kxz.T)
    trace = mp.fsum((mp_ref.gram(spec, [rows[a]])[0, 0] - Q[a, a]) / mp.mpf(float(noise[a])) for a in range(len(y)))
    assert abs(b["dtc"] - trace / 2 - b["vfe"]) < mp.mpf(10) ** -40 * abs(b["vfe"])
    assert b["fitc"] != b["dtc"]
    # FITC's n x n definition
    S = Q.copy()
    for a in range(len(y)):
        S[a, a] += mp.mpf(float(noise[a])) + mp_ref.gram(spec, [rows[a]])[0, 0] - Q[a, a]
    assert abs(mp_ref._mvn_logpdf(S, mp_ref._col(y)) - b["fitc"]) < mp.mpf(10) ** -40 * abs(b["fitc"])
    # Z = X: Q = K (K + eps I)^-1 K is K up to eps, so FITC (and VFE, whose trace term is then eps-sized) is the dense log-density
    dense = mp_ref.logpdf(spec, rows, y, noise, eps=0)
    at_x = mp_ref.sparse_bounds(spec, rows, y, noise, rows)
    assert abs(at_x["fitc"] - dense) < 1e-9 * abs(dense) and abs(at_x["vfe"] - dense) < 1e-9 * abs(dense)
    # ... and the posterior the dense posterior
    xs = _rows(np.random.default_rng(5).uniform(-2, 2, (4, 2)))
    mean, cov = mp_ref.sparse_posterior(spec, rows, y, noise, rows, xs, "fitc")
    dmean, dcov = mp_ref.posterior(spec, rows, y, noise, xs, eps=0)
    assert max(abs(mean[i] - dmean[i]) for i in range(4)) < 1e-8
    assert max(abs(cov[i][j] - dcov[i, j]) for i in range(4) for j in range(4)) < 1e-8


def test_posterior_against_the_n_by_n_closed_form():
    """mean* = K_*z Sigma^-1 K_zx D^-1 y and cov* = K_** - K_*z K_zz^-1 K_z* + K_*z Sigma^-1 K_z* with explicit solves."""
    spec, x, y, noise, z = _small_problem(6)
    xs = _rows(np.random.default_rng(7).uniform(-2, 2, (5, 2)))
    mean, cov = mp_ref.sparse_posterior(spec, _rows(x), y, noise, _rows(z), xs, "vfe")
    Kzz, Kxz, Ksz = mp_ref.gram(spec, _rows(z), None, None, 1e-12), mp_ref.gram(spec, _rows(x), _rows(z)), mp_ref.gram(spec, xs, _rows(z))
    Dinv = mp.diag([1 / mp.mpf(float(v)) for v in noise])
    Sigma = Kzz + Kxz.T * Dinv * Kxz
    want_mean = Ksz * mp.lu_solve(Sigma, Kxz.T * Dinv * mp_ref._col(y))
    want_cov = mp_ref.gram(spec, xs) - Ksz * mp_ref._solve(Kzz, Ksz.T) + Ksz * mp_ref._solve(Sigma, Ksz.T)
    assert max(abs(mean[i] - want_mean[i]) for i in range(5)) < mp.mpf(10) ** -38
    assert max(abs(cov[i][j] - want_cov[i, j]) for i in range(5) for j in range(5)) < mp.mpf(10) ** -38


def test_mp_central_differences_against_a_closed_form():
    """d/d noise of DTC's log N(y; 0, Q + s I) is 1/2 (|S^-1 y|^2 - tr S^-1); the differences reproduce it to 30 digits, and a coefficient
    that scales the whole kernel AND the noise (Euler: S -> c S) has the derivative -(n - y^T S^-1 y) / 2."""
    spec, x, y, _, z = _small_problem(8, vector_noise=False)
    noise = 0.08
    n = len(y)
    Kzz, Kxz = mp_ref.gram(spec, _rows(z), None, None, 1e-12), mp_ref.gram(spec, _rows(x), _rows(z))
    S = Kxz * mp_ref._solve(Kzz, Kxz.T)
    for a in range(n):
        S[a, a] += mp.mpf(noise)
    alpha = mp.lu_solve(S, mp_ref._col(y))
    Sinv = mp_ref._solve(S, mp.eye(n))
    want = (mp.fsum(v * v for v in alpha) - mp.fsum(Sinv[a, a] for a in range(n))) / 2
    got = mp_ref.sparse_bound_derivatives(spec, _rows(x), y, noise, _rows(z), [{"kind": "noise"}], ("dtc",))["dtc"][0]
    assert abs(got - want) < mp.mpf(10) ** -30 * abs(want)


def test_fixture_meets_its_conditions():
    shapes = {(c["n"], c["M"], c["dims"]) for c in CASES}
    assert shapes == {(30, 5, 1), (65, 33, 2), (130, 64, 2), (129, 65, 1)}
    assert {c["kernel"] for c in CASES if c["n"] == 65} == {"layer", "matern52", "spectral"}
    assert any(isinstance(c["noise"], list) for c in CASES)
    assert any(0 < c["fitc_clamped_on_oracle"] < c["n"] for c in CASES)
    for c in CASES:
        assert (not c["wrt"]) == (c["n"] == 129)
        if c["wrt"]:
            kinds = [e["kind"] for e in c["wrt"]]
            assert kinds.count("z") == 6 and kinds.count("x") == 6 and kinds.count("zdir") == 2 and kinds.count("xdir") == 2 and "noise" in kinds
            nparams = len(c["spec"]["terms"]) + sum(len(f["scales"]) for t in c["spec"]["terms"] for f in t["factors"])
            assert sum(k in ("coef", "scales") for k in kinds) == nparams
        if c["inducing"] == "well":
            assert c["cond_kzz"] <= 1e6
            for method in sp.METHODS:
                t = c["truth"][method]
                assert t["yardstick"]["bound"] <= 1e-11 * abs(t["bound"])
                assert t["yardstick"]["mean"] <= 1e-11 * np.max(np.abs(t["mean"])) and t["yardstick"]["cov"] <= 1e-11 * np.max(np.abs(t["cov"]))
        else:
            # (the usual 1e9 or worse; five points, and the Matern kernel's slower spectral decay, stay below it)
            assert c["cond_kzz"] >= 1e9 or c["M"] == 5 or c["kernel"] == "matern52"


def test_fixture_truth_is_what_mp_ref_computes():
    """The smallest case once more from oracle/mp_ref.py (values, moments and three of the derivatives): the file is this code's output."""
    c = next(c for c in CASES if c["n"] == 30 and c["inducing"] == "well")
    bounds = mp_ref.sparse_bounds(c["spec"], c["x"], c["y"], c["noise"], c["z"])
    wrt = [c["wrt"][0], next(e for e in c["wrt"] if e["kind"] == "z"), next(e for e in c["wrt"] if e["kind"] == "xdir")]
    idx = [c["wrt"].index(e) for e in wrt]
    derivs = mp_ref.sparse_bound_derivatives(c["spec"], c["x"], c["y"], c["noise"], c["z"], wrt)
    for method in sp.METHODS:
        t = c["truth"][method]
        assert float(bounds[method]) == t["bound"]
        mean, cov = mp_ref.sparse_posterior(c["spec"], c["x"], c["y"], c["noise"], c["z"], c["xs"], method)
        assert [float(v) for v in mean] == t["mean"] and [[float(v) for v in r] for r in cov] == t["cov"]
        assert [float(v) for v in derivs[method]] == [t["derivatives"][i] for i in idx]


@pytest.mark.parametrize("method", sp.METHODS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_oracle_engine_through_pseudo_obs_reproduces_the_yardstick(case, method, oracle_engine):
    """gp.py's algebra on the numpy engine against the truth, every quantity twice:
      not stale   within STALE x max(the engine's stored error, n roundings of the scale);
      not wrong   within STALE x max(the stored yardstick - for values and moments the error of ANOTHER fp64 route, gp_ref's n x n
                  forms - , cond(K_zz) roundings of the scale: what the conditioning explains, ~1e-14 on the well-conditioned sets)."""
    got = sp.evaluate(case, method, oracle_engine)
    want = sp.truth(case, method)
    yard, stored = sp.yardstick(case, method), case["truth"][method]["engine_error"]
    stale, wrong = {}, {}
    for quantity, (err, scale) in sp.errors(got, want).items():
        stale[quantity] = err / max(stored[quantity], sp.floor(case["n"], scale))
        wrong[quantity] = err / max(yard[quantity], sp.floor(max(case["n"], case["cond_kzz"]), scale))
    print(f"[sparse precision] oracle engine {case['name']} {method}: error / stored = " + ", ".join(f"{k} {v:.3g}" for k, v in stale.items())
          + "; error / yardstick = " + ", ".join(f"{k} {v:.3g}" for k, v in wrong.items()))
    bad = {k: (stale[k], wrong[k]) for k in stale if not (stale[k] <= sp.STALE and wrong[k] <= sp.STALE)}
    assert not bad, bad
    if method == "fitc" and case["fitc_clamped_on_oracle"]:   # (which points clamp is decided by rounding; that some do and some do not, by the inputs)
        assert 0 < got["_clamped"] < case["n"]
