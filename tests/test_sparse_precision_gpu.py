"""The inducing-point layer (gp.PseudoObs: VFE, FITC, DTC) on the HIP engine against 50-digit arithmetic, and once on each side of the
sizes at which its device routes switch.

Fixture half (tests/golden/sparse_cases.json, made by tests/golden/make_sparse_golden.py): for each case x method x inducing set the
bound (fused scalar side and GPAR_VFE_FUSED_SCALARS=0), the posterior through `f | obs` (mean, full covariance, marginal moments, the
cross-covariance) and the autograd gradient of the bound (kernel parameters, noise, coordinates and contracted directions of Z and X),
each held to

    err_hip <= 8 x max(err_oracle, n 2^-53 scale)

where err_* is the max-abs error of the quantity against the truth, err_oracle the stored error of the fp64 numpy oracle on the SAME
problem and scale the max-abs truth.  The margin 8 is that of tests/test_update_gpu.py, for the same reason: a different but equally long
chain of roundings, a different summation order (tiles, slices); the floor keeps a lucky oracle draw from failing a correct kernel.  On
the well-conditioned inducing sets the yardstick is ~1e-14 .. 1e-13 relative: a wrong term of size 1e-6 is seven orders above it.
Every ratio is printed (pytest -s); with GPAR_SPARSE_PRECISION_REPORT=<file> the worst per method and quantity are written there
(profiles/sparse_precision.txt is such a file).

`gpar_vfe_assemble` / `gpar_vfe_value` through the raw binding, and the size thresholds (side streams from n M >= 2^22, split-K from
k >= 8192), follow below.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

from . import sparse_precision_support as sp
from .conftest import make_engine

pytestmark = pytest.mark.gpu

CASES = sp.load_cases()
_WORST = {}       # (method, quantity) -> (ratio, case name)
_THRESHOLD = []   # report lines of the size-threshold tests


@pytest.fixture(scope="module")
def hip():
    eng = make_engine("hip")
    with sp.installed(eng):
        yield eng
    path = os.environ.get("GPAR_SPARSE_PRECISION_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("# worst err_hip / max(err_oracle, n 2^-53 scale) per method and quantity over tests/golden/sparse_cases.json (bound: 8)\n")
            for (method, quantity), (ratio, name) in sorted(_WORST.items()):
                f.write(f"{method:5s} {quantity:18s} {ratio:10.3g}  {name}\n")
            f.write("# size thresholds: HIP against the oracle engine on the same inputs\n")
            f.writelines(line + "\n" for line in _THRESHOLD)


# Case-specific bounds (the general margin stays 8).  On these two ILL-CONDITIONED sets the bound's error is above 8 x the yardstick on
# every engine: the numpy engine running the same algebra (L_z = chol(K_zz + eps I) first, B = L_z^-1 K_zx, A = I + B D^-1 B^T) is off by
# as much or more - its stored `engine_error` is 2.2e-10 and 1.4e-9 where HIP measured 5.5e-10 and 8.3e-10 - so the digits go in the
# formulation, not in a kernel.  Derivation: chol(K_zz) is backward stable, i.e. exact for K_zz (1 + O(2^-53)), and the bound moves by
# up to cond(K_zz) 2^-53 of its size under such a perturbation - 2.8e-8 at cond 9.9e6 (|bound| 26) and far more at cond 6.2e13; the
# yardstick (gp_ref's n x n forms through an LU solve) is ONE draw from that range, 5.6e-11 and 8.5e-11 here, and happened to be the
# luckier one.  For these the yardstick is the larger of the two fp64 draws, under the same margin.
_SAME_ALGEBRA_YARDSTICK = {("n30-M5-d1-layer-used", "vfe"), ("n130-M64-d2-layer-used", "fitc")}


@pytest.mark.parametrize("method", sp.METHODS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_fixture_case_within_eight_times_the_oracles_error(case, method, hip, monkeypatch):
    got = sp.evaluate(case, method, hip)
    monkeypatch.setenv("GPAR_VFE_FUSED_SCALARS", "0")
    got["bound_unfused"] = sp.evaluate(case, method, hip, gradients=False, posterior=False)["bound"]
    monkeypatch.delenv("GPAR_VFE_FUSED_SCALARS")
    want = sp.truth(case, method)
    want["bound_unfused"] = want["bound"]
    yard = sp.yardstick(case, method)
    if (case["name"], method) in _SAME_ALGEBRA_YARDSTICK:
        assert case["inducing"] == "used" and case["cond_kzz"] > 1e6
        stored = case["truth"][method]["engine_error"]["bound"]
        yard.update({k: max(yard[k], stored) for k in ("bound", "bound_unfused", "bound_with_graph")})
    ratios = {}
    for quantity, (err, scale) in sp.errors(got, want).items():
        ratios[quantity] = err / max(yard[quantity], sp.floor(case["n"], scale))
        if ratios[quantity] > _WORST.get((method, quantity), (-1.0, ""))[0]:
            _WORST[(method, quantity)] = (ratios[quantity], case["name"])
    print(f"[sparse precision] hip {case['name']} {method} (cond {case['cond_kzz']:.1e}): err / max(oracle, floor) = "
          + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    expected = {"bound", "bound_unfused", "mean", "cov", "marginal_mean", "marginal_var", "cross"}
    if case["wrt"]:
        expected |= {"bound_with_graph", "grad_params", "grad_noise", "grad_z", "grad_x", "grad_zdir", "grad_xdir"}
    assert set(ratios) == expected
    bad = {k: v for k, v in ratios.items() if not v <= sp.MARGIN}
    assert not bad, bad
    if method == "fitc" and case["fitc_clamped_on_oracle"]:
        assert 0 < got["_clamped"] < case["n"]


# ---- gpar_vfe_assemble + gpar_vfe_value through the raw binding ----------------------------------------------------------------------
def _sequential(values):
    s = 0.0
    for v in values:
        s += float(v)
    return s


@pytest.mark.parametrize("M", [1, 64, 257])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_vfe_assemble_and_value_through_the_raw_binding(n, M, hip):
    """A <- [[G + diag_add I (lower), .], [c^T, 0]] bit for bit with an odd leading dimension and nothing else written (A and the sums
    start as NaN); the four sums against math.fsum to (number of terms) 2^-52 relative - n for sum ys^2, sum kdiag / d and sum log d, M for
    tr G, all four of one sign so that "relative" means what it says; the value from the device's own sums for both `with_trace`."""
    from gpar_amd import _lib
    from gpar_amd.hip import stream_ptr

    lib = _lib.load()
    dev = hip.device
    rng = np.random.default_rng(1000 * n + M)
    lda = M + 2 if M % 2 else M + 3
    ldg = M + 1 if M % 2 == 0 else M + 2
    assert lda % 2 == 1 and ldg % 2 == 1
    G = np.full((M, ldg), np.nan)
    G[:, :M] = rng.standard_normal((M, M))
    G[np.arange(M), np.arange(M)] = rng.uniform(0.5, 2.0, M)
    c, ys, kdiag, d = rng.standard_normal(M), rng.standard_normal(n), rng.uniform(0.5, 2.0, n), rng.uniform(0.05, 0.5, n)
    dG, dc, dys, dk, dd = (torch.tensor(a, device=dev) for a in (G, c, ys, kdiag, d))
    A = torch.full((M + 1, lda), float("nan"), dtype=torch.float64, device=dev)
    scal = torch.full((256,), float("nan"), dtype=torch.float64, device=dev)
    logdet = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    info = torch.full((1,), -7, dtype=torch.int32, device=dev)
    st = stream_ptr(dev)
    _lib.check(lib.gpar_vfe_assemble(dG.data_ptr(), M, ldg, dc.data_ptr(), dys.data_ptr(), dk.data_ptr(), dd.data_ptr(), n, 1.0, A.data_ptr(), lda,
                                     scal.data_ptr(), logdet.data_ptr(), info.data_ptr(), st), "gpar_vfe_assemble")
    torch.cuda.synchronize()
    got = A.cpu().numpy()
    want = np.full((M + 1, lda), np.nan)
    il = np.tril_indices(M)
    want[:M, :M][il] = (G[:, :M] + np.eye(M))[il]
    want[M, :M] = c
    want[M, M] = 0.0
    assert np.array_equal(got.view(np.int64), want.view(np.int64))   # lower triangle and last row to the bit; upper triangle and padding still NaN
    assert float(logdet[0]) == 0.0 and int(info[0]) == 0
    parts = scal.cpu().numpy().reshape(64, 4)
    assert np.all(np.isfinite(parts))
    exact = [math.fsum(float(v) * float(v) for v in ys), math.fsum(float(k) / float(e) for k, e in zip(kdiag, d)),
             math.fsum(math.log(float(e)) for e in d), math.fsum(float(G[i, i]) for i in range(M))]
    for q, terms in enumerate((n, n, n, M)):
        rel = abs(math.fsum(parts[:, q]) - exact[q]) / abs(exact[q])
        assert rel <= terms * 2.0 ** -52, (q, rel, terms * 2.0 ** -52)
    # the value: the corner of A and the log-determinant word as a factorisation would leave them
    corner, ld = -float(rng.uniform(0.5, 3.0)), float(rng.uniform(-5.0, 5.0))
    A[M, M] = corner
    logdet[0] = ld
    s = [_sequential(parts[:, q]) for q in range(4)]
    nlog = n * 1.8378770664093453
    for with_trace in (0, 1):
        out = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
        _lib.check(lib.gpar_vfe_value(scal.data_ptr(), logdet.data_ptr(), A.data_ptr(), lda, M, n, with_trace, out.data_ptr(), st), "gpar_vfe_value")
        terms = ([s[1], -s[3]] if with_trace else []) + [s[2], nlog, ld, s[0], corner]
        want_value = -0.5 * math.fsum(terms)
        # at most seven roundings, each of a partial sum no larger than the sum of the magnitudes
        assert abs(float(out[0]) - want_value) <= 0.5 * 7 * 2.0 ** -53 * sum(abs(t) for t in terms), (with_trace, float(out[0]), want_value)


# ---- once on each side of the size thresholds ---------------------------------------------------------------------------------------
# (8192, 512): n M = 2^22 puts the factorisation of K_zz and the matrix-vector pass on side streams, k = n = 8192 with 10 lower tiles makes
# the Bs^T Bs product split-K; (8191, 512) - the same data without its last row - has neither.  Eight uniform input dimensions keep
# K_zz well-conditioned.
_BIG_M, _BIG_DIMS = 512, 8


@functools.lru_cache(maxsize=None)
def _big_problem():
    rng = np.random.default_rng(8192)
    n = 8192
    x = np.concatenate([rng.uniform(0, 1, (n, _BIG_DIMS)), rng.standard_normal((n, 1))], axis=1)
    z = np.concatenate([rng.uniform(0, 1, (_BIG_M, _BIG_DIMS)), rng.standard_normal((_BIG_M, 1))], axis=1)
    y = np.sin(2 * np.pi * x[:, :_BIG_DIMS] @ rng.uniform(0.5, 1.5, _BIG_DIMS)) + 0.3 * x[:, -1] + 0.1 * rng.standard_normal(n)
    spec = {"terms": [{"coef": 1.2, "factors": [{"type": "eq", "cols": list(range(_BIG_DIMS)), "scales": list(rng.uniform(0.4, 0.6, _BIG_DIMS)),
                                                 "periods": None, "alpha": 0.0}]},
                      {"coef": 1.0, "factors": [{"type": "linear", "cols": [_BIG_DIMS], "scales": [2.5], "periods": None, "alpha": 0.0}]}]}
    return spec, x, y, 0.1, z


def _value_and_gradient(eng, n, method):
    """(bound, {kernel parameters, noise, Z} gradient as one vector) at the first n rows of the problem."""
    from gpar_amd.gp import GP

    spec, x, y, noise, z = _big_problem()
    kernel, leaves = sp.kernel_from_spec(spec, grad=True)
    zt, nt = torch.tensor(z, requires_grad=True), torch.tensor(noise, dtype=torch.float64, requires_grad=True)
    f = GP(kernel, engine=eng)
    with sp.installed(eng):
        value = sp._obs_class(method)(f(zt), f(x[:n], nt), y[:n]).logpdf()
        value.backward()
    grads = {"params": torch.cat([t.grad.reshape(-1) for *_, t in leaves]).numpy().copy(), "noise": nt.grad.reshape(-1).numpy().copy(),
             "z": zt.grad.numpy().reshape(-1).copy()}
    return float(value.detach()), grads


@functools.lru_cache(maxsize=None)
def _oracle_big(n, method):
    return _value_and_gradient(make_engine("oracle"), n, method)


@functools.lru_cache(maxsize=None)
def _hip_big(n, method):
    return _value_and_gradient(make_engine("hip"), n, method)


@pytest.mark.parametrize("method", sp.METHODS)
@pytest.mark.parametrize("n", [8192, 8191])
def test_value_and_gradient_on_each_side_of_the_thresholds(n, method, hip):
    """The project's existing inducing-point bounds as a ceiling - 1e-8 relative on the value, rtol 1e-4 / atol 1e-5 max on gradients -
    with what is measured printed, for a later tightening from data."""
    assert (hip.side_stream() is not None and n * _BIG_M >= 1 << 22) == (n == 8192)   # (the side streams are there to be switched)
    value, grads = _hip_big(n, method)
    want_value, want = _oracle_big(n, method)
    rel = abs(value - want_value) / abs(want_value)
    line = f"n {n} M {_BIG_M} {method:5s} value rel {rel:.2e}"
    for k in ("params", "noise", "z"):
        err = np.max(np.abs(grads[k] - want[k]) / (1e-4 * np.abs(want[k]) + 1e-5 * np.max(np.abs(want[k]))))
        line += f"  grad {k} err/tol {err:.2e} (max-abs rel {np.max(np.abs(grads[k] - want[k])) / np.max(np.abs(want[k])):.2e})"
    print("[sparse precision] " + line)
    _THRESHOLD.append(line)
    assert rel <= 1e-8, (value, want_value)
    for k in ("params", "noise", "z"):
        assert np.all(np.isfinite(grads[k]))
        np.testing.assert_allclose(grads[k], want[k], rtol=1e-4, atol=1e-5 * np.max(np.abs(want[k])))


@pytest.mark.parametrize("method", sp.METHODS)
def test_same_bits_twice_with_the_side_streams_on(method, hip):
    """Two evaluations at (8192, 512) return the same bits in value and gradient: a missing stream join shows up here."""
    first = _hip_big(8192, method)
    again = _value_and_gradient(hip, 8192, method)
    assert np.float64(first[0]).tobytes() == np.float64(again[0]).tobytes()
    for k in first[1]:
        assert np.array_equal(first[1][k].view(np.int64), again[1][k].view(np.int64)), k


@pytest.mark.parametrize("method", sp.METHODS)
def test_last_row_removed_moves_the_value_as_on_the_oracle(method, hip):
    """(8191, 512) is (8192, 512) without its last data row: what that row contributes - the difference of the two values, one from
    each side of the switches - agrees with the oracle's to the bound on the value itself, 1e-8 relative."""
    got = _hip_big(8192, method)[0] - _hip_big(8191, method)[0]
    want = _oracle_big(8192, method)[0] - _oracle_big(8191, method)[0]
    scale = abs(_oracle_big(8192, method)[0])
    line = f"last row {method:5s} contribution {want:.6g}, hip - oracle {got - want:.2e} ({abs(got - want) / scale:.2e} of the value)"
    print("[sparse precision] " + line)
    _THRESHOLD.append(line)
    assert abs(want) > 1e-3   # the row does count
    assert abs(got - want) <= 1e-8 * scale
