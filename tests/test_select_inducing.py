"""Greedy inducing-point selection (`gp.greedy_inducing`, `GPARRegressor.select_inducing`) on the CPU oracle: the route composed of engine
primitives against a numpy greedy pivoted Cholesky kept in this file, which works on the oracle's dense Gram matrix with the same tie
and stop rules (ties to the smallest row, stop at d_p <= floor, at trace_j <= tol trace_0, at a non-finite pivot).

Pivot orders of two roundings are only comparable where the maximum is clear, so every comparison first asserts ON THE REFERENCE ALONE
that the two largest residuals differ by more than 1e-9 relative at every step (`GAP`).  One kind of step cannot have a gap: under a
stationary kernel every row starts with the same variance, d_i = the kernel's coefficient, bit for bit in every implementation; that is
an exact tie, which the tie rule settles (row 0), not a near tie.  `_reference` therefore accepts a step whose residuals are all
bitwise equal and reports the gap of every other step.

Tolerance (`bound`): a Cholesky of rank k has backward error at most (k + 1) 2^-53 |L||L^T|, and |L||L^T|_ij <= max diag K; to that the
tolerance tests/test_hip_primitives.py holds gpar_gram to against the oracle is added (rtol 1e-13, atol 1e-14: the fused column kernel
uses libm's exp, gpar_gram its tables), and the sum is taken 8 times.  `Lt` and the residual traces of two routes are both held to
it.  The bound is a backward error; a column of the factor is divided by sqrt(d_p), which
magnifies a rounding-level difference (2^-52 max diag K) between two routes by 1 / sqrt(d_p).  The kernels' length scales are chosen so
that forty pivots stay above 1e-5 (asserted on the reference: `PIVOT_MIN`), a magnification of about 300, which the bound covers - and
long enough that no k(x_i, x_p)^2 vanishes against d_i, which would leave exact-looking ties that two roundings may break apart.
"""
import numpy as np
import pytest

from gpar_amd import greedy_inducing
from gpar_amd.kernels import EQ, RQ, Cosine, Linear, Matern32
from gpar_amd.regression import GPARRegressor

from .conftest import to_np

GAP = 1e-9
PIVOT_MIN = 1e-5
FLOOR = 1e-12   # the engines' jitter: what `floor=None` means


def bound(rank, kmax):
    """8 x ((rank + 1) 2^-53 kmax + (1e-13 kmax + 1e-14)): see the module docstring."""
    return 8.0 * ((rank + 1) * 2.0**-53 * kmax + (1e-13 * kmax + 1e-14))


def _reference(K, num, tol=0.0, floor=FLOOR):
    """Greedy pivoted Cholesky of the dense matrix K in numpy: (Lt, piv, trace, rank, smallest relative gap between the two largest
    residuals over the steps taken - steps whose residuals are all bitwise equal excepted -, smallest pivot)."""
    n = K.shape[0]
    d, Lt, piv, trace = np.diag(K).copy(), np.zeros((num, n)), np.full(num, -1), np.zeros(num + 1)
    rank, gap, smallest = num, np.inf, np.inf
    for j in range(num + 1):
        trace[j] = d.sum()
        if j == num:
            break
        p = int(np.argmax(d))   # (the first of equal maxima, the first NaN)
        if d[p] <= floor or trace[j] <= tol * trace[0] or not np.isfinite(d[p]):
            rank = j
            break
        if n > 1 and not np.all(d == d[0]):
            gap = min(gap, (d[p] - np.partition(d, -2)[-2]) / d[p])
        smallest = min(smallest, d[p])
        col = (K[:, p] - Lt[:j].T @ Lt[:j, p]) / np.sqrt(d[p])
        col[p] = np.sqrt(d[p])
        Lt[j], piv[j] = col, p
        d = d - col**2
        d[p] = 0.0
    return Lt, piv, trace, rank, gap, smallest


def _reference_matrix_free(column, diag, num, tol=0.0, floor=FLOOR, ties="first"):
    """The matrix-free twin of `_reference`, for candidate sets whose Gram matrix cannot be held: `column(p)` returns column p of K and
    `diag` its diagonal, both in np.longdouble; only d and the `num` rows of Lt are kept.  The same tuple, Lt and the traces rounded to
    float64 at the end.  `ties`: "first" - the smallest row among equal maxima, the rule - or "last" (tests only: the tie cases must
    tell the two apart)."""
    n = len(diag)
    d, Lt, piv, trace = np.array(diag, dtype=np.longdouble), np.zeros((num, n), dtype=np.longdouble), np.full(num, -1), np.zeros(num + 1, dtype=np.longdouble)
    rank, gap, smallest = num, np.inf, np.inf
    for j in range(num + 1):
        trace[j] = d.sum()
        if j == num:
            break
        p = int(np.argmax(d)) if ties == "first" else n - 1 - int(np.argmax(d[::-1]))
        if d[p] <= floor or trace[j] <= tol * trace[0] or not np.isfinite(d[p]):
            rank = j
            break
        if n > 1 and not np.all(d == d[0]):
            gap = min(gap, float((d[p] - np.partition(d, -2)[-2]) / d[p]))
        smallest = min(smallest, float(d[p]))
        col = (column(p) - Lt[:j].T @ Lt[:j, p]) / np.sqrt(d[p])
        col[p] = np.sqrt(d[p])
        Lt[j], piv[j] = col, p
        d = d - col**2
        d[p] = 0.0
    return Lt.astype(float), piv, trace.astype(float), rank, gap, smallest


def columns2d(name, x):
    """(column, diag) of kernels2d()[name] over the rows of x in np.longdouble, written out from the kernels' definitions: "eq" -
    1.3 exp(-1/2 sum_d ((x_d - x'_d) / s_d)^2) - and "eq+linear" - that with coefficient 1 plus sum_d (x_d / t_d) (x'_d / t_d),
    s = (0.3, 0.36), t = (1.5, 2.5)."""
    ld = np.longdouble
    xs, xt = x.astype(ld) / np.array([0.3, 0.36], dtype=ld), x.astype(ld) / np.array([1.5, 2.5], dtype=ld)
    coef = ld(13) / ld(10) if name == "eq" else ld(1)

    def column(p):
        col = coef * np.exp(-0.5 * np.sum((xs - xs[p]) ** 2, axis=1))
        return col + xt @ xt[p] if name == "eq+linear" else col

    diag = np.full(len(x), coef) + (np.sum(xt * xt, axis=1) if name == "eq+linear" else 0)
    return column, diag


def kernels2d():
    """The kernels of the comparisons, over two input columns (the choice of scales: module docstring)."""
    s = np.array([0.3, 0.36])
    return {
        "eq": (1.3 * EQ().stretch(s)).select([0, 1]),
        "rq": (0.9 * RQ(0.7).stretch(s)).select([0, 1]),
        "matern32": (1.1 * Matern32().stretch(s)).select([0, 1]),
        "eq*periodic": (1.2 * EQ().stretch(np.array([1.5, 1.65, 1.35, 1.8])).periodic(np.array([0.7, 0.9])) * EQ().stretch(np.array([1.0, 1.2]))).select([0, 1]),
        "eq+linear": (1.0 * EQ().stretch(s) + Linear().stretch(np.array([1.5, 2.5]))).select([0, 1]),
        # one component of a spectral mixture: the envelope keeps forty pivots apart, the cosine (periods 0.7 and 0.9) changes sign over the box
        "eq x cos": (1.2 * EQ().stretch(s) * Cosine().stretch(np.array([0.7, 0.9]))).select([0, 1]),
    }


def points(n, seed=20260):
    return np.random.default_rng(seed + n).uniform(0.0, 1.0, (n, 2))


def dense_gram(oracle, kernel, x):
    """The oracle's dense Gram matrix of `kernel` over the rows of x."""
    from oracle import kernels as ok

    return ok.gram(ok.spec_to_dict(kernel.resolve(x.shape[1])), x, None)


def assert_same(got, ref, kmax):
    """(Lt, piv, trace, rank) of a route against the reference's: pivots, rank and tails identical, Lt and trace within the bound."""
    Lt, piv, trace, rank = (to_np(t) for t in got)
    rLt, rpiv, rtrace, rrank = ref[:4]
    rank = int(rank.reshape(-1)[0])
    assert rank == rrank
    np.testing.assert_array_equal(piv, rpiv)
    assert np.all(piv[rank:] == -1) and np.all(Lt[rank:] == 0.0)
    b = bound(max(rank, 1), kmax)
    err_l, err_t = np.max(np.abs(Lt - rLt)), np.max(np.abs(trace[: rank + 1] - rtrace[: rank + 1]))
    print(f"rank {rank}: |Lt - ref| {err_l:.3g}, |trace - ref| {err_t:.3g} (bound {b:.3g})")
    assert err_l <= b and err_t <= b
    assert np.all(trace[rank + 1:] == 0.0)


@pytest.mark.parametrize("name", list(kernels2d()))
def test_composed_route_matches_the_numpy_reference(oracle_engine, name):
    kernel, x = kernels2d()[name], points(200)
    K = dense_gram(oracle_engine, kernel, x)
    ref = _reference(K, 40)
    assert ref[4] > GAP, f"the pivot order is not comparable between two roundings: smallest gap {ref[4]:.3g}"
    assert ref[3] == 40 and ref[5] > PIVOT_MIN
    got = greedy_inducing(oracle_engine, oracle_engine.compile(kernel, 2), x, 40)
    assert_same(got, ref, np.max(np.diag(K)))


@pytest.mark.parametrize("name", ["eq", "eq+linear"])
def test_matrix_free_reference_equals_the_dense_one(name):
    x = points(600)
    K = dense_gram(None, kernels2d()[name], x)
    ref = _reference(K, 40)
    assert ref[4] > GAP and ref[3] == 40 and ref[5] > PIVOT_MIN
    free = _reference_matrix_free(*columns2d(name, x), 40)
    assert free[3] == 40 and free[4] > GAP and free[5] > PIVOT_MIN
    np.testing.assert_array_equal(free[1], ref[1])
    b = bound(40, np.max(np.diag(K)))
    err_l, err_t = np.max(np.abs(free[0] - ref[0])), np.max(np.abs(free[2] - ref[2]))
    print(f"{name}: matrix-free longdouble against dense float64: |Lt| {err_l:.3g}, |trace| {err_t:.3g} (bound {b:.3g})")
    assert err_l <= b and err_t <= b
    # the tie rule is part of the twin: on exact ties (a stationary kernel: every d_i the same number) the smallest row, and a twin
    # that breaks ties towards the larger row is told apart by the cases that rest on it
    column, diag = columns2d("eq", x)
    assert _reference_matrix_free(column, diag, 1)[1][0] == 0 and _reference_matrix_free(column, diag, 1, ties="last")[1][0] == 599
    x[41] = x[17] = [1.5, 1.5]
    column, diag = columns2d("eq+linear", x)
    first, last = _reference_matrix_free(column, diag, 8), _reference_matrix_free(column, diag, 8, ties="last")
    assert first[1][0] == 17 and 41 not in first[1] and last[1][0] == 41


def test_tie_goes_to_the_smaller_row_and_the_twin_is_never_picked(oracle_engine):
    # EQ + linear: the row farthest from the origin holds the largest prior variance; its copy sits at a LARGER index
    kernel, x = kernels2d()["eq+linear"], points(60)
    x[17] = [1.5, 1.5]
    x[41] = x[17]
    Lt, piv, trace, rank = (to_np(t) for t in greedy_inducing(oracle_engine, oracle_engine.compile(kernel, 2), x, 30))
    assert piv[0] == 17 and 41 not in piv[: int(rank[0])]
    K = dense_gram(oracle_engine, kernel, x)
    residual = np.diag(K) - np.sum(Lt**2, axis=0)
    assert residual[41] <= FLOOR
    # the same with the copy at the SMALLER index
    x[5] = x[17]
    piv = to_np(greedy_inducing(oracle_engine, oracle_engine.compile(kernel, 2), x, 30)[1])
    assert piv[0] == 5 and 17 not in piv and 41 not in piv


def linear_rank3():
    """300 points under a purely linear kernel on three feature dims: a Gram matrix of rank 3."""
    x = np.random.default_rng(7).standard_normal((300, 3))
    return Linear().stretch(np.array([1.0, 2.0, 0.5])).select([0, 1, 2]), x


def assert_rank3(got):
    Lt, piv, trace, rank = (to_np(t) for t in got)
    assert int(rank[0]) == 3 and np.all(piv[:3] >= 0) and np.all(piv[3:] == -1)
    assert np.all(Lt[3:] == 0.0) and np.any(Lt[2] != 0.0)
    assert trace[3] <= 1e-10 * trace[0]


def test_rank_stop_on_a_linear_kernel(oracle_engine):
    kernel, x = linear_rank3()
    assert_rank3(greedy_inducing(oracle_engine, oracle_engine.compile(kernel, 3), x, 10))


def cosine_rank2():
    """300 points under a pure cosine kernel over two columns: cos(a - b) = cos a cos b + sin a sin b, a Gram matrix of rank 2."""
    x = np.random.default_rng(8).uniform(0.0, 1.0, (300, 2))
    return (1.3 * Cosine().stretch(np.array([0.7, 0.45]))).select([0, 1]), x


def assert_rank2(got, K):
    """As `assert_rank3`; and the residual diagonal after the two pivots is at most 1e-12 everywhere."""
    Lt, piv, trace, rank = (to_np(t) for t in got)
    assert int(rank[0]) == 2 and np.all(piv[:2] >= 0) and np.all(piv[2:] == -1)
    assert np.all(Lt[2:] == 0.0) and np.any(Lt[1] != 0.0)
    assert trace[2] <= 1e-10 * trace[0]
    residual = np.diag(K) - np.sum(Lt[:2] ** 2, axis=0)
    assert np.max(np.abs(residual)) <= 1e-12, np.max(np.abs(residual))


def test_rank_stop_on_a_pure_cosine_kernel(oracle_engine):
    kernel, x = cosine_rank2()
    K = dense_gram(oracle_engine, kernel, x)
    ref = _reference(K, 10)
    assert ref[3] == 2 and np.max(np.abs(np.diag(K) - np.sum(ref[0] ** 2, axis=0))) <= 1e-12   # the reference alone
    assert_rank2(greedy_inducing(oracle_engine, oracle_engine.compile(kernel, 2), x, 10), K)


def test_tol_stop(oracle_engine):
    kernel, x = kernels2d()["eq"], points(200)
    ref = _reference(dense_gram(oracle_engine, kernel, x), 40)
    first = int(np.argmax(ref[2] <= 0.5 * ref[2][0]))   # the first j at which the reference's trace has fallen to half
    assert 0 < first < 40 and abs(ref[2][first] - 0.5 * ref[2][0]) > 1e-6
    Lt, piv, trace, rank = (to_np(t) for t in greedy_inducing(oracle_engine, oracle_engine.compile(kernel, 2), x, 40, tol=0.5))
    assert int(rank[0]) == first and np.all(piv[first:] == -1) and np.all(Lt[first:] == 0.0)
    np.testing.assert_array_equal(piv[:first], ref[1][:first])


_REG = dict(scale=0.3, linear=True, nonlinear=True, noise=0.1, normalise_y=False)


def regression_data(n, p=2, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (n, 2))
    y = np.stack([np.sin(5.0 * x[:, 0]) + x[:, 1], np.cos(4.0 * x[:, 1]) * x[:, 0]], axis=1)[:, :p]
    return x, y + 0.05 * rng.standard_normal(y.shape)


def test_select_inducing_returns_rows_of_x(oracle_engine):
    x, _ = regression_data(150)
    reg = GPARRegressor(**_REG)
    x_ind, index, trace = reg.select_inducing(x, 12)
    assert x_ind.shape == (12, 2) and index.shape == (12,) and trace.shape == (13,)
    np.testing.assert_array_equal(x_ind, x[index])
    assert len(set(index.tolist())) == 12 and np.all(np.diff(trace) < 0.0)
    assert reg.x_ind is None and reg.sparse is False and not reg.is_conditioned
    # the first layer's kernel at the values in reg.vs: the variables exist now, with fit's names and initial values
    assert {"0/input/var", "0/input/scales"} <= set(reg.get_variables())
    np.testing.assert_allclose(reg.get_variables()["0/input/scales"], 0.3)
    K = dense_gram(oracle_engine, (1.0 * EQ().stretch(np.array([0.3, 0.3]))).select([0, 1]), x)
    np.testing.assert_array_equal(index, _reference(K, 12)[1])


def test_select_inducing_assign_equals_the_constructor(oracle_engine):
    x, y = regression_data(150)
    reg = GPARRegressor(**_REG)
    reg.condition(x, y)
    x_ind, _, _ = reg.select_inducing(x, 12, assign=True)
    assert reg.sparse is True and not reg.is_conditioned and reg.x is None
    np.testing.assert_array_equal(to_np(reg.x_ind), x_ind)
    built = GPARRegressor(x_ind=x_ind, **_REG)
    assert float(reg.logpdf(x, y)) == float(built.logpdf(x, y))


def test_select_inducing_assign_replaces_trained_inducing_inputs(oracle_engine):
    """After fit(optimise_x_ind=True) the inducing inputs live on as the variable "x_ind" of the store; assigning selected rows - with
    the trained length scales, the flow the method is for - must make the model see them, whatever their number."""
    x, y = regression_data(120)
    reg = GPARRegressor(x_ind=x[:8], **_REG)
    reg.fit(x, y, iters=2, optimise_x_ind=True)
    assert "x_ind" in reg.vs
    x_ind, _, _ = reg.select_inducing(x, 12, assign=True)
    assert "x_ind" not in reg.vs and to_np(reg.x_ind).shape == (12, 2)
    built = GPARRegressor(x_ind=x_ind, **_REG)
    built.vs = reg.vs.copy(detach=True)
    assert float(reg.logpdf(x, y)) == float(built.logpdf(x, y))
    # ... and they are where a later optimisation of the inducing inputs starts
    reg.fit(x, y, iters=1, optimise_x_ind=True)
    assert to_np(reg.vs["x_ind"]).shape == (12, 2)


def test_composed_route_ranks_a_nan_above_an_infinity(oracle_engine):
    from gpar_amd.gp import _pivoted_cholesky_composed
    from gpar_amd.engine import NotPositiveDefiniteError

    kernel, x = kernels2d()["eq+linear"], points(50)
    x[3, 0] = np.inf    # prior variance +inf at the smaller row
    x[20, 1] = np.nan   # ... NaN at the larger one: the NaN is the pivot (include/gpar_hip.h)
    with pytest.raises(NotPositiveDefiniteError) as caught:
        _pivoted_cholesky_composed(oracle_engine, oracle_engine.compile(kernel, 2), oracle_engine.tensor(x), 5, 0.0, FLOOR)
    assert caught.value.info == 21


def test_select_inducing_argument_errors(oracle_engine):
    x, y = regression_data(50)
    reg = GPARRegressor(**_REG)
    with pytest.raises(ValueError):
        reg.select_inducing(x, 0)
    with pytest.raises(ValueError):
        reg.select_inducing(x, 51)
    reg.condition(x, y)
    with pytest.raises(ValueError):
        reg.select_inducing(x[:, :1], 5)


def test_greedy_rows_beat_random_rows_on_clustered_inputs(oracle_engine):
    """400 points on a line, 90 % of them in [0, 0.1]: twenty greedily chosen rows leave less than half the residual trace
    tr(K - K_xz K_zz^-1 K_zx) that the first twenty rows of a fixed random permutation leave."""
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.uniform(0.0, 0.1, 360), rng.uniform(0.1, 1.0, 40)])[:, None]
    x = x[rng.permutation(400)]
    kernel = (1.0 * EQ().stretch(np.array([0.05]))).select([0])
    K = dense_gram(oracle_engine, kernel, x)
    some = np.random.default_rng(12).permutation(400)[:20]
    Kzz = K[np.ix_(some, some)] + FLOOR * np.eye(20)
    random_trace = np.trace(K) - np.trace(K[:, some] @ np.linalg.solve(Kzz, K[some, :]))
    ref = _reference(K, 20)
    assert ref[3] == 20 and ref[2][20] < 0.5 * random_trace, (ref[2][20], random_trace)   # the reference alone, with that margin
    trace = to_np(greedy_inducing(oracle_engine, oracle_engine.compile(kernel, 1), x, 20)[2])
    assert trace[20] < 0.5 * random_trace
    np.testing.assert_allclose(trace, ref[2], rtol=0, atol=bound(20, 1.0))
