"""The fused greedy pivoted Cholesky (gpar_pivoted_chol through `HipEngine.pivoted_cholesky`) on the GPU: against the route composed of
the engine's own primitives (`gp._pivoted_cholesky_composed`: gpar_gram_diag, gpar_gram against the pivot's row, torch), by invariants
that need no pivot order, and from `GPARRegressor.select_inducing` to a trained sparse model.

The comparisons carry the assertions of tests/test_select_inducing.py on the numpy reference first (gap between the two largest
residuals above 1e-9 at every step, pivots above `PIVOT_MIN`), and its tolerance:

    bound(k, kmax) = 8 ((k + 1) 2^-53 kmax + 1e-13 kmax + 1e-14)

(backward error of a rank-k Cholesky with |L||L^T| <= max diag K = kmax, plus the tolerance tests/test_hip_primitives.py holds gpar_gram
to against the oracle - the fused column kernel uses libm's exp, gpar_gram its tables - taken 8 times).  Evaluated for the cases here:
k = 40, kmax = 1.3 (EQ): 1.2e-12;  k = 64, kmax = 1.60 (EQ + linear, n = 600): 1.4e-12;  k = 96, kmax = 1: 9.7e-13.  `Lt` and the traces
of the two routes are held to it; only where a trace is RECOMPUTED here as a sum of n residuals, each of them held to the bound (the
invariants test), is it held to n times the bound.

Past one workgroup's reach: every launch opens by reducing the previous launch's partials with `for (w = tid; w < nwg; w += 256)`, which
takes a second iteration only from 257 workgroups on - n = 65793 (257 full workgroups and one row, 258 partials) against the matrix-free
longdouble reference of tests/test_select_inducing.py, with a planted maximum and exact ties in workgroup 256 -, and the pivot's row
of the factor is staged with `for (t = tid; t < j; t += 256)`, which takes a second pass from step 257 on - 300 steps at n = 300, 264
at n = 600, under an EQ kernel over six columns (length scales 0.5) that keeps the reference's pivots above 1e-4 and its gaps above
1e-6.  bound(6, 2.36) = 2.0e-12, bound(300, 1) = 1.2e-12.
"""
import numpy as np
import pytest
import torch

from gpar_amd import greedy_inducing
from gpar_amd.engine import NotPositiveDefiniteError
from gpar_amd.gp import _pivoted_cholesky_composed
from gpar_amd.kernels import EQ, Linear
from gpar_amd.regression import GPARRegressor

from .conftest import make_engine, to_np
from .test_select_inducing import (FLOOR, GAP, PIVOT_MIN, _reference, _reference_matrix_free, assert_rank2, assert_rank3, assert_same, bound,
                                   columns2d, cosine_rank2, dense_gram, kernels2d, linear_rank3, points, regression_data)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from gpar_amd.engine import set_engine

    engine = make_engine("hip")
    previous = set_engine(engine)
    yield engine
    set_engine(previous)


def _wide():
    """A structure of 20 feature dims (more than the 16 up to which Gram kernels are generated): EQ over 16 columns + linear over 4."""
    cols = list(range(20))
    kernel = (1.1 * EQ().stretch(np.full(16, 3.0))).select(cols[:16]) + Linear().stretch(np.full(4, 2.0)).select(cols[16:])
    return kernel, np.random.default_rng(5).uniform(0.0, 1.0, (300, 20))


def _both_routes(eng, kernel, x, num, tol=0.0):
    ck = eng.compile(kernel, x.shape[1])
    z = eng.features(ck, eng.tensor(x))
    fused = eng.pivoted_cholesky(ck, z, num, tol=tol)
    composed = _pivoted_cholesky_composed(eng, ck, z, num, tol, eng.epsilon)
    return fused, composed


def _compare(eng, kernel, x, num):
    K = dense_gram(None, kernel, x)
    ref = _reference(K, num)
    assert ref[4] > GAP, f"the pivot order is not comparable between two roundings: smallest gap {ref[4]:.3g}"
    assert ref[3] == num and ref[5] > PIVOT_MIN
    fused, composed = _both_routes(eng, kernel, x, num)
    cLt, cpiv, ctrace, crank = (to_np(t) for t in composed)
    np.testing.assert_array_equal(cpiv, ref[1])
    assert_same(fused, (cLt, cpiv, ctrace, int(crank[0])), np.max(np.diag(K)))


@pytest.mark.parametrize("name", list(kernels2d()))
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 600])
def test_fused_matches_composed(eng, n, name):
    _compare(eng, kernels2d()[name], points(n), min(n, 40))


def test_fused_matches_composed_on_a_wide_structure(eng):
    kernel, x = _wide()
    assert eng.compile(kernel, 20).dz == 20
    _compare(eng, kernel, x, 40)


@pytest.mark.parametrize("name", list(kernels2d()))
def test_invariants_of_the_fused_result(eng, name):
    """What must hold whatever the pivot order, at n = 600 (three workgroups), 64 steps; K is the engine's own Gram matrix."""
    from gpar_amd import hip

    n, num = 600, 64
    kernel, x = kernels2d()[name], points(n)
    ck = eng.compile(kernel, 2)
    z = eng.features(ck, eng.tensor(x))
    Lt, piv, trace, rank, info, d = (to_np(t) for t in hip.pivoted_chol(ck, z, num, 0.0, eng.epsilon))
    K = to_np(eng.gram(ck, z))
    k = int(rank[0])
    assert int(info[0]) == 0 and 1 <= k <= num
    piv = piv[:k]
    b = bound(k, np.max(np.diag(K)))
    assert len(set(piv.tolist())) == k and np.all((piv >= 0) & (piv < n))
    # Lt[:k, piv] transposed is lower triangular with a positive diagonal: above it stand residual covariances of rows picked earlier,
    # zero up to the bound before the division by the pivot's root Lt[t, piv[t]]
    T = Lt[:k][:, piv].T
    assert np.all(np.diag(T) > 0.0)
    assert np.max(np.abs(np.triu(T, 1)) * np.diag(T)[None, :]) <= b
    # the columns of K at the pivots are reproduced
    err = np.max(np.abs(Lt[:k].T @ Lt[:k][:, piv] - K[:, piv]))
    # the residual diagonal, and the traces recomputed from the factor
    resid = np.diag(K)[None, :] - np.concatenate([np.zeros((1, n)), np.cumsum(Lt[:k] ** 2, axis=0)])   # row j: before step j
    err_d = np.max(np.abs(resid[k] - d))
    err_t = np.max(np.abs(resid.sum(axis=1) - trace[: k + 1]))
    short = np.max([resid[j].max() - resid[j, piv[j]] for j in range(k)])
    print(f"{name}: rank {k}, bound {b:.3g}: columns {err:.3g}, residual {err_d:.3g}, min residual {d.min():.3g}, trace {err_t:.3g} "
          f"(n bound {n * b:.3g}), pivot below the maximum by {short:.3g}")
    assert err <= b and err_d <= b and d.min() >= -b and resid[k].min() >= -b
    assert err_t <= n * b
    assert short <= b


def test_full_rank_reproduces_the_matrix(eng):
    kernel, x = (1.0 * EQ().stretch(np.array([0.15, 0.15]))).select([0, 1]), points(96)
    K = dense_gram(None, kernel, x)
    ref = _reference(K, 96)
    assert ref[3] == 96 and ref[5] > 1e3 * FLOOR   # the residual stays above the floor for all 96 steps
    Lt, piv, trace, rank = (to_np(t) for t in greedy_inducing(eng, eng.compile(kernel, 2), x, 96))
    assert int(rank[0]) == 96 and sorted(piv.tolist()) == list(range(96))
    err = np.max(np.abs(Lt.T @ Lt - K))
    print(f"full rank: |Lt^T Lt - K| {err:.3g} (bound {bound(96, 1.0):.3g}), final trace {trace[96]:.3g}")
    assert err <= bound(96, 1.0) and abs(trace[96]) <= bound(96, 1.0)


def test_two_runs_give_the_same_bits(eng):
    from gpar_amd import hip

    kernel, x = kernels2d()["eq+linear"], points(600)
    ck = eng.compile(kernel, 2)
    z = eng.features(ck, eng.tensor(x))
    first = [to_np(t).copy() for t in eng.pivoted_cholesky(ck, z, 40)]
    second = [to_np(t).copy() for t in eng.pivoted_cholesky(ck, z, 40)]
    # ... and a third while another stream factors a matrix
    A = eng.new_matrix(1536, 1536)
    A.copy_(torch.eye(1536, dtype=torch.float64, device=A.device) * 4.0 + 1e-3)
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream(eng.device))
    with torch.cuda.stream(side):
        _, info = hip.potrf_(A)
    third = [to_np(t).copy() for t in eng.pivoted_cholesky(ck, z, 40)]
    torch.cuda.current_stream(eng.device).wait_stream(side)
    assert int(info.item()) == 0
    for a, b, c in zip(first, second, third):
        assert a.tobytes() == b.tobytes() == c.tobytes()


def test_stops_on_the_device_for_a_pure_cosine_kernel(eng):
    """Rank 2 (tests/test_select_inducing.py: cosine_rank2): the fused route stops after two pivots, with the pivots of the composed
    route and of the numpy reference, and leaves a residual diagonal of at most 1e-12."""
    kernel, x = cosine_rank2()
    K = dense_gram(None, kernel, x)
    ref = _reference(K, 10)
    fused, composed = _both_routes(eng, kernel, x, 10)
    assert_rank2(fused, K)
    assert_rank2(composed, K)
    np.testing.assert_array_equal(to_np(fused[1]), to_np(composed[1]))
    # (the first step is an exact tie, row 0; the second has a clear maximum on the reference)
    np.testing.assert_array_equal(to_np(fused[1])[:2], ref[1][:2])
    np.testing.assert_allclose(to_np(fused[0])[:2], ref[0][:2], rtol=0, atol=bound(2, 1.3))


def test_stops_on_the_device(eng):
    kernel, x = linear_rank3()
    assert_rank3(greedy_inducing(eng, eng.compile(kernel, 3), x, 10))
    kernel, x = kernels2d()["eq"], points(200)
    ref = _reference(dense_gram(None, kernel, x), 40)
    first = int(np.argmax(ref[2] <= 0.5 * ref[2][0]))
    assert 0 < first < 40 and abs(ref[2][first] - 0.5 * ref[2][0]) > 1e-6
    Lt, piv, trace, rank = (to_np(t) for t in greedy_inducing(eng, eng.compile(kernel, 2), x, 40, tol=0.5))
    assert int(rank[0]) == first and np.all(piv[first:] == -1) and np.all(Lt[first:] == 0.0) and np.all(trace[first + 1:] == 0.0)
    np.testing.assert_array_equal(piv[:first], ref[1][:first])


def test_a_nan_row_is_reported_through_the_deferred_check(eng):
    # (EQ + linear: the prior variance of a row depends on its features, so the NaN is in d from the start and ranks first)
    kernel, x = kernels2d()["eq+linear"], points(300)
    x[37, 1] = np.nan
    with pytest.raises(NotPositiveDefiniteError) as caught:
        with eng.defer_checks():
            Lt, piv, trace, rank = greedy_inducing(eng, eng.compile(kernel, 2), x, 20)
    assert caught.value.info == 38
    assert int(rank.item()) == 0 and np.all(to_np(piv) == -1) and np.all(to_np(Lt) == 0.0)
    # a NaN ranks above every number, +inf at a smaller row included
    x[5, 0] = np.inf
    with pytest.raises(NotPositiveDefiniteError) as caught:
        greedy_inducing(eng, eng.compile(kernel, 2), x, 20)
    assert caught.value.info == 38


def test_select_inducing_to_a_trained_sparse_model(eng):
    x, y = regression_data(500)
    kw = dict(replace=True, scale=0.3, linear=True, nonlinear=True, noise=0.1)
    reg = GPARRegressor(**kw)
    x_ind, index, trace = reg.select_inducing(x, 32, assign=True)
    assert x_ind.shape == (32, 2) and reg.sparse and np.all(np.diff(trace) < 0.0)
    np.testing.assert_array_equal(x_ind, x[index])
    built = GPARRegressor(x_ind=x_ind, **kw)
    value = float(reg.logpdf(x, y))
    np.testing.assert_allclose(value, float(built.logpdf(x, y)), rtol=1e-8)   # (the sparse parity tolerance of tests/test_parity_gpu.py)
    reg.fit(x, y, iters=3)
    assert np.isfinite(float(reg.logpdf(x, y)))
    mean, var = reg.predict_moments(x[:50])
    assert mean.shape == (50, 2) and np.all(np.isfinite(mean)) and np.all(var > 0.0)


# ---- past one workgroup's reach: more than 256 workgroups, more than 256 steps, the raw entry's corners -----------------------------------
MANY = 65793   # 257 full workgroups and one row: 258 partials, thread 0 of the reduction reads workgroups 0 and 256, thread 1 reads 1 and 257


def _fused_raw(eng, kernel, x, num, floor=None):
    from gpar_amd import hip

    ck = eng.compile(kernel, x.shape[1])
    z = eng.features(ck, eng.tensor(x))
    out = hip.pivoted_chol(ck, z, num, 0.0, eng.epsilon if floor is None else floor)
    torch.cuda.synchronize()
    return [to_np(t).copy() for t in out]   # Lt, piv, trace, rank, info, d


def _against_matrix_free(got, ref, kmax, n):
    """Lt, piv, trace of `hip.pivoted_chol` against the matrix-free reference: the preconditions on the reference first."""
    Lt, piv, trace, rank, info, _ = got
    num = len(piv)
    assert ref[4] > GAP, f"the pivot order is not comparable between two roundings: smallest gap {ref[4]:.3g}"
    assert ref[3] == num and ref[5] > PIVOT_MIN
    assert int(info[0]) == 0 and int(rank[0]) == num
    np.testing.assert_array_equal(piv, ref[1])
    b = bound(num, kmax)
    err_l, err_t = np.max(np.abs(Lt - ref[0])), np.max(np.abs(trace - ref[2]))
    print(f"n = {n}, {num} steps: |Lt - ref| {err_l:.3g} (bound {b:.3g}), |trace - ref| {err_t:.3g} (n bound {n * b:.3g})")
    assert err_l <= b
    assert err_t <= n * b   # (each trace is a sum of n residuals, every one of them within the bound: the invariants test's rule)


def test_a_planted_maximum_in_workgroup_256_is_found_through_the_second_pass_over_the_partials(eng):
    n = MANY
    x = points(n)
    x[65600] = [1.5, 1.5]   # the largest norm: the largest prior variance under EQ + linear; 65600 = 256 * 256 + 64
    column, diag = columns2d("eq+linear", x)
    ref = _reference_matrix_free(column, diag, 6)
    got = _fused_raw(eng, kernels2d()["eq+linear"], x, 6)
    assert ref[1][0] == 65600 and got[1][0] == 65600
    groups = ref[1] // 256
    assert (groups < 256).any() and (groups >= 256).any()
    _against_matrix_free(got, ref, float(np.max(diag)), n)
    again = _fused_raw(eng, kernels2d()["eq+linear"], x, 6)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()


def test_exact_ties_across_the_two_passes_over_the_partials_go_to_the_smaller_row(eng):
    n = MANY
    x = points(n)
    # a stationary kernel: every d_i is the same number, in every workgroup's partial - thread 0 meets the rows 0 and 65536
    Lt, piv, trace, rank, info, _ = _fused_raw(eng, kernels2d()["eq"], x, 2)
    ref = _reference_matrix_free(*columns2d("eq", x), 2)
    assert int(info[0]) == 0 and int(rank[0]) == 2 and piv[0] == 0 and ref[1][0] == 0
    assert abs(trace[0] - ref[2][0]) <= n * bound(2, 1.3)
    # two bit-identical points of largest norm, rows 300 (workgroup 1) and 65700 (workgroup 256)
    x[300] = x[65700] = [1.5, 1.5]
    column, diag = columns2d("eq+linear", x)
    ref = _reference_matrix_free(column, diag, 6)
    got = _fused_raw(eng, kernels2d()["eq+linear"], x, 6)
    assert ref[1][0] == 300 and 65700 not in ref[1] and ref[5] > PIVOT_MIN
    assert got[1][0] == 300 and 65700 not in got[1] and int(got[3][0]) == 6
    np.testing.assert_array_equal(got[1], ref[1])
    b = bound(6, float(np.max(diag)))
    assert np.max(np.abs(got[0] - ref[0])) <= b and abs(got[2][0] - ref[2][0]) <= n * b


def long_run(n):
    """EQ over six columns, length scales 0.5, on n uniform points: full rank far above the floor (the module docstring)."""
    cols = list(range(6))
    return (1.0 * EQ().stretch(np.full(6, 0.5))).select(cols), np.random.default_rng(77 + n).uniform(0.0, 1.0, (n, 6))


@pytest.mark.parametrize("n,num", [(300, 300), (600, 264)])
def test_more_than_256_steps_against_the_dense_reference(eng, n, num):
    kernel, x = long_run(n)
    K = dense_gram(None, kernel, x)
    ref = _reference(K, num)
    assert ref[3] == num and ref[5] > 1e3 * FLOOR   # the residual stays above the floor for all the steps ...
    assert ref[4] > GAP and ref[5] > PIVOT_MIN      # ... and the pivot order is comparable between two roundings
    got = greedy_inducing(eng, eng.compile(kernel, 6), x, num)
    assert_same(got, ref, 1.0)
    if n == num:
        Lt = to_np(got[0])
        err = np.max(np.abs(Lt.T @ Lt - K))
        print(f"full rank at {n}: |Lt^T Lt - K| {err:.3g} (bound {bound(n, 1.0):.3g})")
        assert sorted(to_np(got[1]).tolist()) == list(range(n)) and err <= bound(n, 1.0)


@pytest.mark.parametrize("n,max_rank", [(2, 5), (257, 300)])
def test_more_steps_than_rows_stop_at_rank_n(eng, n, max_rank):
    kernel, x = long_run(300)
    x = x[:n]
    ref = _reference(dense_gram(None, kernel, x), n)
    assert ref[3] == n and ref[5] > PIVOT_MIN
    Lt, piv, trace, rank, info, d = _fused_raw(eng, kernel, x, max_rank)
    assert int(rank[0]) == n and int(info[0]) == 0
    assert sorted(piv[:n].tolist()) == list(range(n)) and np.all(piv[n:] == -1)
    assert np.all(Lt[n:] == 0.0) and np.all(trace[n + 1:] == 0.0)
    assert np.all(d <= 0.0) and d.min() >= -bound(n, 1.0)   # (every row was picked: 0 then, and below it only by later steps' rounding)
    np.testing.assert_array_equal(piv[:n], ref[1])
    assert np.max(np.abs(Lt[:n] - ref[0])) <= bound(n, 1.0)


def _raw_call(eng, ck, z, n, max_rank, ldz, ldl, tol=0.0, floor=FLOOR):
    """gpar_pivoted_chol with every buffer allocated here and prefilled with -7: (status, z buffer, Lt buffer, piv, trace, words)."""
    import ctypes

    from gpar_amd import _lib
    from gpar_amd import hip

    lib, dev = _lib.load(), z.device
    zb = torch.full((n, ldz), -7.0, dtype=torch.float64, device=dev)
    zb[:, : z.shape[1]] = z
    Lb = torch.full((max_rank, max(ldl, 1)), -7.0, dtype=torch.float64, device=dev)
    piv = torch.full((max_rank,), -7, dtype=torch.int32, device=dev)
    trace = torch.full((max_rank + 1,), -7.0, dtype=torch.float64, device=dev)
    words = torch.full((2,), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.gpar_workspace_doubles(_lib.WS_PIVOTED_CHOL, n, 0, 0), dtype=torch.float64, device=dev)
    rc = lib.gpar_pivoted_chol(ctypes.byref(ck.kspec), zb.data_ptr(), n, ldz, ck.dz, max_rank, float(tol), float(floor), Lb.data_ptr(), ldl,
                               piv.data_ptr(), trace.data_ptr(), words.data_ptr(), words[1:].data_ptr(), ws.data_ptr(), hip.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, zb, Lb, piv, trace, words


def test_padded_leading_dimensions_give_the_same_bits_and_leave_the_padding(eng):
    n, num = 257, 40
    kernel, x = kernels2d()["eq+linear"], points(n)
    ck = eng.compile(kernel, 2)
    z = eng.features(ck, eng.tensor(x))
    dz = ck.dz
    assert z.shape[1] == dz
    rc, _, Lt, piv, trace, words = _raw_call(eng, ck, z, n, num, dz, n)
    assert rc == 0 and words.tolist() == [num, 0]
    rc, zp, Lp, pivp, tracep, wordsp = _raw_call(eng, ck, z, n, num, dz + 3, n + 5)
    assert rc == 0 and wordsp.tolist() == [num, 0]
    assert torch.equal(Lp[:, :n], Lt) and torch.equal(pivp, piv) and torch.equal(tracep, trace)
    assert bool((Lp[:, n:] == -7.0).all()) and bool((zp[:, dz:] == -7.0).all()) and torch.equal(zp[:, :dz], z)


def test_argument_errors_of_the_raw_entry_touch_nothing(eng):
    n = 257
    kernel, x = kernels2d()["eq+linear"], points(n)
    ck = eng.compile(kernel, 2)
    z = eng.features(ck, eng.tensor(x))
    for told in (dict(max_rank=4097), dict(ldl=n - 1), dict(floor=-1e-12)):
        args = dict(max_rank=8, ldz=ck.dz, ldl=n, floor=FLOOR)
        args.update(told)
        rc, _, Lt, piv, trace, words = _raw_call(eng, ck, z, n, **args)
        assert -1100 < rc <= -1001, (told, rc)   # (an argument error: -(1000 + the argument group))
        assert words.tolist() == [-7, -7], told
        assert bool((Lt == -7.0).all()) and bool((piv == -7).all()) and bool((trace == -7.0).all()), told
