"""Streaming conditioning on the GPU: gpar_chol_drop_leading and gpar_chol_append through the C ABI, then `GPARRegressor.update` end to end.

Matrices: EQ (length scale 0.3 on [0, 1]) + noise 0.05 + jitter 1e-12.  The updated factor cannot be held to an absolute figure that can
be derived, so it is measured against the reference: the residual |L' L'^T - S22|_max (products in extended precision, so that the
figure is the factor's and not the product's) may be at most 8 x the residual of the reference's own factor of the same matrix - the
margin covers the longer chain of roundings, n + k products per entry against n.  Entries of the factor, L^-1 y, the log-determinant and
the corner follow the parity rules of tests/test_loo_gpu.py for means and variances: rtol 1e-8 / atol 1e-10.  Every test prints the
ratio it measured (run with -s; the worst ones are recorded in profiles/update_times.txt).

Sizes (n, k) of the drop: below one 64-column panel, exactly one, one over, across a 128-wide GEMM tile, across the first 512-column
boundary, and k at and above one slab of 64 update vectors.  Nothing here uses more than 513 rows."""
import numpy as np
import pytest
import torch

from .conftest import make_engine
from .test_update import CONFIG, assert_same_posterior, fresh_like, make_data, run_steps

pytestmark = pytest.mark.gpu

DROP_SIZES = [(7, 1), (64, 1), (65, 5), (130, 64), (130, 65), (513, 3), (513, 130)]
APPEND_SIZES = [(7, 1), (64, 1), (64, 65), (130, 3), (512, 1), (513, 64)]
RTOL, ATOL, MARGIN = 1e-8, 1e-10, 8.0


@pytest.fixture
def hip():
    from gpar_amd.engine import set_engine

    eng = make_engine("hip")
    previous = set_engine(eng)
    yield eng
    set_engine(previous)


_PROBLEMS = {}


def _problem(n):
    """(S, y) of n rows, computed once and shared (never modified)."""
    if n not in _PROBLEMS:
        rng = np.random.default_rng(1000 + n)
        x = np.sort(rng.uniform(0, 1, n))
        S = np.exp(-0.5 * (x[:, None] - x[None, :]) ** 2 / 0.3 ** 2) + (0.05 + 1e-12) * np.eye(n)
        _PROBLEMS[n] = (S, rng.standard_normal(n))
    return _PROBLEMS[n]


def _augmented(S, y):
    """numpy's augmented factor [[L, nan], [z^T, -|z|^2]] and log-determinant."""
    import scipy.linalg

    n = len(y)
    L = np.linalg.cholesky(S)
    z = scipy.linalg.solve_triangular(L, y, lower=True)
    A = np.full((n + 1, n + 1), np.nan)   # (the strict upper triangle is never read: NaN there must not surface)
    A[np.tril_indices(n)] = L[np.tril_indices(n)]
    A[n, :n], A[n, n] = z, -(z @ z)
    return A, 2.0 * np.sum(np.log(np.diag(L)))


def _residual(L, S):
    Lx = np.tril(L).astype(np.longdouble)
    return float(np.max(np.abs(Lx @ Lx.T - S.astype(np.longdouble))))


def _upload(A, dev, ld=None):
    from gpar_amd import hip as h

    rows, cols = A.shape
    if ld is None:
        out = h.alloc_matrix(rows, cols, dev)
    else:
        out = torch.empty(rows, ld, dtype=torch.float64, device=dev)[:, :cols]
    out.copy_(torch.from_numpy(A))
    return out


def _drop(A, k, out):
    """gpar_chol_drop_leading through the binding's raw entry: (logdet, info) as host numbers after one synchronisation."""
    from gpar_amd import _lib, hip as h

    lib = _lib.load()
    n = A.shape[0] - 1
    ws = torch.empty(lib.gpar_workspace_doubles(_lib.WS_CHOL_UPDATE, n, k, 0), dtype=torch.float64, device=A.device)
    logdet = torch.full((1,), np.nan, dtype=torch.float64, device=A.device)
    info = torch.zeros(1, dtype=torch.int32, device=A.device)
    rc = lib.gpar_chol_drop_leading(A.data_ptr(), n, k, h._ld(A), out.data_ptr(), h._ld(out), ws.data_ptr(), logdet.data_ptr(),
                                    info.data_ptr(), h.stream_ptr(A.device))
    assert rc == 0
    return float(logdet.cpu()), int(info.cpu())


def _check_against(got, want, got_logdet, want_logdet, S, what):
    size = want.shape[0] - 1
    il = np.tril_indices(size + 1)
    ratio = _residual(got[:size, :size], S) / _residual(want[:size, :size], S)
    print(f"{what}: residual ratio {ratio:.3f}, max |dL| {np.max(np.abs(got[il] - want[il])):.3e}, dlogdet {abs(got_logdet - want_logdet):.3e}")
    assert ratio <= MARGIN
    np.testing.assert_allclose(got[il], want[il], rtol=RTOL, atol=ATOL)   # the factor, L^-1 y and the corner
    np.testing.assert_allclose(got_logdet, want_logdet, rtol=RTOL, atol=ATOL)


def test_workspace_and_limits(hip):
    from gpar_amd import _lib

    lib = _lib.load()
    assert lib.gpar_workspace_doubles(_lib.WS_CHOL_UPDATE, 130, 65, 0) == (130 - 65 + 1) * 66 + 128 * 65
    assert lib.gpar_workspace_doubles(_lib.WS_CHOL_UPDATE, 130, 130, 0) == -1
    assert lib.gpar_workspace_doubles(_lib.WS_CHOL_UPDATE, 4096, _lib.CHOL_UPDATE_MAX_RANK + 1, 0) == -1
    A = torch.zeros(8, 8, dtype=torch.float64, device=hip.device)
    for k in (0, 7):
        assert lib.gpar_chol_drop_leading(A.data_ptr(), 7, k, 8, A.data_ptr(), 8, A.data_ptr(), None, None, None) < -1000


@pytest.mark.parametrize("n,k", DROP_SIZES)
def test_drop_leading(hip, n, k):
    from gpar_amd import hip as h

    S, y = _problem(n)
    A, _ = _augmented(S, y)
    want, want_logdet = _augmented(S[k:, k:], y[k:])
    dev = hip.device
    m = n - k
    out = h.alloc_matrix(m + 1, m + 1, dev)
    out.fill_(float("nan"))
    logdet, info = _drop(_upload(A, dev), k, out)
    assert info == 0
    got = out.cpu().numpy()
    assert np.all(np.isnan(got[np.triu_indices(m + 1, 1)]))   # the strict upper triangle is left alone
    _check_against(got, want, logdet, want_logdet, S[k:, k:], f"drop n={n} k={k}")


@pytest.mark.parametrize("n,k", [(65, 5), (130, 65)])
def test_drop_leading_is_deterministic(hip, n, k):
    from gpar_amd import hip as h

    S, y = _problem(n)
    A = _upload(_augmented(S, y)[0], hip.device)
    runs = []
    for _ in range(2):
        out = h.alloc_matrix(n - k + 1, n - k + 1, hip.device)
        out.zero_()
        logdet, _ = _drop(A, k, out)
        runs.append((out.cpu().numpy(), logdet))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


def test_drop_leading_reports_nan(hip):
    from gpar_amd import hip as h

    n, k = 65, 5
    S, y = _problem(n)
    A, _ = _augmented(S, y)
    A[k + 2, 0] = np.nan   # v_0[2]: the pivot of column 2 (1-based 3) is the first non-finite r
    out = h.alloc_matrix(n - k + 1, n - k + 1, hip.device)
    _, info = _drop(_upload(A, hip.device), k, out)
    assert info == 3


@pytest.mark.parametrize("n,k", [(65, 5), (130, 64)])
def test_drop_leading_odd_leading_dimensions(hip, n, k):
    """An odd leading dimension of `out` (and of the input) takes the scalar path: same bits as the vector path."""
    from gpar_amd import hip as h

    S, y = _problem(n)
    A, _ = _augmented(S, y)
    dev, m = hip.device, n - k
    even = h.alloc_matrix(m + 1, m + 1, dev)
    _drop(_upload(A, dev), k, even)
    odd = torch.empty(m + 1, (m + 1) | 1, dtype=torch.float64, device=dev)[:, :m + 1]
    logdet, info = _drop(_upload(A, dev, ld=(n + 1) | 1), k, odd)
    assert info == 0 and odd.stride(0) % 2 == 1
    il = np.tril_indices(m + 1)
    assert np.array_equal(odd.cpu().numpy()[il], even.cpu().numpy()[il])
    want, want_logdet = _augmented(S[k:, k:], y[k:])
    _check_against(odd.cpu().numpy(), want, logdet, want_logdet, S[k:, k:], f"drop (odd ld) n={n} k={k}")


@pytest.mark.parametrize("n0,k", APPEND_SIZES)
def test_append(hip, n0, k):
    from gpar_amd import hip as h

    n = n0 + k
    S, y = _problem(n)
    dev = hip.device

    def potrf_augmented(rows):
        B = np.zeros((rows + 1, rows + 1))
        B[:rows, :rows], B[rows, :rows] = S[:rows, :rows], y[:rows]
        Bd = _upload(B, dev)
        logdet, info = h.potrf_(Bd, nf=rows)
        assert int(info.cpu()) == 0
        return Bd.cpu().numpy(), logdet

    want, want_logdet = potrf_augmented(n)
    old, old_logdet = potrf_augmented(n0)
    A = np.full((n + 1, n + 1), np.nan)
    A[:n0, :n0] = old[:n0, :n0]
    A[n0:n, :n] = S[n0:, :]
    A[n, :n0], A[n, n0:n] = old[n0, :n0], y[n0:]
    Ad = _upload(A, dev)
    logdet, info = h.chol_append_(Ad, n0, k, old_logdet.clone())
    assert int(info.cpu()) == 0
    _check_against(Ad.cpu().numpy(), want, float(logdet.cpu()), float(want_logdet.cpu()), S, f"append n0={n0} k={k}")


# ---- end to end --------------------------------------------------------------------------------------------------------------------
STEPS = {"append1": [(0, 1)], "append5": [(0, 5)], "drop3": [(3, 0)], "drop4_append4": [(4, 4)], "three_steps": [(2, 3), (3, 1), (1, 2)]}
_DATA = {}


def _data(rows):
    if rows not in _DATA:
        _DATA[rows] = make_data(rows, seed=rows)
    return _DATA[rows]


@pytest.mark.parametrize("n0", [130, 513])
@pytest.mark.parametrize("name", list(STEPS))
def test_update_end_to_end(hip, monkeypatch, n0, name):
    from gpar_amd.regression import GPARRegressor

    x, y, xs = _data(n0 + 30)
    monkeypatch.setenv("GPAR_UPDATE_DROP_FRACTION", "0.0625")   # the rank-k route for forgotten rows is opt-in
    routes = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("GPAR_CHOL_UPDATE", fused)
        reg = GPARRegressor(**CONFIG, normalise_y=False)
        reg.condition(x[:n0], y[:n0])
        lo, hi = run_steps(reg, x, y, STEPS[name], hi=n0)
        assert reg.last_update_incremental_ is True and reg.n == hi - lo
        routes[fused] = reg
    assert_same_posterior(hip, routes["1"], fresh_like(routes["1"], x[lo:hi], y[lo:hi]), xs, x[n0 + 20:], y[n0 + 20:])
    assert_same_posterior(hip, routes["1"], routes["0"], xs, x[n0 + 20:], y[n0 + 20:])   # the library calls against the composed routes


def test_twenty_steps_do_not_drift(hip, monkeypatch):
    from gpar_amd.regression import GPARRegressor

    monkeypatch.setenv("GPAR_UPDATE_DROP_FRACTION", "0.0625")
    n, step, rounds = 256, 8, 20
    x, y, xs = _data(n + step * rounds + 20)
    reg = GPARRegressor(**CONFIG, normalise_y=False)
    reg.condition(x[:n], y[:n])
    lo, hi = run_steps(reg, x, y, [(step, step)] * rounds, hi=n)
    assert reg.last_update_incremental_ is True and (lo, hi) == (step * rounds, n + step * rounds)
    assert_same_posterior(hip, reg, fresh_like(reg, x[lo:hi], y[lo:hi]), xs, x[hi:], y[hi:])
