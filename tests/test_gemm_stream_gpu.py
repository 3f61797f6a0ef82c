"""The fast K loop of the fp64 GEMM (gpar_amd/csrc/gemm_f64.h: gemm_mainloop_pf2 / gemm_stage) at the shapes where it branches,
against values that do not come from the device.

Exact cases: integer-valued operands (oracle/exact.py) whose products and sums are exact in fp64 - every element has one right answer
whatever the order of the sums -, at the stage counts 1, 2, 3 (an odd count: the pair loop runs once and the tail stage follows), 4
and 96; one interior tile, the diagonal / interior / preloaded tiles of a lower-triangular C, tiles that overhang the last row (the
clamped-row loads), half-tile launches (at most 256 tiles, K >= 64) and whole-tile ones, a lone factorisation whose update takes the
mixed last round; batch 1 and batch 3.  Which kernel a shape reaches is restated from gemm_launch in `tile_rows` and asserted.

Random case: gpar_potrf_batch on 3 x 2689 rows (nf = 2688) against numpy's Cholesky at the tolerances of tests/test_hip_primitives.py.
"""
import functools

import numpy as np
import pytest
import scipy.linalg

from oracle import exact

pytestmark = pytest.mark.gpu

ALPHA_BETA = [(1.0, 0.0), (-1.0, 1.0)]   # beta = 0: zero accumulators; (-1, 1): the update, interior tiles start from C (PRELOAD)


def tile_rows(m, n, k, batch, c_lower):
    """gemm_launch's choice (the NT / NN forms without triangular operands): 64-row half tiles while the launch has at most 256 tiles
    over the batch and K >= 64, whole 128-row tiles otherwise."""
    tm, tn = -(-m // 128), -(-n // 128)
    tiles = tn * (tn + 1) // 2 + (tm - tn) * tn if c_lower else tm * tn
    return 64 if tiles * batch <= 256 and k >= 64 else 128


# (id, tb, m, n, k, batch, c_lower, the tile height the id names)
CASES = [
    ("one-interior-tile-k%d" % k, True, 128, 128, k, 1, False, 64 if k >= 64 else 128) for k in (16, 32, 48, 64, 1536)
] + [
    ("lower-256-diagonal-interior-preload-k%d" % k, True, 256, 256, k, 1, True, 64 if k >= 64 else 128) for k in (16, 32, 48, 64, 1536)
] + [
    ("129-rows-clamped-half-tiles-k64", True, 129, 129, 64, 1, False, 64),
    ("129-rows-clamped-whole-tiles-k48", True, 129, 129, 48, 1, False, 128),
    ("129-rows-clamped-batch3-k1536", True, 129, 129, 1536, 3, False, 64),
    ("1281-rows-clamped-whole-tiles-batch3-k80", True, 1281, 1281, 80, 3, False, 128),
    ("384-half-tiles-batch3-k64", True, 384, 384, 64, 3, False, 64),
    ("289-whole-tiles-k80-odd-stage-count", True, 2176, 2176, 80, 1, False, 128),
    ("289-whole-tiles-k1536", True, 2176, 2176, 1536, 1, False, 128),
    ("nn-289-whole-tiles-k48", False, 2176, 2176, 48, 1, False, 128),
    ("nn-384-half-tiles-batch3-k64", False, 384, 384, 64, 3, False, 64),
]


@pytest.fixture(scope="module")
def env():
    import torch

    from gpar_amd import hip

    assert torch.cuda.is_available()
    return torch, hip, torch.device("cuda:0")


def _to_device(torch, hip, dev, host):
    out = hip.alloc_matrix(host.shape[0], host.shape[1], dev)
    out.copy_(torch.from_numpy(np.ascontiguousarray(host)))
    return out


def _first_difference(got, want):
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if len(bad) == 0:
        return None
    r, c = bad[0]
    return "%d entries differ, the first at (row %d, column %d): got %r, want %r" % (len(bad), r, c, got[r, c], want[r, c])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fast_loop_products_are_exact(env, case):
    """C <- alpha A op(B) + beta C to the bit; beta == 0: C starts NaN-filled (never read); c_lower: the strict upper triangle is NaN
    and stays NaN."""
    torch, hip, dev = env
    name, tb, m, n, k, batch, c_lower, rows = case
    assert tile_rows(m, n, k, batch, c_lower) == rows, "the case no longer reaches the kernel its id names"
    seed = 9100 + CASES.index(case)
    A = np.concatenate([exact.exact_operands((m, k), seed * 1000 + 3 * b) for b in range(batch)])
    B = np.concatenate([exact.exact_operands((n, k) if tb else (k, n), seed * 1000 + 3 * b + 1) for b in range(batch)])
    C = np.concatenate([exact.exact_operands((m, n), seed * 1000 + 3 * b + 2) for b in range(batch)])
    rb = n if tb else k
    P = np.concatenate([exact.exact_product(A[b * m:(b + 1) * m], B[b * rb:(b + 1) * rb].T if tb else B[b * rb:(b + 1) * rb])
                        for b in range(batch)])
    upper = np.concatenate([np.triu(np.ones((m, n), dtype=bool), 1)] * batch)
    dA, dB = _to_device(torch, hip, dev, A), _to_device(torch, hip, dev, B)
    for alpha, beta in ALPHA_BETA:
        start = np.full(C.shape, np.nan) if beta == 0.0 else C.copy()
        want = alpha * P + (beta * C if beta != 0.0 else 0.0)
        if c_lower:
            start[upper] = np.nan
            want[upper] = np.nan
        dC = _to_device(torch, hip, dev, start)
        if batch > 1:
            hip.gemm_batch_(dA, dB, dC, batch, ta=False, tb=tb, alpha=alpha, beta=beta, c_lower=c_lower)
        else:
            hip.gemm(dA, dB, ta=False, tb=tb, alpha=alpha, beta=beta, out=dC, c_lower=c_lower)
        diff = _first_difference(dC.cpu().numpy(), want)
        assert diff is None, "alpha %g beta %g: %s" % (alpha, beta, diff)


def test_a_lone_factorisation_with_a_mixed_last_round_is_exact(env, monkeypatch):
    """5121 rows, nf = 5120, single panels: the case "5121-lone-mixed-last-round" of tests/test_exact_arithmetic_gpu.py, whose schedule
    tests/test_exact_cases.py checks - its first trailing update runs one full round of 512 whole tiles and the rest as half tiles
    (the MIXED launch of the update kernel).  Factor and solved row to the bit."""
    torch, hip, dev = env
    monkeypatch.setenv("GPAR_POTRF_FUSE2_ROWS", "0")
    N, nf = 5121, 5120
    L = exact.exact_factor(N, 100)
    A = np.tril(exact.exact_spd(L)) + np.triu(np.full((N, N), np.nan), 1)
    dA = _to_device(torch, hip, dev, A)
    _, info = hip.potrf_(dA, nf)
    got = dA.cpu().numpy()
    assert int(info.item()) == 0
    have = got[:, :nf].copy()
    have[:nf] = np.tril(have[:nf])
    diff = _first_difference(have, np.tril(L[:, :nf]))
    assert diff is None, diff
    assert got[nf, nf] == L[nf, nf] ** 2


@functools.lru_cache(maxsize=1)
def _random_spd_batch(batch, N):
    rng = np.random.default_rng(2689)
    out = []
    for _ in range(batch):
        G = rng.standard_normal((N, N))
        out.append(G @ G.T / N + np.eye(N))
    return out


def test_random_lockstep_factorisation_matches_numpy(env):
    """gpar_potrf_batch on three seeded SPD matrices of 2689 rows, nf = 2688 (the augmented shape): factor, solved row and Schur
    complement against numpy / scipy at the tolerances tests/test_hip_primitives.py::test_potrf_partial_schur uses."""
    torch, hip, dev = env
    batch, N, nf = 3, 2689, 2688
    mats = _random_spd_batch(batch, N)
    dA = _to_device(torch, hip, dev, np.concatenate(mats))
    logdet, info = hip.potrf_batch_(dA, batch, nf)
    got = dA.cpu().numpy().reshape(batch, N, N)
    assert info.cpu().tolist() == [0] * batch
    for b in range(batch):
        A = mats[b]
        L11 = np.linalg.cholesky(A[:nf, :nf])
        L21 = scipy.linalg.solve_triangular(L11, A[:nf, nf:], lower=True).T
        S = A[nf:, nf:] - L21 @ L21.T
        assert np.allclose(np.tril(got[b][:nf, :nf]), L11, rtol=1e-10, atol=1e-12)
        assert np.allclose(got[b][nf:, :nf], L21, rtol=1e-9, atol=1e-11)
        assert np.allclose(got[b][nf:, nf:], S, rtol=1e-9, atol=1e-10)
        assert np.isclose(logdet[b].item(), 2 * np.sum(np.log(np.diag(L11))), rtol=1e-12)
