"""Inputs on which fp64 arithmetic is exact: every intermediate of every correct algorithm is representable, so the result does not
depend on summation order, tile shape, fusion, look-ahead or batch geometry and must equal the known answer to the bit.

    exact_factor    a lower-triangular L with small integer entries and power-of-two pivots
    exact_spd       A = L L^T: an integer matrix whose Cholesky factor is L, every Schur complement an integer matrix,
                    every pivot the square of a power of two, every reciprocal pivot a power of two
    exact_operands  small-integer operands of a product

and the restatements the CPU premise tests run (tests/test_exact_cases.py): the explicit inverse of a triangular block composed
from 8 x 8 inverses the way the panel kernels compose theirs, a blocked right-looking factorisation that multiplies by those
inverses, and a blocked triangular solve of the same kind.  numpy only.
"""
import numpy as np

LIMIT = 2.0 ** 53


def _assert_integers(M):
    assert np.all(np.isfinite(M)) and np.array_equal(M, np.rint(M)), "not integer-valued"
    assert np.abs(M).max(initial=0.0) < LIMIT, "an entry of 2^53 or more: integers are no longer exact"


def exact_factor(n, seed, diag=(1.0, 2.0, 4.0), in_block=0.125):
    """Lower-triangular n x n: outside the 64-aligned diagonal blocks the strictly lower entries are uniform integers in [-2, 2];
    inside such a block they are non-zero with probability `in_block`, values +-1 (this keeps the inverses of the diagonal blocks
    small); the diagonal is drawn from `diag` (powers of two)."""
    rng = np.random.default_rng(seed)
    L = rng.integers(-2, 3, size=(n, n)).astype(np.float64)
    sparse = np.where(rng.random((n, n)) < in_block, rng.choice(np.array([-1.0, 1.0]), size=(n, n)), 0.0)
    blk = np.arange(n) // 64
    same = blk[:, None] == blk[None, :]
    L = np.tril(np.where(same, sparse, L), -1)
    d = rng.choice(np.asarray(diag, dtype=np.float64), size=n)
    assert np.all(np.frexp(d)[0] == 0.5), "pivots must be powers of two"
    L[np.diag_indices(n)] = d
    return L


def exact_spd(L):
    """L L^T (fp64 BLAS is exact here: every partial sum is a small integer)."""
    A = L @ L.T
    _assert_integers(A)
    return A


def exact_operands(shape, seed, lo=-3, hi=3):
    """Integer-valued fp64 matrix with entries in [lo, hi]."""
    M = np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float64)
    _assert_integers(M)
    return M


def exact_product(opA, opB):
    """numpy's fp64 matmul of integer operands, checked to be integer-valued and below 2^53."""
    P = opA @ opB
    _assert_integers(P)
    assert np.abs(opA).max(initial=0.0) * np.abs(opB).max(initial=0.0) * opA.shape[1] < LIMIT
    return P


def composed_inverse(D, leaf=8):
    """Inverse of the lower-triangular block D as the panel kernels build it: `leaf` x `leaf` inverses by substitution with
    reciprocal pivots, then [Wa 0; -Wb Lba Wa, Wb] level by level (16, 32, ... up to the block)."""
    n = D.shape[0]
    if n <= leaf:
        W = np.zeros_like(D)
        for j in range(n):
            x = np.zeros(n)
            x[j] = 1.0
            for k in range(n):
                x[k] = x[k] * (1.0 / D[k, k])
                x[k + 1:] -= D[k + 1:, k] * x[k]
            W[:, j] = x
        return W
    h = (n + 1) // 2
    Wa, Wb = composed_inverse(D[:h, :h], leaf), composed_inverse(D[h:, h:], leaf)
    W = np.zeros_like(D)
    W[:h, :h], W[h:, h:] = Wa, Wb
    W[h:, :h] = -(Wb @ (D[h:, :h] @ Wa))
    return W


def blocked_cholesky(A, nf=None, block=64):
    """Right-looking (partial) factorisation of the lower triangle of A with explicit inverses of the `block`-wide diagonal blocks:
    returns (the matrix after nf columns - factor in columns < nf, Schur complement behind -, [(D, Dinv) per block])."""
    A = np.tril(A).copy()
    N = A.shape[0]
    nf = N if nf is None else nf
    pairs = []
    for k in range(0, nf, block):
        e = min(k + block, nf)
        D = np.linalg.cholesky(A[k:e, k:e])
        A[k:e, k:e] = D
        Dinv = composed_inverse(D)
        pairs.append((D, Dinv))
        if e < N:
            A[e:, k:e] = A[e:, k:e] @ Dinv.T
            P = A[e:, k:e]
            A[e:, e:] -= np.tril(P @ P.T)
    return A, pairs


def blocked_solve(L, B, forward=True, block=64):
    """X with X L^T = B (forward) or X L = B (backward), column block by column block through the explicit inverse of each
    `block`-wide diagonal block."""
    X = B.copy()
    n = L.shape[0]
    starts = list(range(0, n, block))
    for k in (starts if forward else reversed(starts)):
        e = min(k + block, n)
        Dinv = composed_inverse(L[k:e, k:e])
        if forward:
            X[:, k:e] = X[:, k:e] @ Dinv.T
            X[:, e:] -= X[:, k:e] @ L[e:, k:e].T
        else:
            X[:, k:e] = X[:, k:e] @ Dinv
            X[:, :k] -= X[:, k:e] @ L[k:e, :k]
    return X
