"""The augmented rows of a partial factorisation (0 < N - nf <= 16) leave the matrix-core updates: the schedule's tail split
(potrf_tail_split, csrc/potrf_schedule.h) and its companion kernel (potrf_tail_update_kernel, csrc/potrf.h).

The split applies to lock-step batches only; a lone factorisation keeps every row in its updates and is covered as the unchanged path.

Partial factorisations with a tail of 1, 2, 16 and 17 rows (17: just over the rule's limit - those go through the tile launches as
before), nf a multiple of 128 and not (5000: leaving the tail out never removes a tile row, the rule keeps all rows in the update;
5112 = 39 * 128 + 120: it removes one for tails of 16 rows only), sizes on both sides of the grouping / fusing thresholds, alone and
as a lock-step batch of 3, against numpy / scipy in fp64 with the tolerances of test_potrf_partial_schur.
"""
import functools

import numpy as np
import pytest
import scipy.linalg

pytestmark = pytest.mark.gpu

MAX_TAIL = 17
SIZES = [1024, 2688, 5120, 6656, 8192, 5000, 5112]
TAILS = [1, 2, 16, 17]


@pytest.fixture(scope="module")
def env():
    import torch

    from gpar_amd import hip

    assert torch.cuda.is_available()
    return torch, hip, torch.device("cuda:0")


@functools.lru_cache(maxsize=3)
def _problem(nf, b):
    """A well-conditioned (cond ~ n / 64) SPD matrix of nf + MAX_TAIL rows and its reference: the factor of the leading nf x nf block,
    the solved rows below it and their Schur complement.  The problem with a shorter tail is a leading submatrix of everything."""
    rng = np.random.default_rng(1000 * nf + b)
    N = nf + MAX_TAIL
    B = rng.standard_normal((N, 64))
    A = B @ B.T / 64.0
    A[np.diag_indices(N)] += 1.0 + 0.1 * b
    L11 = np.linalg.cholesky(A[:nf, :nf])
    L21 = scipy.linalg.solve_triangular(L11, A[:nf, nf:], lower=True).T
    S = A[nf:, nf:] - L21 @ L21.T
    return A, L11, L21, S


def _stack(hip, torch, dev, nf, tail, batch, upper=None):
    """Device matrix of `batch` problems stacked by rows, and a pristine host copy."""
    N = nf + tail
    host = np.concatenate([_problem(nf, b)[0][:N, :N] for b in range(batch)], axis=0)
    if upper is not None:
        for b in range(batch):
            blk = host[b * N:(b + 1) * N]
            blk[np.triu_indices(N, 1)] = upper
    dA = hip.alloc_matrix(batch * N, N, dev)
    dA.copy_(torch.tensor(host, dtype=torch.float64))
    return dA, host


def _factor(hip, dA, batch, nf, lookahead=True):
    if batch == 1:
        logdet, info = hip.potrf_(dA, nf, lookahead=lookahead)
    else:
        logdet, info = hip.potrf_batch_(dA, batch, nf)
    assert info.cpu().tolist() == [0] * batch
    return logdet


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("nf", SIZES)
def test_partial_factorisation_with_a_short_tail(env, nf, tail, batch):
    """Factor, solved tail rows and corner against scipy; the strict upper triangle - of the tail block too - is never read or
    written (NaN-filled input); the same call twice returns the same bits.

    One exception to "never written", by the library's own convention and older than the split: the strict upper triangle of every
    whole 64-aligned diagonal block [64 b, 64 b + 64)^2, b < N // 64, is the panel kernels' scratch (their hand-off words live there,
    csrc/panel.h: potrf_zero_flags).  Those words are left out of the check; the part of the tail block above its diagonal is not."""
    torch, hip, dev = env
    N = nf + tail
    dA, _ = _stack(hip, torch, dev, nf, tail, batch, upper=np.nan)
    start = dA.clone()
    logdet = _factor(hip, dA, batch, nf)
    got_all = dA.cpu().numpy()[:, :N].reshape(batch, N, N)
    il = np.tril_indices(tail)
    iu = np.triu_indices(N, 1)
    scratch = (iu[0] // 64 == iu[1] // 64) & (iu[1] // 64 < N // 64) & (iu[0] < nf)
    iu = (iu[0][~scratch], iu[1][~scratch])
    for b in range(batch):
        _, L11, L21, S = _problem(nf, b)
        got = got_all[b]
        assert np.all(np.isnan(got[iu]))   # never written (and, the rest being finite, never read)
        assert np.allclose(np.tril(got[:nf, :nf]), L11, rtol=1e-10, atol=1e-12)
        assert np.allclose(got[nf:, :nf], L21[:tail], rtol=1e-9, atol=1e-11)
        assert np.allclose(got[nf:, nf:][il], S[:tail, :tail][il], rtol=1e-9, atol=1e-10)
        assert np.isclose(float(logdet[b]), 2 * np.sum(np.log(np.diag(L11))), rtol=1e-12)
    dB = hip.alloc_matrix(batch * N, N, dev)   # (a clone would drop the padded leading dimension, and with it the aligned kernels)
    dB.copy_(start)
    logdet2 = _factor(hip, dB, batch, nf)
    lower = lambda M: torch.tril(M[:, :N].reshape(batch, N, N))   # (the scratch words above the diagonal depend on timing)
    assert torch.equal(logdet, logdet2)
    assert torch.equal(lower(dB), lower(dA))


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("nf,tail", [(2688, 1), (5120, 1), (5120, 16), (5112, 16), (6656, 2), (8192, 1)])
def test_look_ahead_on_off_on_returns_the_same_bits(env, monkeypatch, nf, tail, batch):
    """Every element of the tail rows receives the same K ranges in the same order on one stream and on two."""
    torch, hip, dev = env
    dA, _ = _stack(hip, torch, dev, nf, tail, batch)
    start = dA.clone()
    out = []
    for la in (True, False, True):
        dA.copy_(start)
        if batch > 1:   # a lock-step batch has no flag for it: the switch of DESIGN 3.9
            monkeypatch.setenv("GPAR_POTRF_BATCH_LOOKAHEAD", "1" if la else "0")
        logdet = _factor(hip, dA, batch, nf, lookahead=la)
        out.append((torch.tril(dA[:, :nf + tail].reshape(batch, nf + tail, nf + tail)).clone(), logdet.clone()))
    for other in out[1:]:
        assert torch.equal(out[0][0], other[0]) and torch.equal(out[0][1], other[1])
