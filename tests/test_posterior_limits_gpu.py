"""The three fused posterior passes - gram_terms.h (decompose), pathwise.h (pathwise sampling), gram_deriv.h (derivative) - at the limits of
the kernel specification: up to GPAR_MAX_DIMS = 96 feature dims, GRAD_MAXF = 4 factors in a term, GPAR_MAX_FACTORS = 12 factors,
GPAR_MAX_TERMS = 8 directions or components; on both sides of the dz at which a launch asks for more than 48 KB of dynamic LDS (and so
calls gpar_set_max_lds for its kernel), on both sides of the dz at which gpar_posterior_deriv refuses a tile set that does not fit 160 KB,
and with workspaces that give chunks of test rows and splits of the training rows strictly between one and all.

The 48 KB edges, from the launch functions (GRAM_LD = 68 and GRAM_T = 64, gram_math.inc; GRAM_TAB_DOUBLES = 64 + 256 = 320; PW_ROWS =
PW_FREQS = 64, PW_COLS = PW_SLICES = 4, GA_COLS = 4, pathwise.h).  48 KB = 6144 doubles, 160 KB = 20480 doubles; a launch takes the
branch when its doubles EXCEED 6144:
  posterior_deriv_mean_kernel   pd_lds_bytes(dz, ndir, true) = (2 + ndir) dz 68 + 68 + 64 ndir doubles
      ndir = 1: 204 dz + 132   dz = 29: 6048   dz = 30: 6252 >      ndir = 3: 340 dz + 260   dz = 17: 6040   dz = 18: 6380 >
      ndir = 8: 680 dz + 580   dz = 8: 6020    dz = 9: 6700 >
  posterior_deriv_stack_kernel  pd_lds_bytes(dz, ndir, false) = (2 + ndir) dz 68:    ndir = 1: 204 dz   dz = 30: 6120   dz = 31: 6324 >
  gpar_posterior_deriv's GPAR_ARG_ERROR(9): pd_lds_bytes(dz, ndir, true) > 20480 doubles
      ndir = 8: dz = 29: 20300   dz = 30: 20980 >      ndir = 3: dz = 59: 20320   dz = 60: 20660 >      ndir = 1: dz = 96: 19716 (fits)
  gram_terms_kernel             2 dz 68 + 320 = 136 dz + 320:                        dz = 42: 6032   dz = 43: 6168 >
  posterior_terms_mean_kernel   136 dz + 320 + 68 + 64 G:    G = 8: 136 dz + 900   dz = 38: 6068   dz = 39: 6204 >
                                                             G = 1: 136 dz + 452   dz = 41: 6028   dz = 42: 6164 >
  gram_apply_groups_kernel      136 dz + 320 + 4 68 + 4 64 = 136 dz + 848:           dz = 38: 6016   dz = 39: 6152 >
  rff_apply_kernel              rff_lds_bytes = dz (64 + 64) + 2 4 64 + 3 4 64 = 128 dz + 1280:   dz = 38: 6144 (not above)   dz = 39: 6272 >
`lds_doubles` below restates these formulas; tests/test_posterior_limits.py checks the table against it, and the constants against the sources.

References and tolerances - none is new:
  derivative moments        tests/derivative_reference.py, rtol 1e-8 / atol 1e-10 (tests/test_derivative_gpu.py); the prior term alone rtol
                            1e-12 / atol 1e-13 (test_no_training_rows_gives_zero_means_and_the_prior_term there)
  decompose                 the numpy route of tests/test_decompose_gpu.py: Gram entries 1e-12, diagonals rtol 1e-12 / atol 1e-14, the sum of
                            the components within 8 eps of the sum of the terms' magnitudes, moments rtol 1e-8 / atol 1e-10
  gpar_rff_apply            the long-double twin and the 8 x own-error rule of tests/test_pathwise_gpu.py
  gpar_gram_apply_groups    1e-11 sum |k| |v| (tests/test_pathwise_gpu.py), against eng.gram and against numpy's oracle.kernels Gram
  end to end                the tolerances of the three tests this file borrows from

Non-vacuity is a condition on the reference alone, checked before any device call (`assert_not_vacuous`): a posterior that equals the prior
would pass every comparison above, so the stretches grow with sqrt(dz) (0.7 sqrt(dz / 2)) and the linear products see inputs on [0, 2]."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from . import derivative_reference as dr
from . import test_decompose_gpu as tc
from . import test_derivative_gpu as td
from . import test_pathwise_gpu as tp
from .conftest import to_np
from .test_derivative_gpu import hip  # noqa: F401  (the fixture: the HIP engine installed for one test)

pytestmark = pytest.mark.gpu

RTOL, ATOL = td.RTOL, td.ATOL
NOISE = td.NOISE          # (tests/test_decompose_gpu.py conditions at the same 0.1)
SENTINEL = td.SENTINEL
EPS = tc.EPS

# ---- the dynamic LDS of the launches, in doubles (the docstring's arithmetic) -------------------------------------------------------------------
GRAM_T, GRAM_LD, GRAM_TAB_DOUBLES = 64, 68, 320
PW_ROWS, PW_FREQS, PW_COLS, PW_SLICES, GA_COLS = 64, 64, 4, 4, 4
LDS_48K, LDS_160K = 48 * 1024 // 8, 160 * 1024 // 8


def lds_doubles(kernel, dz, count=1):
    """What the launch function of `kernel` asks for at `dz` feature dims and `count` directions or components (csrc/gram_deriv.h pd_lds_bytes,
    gram_terms.h gram_terms_launch and posterior_terms_run, pathwise.h rff_lds_bytes and gram_apply_groups_run)."""
    dzl = max(dz, 1)
    return {
        "deriv_mean": (2 + count) * dzl * GRAM_LD + GRAM_LD + count * GRAM_T,
        "deriv_stack": (2 + count) * dzl * GRAM_LD,
        "gram_terms": 2 * dzl * GRAM_LD + GRAM_TAB_DOUBLES,
        "terms_mean": 2 * dzl * GRAM_LD + GRAM_TAB_DOUBLES + GRAM_LD + count * GRAM_T,
        "gram_apply": 2 * dzl * GRAM_LD + GRAM_TAB_DOUBLES + GA_COLS * GRAM_LD + GA_COLS * GRAM_T,
        "rff": dzl * (PW_ROWS + PW_FREQS) + 2 * PW_COLS * PW_FREQS + (PW_SLICES - 1) * PW_COLS * PW_ROWS,
    }[kernel]


#: (kernel, count, the largest dz at or below 48 KB, the smallest above): the issue's table and gram_terms_kernel's row
EDGES_48K = (("deriv_mean", 1, 29, 30), ("deriv_mean", 3, 17, 18), ("deriv_mean", 8, 8, 9), ("deriv_stack", 1, 30, 31), ("terms_mean", 8, 38, 39),
             ("terms_mean", 1, 41, 42), ("gram_apply", 1, 38, 39), ("rff", 1, 38, 39), ("gram_terms", 1, 42, 43))
#: (ndir, the largest dz gpar_posterior_deriv takes, the smallest it refuses; None: every dz up to GPAR_MAX_DIMS fits)
EDGES_160K = ((8, 29, 30), (3, 59, 60), (1, 96, None))


# ---- the kernel structures ------------------------------------------------------------------------------------------------------------------------
def _ell(nd):
    return 0.7 * np.sqrt(nd / 2.0)


def _vary(nd, k=0):
    return 1.0 + 0.1 * np.cos(np.arange(nd) + k)   # (no two dims with the same scale)


def _twelve_dims(dz):
    """Feature dims of the twelve factors: one each (the periodic embedding two), the rest dealt round the factors."""
    nd = [1] * 12
    nd[8] = 2
    left, i = dz - 13, 0
    assert left >= 0
    while left > 0:
        step = 2 if i == 8 else 1
        if left >= step:
            nd[i] += step
            left -= step
        i = (i + 1) % 12
    return nd


def structure(name, dz):
    """(kernel, width of the design matrix, shift of the inputs): a kernel with exactly `dz` feature dims.
    wide_eq         one EQ factor over dz plain columns
    wide_mixed      EQ(cols 0..a) * RQ(cols a..b) * Matern52(cols b..c) * Cosine(cols c, c + 1): four factors in one term
    lin3_eq         Linear * Linear * Linear * EQ on overlapping column sets, inputs on [0, 2] so that every linear factor is about 1
    twelve_factors  8 terms and 12 factors: EQ * RQ * Matern52 * Cosine, Linear * Linear * EQ, Matern32, a periodic EQ, Linear, RQ, Cosine, 0.3
    wide_periodic   an EQ over the periodic embeddings of dz / 2 columns"""
    from gpar_amd.kernels import EQ, RQ, Cosine, Kernel, Linear, Matern32, Matern52, ZeroKernel

    if name == "wide_eq":
        return 1.3 * EQ().stretch(_ell(dz) * _vary(dz)).select(range(dz)), dz, 0.0
    if name == "wide_mixed":
        a, b, c = (dz - 2) // 3, 2 * (dz - 2) // 3, dz - 2
        assert 0 < a < b < c
        ell = _ell(c)
        return 1.1 * (EQ().stretch(ell * _vary(a)).select(range(a)) * RQ(1.5).stretch(ell * _vary(b - a, 1)).select(range(a, b))
                      * Matern52().stretch(ell * _vary(c - b, 2)).select(range(b, c)) * Cosine().stretch(np.array([3.0, 4.0])).select([c, c + 1])), dz, 0.0
    if name == "lin3_eq":
        q = [dz // 4 + (i < dz % 4) for i in range(4)]
        assert min(q) >= 1
        width = max(q) + 2
        cols = [[(i + j) % width for j in range(q[i])] for i in range(4)]
        lin = [Linear().stretch(np.sqrt(q[i] * 4.0 / 3.0) * _vary(q[i], i)).select(cols[i]) for i in range(3)]   # E x^2 = 4 / 3 on [0, 2]
        return 0.8 * (lin[0] * lin[1] * lin[2] * EQ().stretch(_ell(q[3]) * _vary(q[3], 3)).select(cols[3])), width, 1.0
    if name == "twelve_factors":
        nd = _twelve_dims(dz)
        ncol = [v // 2 if i == 8 else v for i, v in enumerate(nd)]
        width = max(ncol) + 3
        cols = [[(2 * i + j) % width for j in range(ncol[i])] for i in range(12)]
        lin = lambda i: Linear().stretch(np.sqrt(nd[i] / 3.0) * _vary(nd[i], i)).select(cols[i])   # E x^2 = 1 / 3 on [-1, 1]
        cos = lambda i: Cosine().stretch(3.0 * np.sqrt(nd[i]) * _vary(nd[i], i)).select(cols[i])
        stat = lambda make, i, total: make.stretch(_ell(total) * _vary(nd[i], i)).select(cols[i])
        d0 = nd[0] + nd[1] + nd[2]
        terms = [
            1.0 * (stat(EQ(), 0, d0) * stat(RQ(1.5), 1, d0) * stat(Matern52(), 2, d0) * cos(3)),
            0.6 * (lin(4) * lin(5) * stat(EQ(), 6, nd[6])),
            0.7 * stat(Matern32(), 7, nd[7]),
            0.8 * EQ().stretch(_ell(nd[8]) * _vary(nd[8], 8)).periodic(3.0 + 0.1 * np.arange(ncol[8])).select(cols[8]),
            0.5 * lin(9),
            0.6 * stat(RQ(0.7), 10, nd[10]),
            0.4 * cos(11),
            ZeroKernel() + 0.3,
        ]
        return Kernel([t for k in terms for t in k.terms]), width, 0.0
    if name == "wide_periodic":
        assert dz % 2 == 0
        ncol = dz // 2
        return 1.2 * EQ().stretch(_ell(dz) * _vary(dz)).periodic(3.0 + 0.1 * np.arange(ncol)).select(range(ncol)), ncol, 0.0
    raise KeyError(name)


def spec_of(kernel):
    from oracle import kernels as ok

    return ok.spec_to_dict(kernel)


def feature_dims(kernel):
    return sum(f.num_features() for t in kernel.terms for f in t.factors)


def data(name, dz, n, ns, ndir=0, seed=0):
    """(kernel, x, y, xs, U) for one structure: inputs uniform on [-1, 1] + the structure's shift, standard-normal targets and directions."""
    kernel, width, shift = structure(name, dz)
    assert feature_dims(kernel) == dz and len(kernel.terms) <= 8 and sum(len(t.factors) for t in kernel.terms) <= 12
    rng = np.random.default_rng([seed, sum(map(ord, name)), dz, n, ns, ndir])
    return (kernel, shift + rng.uniform(-1, 1, (n, width)), rng.standard_normal(n), shift + rng.uniform(-1, 1, (ns, width)),
            rng.standard_normal((ndir, ns, width)))


def assert_not_vacuous(mean, var, prior, what):
    """The reference has something to say: max |mean| >= 1e-2 and, at half the test rows at least, a variance below 0.95 of the prior term."""
    mean, var, prior = (np.atleast_2d(a) for a in (mean, var, prior))
    for c in range(mean.shape[0]):
        assert np.abs(mean[c]).max() >= 1e-2, (what, c, np.abs(mean[c]).max())
        assert 2 * np.count_nonzero(var[c] < 0.95 * prior[c]) >= mean.shape[1], (what, c, float(np.median(var[c] / prior[c])))


# ---- the references, each computed once ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def deriv_case(name, dz, n, ns, ndir, zero=None):
    """Data and the restatement's (dmean, dvar) for ndir directions, direction `zero` all zero; non-vacuous in every other direction."""
    kernel, x, y, xs, U = data(name, dz, n, ns, ndir)
    if zero is not None:
        U[zero] = 0.0
    mean, var, prior = dr.layer_derivatives(spec_of(kernel), x, y, NOISE, xs, U)
    live = [c for c in range(ndir) if c != zero]
    assert_not_vacuous(mean[live], var[live], prior[live], f"{name} dz={dz} n={n} n*={ns} ndir={ndir}")
    return kernel, x, y, xs, U, mean, var


@functools.lru_cache(maxsize=None)
def terms_case(name, dz, n, ns):
    """Data, the numpy route's per-term matrices k_t(x*, X), and the moments of every term as its own component and of one component that
    holds them all (tests/test_decompose_gpu.py _numpy_terms, _numpy_posterior); non-vacuous as a whole."""
    kernel, x, y, xs, _ = data(name, dz, n, ns)
    nterms = len(kernel.terms)
    each = tc._numpy_posterior(kernel, x, y, xs, list(range(nterms)), nterms)
    whole = tc._numpy_posterior(kernel, x, y, xs, [0] * nterms, 1)
    cross = tc._numpy_terms(kernel, xs, x)
    prior = sum(np.diag(k) for k in tc._numpy_terms(kernel, xs, xs))
    assert_not_vacuous(whole[0], whole[1], prior, f"{name} dz={dz} n={n} n*={ns}")
    return kernel, x, y, xs, cross, each, whole


DERIV_EDGE_CASES = (   # (ndir, dz, structure): both sides of an edge meet the same structure
    (1, 29, "wide_mixed"), (1, 30, "wide_mixed"), (1, 31, "wide_mixed"), (1, 30, "wide_periodic"), (3, 17, "twelve_factors"), (3, 18, "twelve_factors"),
    (8, 8, "lin3_eq"), (8, 9, "lin3_eq"),
    (8, 29, "wide_mixed"), (3, 59, "twelve_factors"), (1, 96, "wide_eq"), (1, 96, "wide_periodic"))   # the three largest shapes that fit
EIGHT_DIRECTION_CASES = (("twelve_factors", 29), ("lin3_eq", 29), ("wide_mixed", 29))
PRIOR_ONLY_CASES = (("lin3_eq", 31), ("twelve_factors", 30))
CHUNK_DERIV = ("wide_mixed", 31, 3)       # (structure, dz, ndir): above 48 KB in both kernels
CHUNK_TERMS = ("twelve_factors", 39)      # (structure, dz): the mean kernel above 48 KB at 8 components
TERMS_DZS = (38, 39, 41, 42, 43, 96)
APPLY_CASES = tuple((name, dz) for dz in (38, 39, 96) for name in ("twelve_factors", "wide_mixed"))


def sizes(i):
    """(n, n*): 65 training rows against 129 test rows, or 130 against 65."""
    return ((65, 129), (130, 65))[i % 2]


def every_reference():
    """Every (reference function, arguments) the device tests below use: tests/test_posterior_limits.py runs them all on the CPU, so that a
    vacuous case fails there and not only where a GPU is."""
    out = [(deriv_case, (name, dz, *sizes(i), ndir)) for i, (ndir, dz, name) in enumerate(DERIV_EDGE_CASES)]
    out += [(deriv_case, (name, dz, 130, 129, 8, 5)) for name, dz in EIGHT_DIRECTION_CASES]
    out += [(deriv_case, (*CHUNK_DERIV[:2], 130, 129, CHUNK_DERIV[2]))]
    out += [(terms_case, (*CHUNK_TERMS, 130, 129))]
    out += [(terms_case, ("twelve_factors", dz, *sizes(i))) for i, dz in enumerate(TERMS_DZS)]
    out += [(terms_case, (name, dz, 130, 65)) for name, dz in APPLY_CASES]
    return out


# ---- derivative: across the 48 KB edges, the largest shapes that fit ---------------------------------------------------------------------------------
def _check_deriv(hip, case, what, **kwargs):
    kernel, x, y, xs, U, want_mean, want_var = case
    f, obs = td._conditioned(hip, kernel, x, y)
    p = f._pts(hip.tensor(xs))
    assert p.ck.dz == feature_dims(kernel)
    mean, var = td._deriv(hip, obs, p, U, **kwargs)   # (padded leading dimensions, the padding checked against the sentinel)
    np.testing.assert_allclose(mean, want_mean, rtol=RTOL, atol=ATOL, err_msg=what)
    np.testing.assert_allclose(var, want_var, rtol=RTOL, atol=ATOL, err_msg=what)
    return obs, p, mean, var


@pytest.mark.parametrize("i", range(len(DERIV_EDGE_CASES)))
def test_derivative_on_both_sides_of_the_48k_edges_and_at_the_largest_shapes(hip, i):
    """(ndir, dz) = (1, 29 | 30 | 31), (3, 17 | 18), (8, 8 | 9): the mean kernel and (at ndir = 1, dz = 31) the stack kernel below and above
    48 KB of dynamic LDS; (8, 29), (3, 59), (1, 96): the largest that fit 160 KB - the arithmetic is in the module docstring.  Means and
    variances against the restatement, padded outputs, the same bits from a second call and, for the means, from a call without variances."""
    ndir, dz, name = DERIV_EDGE_CASES[i]
    n, ns = sizes(i)
    what = f"{name} ndir={ndir} dz={dz} n={n} n*={ns}"
    case = deriv_case(name, dz, n, ns, ndir)
    assert (lds_doubles("deriv_mean", dz, ndir) > LDS_48K) == (dz >= {1: 30, 3: 18, 8: 9}[ndir]) and lds_doubles("deriv_mean", dz, ndir) <= LDS_160K
    obs, p, mean, var = _check_deriv(hip, case, what)
    again = td._deriv(hip, obs, p, case[4])
    np.testing.assert_array_equal(mean, again[0], err_msg=what)
    np.testing.assert_array_equal(var, again[1], err_msg=what)
    np.testing.assert_array_equal(td._deriv(hip, obs, p, case[4], variance=False)[0], mean, err_msg=what)


@pytest.mark.parametrize("ndir,dz", [(8, 30), (3, 60)])
def test_derivative_over_the_lds_limit_is_an_argument_error_that_touches_nothing(hip, ndir, dz):
    """The smallest shapes whose tiles exceed 160 KB (the shapes one dz below are computed above): GPAR_ARG_ERROR(9) = -1009, with `mean`, `var`
    and the workspace untouched, and the same code in the error the Python binding raises.  GPARRegressor.derivative cannot get here: it
    hands over ONE direction per layer (GPAR._derivative), and one direction fits at every dz up to GPAR_MAX_DIMS (19716 doubles at 96)."""
    from gpar_amd import _lib
    from gpar_amd import hip as hipmod

    assert lds_doubles("deriv_mean", dz, ndir) > LDS_160K >= lds_doubles("deriv_mean", dz - 1, ndir)
    lib, stream = td._lib_and_stream(hip)
    n, ns = 20, 9
    kernel, x, y, xs, U = data("wide_eq", dz, n, ns, ndir)
    f, obs = td._conditioned(hip, kernel, x, y)
    p = f._pts(hip.tensor(xs))
    fac = obs.factor()
    ck, z = obs.fdd.features()
    J = hipmod.feature_directions(ck, p.x, hip.tensor(U))
    alpha = fac.alpha().reshape(-1).contiguous()
    nws = int(lib.gpar_workspace_doubles(_lib.WS_POSTERIOR_DERIV, n, ns, ndir))
    ws, mean, var = (torch.full(shape, SENTINEL, dtype=torch.float64, device=hip.device) for shape in ((nws,), (ndir, ns), (ndir, ns)))
    rc = lib.gpar_posterior_deriv(ctypes.byref(ck.kspec), p.z.data_ptr(), ns, int(p.z.stride(0)), J.data_ptr(), dz, ns * dz, ndir, z.data_ptr(), n,
                                  int(z.stride(0)), dz, alpha.data_ptr(), fac.L.data_ptr(), int(fac.L.stride(0)), mean.data_ptr(), ns, var.data_ptr(), ns,
                                  ws.data_ptr(), nws, stream)
    assert rc == -1009
    torch.cuda.synchronize()
    for out in (ws, mean, var):
        assert bool((out == SENTINEL).all())
    with pytest.raises(_lib.HipLibraryError, match="gpar_posterior_deriv failed with status -1009"):
        hipmod.posterior_deriv(ck, p.z, J, z, alpha, fac.L)


@pytest.mark.parametrize("name,dz", EIGHT_DIRECTION_CASES)
def test_eight_directions_one_of_them_zero(hip, name, dz):
    """GPAR_MAX_TERMS directions at n = 130, n* = 129 on the structures with 12 factors, with three linear factors in a term and with four
    factors in a term; direction 5 is all zero and comes back exactly zero (test_a_zero_direction_gives_exactly_zero)."""
    case = deriv_case(name, dz, 130, 129, 8, 5)
    _, _, mean, var = _check_deriv(hip, case, f"{name} dz={dz}")
    assert np.all(mean[5] == 0.0) and np.all(var[5] == 0.0)
    live = [c for c in range(8) if c != 5]
    assert np.all(mean[live] != 0.0) and np.all(var[live] > 0.0)


@pytest.mark.parametrize("name,dz", PRIOR_ONLY_CASES)
def test_the_prior_term_alone_with_three_linear_factors_and_twelve_factors(hip, name, dz):
    """n = 0: zero means and J^T H J, whose cross term l_f l_g prod_{h != f, g} v_h is more than l_f l_g only with a third factor whose value is
    not 1 - three linear factors in a term (lin3_eq).  rtol 1e-12 / atol 1e-13, as test_no_training_rows_gives_zero_means_and_the_prior_term."""
    from gpar_amd.hip import feature_directions

    lib, stream = td._lib_and_stream(hip)
    ns, ndir = 65, 3
    kernel, _, _, xs, U = data(name, dz, 0, ns, ndir)
    want = np.stack([dr.prior_term(spec_of(kernel), xs, U[c]) for c in range(ndir)])
    assert np.all(want > 1e-2)
    ck = hip.compile(kernel, xs.shape[1])
    xs_t = hip.tensor(xs)
    zs = hip.features(ck, xs_t)
    J = feature_directions(ck, xs_t, hip.tensor(U))
    ws = torch.empty(ndir * ns, dtype=torch.float64, device=hip.device)
    mbuf, mean = td._padded(ndir, ns, ns + 3, hip.device)
    vbuf, var = td._padded(ndir, ns, ns + 4, hip.device)
    rc = lib.gpar_posterior_deriv(ctypes.byref(ck.kspec), zs.data_ptr(), ns, int(zs.stride(0)), J.data_ptr(), dz, ns * dz, ndir, None, 0, dz, dz, None,
                                  None, 1, mbuf.data_ptr(), ns + 3, vbuf.data_ptr(), ns + 4, ws.data_ptr(), ndir * ns, stream)
    assert rc == 0
    assert np.all(to_np(mean) == 0.0)
    np.testing.assert_allclose(to_np(var), want, rtol=1e-12, atol=1e-13)
    assert np.all(to_np(mbuf)[:, ns:] == SENTINEL) and np.all(to_np(vbuf)[:, ns:] == SENTINEL)


# ---- chunks of test rows and splits of the training rows strictly between one and all ------------------------------------------------------------------
def _row_doubles(n, count):
    """pt_row_doubles (gram_terms.h; include/gpar_hip.h documents it as the stack of one test row): count * (n rounded up to even + 1)."""
    return count * (((max(n, 1) + 1) & ~1) + 1)


def test_derivative_in_chunks_of_63_64_65_rows_and_in_two_of_three_splits(hip):
    """n = 130 (three column tiles: pt_nsplit gives three splits), n* = 129.  A workspace of c * pt_row_doubles makes the variance pass take
    chunks of c = 63, 64, 65 rows (129 = 63 + 63 + 3 = 64 + 64 + 1 = 65 + 64: a remainder chunk, `var + c0`, `rn` and ldsub = cc all differ
    from n*) and is large enough for all three splits; one of 3 ndir n* - 1 doubles holds two splits, so split 0 walks tiles 0 and 2.
    Variances: the same BITS as the one-chunk call.  trsm_rlt_run solves every row of the stack on its own - at n = 130 one fused block
    kernel over columns 0 .. 127 (a workgroup per 64 rows), one GEMM update and a 2-column strip; the only thing the row count selects is
    gemm_launch's half-tile kernel, which every call here gets (at most 256 tiles) - so a row's arithmetic does not depend on the chunk it is
    in.  The means' splits are summed in another order: tolerance only."""
    name, dz, ndir = CHUNK_DERIV
    n, ns = 130, 129
    case = deriv_case(name, dz, n, ns, ndir)
    what = f"{name} dz={dz} ndir={ndir}"
    _, _, mean, var = _check_deriv(hip, case, what)
    for c in (63, 64, 65):
        ws = c * _row_doubles(n, ndir)
        assert ws // _row_doubles(n, ndir) == c and ws // (ndir * ns) >= 3
        _, _, m, v = _check_deriv(hip, case, f"{what} chunk={c}", ws_doubles=ws)
        np.testing.assert_array_equal(v, var, err_msg=f"{what} chunk={c}")
        np.testing.assert_array_equal(m, mean, err_msg=f"{what} chunk={c}")   # (all three splits, as in the recommended workspace)
    ws = 3 * ndir * ns - 1
    assert ws // (ndir * ns) == 2 and ws >= _row_doubles(n, ndir)
    _, _, m, v = _check_deriv(hip, case, f"{what} two splits", ws_doubles=ws)
    np.testing.assert_array_equal(v, var, err_msg=f"{what} two splits")   # (chunks of two rows)


def test_posterior_terms_in_chunks_of_63_64_65_rows_and_in_two_of_three_splits(hip):
    """The same workspaces for gpar_posterior_terms with every term of twelve_factors its own component (see the test above for the sizes
    and for why the variances keep their bits)."""
    name, dz = CHUNK_TERMS
    n, ns, G = 130, 129, 8
    kernel, x, y, xs, _, each, _ = terms_case(name, dz, n, ns)
    f, obs = tc._conditioned(hip, kernel, x, y)
    p = f._pts(hip.tensor(xs))
    comp = list(range(G))
    mean, var = tc._posterior_terms(hip, obs, p, comp, G)
    np.testing.assert_allclose(mean, each[0], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(var, each[1], rtol=RTOL, atol=ATOL)
    for c in (63, 64, 65, None):
        ws = c * _row_doubles(n, G) if c else 3 * G * ns - 1
        assert (ws // _row_doubles(n, G) == c and ws // (G * ns) >= 3) if c else (ws // (G * ns) == 2 and ws >= _row_doubles(n, G))
        m, v = tc._posterior_terms(hip, obs, p, comp, G, ws_doubles=ws)
        np.testing.assert_allclose(m, each[0], rtol=RTOL, atol=ATOL, err_msg=f"chunk={c}")
        np.testing.assert_allclose(v, each[1], rtol=RTOL, atol=ATOL, err_msg=f"chunk={c}")
        np.testing.assert_array_equal(v, var, err_msg=f"chunk={c}")
        if c:
            np.testing.assert_array_equal(m, mean, err_msg=f"chunk={c}")


# ---- decompose: eight components, both sides of the 48 KB edges, dz = 96 ----------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(TERMS_DZS)))
def test_decompose_passes_with_eight_components_across_their_48k_edges(hip, i):
    """gpar_gram_terms, gpar_gram_terms_diag and gpar_posterior_terms on twelve_factors with every term its own component (ncomp = 8) and
    with one component of all terms, at dz = 38 | 39 (the mean kernel's edge at 8 components), 41 | 42 (at 1 component), 42 | 43
    (gram_terms_kernel's) and 96.  Against numpy, against `eng.gram` of each component's sub-kernel and of the whole; the tolerances of
    tests/test_decompose_gpu.py (module docstring)."""
    from gpar_amd.kernels import Kernel

    dz = TERMS_DZS[i]
    n, ns = sizes(i)
    lib, stream = tc._lib_and_stream(hip)
    kernel, x, y, xs, ref, each, whole_moments = terms_case("twelve_factors", dz, n, ns)
    G = len(kernel.terms)
    assert G == 8
    width = x.shape[1]
    ck = hip.compile(kernel, width)
    assert ck.dz == dz
    z, zs = hip.features(ck, hip.tensor(x)), hip.features(ck, hip.tensor(xs))
    whole = to_np(hip.gram(ck, zs, z))
    magnitude = sum(np.abs(r) for r in ref)
    # gpar_gram_terms: odd and even leading dimensions (the scalar and the 16-byte store path)
    for (comp, ncomp), ldk in (((list(range(G)), G), n + 3), (([0] * G, 1), n + (n & 1) + 2)):
        stride = ns * ldk + (6 if ldk % 2 == 0 else 5)
        buf = torch.full((ncomp * stride + 8,), SENTINEL, dtype=torch.float64, device=hip.device)
        rc = lib.gpar_gram_terms(ctypes.byref(ck.kspec), tc._comp(comp), ncomp, zs.data_ptr(), ns, int(zs.stride(0)), z.data_ptr(), n, int(z.stride(0)),
                                 dz, buf.data_ptr(), ldk, stride, stream)
        assert rc == 0, (rc, dz, ncomp)
        got = to_np(buf)
        blocks = [got[g * stride:g * stride + ns * ldk].reshape(ns, ldk) for g in range(ncomp)]
        for g, block in enumerate(blocks):
            assert np.all(block[:, n:] == SENTINEL) and np.all(got[g * stride + ns * ldk:(g + 1) * stride] == SENTINEL)
            want = ref[g] if ncomp == G else sum(ref)
            np.testing.assert_allclose(block[:, :n], want, rtol=1e-12, atol=1e-12 * (1 + np.abs(want).max()), err_msg=f"dz={dz} ncomp={ncomp} g={g}")
        if ncomp == 1:
            np.testing.assert_array_equal(blocks[0][:, :n], whole, err_msg=f"bits of gpar_gram: dz={dz}")
        else:
            assert np.all(np.abs(sum(b[:, :n] for b in blocks) - whole) <= 8 * EPS * magnitude), dz
            for g, term in enumerate(kernel.terms):   # the component's sub-kernel through eng.gram, compiled on its own
                sub = hip.compile(Kernel([term]), width)
                own = to_np(hip.gram(sub, hip.features(sub, hip.tensor(xs)), hip.features(sub, hip.tensor(x))))
                assert np.all(np.abs(blocks[g][:, :n] - own) <= 8 * EPS * np.abs(ref[g])), (dz, g)
    # gpar_gram_terms_diag
    diag_ref = [np.diag(k) for k in tc._numpy_terms(kernel, xs, xs)]
    buf, out = tc._padded(G, ns, ns + 3, hip.device)
    assert lib.gpar_gram_terms_diag(ctypes.byref(ck.kspec), tc._comp(list(range(G))), G, zs.data_ptr(), ns, int(zs.stride(0)), dz, buf.data_ptr(), ns + 3,
                                    stream) == 0
    assert np.all(to_np(buf)[:, ns:] == SENTINEL)
    for g in range(G):
        np.testing.assert_allclose(to_np(out)[g], diag_ref[g], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(to_np(out).sum(0), to_np(hip.gram_diag(ck, zs)), rtol=1e-12, atol=1e-14)
    # gpar_posterior_terms: 8 components and 1
    f, obs = tc._conditioned(hip, kernel, x, y)
    p = f._pts(hip.tensor(xs))
    for (comp, ncomp), want in (((list(range(G)), G), each), (([0] * G, 1), whole_moments)):
        assert (lds_doubles("terms_mean", dz, ncomp) > LDS_48K) == (dz >= (39 if ncomp == 8 else 42))
        mean, var = tc._posterior_terms(hip, obs, p, comp, ncomp)
        np.testing.assert_allclose(mean, want[0], rtol=RTOL, atol=ATOL, err_msg=f"dz={dz} ncomp={ncomp}")
        np.testing.assert_allclose(var, want[1], rtol=RTOL, atol=ATOL, err_msg=f"dz={dz} ncomp={ncomp}")
        again = tc._posterior_terms(hip, obs, p, comp, ncomp)
        np.testing.assert_array_equal(mean, again[0])
        np.testing.assert_array_equal(var, again[1])
        np.testing.assert_array_equal(tc._posterior_terms(hip, obs, p, comp, ncomp, variance=False)[0], mean)
        cm, cv = obs._components_composed(p, comp, ncomp, True)
        np.testing.assert_allclose(mean, to_np(cm), rtol=RTOL, atol=ATOL, err_msg=f"dz={dz} ncomp={ncomp}")
        np.testing.assert_allclose(var, to_np(cv), rtol=RTOL, atol=ATOL, err_msg=f"dz={dz} ncomp={ncomp}")


# ---- pathwise ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dz", [38, 39, 96])
def test_rff_apply_at_wide_dz_matches_the_long_double_twin(hip, dz):
    """rff_lds_bytes is exactly 48 KB at dz = 38 and above it from 39 on.  The grid of test_rff_apply_matches_the_long_double_twin reduced to
    rows 1, 65, 129 and F = 63, 65, 300 (S = 1 and 3; groups of 1 and 65 rows), its rule for the tolerance unchanged: 8 x the float64
    restatement's own largest distance from the long-double twin over the cases with this dz, never below 8 F 2^-52 max |theta|.  The
    figures are printed."""
    assert (lds_doubles("rff", dz) > LDS_48K) == (dz >= 39)
    cases = []
    for F in (63, 65, 300):
        for S in (1, 3):
            for rows in (1, 65, 129):
                cases.append(tp._measure_rff(hip, *tp._rff_case(rows, F, dz, S, seed=rows + F + S), dz, 0))
            for ns in (1, 65):
                cases.append(tp._measure_rff(hip, *tp._rff_case(S * ns, F, dz, S, seed=ns + F + S + 1), dz, ns))
    own = max(c[1] for c in cases)
    print(f"dz = {dz}: device against the long-double twin {max(c[0] for c in cases):.3e}, the float64 restatement's own error {own:.3e}")
    for err, _, floor, what in cases:
        assert err <= max(8.0 * own, floor), (what, err, own, floor)


@pytest.mark.parametrize("name,dz", APPLY_CASES)
def test_gram_apply_groups_at_wide_dz_against_numpy_and_gram(hip, name, dz):
    """gpar_gram_apply_groups below (38) and above (39, 96) its 48 KB edge, n = 130 (three splits), n* = 65, S = 5: with group_rows = 0 the
    second chunk of GA_COLS = 4 columns holds one column.  The recommended workspace and one that holds two of the three splits.  Against
    `eng.gram` times the vectors and against numpy's oracle.kernels Gram times the vectors, 1e-11 sum |k| |v|
    (test_gram_apply_groups_matches_gram_times_vector)."""
    from gpar_amd import hip as hipmod
    from oracle import kernels as ok

    assert (lds_doubles("gram_apply", dz) > LDS_48K) == (dz >= 39)
    n, ns, S = 130, 65, 5
    kernel, x, _, _, _, _, _ = terms_case(name, dz, n, ns)   # (the non-vacuity of kernel and inputs)
    width, shift = x.shape[1], structure(name, dz)[2]
    rng = np.random.default_rng(dz)
    xg, v = shift + rng.uniform(-1, 1, (S * ns, width)), rng.standard_normal((S, n))
    ck = hip.compile(kernel, width)
    assert ck.dz == dz
    z, zs, vt = hip.features(ck, hip.tensor(x)), hip.features(ck, hip.tensor(xg)), hip.tensor(v)
    pick = np.arange(S * ns) // ns
    Kn = ok.gram(spec_of(kernel), xg, x)
    Kd = to_np(hip.gram(ck, zs, z))
    for Ks in (Kn, Kd):
        full, scale = Ks @ v.T, np.abs(Ks) @ np.abs(v).T   # (S ns) x S
        for ws in (None, 2 * S * ns):
            got = to_np(hipmod.gram_apply_groups(ck, zs, z, vt, group_rows=ns, ws_doubles=ws))
            assert np.all(np.abs(got - full[np.arange(S * ns), pick]) <= 1e-11 * scale[np.arange(S * ns), pick]), (name, dz, ws)
        for ws in (None, 2 * ns * S):
            got = to_np(hipmod.gram_apply_groups(ck, zs[:ns], z, vt, group_rows=0, ws_doubles=ws))
            assert got.shape == (ns, S) and np.all(np.abs(got - full[:ns]) <= 1e-11 * scale[:ns]), (name, dz, ws)
    a = hipmod.gram_apply_groups(ck, zs, z, vt, group_rows=ns)
    assert torch.equal(a, hipmod.gram_apply_groups(ck, zs, z, vt, group_rows=ns))   # the same bits every time


# ---- end to end: a regressor whose layers are wide -------------------------------------------------------------------------------------------------
#: name -> (input columns, configuration, the layers' feature dims).  `per=True` costs 4 feature dims per input column (the EQ over the
#: inputs, two per column for the periodic embedding, the decay): 23 columns is the most GPAR_MAX_DIMS = 96 admits with three outputs - 40
#: columns would be 160 dims, which compile_kernel refuses (tests/test_posterior_limits.py).  The linear model over the inputs takes 40.
#: The periodic term's stretches follow the structures above (period 3 as wide_periodic, 0.7 sqrt(dims / 2) over its 46 embedded and 23 plain
#: dims): at the defaults (period 1, unit scales) the data leave the derivative's variance at 0.998 of its prior term.
WIDE_MODELS = {"per": (23, dict(per=True, per_period=3.0, per_scale=float(_ell(46)), per_decay=float(_ell(23))), (92, 93, 94)), "input_linear": (40, dict(input_linear=True, nonlinear=True), (80, 82, 84))}
N, NS, P = 70, 9, 3


def _assert_wide(reg, name):
    """The layers' feature dims, read off the conditioned model's variables (they exist once a layer has been built): every pass of every
    layer is above its 48 KB edge, so the test cannot silently go narrow."""
    from oracle import gpar_ref

    m, _, dims = WIDE_MODELS[name]
    got = tuple(sum(len(f["scales"]) for t in gpar_ref.layer_spec(reg.get_variables(), m, i, reg.model_config)[0]["terms"] for f in t["factors"])
                for i in range(P))
    assert got == dims and max(got) >= 42, got


def _wide_model(name, replace):
    from gpar_amd import GPARRegressor

    m, config, dims = WIDE_MODELS[name]
    rng = np.random.default_rng(m)
    x = rng.uniform(0, 1, (N, m))
    y = np.stack([np.sin(6 * x[:, 0]) + x[:, 1], np.cos(5 * x[:, m - 1]) * x[:, 0], x[:, 0] - x[:, m - 1] ** 2], axis=1) + 0.05 * rng.standard_normal((N, P))
    y[rng.uniform(size=y.shape) < 0.1] = np.nan
    y[0] = [0.3, -0.2, 0.1]
    xs = rng.uniform(0.05, 0.95, (NS, m))
    # inputs on [0, 1]: differences half as wide as on [-1, 1], so half the stretch of the structures above
    reg = GPARRegressor(replace=replace, impute=True, normalise_y=True, noise=0.1, scale=0.5 * _ell(m), **config)
    reg.condition(x, y)
    return reg, x, y, xs, m


@pytest.mark.parametrize("name", sorted(WIDE_MODELS))
def test_wide_regressor_derivative_against_the_restatement(hip, name):
    """derivative(wrt = 0) and derivative(wrt = m - 1) against dr.model_derivative, rtol 1e-8 / atol 1e-10
    (test_regressor_derivative_against_the_restatement).  Non-vacuity, on the restatement: max |mean| >= 1e-2 per output, and the first
    layer's variance (the one whose prior term the restatement gives without the chain) below 0.95 of it at half the rows - asserted
    before the comparison, though after the call: the model's variables, which the restatement reads, exist once a layer has been built."""
    from oracle import gpar_ref

    replace = name == "input_linear"
    reg, x, y, xs, m = _wide_model(name, replace)
    scale0 = gpar_ref._normalisation(y, True)[1][0]
    for wrt in (0, m - 1):
        mean, var = reg.derivative(xs, wrt=wrt)
        _assert_wide(reg, name)
        hypers = reg.get_variables()
        want_mean, want_var = dr.model_derivative(x, y, hypers, reg.model_config, xs, wrt, impute=True, replace=replace, normalise_y=True)
        U = np.zeros_like(xs)
        U[:, wrt] = 1.0
        prior0 = dr.prior_term(gpar_ref.layer_spec(hypers, m, 0, reg.model_config)[0], xs, U) * scale0 ** 2
        assert np.all(np.abs(want_mean).max(axis=0) >= 1e-2), (name, wrt)
        assert_not_vacuous(want_mean[:, 0], want_var[:, 0], prior0, f"{name} wrt={wrt}")
        np.testing.assert_allclose(mean, want_mean, rtol=RTOL, atol=ATOL, err_msg=f"{name} wrt={wrt}")
        np.testing.assert_allclose(var, want_var, rtol=RTOL, atol=ATOL, err_msg=f"{name} wrt={wrt}")


@pytest.mark.parametrize("name", sorted(WIDE_MODELS))
def test_wide_regressor_decompose_fused_against_composed(hip, monkeypatch, name):
    """GPAR_FUSED_TERMS on against off, rtol 1e-8 / atol 1e-10, and the components' sum against predict_moments
    (test_regressor_decompose_fused_against_composed)."""
    reg, _, _, xs, _ = _wide_model(name, True)
    results = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("GPAR_FUSED_TERMS", switch)
        results[switch] = reg.decompose(xs)
    _assert_wide(reg, name)
    fused, composed = results["1"], results["0"]
    assert fused.names == composed.names
    mean, _ = reg.predict_moments(xs, latent=True)
    for i in range(P):
        assert np.abs(fused.mean[i]).max() >= 1e-2
        np.testing.assert_allclose(fused.mean[i], composed.mean[i], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(fused.var[i], composed.var[i], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(fused.offset[i] + fused.mean[i].sum(0), mean[:, i], rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("name", sorted(WIDE_MODELS))
def test_wide_regressor_pathwise_fused_against_composed(hip, monkeypatch, name):
    """sample(sampler="pathwise") through the two library calls against GPAR_FUSED_PATHWISE=0 with the same seed, to 1e-9
    (test_fused_route_equals_the_composed_route)."""
    reg, _, _, xs, _ = _wide_model(name, False)
    out = []
    for flag in ("1", "0"):
        monkeypatch.setenv("GPAR_FUSED_PATHWISE", flag)
        hip.seed(11)
        out.append(np.stack(reg.sample(xs, posterior=True, num_samples=3, sampler="pathwise", features=256)))
    _assert_wide(reg, name)
    assert out[0].shape == (3, NS, P) and np.all(np.isfinite(out[0])) and np.abs(out[0]).max() >= 1e-2
    np.testing.assert_allclose(out[0], out[1], rtol=1e-9, atol=1e-9)
