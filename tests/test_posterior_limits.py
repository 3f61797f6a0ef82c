"""The references of tests/test_posterior_limits_gpu.py, checked where no GPU is: the restatement's cross-covariance rows and prior term
for the structures with three linear factors and with four factors in a term against central differences of oracle.mp_ref.gram in
extended precision; the non-vacuity condition of every case the device tests use; the arithmetic of the 48 KB and 160 KB edges of the
dynamic LDS; and the shapes of the structures themselves."""
import os
import re

import mpmath as mp
import numpy as np
import pytest

from oracle import mp_ref

from . import derivative_reference as dr
from . import test_posterior_limits_gpu as lim
from .test_derivative import _shift

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpar_amd", "csrc")
FD_CASES = (("lin3_eq", 31), ("wide_mixed", 29), ("twelve_factors", 30))


def _points(name, dz):
    kernel, x, _, xs, U = lim.data(name, dz, 4, 3, 1)
    return lim.spec_of(kernel), x, xs, U[0]


# ---- the restatement against central differences (tests/test_derivative.py does this for the narrow structures) ------------------------------
# Step 1e-20.  The first difference runs at mp_ref's 50 digits: k is known to 1e-50, the quotient by 2 h to 1e-30, the truncation is h^2.
# The MIXED second difference divides four values of k by 4 h^2 = 4e-40: at 50 digits ten digits would be left, so it runs at 80 (as
# tests/test_derivative.py's does), where 1e-40 are.  Tolerance: that file's 1e-12 (1 + max |reference|) absolute.
@pytest.mark.parametrize("name,dz", FD_CASES)
def test_cross_rows_of_the_wide_structures_against_mpmath_central_differences(name, dz):
    spec, x, xs, U = _points(name, dz)
    got = dr.cross_rows(spec, xs, x, U)
    assert mp.mp.dps == 50
    h = mp.mpf(10) ** -20
    rows = [[mp.mpf(float(v)) for v in row] for row in x]
    up, down = mp_ref.gram(spec, _shift(xs, U, h), rows), mp_ref.gram(spec, _shift(xs, U, -h), rows)
    want = np.array([[float((up[a, b] - down[a, b]) / (2 * h)) for b in range(x.shape[0])] for a in range(xs.shape[0])])
    assert np.abs(want).max() > 1e-3
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * (1 + np.abs(want).max()))
    many = dr.layer_derivatives(spec, x, np.array([0.3, -1.2, 0.8, 0.5]), 0.1, xs, U[None])
    one = dr.layer_derivative(spec, x, np.array([0.3, -1.2, 0.8, 0.5]), 0.1, xs, U)
    np.testing.assert_allclose(many[0][0], one[0], rtol=1e-13, atol=1e-15)   # (the stacked form is the same restatement)
    np.testing.assert_allclose(many[1][0], one[1], rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("name,dz", FD_CASES)
def test_prior_term_of_the_wide_structures_against_mpmath_mixed_central_differences(name, dz):
    spec, _, xs, U = _points(name, dz)
    got = dr.prior_term(spec, xs, U)
    want = np.zeros(xs.shape[0])
    with mp.workdps(80):
        h = mp.mpf(10) ** -20
        for a in range(xs.shape[0]):
            up, down = _shift(xs[a:a + 1], U[a:a + 1], h), _shift(xs[a:a + 1], U[a:a + 1], -h)
            k = lambda p, q: mp_ref.gram(spec, p, q)[0, 0]
            want[a] = float((k(up, up) - k(up, down) - k(down, up) + k(down, down)) / (4 * h * h))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * (1 + np.abs(want).max()))
    assert np.all(got > 0.0)


def test_three_linear_factors_make_the_cross_term_more_than_a_product_of_two():
    """In lin3_eq the third linear factor's value |z|^2 multiplies l_f l_g: the structure exercises `rest2`."""
    spec, _, xs, _ = _points("lin3_eq", 31)
    (term,) = spec["terms"]
    assert [f["type"] for f in term["factors"]] == ["linear", "linear", "linear", "eq"]
    from oracle import kernels as ok

    values = [float((ok.features(f, xs[:1]) ** 2).sum()) for f in term["factors"][:3]]
    assert all(abs(v - 1.0) > 0.02 and 0.3 < v < 3.0 for v in values), values   # O(1), and not 1


# ---- non-vacuity, for every structure and size of the device tests ------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(lim.every_reference())))
def test_every_reference_of_the_device_tests_is_not_vacuous(i):
    fn, args = lim.every_reference()[i]
    fn(*args)   # (asserts the condition: max |mean| >= 1e-2, half the rows' variance below 0.95 of the prior term)


def test_the_condition_refuses_a_posterior_that_equals_the_prior():
    """Unit length scales over 40 dims: the EQ vanishes between any two points, and the condition says so."""
    from gpar_amd.kernels import EQ

    rng = np.random.default_rng(0)
    x, y, xs, U = rng.uniform(-1, 1, (65, 40)), rng.standard_normal(65), rng.uniform(-1, 1, (65, 40)), rng.standard_normal((1, 65, 40))
    mean, var, prior = dr.layer_derivatives(lim.spec_of(EQ().stretch(np.full(40, 0.3)).select(range(40))), x, y, lim.NOISE, xs, U)
    with pytest.raises(AssertionError):
        lim.assert_not_vacuous(mean, var, prior, "unit scales")


# ---- the structures -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dz", [13, 17, 29, 30, 38, 59, 96])
def test_twelve_factors_has_eight_terms_and_twelve_factors_at_every_width(dz):
    from gpar_amd.kernels import compile_kernel

    kernel, width, _ = lim.structure("twelve_factors", dz)
    assert sorted(len(t.factors) for t in kernel.terms) == [0, 1, 1, 1, 1, 1, 3, 4]
    ck = compile_kernel(kernel, width)
    assert ck.dz == dz and ck.kspec.nterms == 8 and ck.kspec.nfactors == 12


@pytest.mark.parametrize("name,dz,factors", [("wide_eq", 96, 1), ("wide_mixed", 8, 4), ("wide_mixed", 59, 4), ("lin3_eq", 8, 4), ("lin3_eq", 29, 4),
                                             ("wide_periodic", 96, 1), ("wide_periodic", 18, 1)])
def test_the_other_structures_have_the_dims_they_are_asked_for(name, dz, factors):
    from gpar_amd.kernels import compile_kernel

    kernel, width, _ = lim.structure(name, dz)
    ck = compile_kernel(kernel, width)
    assert ck.dz == dz and ck.kspec.nterms == 1 and ck.kspec.nfactors == factors
    if name == "wide_periodic":
        assert width == dz // 2   # the embedding doubles the columns


def test_forty_columns_with_a_periodic_term_do_not_fit_the_specification():
    """Why the wide `per=True` model of the device tests has 23 input columns: the layer kernel takes 4 feature dims per column - 160 at 40
    columns, which compile_kernel refuses -, and 94 in the last of three layers at 23."""
    from gpar_amd import GPARRegressor
    from gpar_amd.kernels import EQ, compile_kernel
    from gpar_amd.regression import _layer_kernel_size

    config = GPARRegressor(per=True).model_config
    assert _layer_kernel_size(config, 40, 3)[2] == 162 and _layer_kernel_size(config, 23, 3)[2] == 94
    cols = range(40)
    layer = EQ().stretch(np.ones(40)).select(cols) + EQ().stretch(np.ones(80)).periodic(np.ones(40)).select(cols) * EQ().stretch(np.ones(40)).select(cols)
    with pytest.raises(ValueError, match="too many kernel feature dimensions"):
        compile_kernel(layer, 40)
    for name, (m, model, dims) in lim.WIDE_MODELS.items():
        assert _layer_kernel_size(GPARRegressor(**model).model_config, m, 3)[2] == max(dims) and 42 <= min(dims) and max(dims) <= 96, name


# ---- the LDS edges ------------------------------------------------------------------------------------------------------------------------------
def _constant(name, *files):
    for file in files:
        found = re.search(rf"constexpr int {name} = ([^;]+);", open(os.path.join(CSRC, file)).read())
        if found:
            return found.group(1).strip()
    raise AssertionError(name)


def test_the_constants_of_the_restated_formulas_are_the_sources():
    assert int(_constant("GRAM_T", "gram_math.inc")) == lim.GRAM_T and int(_constant("GRAM_LD", "gram_math.inc")) == lim.GRAM_LD
    assert _constant("GRAM_TAB_DOUBLES", "gram_math.inc") == "GRAM_EXP_TAB + 256" and int(_constant("GRAM_EXP_TAB", "gram_math.inc")) + 256 == lim.GRAM_TAB_DOUBLES
    for name in ("PW_ROWS", "PW_FREQS", "PW_COLS", "PW_SLICES", "GA_COLS"):
        assert int(_constant(name, "pathwise.h")) == getattr(lim, name)
    deriv, terms, path = (open(os.path.join(CSRC, f)).read() for f in ("gram_deriv.h", "gram_terms.h", "pathwise.h"))
    # the formulas `lim.lds_doubles` mirrors, and the 48 KB test each launch makes
    assert "((size_t)(2 + ndir) * dzl * GRAM_LD + (mean ? GRAM_LD + (size_t)ndir * GRAM_T : 0)) * sizeof(double)" in deriv
    assert "constexpr size_t PD_MAX_LDS = 160 * 1024;" in deriv and deriv.count("if (lds > 48 * 1024)") == 2
    assert "((size_t)2 * (dz > 0 ? dz : 1) * GRAM_LD + GRAM_TAB_DOUBLES) * sizeof(double)" in terms
    assert "((size_t)2 * (dz > 0 ? dz : 1) * GRAM_LD + GRAM_TAB_DOUBLES + GRAM_LD + (size_t)G * GRAM_T) * sizeof(double)" in terms
    assert terms.count("if (lds > 48 * 1024)") == 2
    assert "((size_t)2 * (dz > 0 ? dz : 1) * GRAM_LD + GRAM_TAB_DOUBLES + GA_COLS * GRAM_LD + GA_COLS * GRAM_T) * sizeof(double)" in path
    assert "((size_t)dzl * (PW_ROWS + PW_FREQS) + 2 * PW_COLS * PW_FREQS + (PW_SLICES - 1) * PW_COLS * PW_ROWS) * sizeof(double)" in path
    assert path.count("if (lds > 48 * 1024)") == 2


@pytest.mark.parametrize("kernel,count,below,above", lim.EDGES_48K)
def test_the_48k_edges(kernel, count, below, above):
    assert above == below + 1
    assert lim.lds_doubles(kernel, below, count) <= lim.LDS_48K < lim.lds_doubles(kernel, above, count)


@pytest.mark.parametrize("ndir,fits,refused", lim.EDGES_160K)
def test_the_160k_edges_of_gpar_posterior_deriv(ndir, fits, refused):
    from gpar_amd import _lib

    assert lim.lds_doubles("deriv_mean", fits, ndir) <= lim.LDS_160K
    if refused is None:
        assert fits == _lib.GPAR_MAX_DIMS
    else:
        assert refused == fits + 1 and lim.lds_doubles("deriv_mean", refused, ndir) > lim.LDS_160K


def test_the_device_cases_sit_on_the_edges():
    """The parametrisation of the device tests holds both sides of every edge."""
    deriv = {(ndir, dz) for ndir, dz, _ in lim.DERIV_EDGE_CASES}
    for kernel, count, below, above in lim.EDGES_48K:
        if kernel in ("deriv_mean", "deriv_stack"):
            assert {(count, below), (count, above)} <= deriv
        elif kernel in ("terms_mean", "gram_terms"):
            assert {below, above} <= set(lim.TERMS_DZS)
        else:
            assert {below, above} <= {dz for _, dz in lim.APPLY_CASES}
    assert {(8, 29), (3, 59), (1, 96)} <= deriv and 96 in lim.TERMS_DZS
