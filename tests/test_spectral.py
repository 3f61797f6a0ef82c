"""The cosine factor and the spectral-mixture keyword on the host (no GPU): kernel algebra and `compile_kernel`, the regressor's
variables and limits, the generated kernels' compilation for gfx950, and the written form cospi(2 s) / -2 pi sinpi(2 s) over the
whole range (tests/cosine_math_emulation.py).  The numeric parity of the device code is in tests/test_spectral_gpu.py."""
import ctypes

import numpy as np
import pytest

from . import cosine_math_emulation as em


# ---- algebra and compile_kernel ---------------------------------------------------------------------------------------------------
def test_cosine_alone_and_stretched():
    from gpar_amd import Cosine, _lib
    from gpar_amd.kernels import compile_kernel

    assert _lib.K_COS == 6
    import os
    import re

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpar_hip.h")).read()
    assert re.findall(r"#define GPAR_K_COS \((\d+)\)", header) == ["6"]
    k = Cosine()
    assert len(k.terms) == 1 and k.terms[0].coef == 1.0 and [f.type for f in k.terms[0].factors] == ["cos"]
    ck = compile_kernel(k, 3)
    fa = ck.kspec.factor[0]
    assert (ck.dz, ck.kspec.nterms, ck.kspec.nfactors) == (3, 1, 1)
    assert (fa.type, fa.term, fa.off, fa.nd) == (6, 0, 0, 3)
    assert [ck.fspec.inv_scale[q] for q in range(3)] == [1.0, 1.0, 1.0]
    assert [ck.fspec.embed[q] for q in range(3)] == [_lib.EMBED_ID] * 3
    periods = np.array([0.5, 0.25, 4.0])
    ck = compile_kernel(Cosine().stretch(periods), 3)
    assert [ck.fspec.inv_scale[q] for q in range(3)] == [2.0, 4.0, 0.25]   # the period of a dim is its length scale
    assert [ck.fspec.col[q] for q in range(3)] == [0, 1, 2]


def test_cosine_selected_and_in_products():
    from gpar_amd import Cosine
    from gpar_amd.kernels import EQ, Linear, compile_kernel

    k = 0.7 * (EQ().stretch(np.array([3.0, 5.0])) * Cosine().stretch(np.array([0.5, 0.125]))).select([2, 0]) + Linear().select([1]) + Cosine().select([1])
    ck = compile_kernel(k, 3)
    got = [(f.type, f.term, f.off, f.nd) for f in ck.kspec.factor[: ck.kspec.nfactors]]
    assert got == [(0, 0, 0, 2), (6, 0, 2, 2), (2, 1, 4, 1), (6, 2, 5, 1)]
    assert [ck.kspec.coef[t] for t in range(3)] == [0.7, 1.0, 1.0]
    assert [ck.fspec.col[q] for q in range(6)] == [2, 0, 2, 0, 1, 1]
    assert [ck.fspec.inv_scale[q] for q in range(2, 4)] == [2.0, 8.0]
    assert ck.layout == [(0, 0, 0, 2), (0, 1, 2, 2), (1, 0, 4, 1), (2, 0, 5, 1)]
    # hyperparameters / stamp see the periods as they see any scales
    import torch

    t = torch.tensor([0.5, 0.25], dtype=torch.float64, requires_grad=True)
    k = Cosine().stretch(t)
    assert k.hyperparameters() == [t] and k.stamp() == ((id(t), t._version),)


def test_periodic_on_a_cosine_factor_raises():
    from gpar_amd import Cosine
    from gpar_amd.kernels import EQ

    with pytest.raises(NotImplementedError, match="SUM of differences"):
        Cosine().periodic(1.0)
    with pytest.raises(NotImplementedError, match="Cosine"):
        (EQ() * Cosine()).periodic(np.array([1.0]))


# ---- the regressor's keyword ------------------------------------------------------------------------------------------------------
def _variables(m, p, **kw):
    from gpar_amd import GPARRegressor
    from gpar_amd.engine import set_engine
    from gpar_amd.regression import _construct_gpar
    from oracle.engine import OracleEngine

    previous = set_engine(OracleEngine())
    try:
        reg = GPARRegressor(**kw)
        gpar = _construct_gpar(reg, reg.vs, m, p)
        kernels = [layer()[0].kernel for layer in gpar.layers]
        return reg, kernels
    finally:
        set_engine(previous)


@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("Q", [1, 3])
def test_variable_names_initial_values_and_bounds(m, Q):
    reg, kernels = _variables(m, 2, spectral=Q, spectral_period=0.6, spectral_scale=7.0, scale_tie=True)
    got = reg.get_variables()
    for pi in range(2):
        for q in range(Q):
            np.testing.assert_allclose(got[f"{pi}/input/sm{q}/var"], 1.0 / Q, rtol=1e-12)
            np.testing.assert_allclose(got[f"{pi}/input/sm{q}/scales"], np.full(m, 7.0), rtol=1e-12)
            np.testing.assert_allclose(got[f"{pi}/input/sm{q}/pers"], np.full(m, 0.6 / (q + 1)), rtol=1e-12)   # the harmonic ladder
            for leaf in ("var", "scales", "pers"):
                var = reg.vs._vars[f"{pi}/input/sm{q}/{leaf}"]
                assert (var.kind, var.lower, var.upper) == ("bnd", 1e-4, 1e4)
        assert f"{pi}/input/sm{Q}/var" not in got
    assert "1/input/scales" not in got and "0/input/scales" in got   # scale_tie ties the EQ scales, not the mixture's
    # the layer kernel: var EQ + sum_q var_q EQ * Cosine over the inputs (+ the linear output term of layer 1)
    for pi, k in enumerate(kernels):
        types = [[f.type for f in t.factors] for t in k.terms]
        assert types == [["eq"]] + [["eq", "cos"]] * Q + ([["linear"]] if pi else [])
        for t in k.terms[1 : 1 + Q]:
            assert all(f.cols == tuple(range(m)) for f in t.factors)


def test_vector_periods_and_envelope_under_matern_and_rq():
    reg, kernels = _variables(2, 1, spectral=3, spectral_period=(0.21, 0.065, 1.5), matern=1.5)
    got = reg.get_variables()
    for q, period in enumerate((0.21, 0.065, 1.5)):
        np.testing.assert_allclose(got[f"0/input/sm{q}/pers"], np.full(2, period), rtol=1e-12)
        np.testing.assert_allclose(got[f"0/input/sm{q}/scales"], np.full(2, 10.0), rtol=1e-12)
    assert [[f.type for f in t.factors] for t in kernels[0].terms] == [["matern32"]] + [["eq", "cos"]] * 3
    _, kernels = _variables(1, 1, spectral=1, rq=True)
    assert [[f.type for f in t.factors] for t in kernels[0].terms] == [["rq"], ["eq", "cos"]]
    with pytest.raises(ValueError, match="2 periods"):
        _variables(1, 1, spectral=3, spectral_period=(0.2, 0.1))


def test_spectral_none_changes_nothing():
    """The variables and the memo keys of a regressor without the keyword, written out as the code before the keyword made them."""
    from gpar_amd import GPARRegressor

    reg, _ = _variables(2, 2)
    assert list(reg.get_variables()) == ["0/input/var", "0/input/scales", "0/noise", "1/input/var", "1/input/scales", "1/output/lin/scales", "1/noise"]
    keys = [repr((2, pi, 1.0, False, False, 1.0, 1.0, 10.0, False, 100.0, True, 100.0, False, 1.0, False, None, 0.1)) for pi in range(2)]
    assert sorted(reg.vs._memo) == sorted(keys)
    assert "spectral" not in GPARRegressor().model_config and GPARRegressor().spectral is None
    assert sorted(GPARRegressor(matern=2.5).model_config) == sorted(list(GPARRegressor().model_config) + ["matern"])
    reg, _ = _variables(2, 1, spectral=2, spectral_period=0.5)
    assert list(reg.vs._memo) == [repr((2, 0, 1.0, False, False, 1.0, 1.0, 10.0, False, 100.0, True, 100.0, False, 1.0, False, None, 0.1)
                                       + (("spectral", 2, 0.5, 10.0),))]


def test_validation_errors():
    from gpar_amd import GPARRegressor

    for bad in (True, False, 0, -1, 2.0, "2"):
        with pytest.raises(ValueError, match="spectral must be"):
            GPARRegressor(spectral=bad)
    with pytest.raises(ValueError, match="GPAR_MAX_TERMS = 8"):
        GPARRegressor(spectral=7)                                  # 1 + 1 (linear output) + 7 terms
    with pytest.raises(ValueError, match="GPAR_MAX_FACTORS = 12"):
        GPARRegressor(spectral=6)                                  # 8 terms, 1 + 1 + 12 factors
    GPARRegressor(spectral=5)
    with pytest.raises(ValueError, match="GPAR_MAX_FACTORS = 12"):
        GPARRegressor(spectral=5, per=True, linear=False)          # 7 terms, 1 + 2 + 10 factors
    GPARRegressor(spectral=4, per=True, linear=False)
    with pytest.raises(ValueError, match="GPAR_MAX_DIMS = 96"):
        _variables(10, 2, spectral=5)                              # 10 + 1 + 2 * 5 * 10 feature dims, known once m and p are
    _variables(8, 2, spectral=5)
    # a cosine over no columns is refused by the library (an argument error, not the constant 1)
    from gpar_amd import Cosine, _lib
    from gpar_amd.kernels import compile_kernel

    ck = compile_kernel(Cosine().select([]), 1)
    assert ck.kspec.factor[0].nd == 0
    log = ctypes.create_string_buffer(4096)
    assert _lib.load().gpar_jit_compile_check(0, ctypes.byref(ck.kspec), ck.dz, b"gfx950", log, len(log)) < -1000


# ---- the generated kernels compile for gfx950 -------------------------------------------------------------------------------------
def _structures():
    from gpar_amd import Cosine
    from gpar_amd.kernels import compile_kernel

    _, kernels = _variables(1, 2, spectral=2)
    return {"cosine only": compile_kernel(Cosine().stretch(np.array([0.5])), 1),
            "regressor Q = 2": compile_kernel(kernels[1], 2),
            "nd = 16": compile_kernel(Cosine().stretch(np.linspace(0.5, 2.0, 16)), 16)}


@pytest.mark.parametrize("name", ["cosine only", "regressor Q = 2", "nd = 16"])
def test_generated_kernels_compile_for_gfx950(name):
    """Kinds (include/gpar_hip.h): 0 Gram build, 1 / 11 parameter-gradient pass (symmetric / rectangular weights), 2 / 12 input-gradient
    pass."""
    from gpar_amd import _lib

    lib, ck = _lib.load(), _structures()[name]
    log = ctypes.create_string_buffer(1 << 16)
    for kind in (0, 1, 11, 2, 12):
        size = lib.gpar_jit_compile_check(kind, ctypes.byref(ck.kspec), ck.dz, b"gfx950", log, len(log))
        assert size > 0, (kind, log.value.decode()[:4000])


def test_wide_cosine_structure_has_no_generated_gram_kernel():
    from gpar_amd import Cosine, _lib
    from gpar_amd.kernels import compile_kernel

    ck = compile_kernel(Cosine().stretch(np.linspace(0.5, 2.0, 17)), 17)
    log = ctypes.create_string_buffer(1 << 16)
    lib = _lib.load()
    assert lib.gpar_jit_compile_check(0, ctypes.byref(ck.kspec), ck.dz, b"gfx950", log, len(log)) < -1000   # refused: the interpreter serves it
    assert lib.gpar_jit_compile_check(1, ctypes.byref(ck.kspec), ck.dz, b"gfx950", log, len(log)) > 0


def test_archive_holds_the_regressors_structures():
    from gpar_amd import aot

    _, keys = aot.read_keys()
    for Q in (1, 2, 4):
        for linear in (True, False):
            _, kernels = _variables(1, 2 if linear else 1, spectral=Q, linear=linear)
            from gpar_amd.kernels import compile_kernel

            ck = compile_kernel(kernels[-1], 1 + (1 if linear else 0))
            sig = f"t{ck.kspec.nterms}d{ck.dz}x" + "{}" + "".join(f"|{f.type},{f.term},{f.off},{f.nd}" for f in ck.kspec.factor[: ck.kspec.nfactors])
            assert "0#" + sig.format(1) in keys and "1#" + sig.format(100) in keys, (Q, linear)


# ---- the written form over the whole range ----------------------------------------------------------------------------------------
SPECIAL = [0.0, 2.0 ** -52, 0.25, 0.5, 1.0, 2.0 ** 20 + 0.25, 1e9]


def _points():
    rng = np.random.default_rng(5)
    special = np.array([sgn * v for v in SPECIAL for sgn in (1.0, -1.0)])
    return np.concatenate([special, rng.uniform(-4, 4, 4000), rng.uniform(-1, 1, 2000) * 10.0 ** rng.uniform(0, 9, 2000),
                           rng.uniform(-1, 1, 500) * 2.0 ** -rng.uniform(1, 60, 500)])


def test_written_form_matches_long_double_over_the_whole_range():
    """cospi(2 s) and -2 pi sinpi(2 s) with the exact reduction: absolute error at most 2^-52 (value; two roundings of a number at most 1)
    and 2 pi 2^-51 (derivative) against long double, at every size of s - where cos(2 pi s) is off by 2 pi |s| 2^-53."""
    s = _points()
    want_c, want_d = em.reference(s)
    got_c, got_d = em.cospi2(s), em.dcospi2(s)
    err_c = np.max(np.abs(got_c.astype(np.longdouble) - want_c))
    err_d = np.max(np.abs(got_d.astype(np.longdouble) - want_d))
    print(f"largest error: value {float(err_c):.3e}, derivative {float(err_d):.3e}")
    assert err_c <= 2.0 ** -52 and err_d <= 2.0 * np.pi * 2.0 ** -51
    # the special points, exactly
    assert em.cospi2(0.0) == 1.0 and em.dcospi2(0.0) == 0.0
    for v in (0.5, 1.0, -1.0, 1e9, -1e9):
        assert em.cospi2(v) == (-1.0 if v in (0.5,) else 1.0) and em.dcospi2(v) == 0.0
    assert abs(em.cospi2(0.25)) <= 2.0 ** -53 and abs(em.cospi2(2.0 ** 20 + 0.25)) <= 2.0 ** -53
    assert abs(em.dcospi2(-(2.0 ** 20 + 0.25)) - em.TWO_PI) <= 2.0 ** -50
    assert np.array_equal(em.cospi2(-s), em.cospi2(s)) and np.array_equal(em.dcospi2(-s), -em.dcospi2(s))   # even / odd in bits
    # ... and the form the device does not use loses the phase at large arguments
    big = np.array([2.0 ** 20 + 0.25, 1e9 + 0.125, 123456789.375])
    assert np.max(np.abs(em.naive(big).astype(np.longdouble) - em.reference(big)[0])) > 1e-10
    assert np.max(np.abs(em.cospi2(big).astype(np.longdouble) - em.reference(big)[0])) <= 2.0 ** -52
