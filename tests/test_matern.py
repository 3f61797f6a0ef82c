"""Matern kernels of smoothness 1/2, 3/2 and 5/2 on the host side: kernel algebra and lowering to the device specification,
the `matern=` keyword of GPARRegressor, and the generated Gram / gradient sources, compiled - not loaded - for gfx950.  No GPU
needed; the numerical tests are in tests/test_matern_gpu.py."""
import ctypes

import numpy as np
import pytest

NUS = [0.5, 1.5, 2.5]


def _constructor(nu):
    from gpar_amd.kernels import Matern12, Matern32, Matern52

    return {0.5: Matern12, 1.5: Matern32, 2.5: Matern52}[nu]


def _code(nu):
    from gpar_amd import _lib

    return {0.5: _lib.K_MATERN12, 1.5: _lib.K_MATERN32, 2.5: _lib.K_MATERN52}[nu]


def test_type_codes_follow_the_header():
    import os
    import re

    from gpar_amd import _lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpar_hip.h")).read()
    codes = {name: int(value) for name, value in re.findall(r"#define GPAR_K_(\w+) (\d+)", header)}
    assert codes == {"EQ": _lib.K_EQ, "RQ": _lib.K_RQ, "LINEAR": _lib.K_LINEAR, "MATERN12": _lib.K_MATERN12,
                     "MATERN32": _lib.K_MATERN32, "MATERN52": _lib.K_MATERN52}
    assert (_lib.K_MATERN12, _lib.K_MATERN32, _lib.K_MATERN52) == (3, 4, 5)


def test_constructors_are_exported():
    import gpar_amd
    from gpar_amd import kernels

    for name in ("Matern12", "Matern32", "Matern52"):
        assert name in kernels.__all__ and name in gpar_amd.__all__
        assert getattr(gpar_amd, name) is getattr(kernels, name)


@pytest.mark.parametrize("nu", NUS)
def test_algebra_and_lowering(nu):
    from gpar_amd import _lib
    from gpar_amd.kernels import EQ, Linear, compile_kernel, linear_tail

    M = _constructor(nu)
    s = np.array([0.5, 2.0, 4.0])
    kernel = (3.0 * M().stretch(s)).select([0, 2, 3]) + (0.25 * M().stretch(8.0) * EQ().stretch(0.1)).select([1]) + Linear().stretch(np.array([10.0])).select([4])
    ck = compile_kernel(kernel, 5)
    ks, fs = ck.kspec, ck.fspec
    assert (ks.nterms, ks.nfactors, ck.dz) == (3, 4, 6)
    assert [ks.coef[t] for t in range(3)] == [3.0, 0.25, 1.0]
    got = [(ks.factor[f].type, ks.factor[f].term, ks.factor[f].off, ks.factor[f].nd, ks.factor[f].alpha) for f in range(4)]
    assert got == [(_code(nu), 0, 0, 3, 0.0), (_code(nu), 1, 3, 1, 0.0), (_lib.K_EQ, 1, 4, 1, 0.0), (_lib.K_LINEAR, 2, 5, 1, 0.0)]
    assert [fs.col[q] for q in range(6)] == [0, 2, 3, 1, 1, 4]
    assert [fs.inv_scale[q] for q in range(6)] == [1 / 0.5, 1 / 2.0, 1 / 4.0, 1 / 8.0, 1 / 0.1, 1 / 10.0]
    assert all(fs.embed[q] == _lib.EMBED_ID for q in range(6))
    assert ck.layout == [(0, 0, 0, 3), (1, 0, 3, 1), (1, 1, 4, 1), (2, 0, 5, 1)]
    # the linear factor over column 4 is a linear tail; a Matern factor over an output column is not
    assert linear_tail(ck, 4) is not None
    assert linear_tail(ck, 3) is None

    # .periodic doubles the features: sin features first, then cos, both with the frequency 2 pi / period
    per = compile_kernel(M().stretch(np.array([1.0, 2.0, 3.0, 4.0])).periodic(np.array([0.5, 0.25])).select([1, 0]), 2)
    assert per.dz == 4 and per.kspec.factor[0].type == _code(nu) and per.kspec.factor[0].nd == 4
    assert [per.fspec.col[q] for q in range(4)] == [1, 0, 1, 0]
    assert [per.fspec.embed[q] for q in range(4)] == [_lib.EMBED_SIN, _lib.EMBED_SIN, _lib.EMBED_COS, _lib.EMBED_COS]
    assert [per.fspec.freq[q] for q in range(4)] == [2 * np.pi / 0.5, 2 * np.pi / 0.25] * 2
    assert [per.fspec.inv_scale[q] for q in range(4)] == [1.0, 0.5, 1 / 3.0, 0.25]

    # products distribute over sums as for EQ
    prod = compile_kernel(((M() + 2.0) * Linear()).select([0]), 1)
    assert prod.kspec.nterms == 2 and prod.kspec.nfactors == 3
    assert [prod.kspec.factor[f].type for f in range(3)] == [_code(nu), _lib.K_LINEAR, _lib.K_LINEAR]


def _layer_kernels(reg, m, p):
    from gpar_amd.regression import _construct_gpar

    gpar = _construct_gpar(reg, reg.vs, m, p)
    return [layer()[0].kernel for layer in gpar.layers]


def _with_oracle_engine(fn):
    """(the numpy engine only creates the variables here; no kernel is evaluated)"""
    from gpar_amd.engine import set_engine
    from oracle.engine import OracleEngine

    previous = set_engine(OracleEngine())
    try:
        return fn()
    finally:
        set_engine(previous)


@pytest.mark.parametrize("nu", NUS)
def test_regressor_keyword_puts_matern_where_the_default_has_eq(nu):
    from gpar_amd.regression import GPARRegressor

    name = {0.5: "matern12", 1.5: "matern32", 2.5: "matern52"}[nu]

    def run():
        kw = dict(scale=0.5, linear=True, nonlinear=True, per=True, input_linear=True, markov=2)
        default, matern = GPARRegressor(**kw), GPARRegressor(matern=nu, **kw)
        kd, km = _layer_kernels(default, 2, 4), _layer_kernels(matern, 2, 4)
        return default, matern, kd, km

    default, matern, kd, km = _with_oracle_engine(run)
    assert matern.matern == nu and default.matern is None
    assert "matern" not in default.model_config and matern.model_config["matern"] == nu
    replaced = 0
    for a, b in zip(kd, km):
        assert len(a.terms) == len(b.terms)
        for ta, tb in zip(a.terms, b.terms):
            assert len(ta.factors) == len(tb.factors)
            locally_periodic = any(f.periods is not None for f in ta.factors)
            for fa, fb in zip(ta.factors, tb.factors):
                assert fa.cols == fb.cols and (fa.periods is None) == (fb.periods is None)
                assert np.array_equal(fa.scales_value(), fb.scales_value())
                if fa.type == "eq" and not locally_periodic:
                    assert fb.type == name and fb.alpha is None
                    replaced += 1
                else:
                    assert fb.type == fa.type   # the locally periodic term keeps its EQ factors, linear stays linear
    assert replaced == 4 + 3   # the input kernel of four layers, the nonlinear output kernel of layers 1 .. 3
    assert sorted(matern.vs.names) == sorted(default.vs.names)
    for n in default.vs.names:
        assert np.array_equal(matern.vs[n].detach().numpy(), default.vs[n].detach().numpy())
    assert not any("alpha" in n for n in matern.vs.names)


def test_regressor_keyword_validation():
    from gpar_amd.regression import GPARRegressor

    for nu in (1 / 2, 3 / 2, 5 / 2, np.float64(1.5)):
        assert GPARRegressor(matern=nu).matern == float(nu)
    for bad in (0.7, 1, 3.5, "1.5", True, float("nan")):
        with pytest.raises(ValueError):
            GPARRegressor(matern=bad)
    with pytest.raises(ValueError):
        GPARRegressor(matern=1.5, rq=True)
    assert GPARRegressor().matern is None and GPARRegressor(rq=True).matern is None


def _specs(nu):
    from gpar_amd.kernels import compile_kernel
    from gpar_amd.regression import GPARRegressor, _construct_gpar

    def run():
        out = []
        for kw, m, p in [
            (dict(linear=True, nonlinear=True, matern=nu, markov=2), 4, 8),      # narrow: the strip form of the Gram kernel
            (dict(per=True, linear=True, nonlinear=True, matern=nu), 3, 16),     # its last layers take the wide 4 x 4 form
        ]:
            reg = GPARRegressor(**kw)
            gpar = _construct_gpar(reg, reg.vs, m, p)
            for layer in sorted({0, 1, p - 1}):
                f, _ = gpar.layers[layer]()
                out.append(compile_kernel(f.kernel, m + layer))
        return out

    return _with_oracle_engine(run)


@pytest.mark.parametrize("nu", NUS)
def test_generated_sources_compile_for_gfx950(nu):
    """Kinds (include/gpar_hip.h): 0 Gram build (strip form up to 16 feature dims, the 4 x 4 micro-tile form above), 1 / 21
    parameter-gradient pass (21: with the frequency derivatives of periodic features), 2 input-gradient pass."""
    from gpar_amd import _lib
    from gpar_amd.engine import GRAM_JIT_MAX_DZ, GRAM_JIT_WIDE_MAX_DZ

    lib = _lib.load()
    log = ctypes.create_string_buffer(1 << 16)
    narrow = wide = 0
    for ck in _specs(nu):
        assert any(ck.kspec.factor[f].type == _code(nu) for f in range(ck.kspec.nfactors))
        assert ck.dz <= GRAM_JIT_WIDE_MAX_DZ
        assert lib.gpar_jit_compile_check(0, ctypes.byref(ck.kspec), ck.dz, b"gfx950", log, len(log)) > 0, log.value.decode()[:4000]
        narrow += ck.dz <= GRAM_JIT_MAX_DZ
        wide += ck.dz > GRAM_JIT_MAX_DZ
        periodic = any(f.periods is not None for t in ck.kernel.terms for f in t.factors)
        kinds = [1, 11] + ([21, 31] if periodic else [])
        if 1 <= ck.dz <= 20:
            kinds += [2, 12]
        for kind in kinds:
            assert lib.gpar_jit_compile_check(kind, ctypes.byref(ck.kspec), ck.dz, b"gfx950", log, len(log)) > 0, (kind, log.value.decode()[:4000])
    assert narrow >= 3 and wide >= 1


def test_archive_holds_the_matern_families():
    """gpar_amd/aot.py: Matern 3/2 and 5/2 are keyword families of the build-time archive; an archive of a library without the Matern
    types has another generator fingerprint and is refused (the probe structure of the fingerprint contains all three types)."""
    import os

    from gpar_amd import aot

    assert aot.FAMILIES["matern32"] == dict(linear=True, nonlinear=True, matern=1.5)
    assert aot.FAMILIES["matern52"] == dict(linear=True, nonlinear=True, matern=2.5)
    assert os.path.exists(aot.ARCHIVE), "build it: python -c 'import __graft_entry__ as g; g.build()'"
    assert aot.is_current()
    _, keys = aot.read_keys()
    for code in (4, 5):
        # layer 1 of m = 2: input kernel over columns 0, 1, linear and Matern output kernels over column 2
        assert f"0#t3d4x1|{code},0,0,2|2,1,2,1|{code},2,3,1" in keys
        assert f"1#t3d4x100|{code},0,0,2|2,1,2,1|{code},2,3,1" in keys
    assert not any("|3," in k for k in keys)   # nu = 1/2 is compiled at first use
