"""The reference of tests/test_grad_rows_limits_gpu.py, checked where no GPU is: the long-double restatement of the per-row parameter
gradients (tests/grad_rows_reference.py) against central differences of oracle.mp_ref.gram in 50-digit arithmetic, for every structure of
the device tests at a narrow and a wide dz; the arithmetic of the 48 KB and 160 KB edges of gram_grad_rows_kernel's dynamic LDS against
the restated formula, the slot counter and the sources; and the non-vacuity of every case the device tests compare."""
import os
import re

import mpmath as mp
import numpy as np
import pytest

from oracle import mp_ref

from . import grad_rows_reference as gr
from . import test_grad_rows_limits_gpu as rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpar_amd", "csrc")
#: every structure of the device tests, at a narrow dz and at the widest it is run at
MP_CASES = (("wide_eq", 5), ("wide_eq", 96), ("wide_mixed", 8), ("wide_mixed", 31), ("wide_periodic", 4), ("wide_periodic", 50),
            ("twelve_rq", 12), ("twelve_rq", 95), ("twelve_factors", 13), ("twelve_factors", 52), ("lin3_eq", 8), ("lin3_eq", 29))
MP_ROWS, MP_COLS = 3, 8


# ---- the restatement against 50-digit central differences ---------------------------------------------------------------------------------------
def _sample(spec):
    """The parameters compared: every coefficient, alpha and period, and the first and last length scale of every factor - as
    (name of the restatement, `wrt` entry of mp_ref._perturbed)."""
    out = []
    for t, term in enumerate(spec["terms"]):
        out.append((f"coef/{t}", {"kind": "coef", "term": t}))
        for f, factor in enumerate(term["factors"]):
            nd = len(factor["scales"])
            for q in sorted({0, nd - 1}):
                out.append((f"scales/{t}/{f}/{q}", {"kind": "scales", "term": t, "factor": f, "index": q}))
            if factor.get("periods") is not None:
                # the sin and cos features of column c: their scales are both compared where the factor has one column only
                for c in range(len(factor["periods"])):
                    out.append((f"periods/{t}/{f}/{c}", {"kind": "periods", "term": t, "factor": f, "index": c}))
            if factor["type"] == "rq":
                out.append((f"alpha/{t}/{f}", {"kind": "alpha", "term": t, "factor": f}))
    return out


def _mp(value):
    """A long double as an mp number, exactly: its double part and the rest."""
    head = float(value)
    return mp.mpf(head) + mp.mpf(float(value - gr.LD(head)))


@pytest.mark.parametrize("name,dz", MP_CASES)
def test_the_restatement_against_mpmath_central_differences(name, dz):
    """d g_a / d theta of 3 rows against 8 columns: one natural parameter moved by +- 1e-20 of its size in mp_ref's 50 digits (k is known
    to 1e-50, the quotient by 2 h to 1e-30; the truncation is h^2), as tests/test_posterior_limits.py differentiates in the inputs.
    Agreement to 1e-15 S_a: long double carries 1e-19, which leaves four digits for the restatement's own sums."""
    kernel, _, x1, x2, v = rows.inputs(name, dz, MP_ROWS, MP_COLS)
    spec = rows.lim.spec_of(kernel)
    grads, mags = gr.row_gradients(spec, x1, x2, v)
    assert mp.mp.dps == 50 and np.finfo(gr.LD).eps < 1e-18
    h = mp.mpf(10) ** -20
    vm = [mp.mpf(float(w)) for w in v]
    sample = _sample(spec)
    assert {k for k, _ in sample} <= set(grads)
    assert {k.split("/")[0] for k in grads} == {k.split("/")[0] for k, _ in sample}   # (every kind of parameter the structure has)
    worst = 0.0
    for key, wrt in sample:
        sides = []
        for sign in (1, -1):
            s, p1, _, p2, unit = mp_ref._perturbed(spec, x1, None, x2, wrt, sign * h)
            K = mp_ref.gram(s, p1, p2)
            sides.append([mp.fsum(K[a, b] * vm[b] for b in range(MP_COLS)) for a in range(MP_ROWS)])
        for a in range(MP_ROWS):
            want = (sides[0][a] - sides[1][a]) / (2 * h * unit)
            err = abs(_mp(grads[key][a]) - want)
            bound = 1e-15 * float(mags[key][a])
            assert bound > 0 and err <= bound, (name, dz, key, a, float(err), bound)
            worst = max(worst, float(err) / bound)
    print(f"{name} dz={dz}: {len(sample)} parameters, worst error {worst:.2e} of 1e-15 S")


# ---- the LDS edges ------------------------------------------------------------------------------------------------------------------------------
def _doubles(name, dz, zd):
    from gpar_amd.kernels import compile_kernel

    kernel, width, _ = rows.structure(name, dz)
    ck = compile_kernel(kernel, width)
    assert ck.dz == dz
    used = gr.slots_used(ck.kspec, zd)
    return len(used), gr.rows_lds_doubles(dz, zd, len(used))


def test_the_constants_of_the_restated_formula_are_the_sources():
    from gpar_amd import _lib

    def constant(name, file):
        found = re.search(rf"constexpr int {name} = ([^;]+);", open(os.path.join(CSRC, file)).read())
        assert found, name
        return found.group(1).strip()

    assert int(constant("GRAM_T", "gram_math.inc")) == gr.GRAM_T and int(constant("GRAM_LD", "gram_math.inc")) == gr.GRAM_LD
    assert (gr.MAX_TERMS, gr.MAX_FACTORS, gr.MAX_DIMS) == (_lib.GPAR_MAX_TERMS, _lib.GPAR_MAX_FACTORS, _lib.GPAR_MAX_DIMS)
    assert gr.GRAD_NACC == _lib.GRAD_NACC == 212 and (gr.K_RQ, gr.K_LINEAR, gr.K_COS) == (_lib.K_RQ, _lib.K_LINEAR, _lib.K_COS)
    assert int(constant("GRAD_MAXF", "gram.h")) == gr.MAXF
    src = open(os.path.join(CSRC, "gram_grad_rows.h")).read()
    assert ("return ((size_t)(has_zd ? 4 : 2) * dzl * GRAM_LD + GRAM_LD + (size_t)nused * GRAM_T) * sizeof(double) + GRAD_NACC * sizeof(int);"
            in src)
    assert "const size_t dzl = dz > 0 ? dz : 1;" in src
    assert "constexpr size_t ROWS_MAX_LDS = 160 * 1024;" in src and src.count("if (lds > 48 * 1024)") == 1
    assert "gpar_set_max_lds(reinterpret_cast<const void*>(&gram_grad_rows_kernel), (int)ROWS_MAX_LDS)" in src
    entry = open(os.path.join(CSRC, "gpar_hip.hip")).read()
    assert "if (rows_lds_bytes(dz, zd1 != nullptr, pl.nused) > ROWS_MAX_LDS) return GPAR_ARG_ERROR(10);" in entry
    # the slot plan `slots_used` mirrors
    assert "if (fa.type == GPAR_K_RQ) used[GRAD_OFF_AL + f] = true;" in src
    assert "if (has_zd && fa.type != GPAR_K_LINEAR && fa.type != GPAR_K_COS) used[GRAD_OFF_P + d] = true;" in src
    assert gr.rows_lds_doubles(0, False, 0) == gr.rows_lds_doubles(1, False, 0) == 2 * 68 + 68 + 106


@pytest.mark.parametrize("name,dz,zd,nused,doubles", [
    ("wide_eq", 29, False, 30, 6038), ("wide_eq", 30, False, 31, 6238), ("wide_eq", 96, False, 97, 19438),
    ("wide_mixed", 29, False, 31, 6102), ("wide_mixed", 30, False, 32, 6302), ("wide_mixed", 31, False, 33, 6502),
    ("wide_periodic", 14, True, 29, 5838), ("wide_periodic", 16, True, 33, 6638), ("wide_periodic", 50, True, 101, 20238),
    ("wide_periodic", 52, True, 105, 21038), ("twelve_rq", 95, False, 115, 20454), ("twelve_rq", 96, False, 116, 20654),
    ("twelve_rq", 47, True, 114, 20254), ("twelve_rq", 48, True, 116, 20654),
    ("twelve_factors", 14, True, 33, 6094), ("twelve_factors", 15, True, 35, 6494), ("twelve_factors", 52, True, 94, 20334),
    ("twelve_factors", 53, True, 96, 20734)])
def test_the_table_of_the_lds_edges(name, dz, zd, nused, doubles):
    assert _doubles(name, dz, zd) == (nused, doubles)


@pytest.mark.parametrize("name,zd,below,above", rows.EDGES_48K)
def test_the_48k_edges(name, zd, below, above):
    assert above == below + (2 if name == "wide_periodic" else 1)   # (wide_periodic has even dz only)
    assert _doubles(name, below, zd)[1] <= gr.LDS_48K < _doubles(name, above, zd)[1]


@pytest.mark.parametrize("name,zd,fits,refused", rows.EDGES_160K)
def test_the_160k_edges(name, zd, fits, refused):
    assert _doubles(name, fits, zd)[1] <= gr.LDS_160K
    if refused is None:
        assert fits == gr.MAX_DIMS
    else:
        assert refused == fits + (2 if name == "wide_periodic" else 1) and _doubles(name, refused, zd)[1] > gr.LDS_160K


def test_the_worst_case_of_the_slot_plan():
    """twelve_rq uses every C_t and Al_f slot and a slot per dim (two with zd): no structure of dz dims asks for more.  Without zd every
    structure fits up to dz 95, with zd up to dz 47: the two figures of include/gpar_hip.h and csrc/gram_grad_rows.h."""
    for zd, fits in ((False, 95), (True, 47)):
        worst = lambda dz: gr.rows_lds_doubles(dz, zd, gr.MAX_TERMS + gr.MAX_FACTORS + (2 if zd else 1) * dz)
        assert worst(fits) <= gr.LDS_160K < worst(fits + 1)
        assert _doubles("twelve_rq", fits, zd)[1] == worst(fits)
    for text in (open(os.path.join(CSRC, "gram_grad_rows.h")).read(), open(os.path.join(ROOT, "include", "gpar_hip.h")).read()):
        assert "without zd dz <= 95" in text and "with zd dz <= 47" in text


def test_the_device_cases_sit_on_the_edges():
    cases = set(rows.EDGE_CASES)
    for name, zd, below, above in rows.EDGES_48K:
        assert {(name, below), (name, above)} <= cases
    refused = {(name, dz) for name, dz, _ in rows.REFUSED_CASES}
    for name, zd, fits, first in rows.EDGES_160K:
        assert (name, fits) in cases | set(rows.ZD_WITHOUT_PERIODS)
        assert first is None or (name, first) in refused
    assert {("wide_mixed", 31), ("lin3_eq", 29)} <= cases
    assert all(_doubles(name, dz, rows.has_periods(rows.lim.spec_of(rows.structure(name, dz)[0])))[1] > gr.LDS_48K for name, dz in rows.SHARED_CASES)
    assert _doubles(*rows.SPLIT_CASE, True)[1] > gr.LDS_48K


def test_twelve_rq_has_eight_terms_and_twelve_rq_factors():
    from gpar_amd.kernels import compile_kernel

    for dz in (12, 47, 95, 96):
        kernel, width, _ = rows.structure("twelve_rq", dz)
        ck = compile_kernel(kernel, width)
        assert ck.dz == dz and ck.kspec.nterms == 8 and ck.kspec.nfactors == 12
        assert all(ck.kspec.factor[f].type == gr.K_RQ for f in range(12))
        assert sorted(len(t.factors) for t in kernel.terms) == [1, 1, 1, 1, 1, 1, 2, 4]


# ---- non-vacuity, for every case of the device tests ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(rows.every_reference())))
def test_every_reference_of_the_device_tests_is_not_vacuous(i):
    rows.reference(*rows.every_reference()[i])   # (asserts, for every parameter, max_a |d g_a / d theta| >= 1e-3 max_a S_a)


def test_the_condition_refuses_sums_that_cancel():
    """A parameter whose weighted sums cancel to 1e-6 of their magnitude sums in every row has nothing to compare at 1e-11 S."""
    grads = {"coef/0": np.array([1e-6, -1e-6], dtype=gr.LD)}
    mags = {"coef/0": np.array([1.0, 1.0], dtype=gr.LD)}
    with pytest.raises(AssertionError):
        rows.assert_not_vacuous(grads, mags, "cancelling weights")
    rows.assert_not_vacuous({"coef/0": np.array([0.1], dtype=gr.LD)}, {"coef/0": np.array([1.0], dtype=gr.LD)}, "live")
