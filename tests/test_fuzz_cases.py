"""What the Matern block (seeds from MATERN_FIRST on) and the spectral block (seeds from SPECTRAL_FIRST on) of the seeded
differential test (tests/test_fuzz_parity_gpu.py) contain - on the CPU, by calling the case generators only: a block that drew no
inducing points, or a single smoothness, would pass on the device and prove little.  The spectral block's cases are also run on the
numpy engine and the stand-alone restatement here, so that the reference is known to hold before the device is compared with it."""
from collections import Counter

import numpy as np
import pytest

from . import test_fuzz_parity_gpu as fuzz


def _census(seeds, case):
    nus, methods, missing, periodic = Counter(), Counter(), 0, 0
    for seed in seeds:
        kw, x, y = case(seed)[:3]
        assert kw["matern"] in (0.5, 1.5, 2.5) and kw["rq"] is False, seed
        nus[kw["matern"]] += 1
        if "x_ind" in kw:
            methods[kw.get("sparse_method", "vfe")] += 1
        missing += bool(np.isnan(y).any())
        periodic += bool(kw["per"])
    return nus, methods, missing, periodic


def test_matern_block_of_the_fuzz_cases():
    assert len(set(fuzz.MATERN_SEEDS)) >= 36 and min(fuzz.MATERN_SEEDS) >= fuzz.MATERN_FIRST
    nus, methods, missing, periodic = _census(fuzz.MATERN_SEEDS, fuzz._case)
    assert all(nus[nu] >= 10 for nu in (0.5, 1.5, 2.5)), nus
    assert sum(methods.values()) >= 8 and all(methods[k] >= 1 for k in ("vfe", "fitc", "dtc")), methods
    assert missing >= 8 and periodic >= 6, (missing, periodic)


def test_matern_block_of_the_gradient_and_blocked_size_cases():
    assert len(set(fuzz.MATERN_GRADIENT_SEEDS)) >= 12 and min(fuzz.MATERN_GRADIENT_SEEDS) >= fuzz.MATERN_FIRST
    nus, _, _, _ = _census(fuzz.MATERN_GRADIENT_SEEDS, fuzz._case)
    assert all(nus[nu] >= 3 for nu in (0.5, 1.5, 2.5)), nus
    assert len(set(fuzz.MATERN_MID_SEEDS)) >= 6 and min(fuzz.MATERN_MID_SEEDS) >= fuzz.MATERN_FIRST
    nus, _, _, _ = _census(fuzz.MATERN_MID_SEEDS, fuzz._mid_case)
    assert all(nus[nu] >= 1 for nu in (0.5, 1.5, 2.5)), nus


def test_seeds_below_the_matern_block_keep_their_cases():
    """The earlier seeds (the first fuzz ids, the gradient test's 200 .., the extended sweep's 500 ..) draw no `matern`, and a seed
    of the block draws everything else exactly as the generator without the block would: the same stream, only rq forced off."""
    for seed in list(range(96)) + list(range(200, 232)) + [507, 516]:
        assert "matern" not in fuzz._case(seed)[0]
    for seed in range(20):
        assert "matern" not in fuzz._mid_case(seed)[0]
    first = fuzz.MATERN_FIRST
    try:
        kw, x, y, w, xs = fuzz._case(first + 1)
        fuzz.MATERN_FIRST = first + 10 ** 6
        kw0, x0, y0, w0, xs0 = fuzz._case(first + 1)
    finally:
        fuzz.MATERN_FIRST = first
    assert "matern" not in kw0 and {k: v for k, v in kw.items() if k not in ("matern", "rq", "x_ind")} == {
        k: v for k, v in kw0.items() if k not in ("rq", "x_ind")}
    np.testing.assert_array_equal(x, x0)
    np.testing.assert_array_equal(y, y0)
    np.testing.assert_array_equal(xs, xs0)


# ---- the spectral block (seeds from SPECTRAL_FIRST on) -------------------------------------------------------------------------

def _feature_dims(kw, m, p):
    """Feature dims of the widest layer of a drawn case (above 16 the Gram of a structure with a cosine stays on the interpreter)."""
    from gpar_amd.regression import _layer_kernel_size

    config = dict(markov=kw["markov"], spectral=kw["spectral"], per=kw["per"], input_linear=kw.get("input_linear", False),
                  linear=kw["linear"], nonlinear=kw["nonlinear"])
    terms, _, dims = _layer_kernel_size(config, m, p)
    assert terms <= 8, kw   # Q <= 2 always fits GPAR_MAX_TERMS: no case may raise the size error
    return dims


def _spectral_census(seeds, case):
    out = Counter()
    for seed in seeds:
        kw, x, y = case(seed)[:3]
        assert kw["spectral"] in (1, 2) and not (kw["rq"] and "matern" in kw), seed
        assert np.size(kw["spectral_period"]) in (1, kw["spectral"]), seed
        out[f"Q{kw['spectral']}"] += 1
        if "x_ind" in kw:
            out["inducing"] += 1
            out[kw.get("sparse_method", "vfe")] += 1
        out["missing"] += bool(np.isnan(y).any())
        out["per"] += bool(kw["per"])
        out["matern"] += "matern" in kw
        out["rq"] += bool(kw["rq"])
        out["wide" if _feature_dims(kw, x.shape[1], y.shape[1]) > 16 else "narrow"] += 1
        out["short-envelope"] += "spectral_scale" in kw
        out["period-vector"] += np.size(kw["spectral_period"]) == 2
    return out


def test_spectral_block_of_the_fuzz_cases():
    """No seed of the block is skipped or filtered out: the parametrisation of the device test holds every one of them."""
    assert len(set(fuzz.SPECTRAL_SEEDS)) >= 36 and min(fuzz.SPECTRAL_SEEDS) >= fuzz.SPECTRAL_FIRST
    census = _spectral_census(fuzz.SPECTRAL_SEEDS, fuzz._case)
    assert census["Q1"] >= 12 and census["Q2"] >= 12, census
    assert census["inducing"] >= 6 and all(census[k] >= 1 for k in ("vfe", "fitc", "dtc")), census
    assert census["missing"] >= 8 and census["per"] >= 4, census
    assert census["wide"] >= 4 and census["narrow"] >= 4, census
    assert census["matern"] >= 4 and census["rq"] >= 2, census
    assert census["short-envelope"] >= 8 and census["period-vector"] >= 2, census
    marks = {m.name: m for m in fuzz.test_random_configuration.pytestmark}
    ids = list(marks["parametrize"].args[1])
    assert all(s in ids for s in fuzz.SPECTRAL_SEEDS) and [-s - 1 for s in fuzz.SPECTRAL_SEEDS[:8]] == [i for i in ids if i <= -fuzz.SPECTRAL_FIRST - 1]


def test_spectral_block_of_the_gradient_and_blocked_size_cases():
    assert len(set(fuzz.SPECTRAL_GRADIENT_SEEDS)) >= 12 and min(fuzz.SPECTRAL_GRADIENT_SEEDS) >= fuzz.SPECTRAL_FIRST
    census = _spectral_census(fuzz.SPECTRAL_GRADIENT_SEEDS, fuzz._case)
    assert census["Q1"] >= 4 and census["Q2"] >= 4 and census["inducing"] >= 2 and census["missing"] >= 3, census
    assert len(set(fuzz.SPECTRAL_MID_SEEDS)) >= 6 and min(fuzz.SPECTRAL_MID_SEEDS) >= fuzz.SPECTRAL_FIRST
    census = _spectral_census(fuzz.SPECTRAL_MID_SEEDS, lambda seed: fuzz._mid_case(seed)[:3])
    assert census["Q1"] >= 2 and census["Q2"] >= 2, census


def test_seeds_below_the_spectral_block_keep_their_cases():
    """Every earlier seed - the Matern block included - draws no `spectral` and keeps its Matern smoothness; a seed of the spectral
    block draws everything else exactly as the generator without the block would."""
    for seed in list(range(96)) + list(range(200, 232)) + [507, 516] + fuzz.MATERN_SEEDS + fuzz.MATERN_GRADIENT_SEEDS:
        kw = fuzz._case(seed)[0]
        assert not any(k.startswith("spectral") for k in kw), seed
        assert kw.get("matern") == (None if seed < fuzz.MATERN_FIRST else [0.5, 1.5, 2.5][(seed - fuzz.MATERN_FIRST) % 3]), seed
    for seed in list(range(20)) + fuzz.MATERN_MID_SEEDS:
        assert not any(k.startswith("spectral") for k in fuzz._mid_case(seed)[0]), seed
    first = fuzz.SPECTRAL_FIRST
    for seed in (first + 1, first + 3, first + 7):
        try:
            kw, x, y, w, xs = fuzz._case(seed)
            fuzz.SPECTRAL_FIRST = first + 10 ** 6
            kw0, x0, y0, w0, xs0 = fuzz._case(seed)
        finally:
            fuzz.SPECTRAL_FIRST = first
        added = ("spectral", "spectral_period", "spectral_scale", "matern", "rq", "x_ind")
        assert "spectral" not in kw0 and {k: v for k, v in kw.items() if k not in added} == {k: v for k, v in kw0.items() if k not in added}
        np.testing.assert_array_equal(x, x0)
        np.testing.assert_array_equal(y, y0)
        np.testing.assert_array_equal(xs, xs0)


@pytest.mark.parametrize("seed", fuzz.SPECTRAL_SEEDS)
def test_spectral_seed_runs_on_the_reference_alone(seed):
    """Before the device is asked: every seed of the block through the product's host algebra on the numpy engine and through the
    stand-alone restatement (its approximation is VFE: the other two run on the engine only).  Neither may meet a matrix that is not
    positive definite, and the two agree to the tolerance of the differential test."""
    from oracle import gpar_ref

    kw, x, y, w, xs = fuzz._case(seed)
    prior, post, sample, hypers, config = fuzz._run("oracle", kw, x, y, w, xs)   # (OracleNotPositiveDefinite would propagate)
    assert np.isfinite(prior) and np.isfinite(post) and np.all(np.isfinite(sample))
    assert config["spectral"] == kw["spectral"] and config.get("matern") == kw.get("matern")
    if kw.get("sparse_method", "vfe") == "vfe":
        want = gpar_ref.gpar_logpdf(x, y, w, hypers, config, impute=kw["impute"], replace=kw["replace"], x_ind=kw.get("x_ind"))
        tol = 1e-6 if "x_ind" in kw else 1e-9
        assert abs(prior - want) <= tol * max(abs(want), 1.0), (kw, prior, want)
