"""What the Matern block of the seeded differential test (tests/test_fuzz_parity_gpu.py, seeds from MATERN_FIRST on) contains - on
the CPU, by calling the case generators only: a block that drew no inducing points, or a single smoothness, would pass on the device
and prove little."""
from collections import Counter

import numpy as np

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
