"""The host side of the periodogram initialisation of spectral-mixture layers - peak picking, the default grid, the constructor's
`spectral_period="auto"` and every refusal - and the numpy restatement of the generalised Lomb-Scargle periodogram (Zechmeister & Kuerster
2009) that tests/test_periodogram_gpu.py measures the device against.  Nothing here needs a GPU.

The restatement states the formula of include/gpar_hip.h twice: `gls(..., ld=False)` in float64 with numpy's sine and cosine of
2 pi f (t - t0), and `gls(..., ld=True)`, its twin in long double, whose argument 2 f (t - t0) is reduced to one period exactly before
pi enters.  Both take the float64 difference t - t0 as given: that rounding is the one loss the ABI allows.  The distance of the plain
restatement from its twin - what float64 itself loses on a case - is the yardstick of the device tolerance; on the cases of the GPU
parity test it is at most `FP64_OWN_ERROR_BOUND` (checked below)."""
import inspect
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
PI_LD = LD("3.14159265358979323846264338327950288")

#: the parity cases of tests/test_periodogram_gpu.py
PARITY_N = (3, 4, 63, 64, 65, 257)
PARITY_NF = (1, 2, 63, 64, 65, 300)
PARITY_P = (1, 3, 4, 5)   # 1, 3, and one value either side of the kernel's output chunk width (PG_CHUNK = 4; the width itself rides along)
#: the largest distance of the float64 restatement from its long-double twin the cases below may show (measured: see the test)
FP64_OWN_ERROR_BOUND = 1e-9


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------------
def gls(t, t0, y, omega, freq, ld=False):
    """power (p x F) by the formula of include/gpar_hip.h, degenerate cases as it defines them: with tiny = 16 n 2^-52, a column with
    fewer than 3 observed rows, YY <= tiny^2 mean^2 or D <= tiny gives 0.  (Three rows of which two share their time stamp - the
    smallest parity case - have D = 0 exactly: without the rule its rounding noise, 1e-17 of either sign, would be divided by.)"""
    T = LD if ld else np.float64
    t, y, omega, freq = (np.asarray(a, dtype=np.float64) for a in (t, y, omega, freq))
    tiny = 16.0 * t.size * 2.0 ** -52
    dt = t - t0   # float64, as the ABI forms it
    power = np.zeros((y.shape[1], freq.size), dtype=T)
    for j in range(y.shape[1]):
        obs = omega[:, j] > 0
        if obs.sum() < 3:
            continue
        w = omega[obs, j].astype(T)
        w = w / w.sum()
        yj = y[obs, j].astype(T)
        if ld:
            turns = np.fmod(T(2) * freq.astype(T)[:, None] * dt[obs].astype(T)[None, :], T(2))   # half periods, reduced exactly
            c, s = np.cos(PI_LD * turns), np.sin(PI_LD * turns)
        else:
            phi = 2.0 * np.pi * freq[:, None] * dt[obs][None, :]
            c, s = np.cos(phi), np.sin(phi)
        C, S, Y = c @ w, s @ w, w @ yj
        YY = w @ (yj * yj) - Y * Y
        YC, YS = c @ (w * yj) - Y * C, s @ (w * yj) - Y * S
        cc = (c * c) @ w
        CC, SS, CS = cc - C * C, (1 - cc) - S * S, (c * s) @ w - C * S
        D = CC * SS - CS * CS
        ok = (D > tiny) & (YY > 0) & (YY > tiny * tiny * Y * Y)
        num = SS * YC * YC + CC * YS * YS - 2 * CS * YC * YS
        power[j] = np.where(ok, num / np.where(ok, YY * D, 1), 0)
    return power


def parity_case(n, nf, p, seed=0):
    """(t, t0, y, omega, freq) of one parity case: random irregular time stamps, unsorted, one duplicated; two tones and noise per
    output; weights in [0.5, 1.5] with a few unobserved entries (never fewer than 3 observed rows); frequencies up to the average
    Nyquist rate."""
    rng = np.random.default_rng(1000 * n + 10 * nf + p + seed)
    t = rng.uniform(0.0, 10.0, n)
    t[n - 1] = t[0]   # a duplicated time stamp
    t = t[rng.permutation(n)]
    y = np.stack([np.sin(2 * np.pi * t / (0.7 + 0.3 * j)) + 0.5 * np.cos(2 * np.pi * t / 2.3 + j) + 0.3 * rng.standard_normal(n) + 0.2 * j
                  for j in range(p)], axis=1)
    omega = rng.uniform(0.5, 1.5, (n, p))
    if n >= 63:
        omega[rng.uniform(size=(n, p)) < 0.1] = 0.0
    span = t.max() - t.min()
    freq = np.sort(rng.uniform(0.2 / span, n / (2 * span), nf))
    return t, float(t.min()), y, omega, freq


def fp64_own_error(cases):
    """max |float64 restatement - long-double twin| over the cases."""
    worst = 0.0
    for case in cases:
        worst = max(worst, float(np.max(np.abs(gls(*case).astype(LD) - gls(*case, ld=True)))))
    return worst


def parity_cases():
    return [parity_case(n, nf, p) for n in PARITY_N for nf in PARITY_NF for p in PARITY_P]


def test_restatement_loses_little_against_its_long_double_twin():
    """What float64 itself loses on the GPU parity cases.  Measured: 2.6e-10 over all of them - the cases with 4 rows, three distinct
    instants and a small D, carry it; from 63 rows on it is 3.2e-15 (DESIGN 3.22 has it per n)."""
    worst = fp64_own_error(parity_cases())
    large = fp64_own_error([parity_case(n, nf, p) for n in PARITY_N if n >= 63 for nf in PARITY_NF for p in PARITY_P])
    print(f"float64 restatement against its long-double twin: {worst:.3e} over all parity cases, {large:.3e} from 63 rows on")
    assert 0 < worst <= FP64_OWN_ERROR_BOUND


def test_restatement_agrees_with_scipy():
    from scipy.signal import lombscargle

    if "floating_mean" not in inspect.signature(lombscargle).parameters:
        pytest.skip("scipy.signal.lombscargle has no floating_mean argument here")
    for n, nf, p in ((65, 64, 3), (257, 300, 1)):
        t, t0, y, omega, freq = parity_case(n, nf, p)
        ours = gls(t, t0, y, omega, freq)
        for j in range(p):
            obs = omega[:, j] > 0
            theirs = lombscargle(t[obs] - t0, y[obs, j], 2 * np.pi * freq, normalize=True, weights=omega[obs, j], floating_mean=True)
            assert np.allclose(ours[j], theirs, rtol=1e-9, atol=1e-12)


def test_power_is_one_for_a_pure_tone_and_invariant_under_affine_maps():
    t = np.sort(np.random.default_rng(5).uniform(0, 10, 40))
    y = (2.0 + 3.0 * np.sin(2 * np.pi * 0.8 * t + 0.3))[:, None]
    ones = np.ones_like(y)
    assert abs(gls(t, t[0], y, ones, np.array([0.8]))[0, 0] - 1) < 1e-12
    freq = np.linspace(0.1, 2.0, 50)
    assert np.allclose(gls(t, t[0], y, ones, freq), gls(t, t[0], 3 * y - 7, ones, freq), atol=1e-12)


# ---- peak picking --------------------------------------------------------------------------------------------------------------------
def _bumps(freq, lines):
    power = np.zeros_like(freq)
    for f0, height, width in lines:
        power = np.maximum(power, height * np.exp(-0.5 * ((freq - f0) / width) ** 2))
    return power


def test_two_separated_lines_strongest_first():
    from gpar_amd import spectral_peaks

    freq = np.arange(1, 201) * 0.02
    power = _bumps(freq, [(1.0, 0.5, 0.03), (2.7, 0.8, 0.03)])
    assert np.allclose(spectral_peaks(freq, power, 2, span=10.0), [2.7, 1.0])
    assert np.allclose(spectral_peaks(freq, power, 1, span=10.0), [2.7])


def test_two_maxima_within_the_rayleigh_resolution_are_one_pick():
    from gpar_amd import spectral_peaks

    freq = np.arange(1, 201) * 0.02
    power = _bumps(freq, [(1.0, 0.8, 0.015), (1.08, 0.7, 0.015), (3.0, 0.3, 0.03)])   # 0.08 apart, 1 / span = 0.1
    assert power[49] > power[51] < power[53]   # two maxima indeed
    assert np.allclose(spectral_peaks(freq, power, 2, span=10.0), [1.0, 3.0])
    # ... and with a longer span the same two are two lines
    assert np.allclose(spectral_peaks(freq, power, 2, span=20.0), [1.0, 1.08])


def test_a_peak_at_a_grid_end_counts():
    from gpar_amd import spectral_peaks

    freq = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6])
    assert np.allclose(spectral_peaks(freq, np.array([0.1, 0.2, 0.5, 0.2, 0.3, 0.9]), 2, span=20.0), [0.6, 0.3])
    assert np.allclose(spectral_peaks(freq, np.array([0.9, 0.2, 0.5, 0.2, 0.1, 0.05]), 2, span=20.0), [0.1, 0.3])
    # an end point that merely equals its neighbour is no peak
    assert np.allclose(spectral_peaks(freq, np.array([0.5, 0.5, 0.1, 0.3, 0.1, 0.1]), 2, span=20.0), [0.4, 0.8])


def test_fewer_peaks_than_components_are_filled_with_harmonics():
    from gpar_amd import spectral_peaks

    freq = np.arange(1, 101) * 0.05
    power = _bumps(freq, [(0.5, 0.9, 0.05)])
    assert np.allclose(spectral_peaks(freq, power, 4, span=10.0), [0.5, 1.0, 1.5, 2.0])
    two = _bumps(freq, [(0.5, 0.9, 0.05), (3.2, 0.4, 0.05)])
    assert np.allclose(spectral_peaks(freq, two, 4, span=10.0), [0.5, 3.2, 1.0, 1.5])
    with pytest.raises(ValueError, match="no peak"):
        spectral_peaks(freq, np.zeros_like(freq), 2, span=10.0)
    with pytest.raises(ValueError, match="no peak"):
        spectral_peaks(freq, np.full_like(freq, 0.3), 2, span=10.0)


def test_ties_go_to_the_lowest_frequency():
    """Documented in `spectral_peaks`: of equal maxima the lowest frequency is taken first, and a plateau is its lowest frequency."""
    from gpar_amd import spectral_peaks

    freq = np.arange(1, 11) * 0.5
    power = np.array([0.1, 0.7, 0.1, 0.1, 0.7, 0.1, 0.1, 0.7, 0.7, 0.1])
    assert np.allclose(spectral_peaks(freq, power, 3, span=10.0), [1.0, 2.5, 4.0])
    assert np.array_equal(spectral_peaks(freq, power, 3, span=10.0), spectral_peaks(freq, power, 3, span=10.0))


def test_peak_picking_refuses_malformed_input():
    from gpar_amd import spectral_peaks

    for args in ((np.array([1.0, 2.0]), np.array([1.0]), 1, 1.0), (np.array([2.0, 1.0]), np.array([0.1, 0.2]), 1, 1.0),
                 (np.array([1.0, 2.0]), np.array([0.1, 0.2]), 0, 1.0), (np.array([1.0, 2.0]), np.array([0.1, 0.2]), 1, 0.0)):
        with pytest.raises(ValueError):
            spectral_peaks(*args)


# ---- the default grid ----------------------------------------------------------------------------------------------------------------
def test_default_grid_against_hand_values():
    from gpar_amd.spectrum import periodogram_grid

    # span 10, 100 observed rows, 5 points per resolution: step 1 / 50, up to 100 / 20 = 5, so 250 frequencies
    grid = periodogram_grid(10.0, 100)
    assert grid.size == 250 and np.isclose(grid[0], 0.02) and np.isclose(grid[-1], 5.0) and np.allclose(np.diff(grid), 0.02)
    # twice the Nyquist factor doubles the top, the step stays; oversample moves the step, the top stays
    assert periodogram_grid(10.0, 100, nyquist=2.0).size == 500 and np.isclose(periodogram_grid(10.0, 100, nyquist=2.0)[-1], 10.0)
    coarse = periodogram_grid(10.0, 100, oversample=2)
    assert coarse.size == 100 and np.isclose(coarse[0], 0.05) and np.isclose(coarse[-1], 5.0)
    # an odd count rounds down; there is always one frequency
    assert periodogram_grid(4.0, 7, oversample=1).size == 3 and np.isclose(periodogram_grid(4.0, 7, oversample=1)[-1], 0.75)
    assert periodogram_grid(4.0, 1, oversample=1).size == 1
    for bad in ((0.0, 10), (-1.0, 10), (np.inf, 10)):
        with pytest.raises(ValueError, match="span"):
            periodogram_grid(*bad)
    with pytest.raises(ValueError):
        periodogram_grid(1.0, 10, oversample=0)


def test_inputs_mark_missing_values_and_refuse_what_has_no_periodogram():
    from gpar_amd.spectrum import periodogram_inputs

    x = np.array([3.0, 1.0, 2.0, 5.0])
    y = np.array([[1.0, np.nan], [2.0, 1.0], [np.nan, 0.5], [0.0, 2.0]])
    t, yy, omega = periodogram_inputs(x[:, None], y, 2 * np.ones_like(y))
    assert np.array_equal(t, x) and np.array_equal(omega, [[2, 0], [2, 2], [0, 2], [2, 2]]) and yy[0, 1] == 0 and yy[2, 0] == 0
    assert np.array_equal(periodogram_inputs(x, y[:, 1])[2][:, 0], [0, 1, 1, 1])
    with pytest.raises(ValueError, match="one input column"):
        periodogram_inputs(np.ones((4, 2)), y)
    with pytest.raises(ValueError, match="at least 3 rows"):
        periodogram_inputs(x[:2], y[:2])
    with pytest.raises(ValueError):
        periodogram_inputs(x, y, np.ones((4, 3)))
    with pytest.raises(ValueError):
        periodogram_inputs(x, y, -np.ones_like(y))


# ---- the constructor, the refusals, unchanged behaviour --------------------------------------------------------------------------------
def _series(n=40, p=2, seed=0):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0, 10, n))[:, None]
    y = np.stack([np.sin(2 * np.pi * x[:, 0] / (0.9 + j)) + 0.1 * rng.standard_normal(n) for j in range(p)], axis=1)
    return x, y


def test_constructor_accepts_auto_and_refuses_other_strings():
    from gpar_amd import GPARRegressor

    reg = GPARRegressor(spectral=2, spectral_period="auto")
    assert reg.model_config["spectral_period"] == "auto" and reg.spectral == 2
    with pytest.raises(ValueError, match="auto"):
        GPARRegressor(spectral=2, spectral_period="periodogram")
    with pytest.raises(ValueError, match="spectral=Q"):
        GPARRegressor(spectral_period="auto")


def test_auto_refuses_what_it_cannot_serve(oracle_engine):
    from gpar_amd import GPARRegressor
    from gpar_amd.parallel import sharded_condition, sharded_fit, sharded_sample

    x, y = _series()
    reg = GPARRegressor(spectral=2, spectral_period="auto")
    with pytest.raises(RuntimeError, match="fit, condition or init_spectral"):
        reg.sample(np.linspace(0, 1, 5)[:, None], p=1)   # no data yet: nothing to pick the periods from
    with pytest.raises(ValueError, match="one input column"):
        reg.fit(np.concatenate([x, x ** 2], axis=1), y, iters=1)
    with pytest.raises(ValueError, match="one input column"):
        reg.periodogram(np.concatenate([x, x ** 2], axis=1), y)
    with pytest.raises(ValueError, match="greedy_order"):
        reg.greedy_order(x, y, iters=1)
    with pytest.raises(ValueError, match="sharded"):
        sharded_fit(reg, x, y, iters=1)
    with pytest.raises(ValueError, match="sharded"):
        sharded_condition(reg)
    with pytest.raises(ValueError, match="sharded"):
        sharded_sample(reg, x, num_samples=2)
    with pytest.raises(ValueError, match="span"):
        reg.periodogram(np.ones(5), np.arange(5.0))
    with pytest.raises(ValueError, match="span"):
        reg.periodogram(np.ones(5), np.arange(5.0), freq=[1.0])
    with pytest.raises(ValueError, match="at least 3 rows"):
        reg.periodogram(np.arange(2.0), np.arange(2.0))
    with pytest.raises(ValueError, match="positive"):
        reg.periodogram(x, y, freq=[0.0, 1.0])
    with pytest.raises(ValueError, match="spectral=Q"):
        GPARRegressor().init_spectral(x, y)


def test_auto_needs_the_device_engine(oracle_engine):
    """The oracle engine has no periodogram and the host has no fallback: NotImplementedError, from every door."""
    from gpar_amd import GPARRegressor

    x, y = _series()
    reg = GPARRegressor(spectral=2, spectral_period="auto")
    for call in (lambda: reg.fit(x, y, iters=1), lambda: reg.condition(x, y), lambda: reg.init_spectral(x, y), lambda: reg.periodogram(x, y)):
        with pytest.raises(NotImplementedError, match="periodogram"):
            call()
    assert reg.vs.names == [] and reg._spectral_auto is None


@pytest.mark.parametrize("period", [1.0, 0.7, (0.5, 0.19)])
def test_float_periods_create_the_variables_they_always_did(oracle_engine, period):
    """With a number or Q numbers nothing moves: the names in their order, the bounds and the initial values are those of the harmonic
    ladder T / (q + 1) (or the given vector), written out here by hand."""
    from gpar_amd import GPARRegressor

    x, y = _series()
    reg = GPARRegressor(spectral=2, spectral_period=period, spectral_scale=3.0, scale=0.7, noise=0.05)
    reg.condition(x, y)
    float(reg.logpdf(x, y))
    expected = [period[q] if isinstance(period, tuple) else period / (q + 1) for q in range(2)]
    names = []
    for i in range(2):
        names += [f"{i}/input/var", f"{i}/input/scales"]
        for q in range(2):
            names += [f"{i}/input/sm{q}/var", f"{i}/input/sm{q}/scales", f"{i}/input/sm{q}/pers"]
        if i:
            names += [f"{i}/output/lin/scales"]
        names += [f"{i}/noise"]
    assert reg.vs.names == names
    values = reg.get_variables()
    for i in range(2):
        for q in range(2):
            assert np.allclose(values[f"{i}/input/sm{q}/pers"], [expected[q]], rtol=1e-14, atol=0)
            assert np.allclose(values[f"{i}/input/sm{q}/var"], 0.5, rtol=1e-14) and np.allclose(values[f"{i}/input/sm{q}/scales"], [3.0], rtol=1e-14)
            var = reg.vs._vars[f"{i}/input/sm{q}/pers"]
            assert (var.lower, var.upper) == (1e-4, 1e4)
    assert reg._spectral_auto is None


def test_picked_periods_stand_where_given_ones_would(oracle_engine):
    """The host logic of "auto" without the device: once periods are picked (here: put in place by hand, as `init_spectral` leaves them)
    the model is the one `spectral_period=(T0, T1)` per layer builds - same names, same order, same values -, existing variables are
    kept, and a second `condition` keeps the picks."""
    from gpar_amd import GPARRegressor

    x, y = _series()
    picked = np.array([[0.9, 0.31], [1.9, 0.47]])
    auto = GPARRegressor(spectral=2, spectral_period="auto", noise=0.05)
    auto._spectral_auto = picked.copy()
    auto.vs.bnd(name="1/input/sm1/pers", init=np.array([0.123]))   # a value the user assigned before the first fit
    auto.condition(x, y)
    got = float(auto.logpdf(x, y))
    assert np.array_equal(auto._spectral_auto, picked)
    values = auto.get_variables()
    assert np.allclose(values["0/input/sm0/pers"], 0.9) and np.allclose(values["0/input/sm1/pers"], 0.31)
    assert np.allclose(values["1/input/sm0/pers"], 1.9) and np.allclose(values["1/input/sm1/pers"], 0.123)
    # layer by layer the same numbers as a model given the periods
    fixed = GPARRegressor(spectral=2, spectral_period=(0.9, 0.31), noise=0.05)
    fixed.vs.bnd(name="1/input/sm0/pers", init=np.array([1.9]))
    fixed.vs.bnd(name="1/input/sm1/pers", init=np.array([0.123]))
    fixed.condition(x, y)
    assert np.isclose(got, float(fixed.logpdf(x, y)), rtol=1e-12)
    assert sorted(auto.vs.names) == sorted(fixed.vs.names)


# ---- the new translation unit compiles for gfx950 --------------------------------------------------------------------------------------
def test_periodogram_kernel_compiles_for_gfx950():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")   # the compiler build() uses
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "periodogram_tu.hip")
        with open(src, "w") as f:
            f.write('#include "periodogram.h"\n')
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "gpar_amd", "csrc"), "-c", "--cuda-device-only",
               "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(tmp, "periodogram_tu.o")]
        done = subprocess.run(cmd, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr[-2000:]
        usage = done.stderr
    assert "periodogram_kernel" in usage
    scratch = [int(line.split(":")[-1].split("[")[0]) for line in usage.splitlines() if "ScratchSize" in line]
    assert scratch and max(scratch) == 0, "the periodogram kernel spills to scratch"


if __name__ == "__main__":
    sys.exit(pytest.main([__file__, "-q"]))
