"""gpar_periodogram through the C ABI on the MI355X, and what it is for: `GPARRegressor(spectral=Q, spectral_period="auto")`.

The reference is the long-double twin of the numpy restatement in tests/test_periodogram.py.  The device sums in another order and has
another sincospi than numpy: the tolerance of a case with n rows is 8 x the largest distance of the plain float64 restatement from the
twin over the parity cases with that n - what float64 itself loses there -, and never below 8 n 2^-52.  Both are computed here."""
import numpy as np
import pytest
import torch

from .conftest import make_engine
from .test_periodogram import LD, PARITY_N, PARITY_NF, PARITY_P, fp64_own_error, gls, parity_case

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
ARG_ERROR = -1000


@pytest.fixture(scope="module")
def eng():
    from gpar_amd.engine import set_engine

    e = make_engine("hip")
    previous = set_engine(e)
    yield e
    set_engine(previous)


def _padded(a, pad, device):
    """A device matrix whose rows are `pad` doubles longer than `a`'s, the padding (and nothing else) holding the sentinel; (buffer, view)."""
    a = np.atleast_2d(np.asarray(a, dtype=np.float64))
    buf = torch.full((a.shape[0], a.shape[1] + pad), SENTINEL, dtype=torch.float64, device=device)
    buf[:, : a.shape[1]] = torch.as_tensor(a, device=device)
    return buf, buf[:, : a.shape[1]]


def periodogram_abi(eng, t, t0, y, omega, freq, pads=(3, 2, 5)):
    """power (p x F) from one gpar_periodogram call with padded ldy, ldo and ldp; the padding must come back as it went in."""
    from gpar_amd import _lib
    from gpar_amd.hip import stream_ptr

    lib = _lib.load()
    dev = eng.device
    n, p, nf = int(np.shape(y)[0]), int(np.shape(y)[1]), int(np.size(freq))
    ybuf, _ = _padded(y, pads[0], dev)
    obuf, _ = _padded(omega, pads[1], dev)
    pbuf = torch.full((p, nf + pads[2]), SENTINEL, dtype=torch.float64, device=dev)
    tt, ff = torch.as_tensor(np.asarray(t, dtype=np.float64), device=dev), torch.as_tensor(np.asarray(freq, dtype=np.float64), device=dev)
    rc = lib.gpar_periodogram(tt.data_ptr(), n, float(t0), ybuf.data_ptr(), p + pads[0], obuf.data_ptr(), p + pads[1], p, ff.data_ptr(), nf,
                              pbuf.data_ptr(), nf + pads[2], stream_ptr(dev))
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = pbuf.cpu().numpy()
    assert np.all(out[:, nf:] == SENTINEL) and np.all(ybuf[:, p:].cpu().numpy() == SENTINEL) and np.all(obuf[:, p:].cpu().numpy() == SENTINEL)
    return out[:, :nf].copy()


@pytest.fixture(scope="module")
def tolerance():
    """n -> 8 x the float64 restatement's own largest error over the parity cases with n rows, at least 8 n 2^-52."""
    own = {n: fp64_own_error([parity_case(n, nf, p) for nf in PARITY_NF for p in PARITY_P]) for n in PARITY_N}
    tol = {n: max(8.0 * own[n], 8.0 * n * 2.0 ** -52) for n in PARITY_N}
    print("float64 restatement's own error per n:", {n: f"{v:.2e}" for n, v in own.items()}, "tolerance:", {n: f"{v:.2e}" for n, v in tol.items()})
    return tol


@pytest.mark.parametrize("n", PARITY_N)
def test_parity_with_the_long_double_twin(eng, tolerance, n):
    """Measured on an MI355X, largest distance from the twin / tolerance: n = 3: 0 / 5.3e-15 (a duplicated time stamp leaves two instants,
    D = 0: zero on both sides), 4: 2.6e-10 / 2.1e-9, 63: 3.0e-15 / 1.1e-13, 64: 5.9e-15 / 1.1e-13, 65: 2.6e-15 / 1.2e-13, 257: 1.4e-15 /
    4.6e-13."""
    worst = 0.0
    for nf in PARITY_NF:
        for p in PARITY_P:
            case = parity_case(n, nf, p)
            got = periodogram_abi(eng, *case)
            want = gls(*case, ld=True)
            assert np.all(np.isfinite(got)) and got.min() >= 0.0 and got.max() <= 1.0
            err = float(np.max(np.abs(got.astype(LD) - want)))
            worst = max(worst, err)
            assert err <= tolerance[n], (n, nf, p, err, tolerance[n])
    print(f"n = {n}: device against the long-double twin {worst:.3e}, tolerance {tolerance[n]:.3e}")


def test_unobserved_short_and_constant_columns_are_exactly_zero_and_disturb_nothing(eng):
    t, t0, y, omega, freq = parity_case(65, 300, 3)
    alone = periodogram_abi(eng, t, t0, y, omega, freq)
    n = t.size
    # columns 1, 3, 5 of six: every entry unobserved (with wild values where nothing is observed), 2 observed rows, constant
    y6, o6 = np.zeros((n, 6)), np.zeros((n, 6))
    y6[:, [0, 2, 4]], o6[:, [0, 2, 4]] = y, omega
    y6[:, 1], o6[:, 1] = 1e300 * np.sin(t), 0.0
    y6[:, 3], o6[:, 3] = np.cos(t), 0.0
    o6[[5, 40], 3] = 1.0
    y6[:, 5], o6[:, 5] = 0.1, 1.0
    got = periodogram_abi(eng, t, t0, y6, o6, freq)
    for col in (1, 3, 5):
        assert np.all(got[col] == 0.0) and not np.any(np.signbit(got[col]))
    assert np.array_equal(got[[0, 2, 4]], alone)
    # a constant column is zero whatever the constant and the weights
    yc = np.stack([np.full(n, 1e6 / 3.0), np.full(n, -7.7e-5), np.zeros(n)], axis=1)
    assert np.all(periodogram_abi(eng, t, t0, yc, np.abs(omega) + 0.1, freq) == 0.0)
    # frequencies that are none: zero as well, their neighbours untouched
    odd = freq.copy()
    odd[[3, 70]] = [0.0, -1.0]
    got = periodogram_abi(eng, t, t0, y, omega, odd)
    assert np.all(got[:, [3, 70]] == 0.0)
    keep = np.setdiff1d(np.arange(300), [3, 70])
    assert np.array_equal(got[:, keep], alone[:, keep])


def test_large_offsets_keep_the_phase(eng, tolerance):
    """t = 1e6 + t' with periods from 0.05 and t0 = min t: the differences t - t0 are t' - min t' up to their rounding (2^-33 here; the
    time stamps below are multiples of 2^-20, so the differences are exact), and the result is the one on t'.  A kernel that took the sine of
    2 pi f t would be off by 1e6 / 0.05 periods x 2^-52 ~ 3e-8 in phase."""
    rng = np.random.default_rng(11)
    n = 257
    tp = np.round(np.cumsum(rng.uniform(0.005, 0.06, n)) * 2.0 ** 20) / 2.0 ** 20
    tp = tp[rng.permutation(n)]
    y = np.stack([np.sin(2 * np.pi * tp / 0.05) + 0.5 * np.sin(2 * np.pi * tp / 0.37) + 0.2 * rng.standard_normal(n),
                  np.cos(2 * np.pi * tp / 0.113) + 0.2 * rng.standard_normal(n)], axis=1)
    omega = rng.uniform(0.5, 1.5, (n, 2))
    freq = np.sort(np.concatenate([rng.uniform(0.1, 20.0, 297), [1 / 0.05, 1 / 0.113, 1 / 0.37]]))
    far = 1e6 + tp
    assert np.array_equal(far - far.min(), tp - tp.min())
    near = periodogram_abi(eng, tp, tp.min(), y, omega, freq)
    got = periodogram_abi(eng, far, far.min(), y, omega, freq)
    assert np.max(np.abs(got - near)) <= tolerance[257]
    assert np.max(np.abs(got.astype(LD) - gls(far, far.min(), y, omega, freq, ld=True))) <= tolerance[257]
    assert got[0, np.searchsorted(freq, 1 / 0.05)] > 0.5   # (the line is there)


def test_bits(eng, tolerance):
    t, t0, y, omega, freq = parity_case(257, 300, 5)
    first = periodogram_abi(eng, t, t0, y, omega, freq)
    assert np.array_equal(first, periodogram_abi(eng, t, t0, y, omega, freq))   # two calls
    for k in (0, 63, 64, 150, 299):   # a frequency alone, and inside a grid of 300
        assert np.array_equal(periodogram_abi(eng, t, t0, y, omega, freq[k : k + 1])[:, 0], first[:, k])
    assert np.array_equal(periodogram_abi(eng, t, t0, y, omega, freq[100:170]), first[:, 100:170])
    # a permutation of the rows changes the order of the sums: equal to tolerance, not in bits
    perm = np.random.default_rng(2).permutation(t.size)
    assert np.max(np.abs(periodogram_abi(eng, t[perm], t0, y[perm], omega[perm], freq) - first)) <= tolerance[257]


def test_affine_maps_of_y_leave_the_power(eng, tolerance):
    t, t0, y, omega, freq = parity_case(257, 300, 3)
    assert np.max(np.abs(periodogram_abi(eng, t, t0, 3 * y - 7, omega, freq) - periodogram_abi(eng, t, t0, y, omega, freq))) <= tolerance[257]


def test_argument_errors_return_before_any_launch(eng):
    from gpar_amd import _lib
    from gpar_amd.hip import stream_ptr

    lib = _lib.load()
    dev = eng.device
    n, p, nf = 20, 2, 7
    t = torch.linspace(0, 1, n, dtype=torch.float64, device=dev)
    y = torch.randn(n, p, dtype=torch.float64, device=dev)
    om = torch.ones(n, p, dtype=torch.float64, device=dev)
    fr = torch.linspace(1, 5, nf, dtype=torch.float64, device=dev)
    out = torch.full((p, nf), SENTINEL, dtype=torch.float64, device=dev)

    def call(n=n, t0=0.0, ldy=p, ldo=p, p=p, nf=nf, ldp=nf, t_ptr=t.data_ptr(), out_ptr=out.data_ptr()):
        return lib.gpar_periodogram(t_ptr, n, t0, y.data_ptr(), ldy, om.data_ptr(), ldo, p, fr.data_ptr(), nf, out_ptr, ldp, stream_ptr(dev))

    for kw in (dict(n=-1), dict(nf=-1), dict(p=0), dict(p=-2), dict(ldy=p - 1), dict(ldo=p - 1), dict(ldp=nf - 1), dict(t0=float("nan")),
               dict(t0=float("inf")), dict(t_ptr=None), dict(out_ptr=None)):
        assert call(**kw) <= ARG_ERROR, kw
    # no rows or no frequencies: nothing to do, and nothing done
    assert call(n=0) == 0 and call(nf=0) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(((out >= 0) & (out <= 1)).all())


def test_engine_and_regressor_calls_agree_with_the_abi(eng):
    from gpar_amd import GPARRegressor

    t, t0, y, omega, freq = parity_case(65, 64, 3)
    want = periodogram_abi(eng, t, t0, y, omega, freq)
    assert np.array_equal(eng.periodogram(t, y, omega, freq).cpu().numpy(), want)
    y_nan = np.where(omega > 0, y, np.nan)
    reg = GPARRegressor(transform_y=(lambda v: 2 * v + 1, lambda v: (v - 1) / 2))
    pg = reg.periodogram(t[:, None], y_nan, w=np.where(omega > 0, omega, 1.0), freq=freq)
    assert np.array_equal(pg.freq, freq) and np.max(np.abs(pg.power - want)) <= 1e-12
    # the default grid: step 1 / (5 span), up to n_obs / (2 span) of the best-observed output
    span, n_obs = t.max() - t.min(), int((omega > 0).sum(0).max())
    grid = reg.periodogram(t, y_nan).freq
    assert np.isclose(grid[0], 1 / (5 * span)) and grid.size == int(np.floor(n_obs * 5 / 2)) and np.isclose(grid[-1], grid.size / (5 * span))


# ---- what it is for --------------------------------------------------------------------------------------------------------------------
def two_tone_series(seed):
    """160 irregular rows on [0, 10]: y = sin(2 pi x / 0.37) + 0.4 sin(2 pi x / 0.113) + 0.1 noise, and a second output with the same two
    lines at other phases, 10 % of whose rows are missing.  The rows and the missing entries are fixed; `seed` draws the noise."""
    x = np.sort(np.random.default_rng(100).uniform(0, 10, 160))
    rng = np.random.default_rng(seed)

    def tone(a, b):
        return np.sin(2 * np.pi * x / 0.37 + a) + 0.4 * np.sin(2 * np.pi * x / 0.113 + b)

    y = np.stack([tone(0, 0), tone(0.9, 2.1)], axis=1) + 0.1 * rng.standard_normal((160, 2))
    y[np.random.default_rng(101).permutation(160)[:16], 1] = np.nan
    return x[:, None], y


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_periods_from_the_periodogram_find_the_lines_a_fixed_ladder_misses(eng, seed):
    """(a) the periods picked from the periodogram are the two lines, strongest first, each within one grid step 1 / (5 span) in frequency;
    (b) after fit(iters=30) the 16-rows-ahead score of the model started there exceeds that of the same model started at the default
    `spectral_period=1.0` (the ladder 1, 1/2).  The second line, 8.85 cycles per unit, lies above the average Nyquist rate of 160 rows on
    10 units (8.0), where the default grid stops: the grid is taken to twice that rate.

    Both legs were run beforehand on the CPU: periodogram by the numpy restatement of tests/test_periodogram.py, its picks given to the
    layers, the oracle engine.  ahead(horizon=16), picked / default ladder: seed 0 155.44 / -180.19, seed 1 220.52 / -319.08, seed 2
    191.37 / -311.83; the picks were 2.7075 and 8.8446 for both outputs and every seed (true 2.7027, 8.8496; step 0.0201), the ladder's
    trained periods never held both lines.  On the device: 155.44 / -180.19, 220.52 / -317.69, 191.37 / -211.41."""
    from gpar_amd import GPARRegressor

    x, y = two_tone_series(seed)
    span = float(x.max() - x.min())
    true = np.array([1 / 0.37, 1 / 0.113])
    auto = GPARRegressor(spectral=2, spectral_period="auto")
    periods = auto.init_spectral(x, y, nyquist=2.0)
    assert periods.shape == (2, 2)
    assert np.all(np.abs(1 / periods - true[None, :]) <= 1 / (5 * span)), 1 / periods
    auto.fit(x, y, iters=30)
    assert np.array_equal(auto._spectral_auto, periods)   # (the fit kept the picks)
    default = GPARRegressor(spectral=2)
    default.fit(x, y, iters=30)
    value = {name: float(np.sum(reg.ahead(x, y, horizon=16)[0])) for name, reg in (("auto", auto), ("default", default))}
    print(f"seed {seed}: picked 1 / periods {1 / periods[0]} {1 / periods[1]}; ahead(horizon=16) auto {value['auto']:.2f}, default {value['default']:.2f}")
    assert np.isfinite(value["auto"]) and value["auto"] > value["default"]


def test_auto_picks_at_the_first_condition_and_keeps_what_exists(eng):
    """`spectral_period="auto"` without `init_spectral`: the first `condition` / `fit` picks on the default grid (the strong line first;
    the weak one is out of that grid's reach), a variable that exists is not overwritten, a second `fit` does not pick again, and
    `init_spectral` does overwrite."""
    from gpar_amd import GPARRegressor

    x, y = two_tone_series(0)
    span = float(x.max() - x.min())
    reg = GPARRegressor(spectral=2, spectral_period="auto")
    reg.vs.bnd(name="1/input/sm1/pers", init=np.array([0.2345]))
    reg.condition(x, y)
    picked = reg._spectral_auto.copy()
    assert picked.shape == (2, 2) and np.all(np.abs(1 / picked[:, 0] - 1 / 0.37) <= 1 / (5 * span))
    assert np.all(1 / picked <= 160 / (2 * span) + 1e-9)   # the default grid's top
    assert np.isfinite(float(reg.logpdf(x, y)))
    values = reg.get_variables()
    for i in range(2):
        for q in range(2):
            want = 0.2345 if (i, q) == (1, 1) else picked[i, q]
            assert np.allclose(values[f"{i}/input/sm{q}/pers"], want, rtol=1e-12)
    reg.fit(x[:100], y[:100], iters=1)
    assert np.array_equal(reg._spectral_auto, picked)
    again = reg.init_spectral(x, y, nyquist=2.0)
    values = reg.get_variables()
    for i in range(2):
        for q in range(2):
            assert np.allclose(values[f"{i}/input/sm{q}/pers"], again[i, q], rtol=1e-12)
    assert abs(1 / again[1, 1] - 1 / 0.113) <= 1 / (5 * span)
