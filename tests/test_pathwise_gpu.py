"""The two device passes of pathwise sampling through the library on the MI355X - gpar_rff_apply against a long-double twin of a numpy
restatement, gpar_gram_apply_groups against `eng.gram` + a product - their bits, their argument errors, `feature_map` against the device
feature map, the fused route of `predict(sampler="pathwise")` against the composed one (GPAR_FUSED_PATHWISE=0), and the law of the samples.

Tolerance of gpar_rff_apply (as DESIGN 3.22 does it for the periodogram): the device has another sincospi and another summation order than
numpy, so a case is allowed 8 x the float64 numpy restatement's own largest distance from the long-double twin over the cases with its
dz, and never less than 8 F 2^-52 max|theta|."""
import ctypes

import numpy as np
import pytest
import torch

from gpar_amd import kernels as K
from gpar_amd.pathwise import feature_map

from .conftest import make_engine
from .test_pathwise import check_law_against_the_closed_form

pytestmark = pytest.mark.gpu

LD = np.longdouble
SENTINEL = -777.25
ARG_ERROR = -1000
ROWS, FREQS, DZS = (1, 63, 64, 65, 129), (1, 63, 64, 65, 300), (1, 4, 5, 17)


@pytest.fixture(scope="module")
def eng():
    from gpar_amd.engine import set_engine

    e = make_engine("hip")
    previous = set_engine(e)
    yield e
    set_engine(previous)


def _dev(eng, a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=eng.device)


def rff_restated(z, shift, omega, thc, ths, group_rows, dtype):
    """sum_j thc[j, c] cos(2 pi omega_j . (z_r - shift)) + ths[j, c] sin(...), in `dtype` throughout."""
    z, shift, omega, thc, ths = (np.asarray(a, dtype=dtype) for a in (z, shift, omega, thc, ths))
    phase = (2 * np.pi if dtype is not LD else 2 * LD(np.pi) + LD(2.4492935982947064e-16)) * ((z - shift) @ omega.T)   # (pi to long-double accuracy)
    c, s = np.cos(phase), np.sin(phase)
    if not group_rows:
        return c @ thc + s @ ths
    col = np.arange(z.shape[0]) // group_rows
    return np.sum(c * thc[:, col].T + s * ths[:, col].T, axis=1)


def _rff_case(rows, F, dz, S, seed):
    rng = np.random.default_rng(seed)
    z = rng.uniform(-3, 3, (rows, max(dz, 1)))
    return z, rng.uniform(-1, 1, max(dz, 1)), rng.standard_normal((F, max(dz, 1))) * 0.4, rng.standard_normal((F, S)), rng.standard_normal((F, S))


def _measure_rff(eng, z, shift, omega, thc, ths, dz, group_rows):
    """(the device's distance from the twin, the float64 restatement's own, the floor 8 F 2^-52 max|theta|, what the case was)."""
    got = eng.rff_apply(_dev(eng, z), dz, _dev(eng, shift), _dev(eng, omega), _dev(eng, thc), _dev(eng, ths), group_rows=group_rows).cpu().numpy()
    want = rff_restated(z[:, :dz], shift[:dz], omega[:, :dz], thc, ths, group_rows, LD)
    assert got.shape == want.shape
    own = float(np.max(np.abs(rff_restated(z[:, :dz], shift[:dz], omega[:, :dz], thc, ths, group_rows, np.float64).astype(LD) - want)))
    floor = 8.0 * omega.shape[0] * 2.0 ** -52 * float(np.max(np.abs(np.concatenate([thc, ths]))))
    return float(np.max(np.abs(got.astype(LD) - want))), own, floor, (z.shape[0], omega.shape[0], thc.shape[1], group_rows)


@pytest.mark.parametrize("dz", DZS)
def test_rff_apply_matches_the_long_double_twin(eng, dz):
    """Every row meets every column (the training rows), S = 1 and 3, and rows in groups (S = 1, 3 with ns = 1, 63, 65): rows and F below,
    at and above the tile sizes.  The tolerance of a case is 8 x the float64 restatement's own LARGEST distance from the twin over the cases
    with this dz (the phase is a dot product over dz dims: what float64 loses grows with dz, and a case of one row and one frequency is
    too small a sample of it), and never below the case's 8 F 2^-52 max|theta|.  Measured on an MI355X: the largest device error and the
    restatement's own are printed."""
    cases = []
    for F in FREQS:
        for S in (1, 3):
            for rows in ROWS:
                cases.append(_measure_rff(eng, *_rff_case(rows, F, dz, S, seed=rows + F + S), dz, 0))
            for ns in (1, 63, 65):
                cases.append(_measure_rff(eng, *_rff_case(S * ns, F, dz, S, seed=ns + F + S + 1), dz, ns))
    own = max(c[1] for c in cases)
    print(f"dz = {dz}: device against the long-double twin {max(c[0] for c in cases):.3e}, the float64 restatement's own error {own:.3e}")
    for err, _, floor, what in cases:
        assert err <= max(8.0 * own, floor), (what, err, own, floor)


def _every_factor_kernel():
    """Every factor type, a periodic embedding, a product and the constant - over three columns."""
    return (1.1 * K.EQ().stretch(0.7).select([0, 1]) + 0.6 * K.RQ(1.5).stretch(0.9).select([0]) * K.Matern32().stretch(1.3).select([1])
            + 0.4 * K.Matern12().stretch(0.8).select([2]) + 0.5 * K.Matern52().stretch(0.6).select([0])
            + 0.7 * K.EQ().stretch(0.8).select([0]) * K.Cosine().stretch(0.45).select([0])
            + 0.9 * K.EQ().stretch(0.7).periodic(0.5).select([1]) + 0.3 * K.Linear().stretch(2.0).select([2]) + 0.2)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_gram_apply_groups_matches_gram_times_vector(eng, n):
    """ns = 1, 63, 64, 65 and S = 1, 2, 3, rows in groups and every row against every vector; a workspace that forces one split of the training
    rows and the recommended one (several).  Tolerance 1e-11 sum |k| |v| (tests/test_switches_gpu.py)."""
    from gpar_amd import hip

    ck = eng.compile(_every_factor_kernel(), 3)
    rng = np.random.default_rng(n)
    z = eng.features(ck, _dev(eng, rng.uniform(0, 2, (n, 3))))
    for ns in (1, 63, 64, 65):
        for S in (1, 2, 3):
            zs = eng.features(ck, _dev(eng, rng.uniform(0, 2, (S * ns, 3))))
            vt = _dev(eng, rng.standard_normal((S, n)))
            Ks = eng.gram(ck, zs, z)
            full, scale = Ks @ vt.T, Ks.abs() @ vt.abs().T   # (S ns) x S
            pick = torch.arange(S * ns, device=eng.device) // ns
            for ws in (None, S * ns):
                got = hip.gram_apply_groups(ck, zs, z, vt, group_rows=ns, ws_doubles=ws)
                assert torch.all((got - full.gather(1, pick[:, None])[:, 0]).abs() <= 1e-11 * scale.gather(1, pick[:, None])[:, 0]), (n, ns, S, ws)
            for ws in (None, S * ns * S):
                got = hip.gram_apply_groups(ck, zs, z, vt, group_rows=0, ws_doubles=ws)
                assert got.shape == full.shape and torch.all((got - full).abs() <= 1e-11 * scale), (n, ns, S, ws)


def test_both_passes_return_the_same_bits_and_rows_do_not_see_their_neighbours(eng):
    """Two calls agree in bits; a group's rows are unchanged when other groups are added, S changes, or the rows are taken as a set that
    meets every column."""
    ck = eng.compile(_every_factor_kernel(), 3)
    rng = np.random.default_rng(0)
    n, ns, S, F = 129, 65, 3, 300
    x, xs = _dev(eng, rng.uniform(0, 2, (n, 3))), _dev(eng, rng.uniform(0, 2, (S * ns, 3)))
    z, zs = eng.features(ck, x), eng.features(ck, xs)
    vt = _dev(eng, rng.standard_normal((S, n)))
    a = eng.gram_apply_groups(ck, zs, z, vt, group_rows=ns)
    assert torch.equal(a, eng.gram_apply_groups(ck, zs, z, vt, group_rows=ns))
    assert torch.equal(a[:ns], eng.gram_apply_groups(ck, zs[:ns], z, vt[:1], group_rows=ns))
    assert torch.equal(a[ns : 2 * ns], eng.gram_apply_groups(ck, zs[ns : 2 * ns], z, vt, group_rows=0)[:, 1])
    shift, omega = _dev(eng, rng.uniform(-1, 1, ck.dz)), _dev(eng, rng.standard_normal((F, ck.dz)))
    thc, ths = _dev(eng, rng.standard_normal((F, S))), _dev(eng, rng.standard_normal((F, S)))
    b = eng.rff_apply(zs, ck.dz, shift, omega, thc, ths, group_rows=ns)
    assert torch.equal(b, eng.rff_apply(zs, ck.dz, shift, omega, thc, ths, group_rows=ns))
    assert torch.equal(b[:ns], eng.rff_apply(zs[:ns], ck.dz, shift, omega, thc[:, :1], ths[:, :1], group_rows=ns))
    assert torch.equal(b[2 * ns :], eng.rff_apply(zs[2 * ns :], ck.dz, shift, omega, thc, ths, group_rows=0)[:, 2])


def test_feature_map_equals_the_device_feature_map(eng):
    """`pathwise.feature_map` against `eng.features`: plain dims to the last bit (one multiplication by the same 1 / scale), periodic dims
    within 2 units in the last place of 1 / scale (sin and cos come from torch here and from the library's kernel there)."""
    kernel = _every_factor_kernel()
    ck = eng.compile(kernel, 3)
    x = _dev(eng, np.random.default_rng(3).uniform(-5, 5, (200, 3)))
    got, want = feature_map(ck.kernel, x), eng.features(ck, x)
    assert got.shape == want.shape == (200, ck.dz)
    periodic = torch.as_tensor([int(ck.fspec.embed[q]) != 0 for q in range(ck.dz)], device=eng.device)
    inv_scale = torch.as_tensor([float(ck.fspec.inv_scale[q]) for q in range(ck.dz)], dtype=torch.float64, device=eng.device)
    assert periodic.any() and torch.equal(got[:, ~periodic], want[:, ~periodic])
    assert torch.all((got - want).abs() <= 2.0 * 2.0 ** -52 * inv_scale)


FAMILIES = {
    "default": dict(linear=True, nonlinear=False),
    "per": dict(per=True, linear=True, nonlinear=False),
    "rq": dict(rq=True, linear=True, nonlinear=False),
    "matern": dict(matern=1.5, linear=True, nonlinear=False),
    "spectral": dict(spectral=2, linear=True, nonlinear=False),
    "nonlinear": dict(linear=True, nonlinear=True),
}


@pytest.mark.parametrize("name", list(FAMILIES))
def test_fused_route_equals_the_composed_route(eng, monkeypatch, name):
    """`predict(sampler="pathwise")` through the two library calls against GPAR_FUSED_PATHWISE=0 (torch features, `eng.gram` + `eng.gemm`):
    one seed - the same basis and the same draws -, n = 70, n* = 65, S = 3, to 1e-9."""
    from gpar_amd import GPARRegressor

    rng = np.random.default_rng(7)
    x = rng.uniform(0, 1, (70, 1))
    y = np.stack([np.sin(6 * x[:, 0]), np.cos(5 * x[:, 0]) ** 2, x[:, 0] ** 2], axis=1) + 0.05 * rng.standard_normal((70, 3))
    xs = np.linspace(0, 1, 65)[:, None]
    reg = GPARRegressor(scale=0.3, noise=0.05, **FAMILIES[name])
    reg.condition(x, y)
    out = []
    for flag in ("1", "0"):
        monkeypatch.setenv("GPAR_FUSED_PATHWISE", flag)
        eng.seed(11)
        out.append(np.stack(reg.sample(xs, posterior=True, num_samples=3, sampler="pathwise", features=256)))
    assert out[0].shape == (3, 65, 3) and np.all(np.isfinite(out[0]))
    np.testing.assert_allclose(out[0], out[1], rtol=1e-9, atol=1e-9)


def test_law_on_the_device(eng):
    check_law_against_the_closed_form()


def test_argument_errors_return_before_any_launch(eng):
    """Negative sizes, dz outside 0 .. GPAR_MAX_DIMS, leading dimensions and a workspace too small: the library's argument-error code, the
    output untouched."""
    from gpar_amd import _lib
    from gpar_amd.hip import stream_ptr

    lib = _lib.load()
    ck = eng.compile(_every_factor_kernel(), 3)
    dz, rows, n, F, S = ck.dz, 10, 12, 7, 2
    z, zs = torch.zeros(n, dz, dtype=torch.float64, device=eng.device), torch.zeros(rows, dz, dtype=torch.float64, device=eng.device)
    shift, omega = torch.zeros(dz, dtype=torch.float64, device=eng.device), torch.zeros(F, dz, dtype=torch.float64, device=eng.device)
    th, vt = torch.zeros(F, S, dtype=torch.float64, device=eng.device), torch.zeros(S, n, dtype=torch.float64, device=eng.device)
    out = torch.full((rows, S), SENTINEL, dtype=torch.float64, device=eng.device)
    ws = torch.zeros(rows * S * 4, dtype=torch.float64, device=eng.device)
    st = stream_ptr(eng.device)

    def rff(rows=rows, ldz=dz, dz=dz, ldw=dz, F=F, ldt=S, count=S, group_rows=0, ldo=S):
        return lib.gpar_rff_apply(zs.data_ptr(), rows, ldz, dz, shift.data_ptr(), omega.data_ptr(), ldw, F, th.data_ptr(), th.data_ptr(), ldt, count,
                                  group_rows, out.data_ptr(), ldo, st)

    def apply(rows=rows, ldzs=dz, n=n, ldz=dz, dz=dz, ldv=n, count=S, group_rows=0, ldo=S, ws_doubles=rows * S):
        return lib.gpar_gram_apply_groups(ctypes.byref(ck.kspec), zs.data_ptr(), rows, ldzs, z.data_ptr(), n, ldz, dz, vt.data_ptr(), ldv, count,
                                          group_rows, out.data_ptr(), ldo, ws.data_ptr(), ws_doubles, st)

    for kw in (dict(rows=-1), dict(F=-1), dict(count=-1), dict(group_rows=-1), dict(dz=-1), dict(dz=_lib.GPAR_MAX_DIMS + 1), dict(ldz=dz - 1),
               dict(ldw=dz - 1), dict(ldt=S - 1), dict(ldo=S - 1), dict(group_rows=3)):
        assert rff(**kw) <= ARG_ERROR, kw
    for kw in (dict(rows=-1), dict(n=-1), dict(count=-1), dict(group_rows=-1), dict(dz=-1), dict(dz=_lib.GPAR_MAX_DIMS + 1), dict(ldzs=dz - 1),
               dict(ldz=dz - 1), dict(ldv=n - 1), dict(ldo=S - 1), dict(ws_doubles=rows * S - 1), dict(group_rows=3)):
        assert apply(**kw) <= ARG_ERROR, kw
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL)
    assert rff() == 0 and apply() == 0 and rff(rows=0) == 0 and apply(count=0) == 0
    torch.cuda.synchronize()
    assert torch.all(out == 0.0)   # (zero features, zero weights: zeros written by the valid calls)
