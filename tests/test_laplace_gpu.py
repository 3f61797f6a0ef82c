"""Hyperparameter uncertainty on the GPU: gpar_gram_grad_rows through the C ABI against gpar_gram_grad_cross(GPAR_GRAD_RECT) called once per
row (n1 = 1, W = v^T: the two routes sum the same terms in a different order), its determinism, row independence and argument errors;
`GPAR.hyper_jacobian` and `DenseLayerObjective.hessian` against central differences; `GPARRegressor.laplace` / `predict_moments_hyper`.

Tolerances.  Kernel parity: 1e-11 of the largest magnitude in the slot's column, the route-parity convention of tests/test_switches_gpu.py.
Jacobian: 1e-6 of the column's largest magnitude against a central difference with h = 1e-5 (its own error: O(h^2) ~ 1e-10 and eps / h ~
1e-11 relative).  Hessian: 1e-4 of the largest entry against the second central difference of the objective values with h = 1e-3."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from .conftest import make_engine, to_np

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
PARITY = 1e-11
N1S = (1, 5, 65)
N2S = (1, 63, 64, 65, 130)


@pytest.fixture
def hip():
    from gpar_amd.engine import set_engine

    eng = make_engine("hip")
    previous = set_engine(eng)
    yield eng
    set_engine(previous)


def _structures():
    """name -> (kernel, width): each factor type alone, RQ (its Al_f slot), a periodic-embedded dim (P_q), the cosine over two dims,
    linear x EQ, a four-factor term, a constant term without feature dims, the default GPAR layer for m = 1 with two previous outputs."""
    from gpar_amd.kernels import EQ, RQ, Cosine, Linear, Matern12, Matern32, Matern52, ZeroKernel
    from gpar_amd.regression import GPARRegressor, _model_generator, layer_config

    out = {
        "eq": (1.3 * EQ().stretch(np.array([0.7, 1.1])).select([0, 2]), 3),
        "rq": (1.3 * RQ(0.7).stretch(0.9).select([1]), 3),
        "linear": (1.3 * Linear().stretch(np.array([2.0, 1.5])).select([0, 1]), 3),
        "matern12": (1.1 * Matern12().stretch(np.array([0.8, 1.3])).select([0, 1]), 3),
        "matern32": (1.3 * Matern32().stretch(np.array([0.8, 1.3])).select([0, 1]), 3),
        "matern52": (1.3 * Matern52().stretch(1.0).select([2]), 3),
        "cos": (1.3 * Cosine().stretch(0.9).select([1]), 3),
        "per_eq_decay": (0.7 * (EQ().stretch(np.array([1.0, 1.4])).periodic(0.6).select([0]) * EQ().stretch(3.0).select([0])), 3),
        "cos_two_dims": (0.4 * (EQ().stretch(1.5).select([0, 1]) * Cosine().stretch(np.array([0.5, 0.9])).select([0, 1])), 3),
        "linear_eq": (0.5 * (Linear().stretch(np.array([2.0, 0.8])).select([1, 2]) * EQ().stretch(np.array([1.2, 0.9])).select([0, 1])), 3),
        "four_factors": (0.6 * (EQ().stretch(1.2).select([0]) * RQ(1.4).stretch(0.9).select([1]) * Linear().stretch(1.7).select([2])
                                * Matern12().stretch(1.1).select([0, 2])), 3),
        "constant": (ZeroKernel() + 0.3, 3),
    }
    reg = GPARRegressor(nonlinear=True, per=True)
    with torch.no_grad():
        f, _ = _model_generator(reg.vs, 1, 2, **layer_config(reg, 1, 2))()
    out["gpar_layer"] = (f.kernel, 3)
    return out


NAMES = ("eq", "rq", "linear", "matern12", "matern32", "matern52", "cos", "per_eq_decay", "cos_two_dims", "linear_eq", "four_factors",
         "constant", "gpar_layer")


def _inputs(hip, kernel, width, n1, n2, seed=0, shared=0):
    """(ck, z1, zd1, z2, zd2, v): features of random design rows; the first `shared` rows of z1 are rows of z2 (r = 0)."""
    rng = np.random.default_rng(seed + 1000 * n1 + n2)
    x1, x2 = rng.uniform(-1, 1, (n1, width)), rng.uniform(-1, 1, (n2, width))
    x1[:min(shared, n1, n2)] = x2[:min(shared, n1, n2)]
    ck = hip.compile(kernel, width)
    t1, t2 = hip.tensor(x1), hip.tensor(x2)
    z1, z2 = hip.features(ck, t1), hip.features(ck, t2)
    zd1 = zd2 = None
    if hip._periodic(ck):
        zd1, zd2 = hip.featurize_dfreq(ck, t1), hip.featurize_dfreq(ck, t2)
    return ck, z1, zd1, z2, zd2, hip.tensor(rng.standard_normal(n2))


def _ld(a):
    return max(int(a.stride(0)), int(a.shape[1]), 1) if a.shape[0] > 1 else max(int(a.shape[1]), 1)


def _rows(hip, ck, z1, zd1, z2, zd2, v, ws_doubles=None, pad=3, expect=0, out=None):
    """gpar_gram_grad_rows through ctypes into a sentinel-filled buffer with a padded leading dimension; returns (status, whole buffer)."""
    from gpar_amd import _lib, hip as hipmod

    lib = _lib.load()
    n1, n2 = int(z1.shape[0]), int(z2.shape[0])
    if ws_doubles is None:
        ws_doubles = lib.gpar_workspace_doubles(_lib.WS_GRAM_GRAD_ROWS, n2, n1, 0)
    ws = torch.empty(max(int(ws_doubles), 1) + 2, dtype=torch.float64, device=hip.device)
    buf = torch.full((max(n1, 1), _lib.GRAD_NACC + pad), SENTINEL, dtype=torch.float64, device=hip.device) if out is None else out
    rc = lib.gpar_gram_grad_rows(ctypes.byref(ck.kspec), z1.data_ptr(), None if zd1 is None else zd1.data_ptr(), n1, _ld(z1), z2.data_ptr(),
                                 None if zd2 is None else zd2.data_ptr(), n2, _ld(z2), ck.dz, v.data_ptr(), buf.data_ptr(), _lib.GRAD_NACC + pad,
                                 ws.data_ptr(), int(ws_doubles), hipmod.stream_ptr(hip.device))
    assert (rc == 0) if expect == 0 else (rc < 0), rc
    return rc, to_np(buf).copy()


def _per_row_reference(ck, z1, zd1, z2, zd2, v):
    """Row a: gpar_gram_grad_cross(GPAR_GRAD_RECT) with n1 = 1, z1 = z1[a], W = v^T."""
    from gpar_amd import hip as hipmod

    W = v.reshape(1, -1).contiguous()
    rows = [hipmod.gram_grad_cross(ck, z1[a:a + 1], None if zd1 is None else zd1[a:a + 1], z2, zd2, W, hipmod.GRAD_RECT) for a in range(z1.shape[0])]
    return to_np(torch.stack(rows))


def _used_slots(ck):
    """The raw slots the structure uses: its terms, its RQ factors, the dims under a factor, and those under a stationary factor again
    (the period sums) when the structure has periodic dims."""
    from gpar_amd import _lib

    ks = ck.kspec
    nT, nF, nD = _lib.GPAR_MAX_TERMS, _lib.GPAR_MAX_FACTORS, _lib.GPAR_MAX_DIMS
    used = set(range(ks.nterms))
    periodic = any(f.periods is not None for t in ck.kernel.terms for f in t.factors)
    for f in range(ks.nfactors):
        fa = ks.factor[f]
        if fa.type == _lib.K_RQ:
            used.add(nT + f)
        for d in range(fa.off, fa.off + fa.nd):
            used.add(nT + nF + d)
            if periodic and fa.type not in (_lib.K_LINEAR, _lib.K_COS):
                used.add(nT + nF + nD + d)
    return sorted(used)


def _assert_parity(got, ref, ck):
    from gpar_amd import _lib

    nacc = _lib.GRAD_NACC
    assert np.all(got[:, nacc:] == SENTINEL)
    got = got[:, :nacc]
    used = _used_slots(ck)
    unused = [s for s in range(nacc) if s not in used]
    assert np.all(got[:, unused] == 0.0)
    scale = np.abs(ref).max(axis=0)
    err = np.abs(got - ref).max(axis=0)
    worst = max(used, key=lambda s: err[s] / scale[s] if scale[s] > 0 else (np.inf if err[s] > 0 else 0.0))
    print(f"largest relative column error {err[worst] / max(scale[worst], 1e-300):.3e} in slot {worst}")
    assert np.all(err <= PARITY * scale), (err[worst], scale[worst], worst)


@pytest.mark.parametrize("name", NAMES)
def test_rows_match_one_cross_call_per_row(hip, name):
    kernel, width = _structures()[name]
    for n1 in N1S:
        for n2 in N2S:
            ck, z1, zd1, z2, zd2, v = _inputs(hip, kernel, width, n1, n2)
            _, got = _rows(hip, ck, z1, zd1, z2, zd2, v)
            _assert_parity(got, _per_row_reference(ck, z1, zd1, z2, zd2, v), ck)


@pytest.mark.parametrize("name", ("matern12", "four_factors", "gpar_layer"))
def test_rows_of_z2_among_z1(hip, name):
    """r = 0 pairs: the Matern-1/2 multiplier is 0 there, as in training."""
    kernel, width = _structures()[name]
    ck, z1, zd1, z2, zd2, v = _inputs(hip, kernel, width, 65, 130, shared=40)
    _, got = _rows(hip, ck, z1, zd1, z2, zd2, v)
    assert np.all(np.isfinite(got))
    _assert_parity(got, _per_row_reference(ck, z1, zd1, z2, zd2, v), ck)


@pytest.mark.parametrize("name", ("gpar_layer", "four_factors"))
def test_splits_and_least_workspace(hip, name):
    """n2 = 300 is five column tiles: the recommended workspace gives five splits for 5 rows, the least workspace one."""
    from gpar_amd import _lib

    kernel, width = _structures()[name]
    ck, z1, zd1, z2, zd2, v = _inputs(hip, kernel, width, 5, 300)
    ref = _per_row_reference(ck, z1, zd1, z2, zd2, v)
    recommended = _lib.load().gpar_workspace_doubles(_lib.WS_GRAM_GRAD_ROWS, 300, 5, 0)
    assert recommended >= 2 * 5 * _lib.GRAD_NACC   # (at least two splits)
    _, split = _rows(hip, ck, z1, zd1, z2, zd2, v, ws_doubles=recommended)
    _, single = _rows(hip, ck, z1, zd1, z2, zd2, v, ws_doubles=5 * _lib.GRAD_NACC)
    _assert_parity(split, ref, ck)
    _assert_parity(single, ref, ck)


def test_same_bits_twice_and_rows_independent(hip):
    from gpar_amd import _lib

    kernel, width = _structures()["gpar_layer"]
    ck, z1, zd1, z2, zd2, v = _inputs(hip, kernel, width, 65, 130)
    _, first = _rows(hip, ck, z1, zd1, z2, zd2, v)
    _, second = _rows(hip, ck, z1, zd1, z2, zd2, v)
    assert np.array_equal(first, second)
    # one split in both calls (the least workspace of each): row a alone has the bits it has among the 65
    _, whole = _rows(hip, ck, z1, zd1, z2, zd2, v, ws_doubles=65 * _lib.GRAD_NACC)
    for a in (0, 37, 64):
        _, alone = _rows(hip, ck, z1[a:a + 1], None if zd1 is None else zd1[a:a + 1], z2, zd2, v, ws_doubles=_lib.GRAD_NACC)
        assert np.array_equal(alone[0], whole[a])


def test_empty_inputs(hip):
    from gpar_amd import _lib

    kernel, width = _structures()["gpar_layer"]
    ck, z1, zd1, z2, zd2, v = _inputs(hip, kernel, width, 5, 64)
    _, got = _rows(hip, ck, z1, zd1, z2[:0], None if zd2 is None else zd2[:0], v[:0])
    assert np.all(got[:, :_lib.GRAD_NACC] == 0.0) and np.all(got[:, _lib.GRAD_NACC:] == SENTINEL)
    _, got = _rows(hip, ck, z1[:0], None if zd1 is None else zd1[:0], z2, zd2, v)
    assert np.all(got == SENTINEL)


def test_argument_errors_touch_nothing(hip):
    """Every error of include/gpar_hip.h: a negative status, the sentinel-filled `out` as it was."""
    from gpar_amd import _lib, hip as hipmod

    lib = _lib.load()
    kernel, width = _structures()["gpar_layer"]
    ck, z1, zd1, z2, zd2, v = _inputs(hip, kernel, width, 5, 64)
    assert zd1 is not None
    n1, n2, nacc = 5, 64, _lib.GRAD_NACC
    ws = torch.empty(n1 * nacc, dtype=torch.float64, device=hip.device)
    out = torch.full((n1, nacc), SENTINEL, dtype=torch.float64, device=hip.device)
    stream = hipmod.stream_ptr(hip.device)
    good = dict(ks=ctypes.byref(ck.kspec), z1=z1.data_ptr(), zd1=zd1.data_ptr(), n1=n1, ldz1=_ld(z1), z2=z2.data_ptr(), zd2=zd2.data_ptr(), n2=n2,
                ldz2=_ld(z2), dz=ck.dz, v=v.data_ptr(), out=out.data_ptr(), ldo=nacc, ws=ws.data_ptr(), ws_doubles=n1 * nacc)

    def call(**change):
        a = dict(good, **change)
        return lib.gpar_gram_grad_rows(a["ks"], a["z1"], a["zd1"], a["n1"], a["ldz1"], a["z2"], a["zd2"], a["n2"], a["ldz2"], a["dz"], a["v"], a["out"],
                                       a["ldo"], a["ws"], a["ws_doubles"], stream)

    def spec(edit):
        ks = type(ck.kspec).from_buffer_copy(ck.kspec)
        edit(ks)
        return ks

    def reach(ks):
        ks.factor[0].nd = ck.dz + 1

    def crowd(ks):   # five factors in term 0
        for f in range(5):
            ks.factor[f].term = 0
        for f in range(5, ks.nfactors):
            ks.factor[f].term = max(ks.factor[f].term, 0)

    assert ck.kspec.nfactors >= 5
    cases = {
        "negative n1": dict(n1=-1), "negative n2": dict(n2=-1), "dz below": dict(dz=-1), "dz above": dict(dz=_lib.GPAR_MAX_DIMS + 1),
        "a factor past dz": dict(ks=ctypes.byref(spec(reach))), "five factors in a term": dict(ks=ctypes.byref(spec(crowd))),
        "ldo": dict(ldo=nacc - 1), "ldz1": dict(ldz1=ck.dz - 1), "ldz2": dict(ldz2=ck.dz - 1), "workspace": dict(ws_doubles=n1 * nacc - 1),
        "NULL z1": dict(z1=None), "NULL z2": dict(z2=None), "NULL v": dict(v=None), "NULL out": dict(out=None), "NULL ws": dict(ws=None),
        "NULL ks": dict(ks=None), "zd1 alone": dict(zd2=None), "zd2 alone": dict(zd1=None),
    }
    for what, change in cases.items():
        rc = call(**change)
        assert rc < 0, (what, rc)
        assert bool((out == SENTINEL).all()), what
    assert call() == 0
    assert not bool((out == SENTINEL).any())


# ---- the host layers on the device ------------------------------------------------------------------------------------------------------------

def _series(n, p, seed=0):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0, 1, (n, 1)), axis=0)
    cols = [np.sin(6 * x[:, 0]), np.cos(5 * x[:, 0]) * x[:, 0], x[:, 0] - np.sin(9 * x[:, 0]) ** 2]
    y = np.stack(cols[:p], axis=1) + 0.05 * rng.standard_normal((n, p))
    return x, y


def _plug_in_means(reg, xs):
    """The closed-form latent means along the plug-in path (`GPAR._moments`, what `predict_moments` walks; the public method refuses
    replace=False, where the training inputs are data and only the test-time inputs are means), in normalised units."""
    from gpar_amd.regression import _construct_gpar, _default_weights

    gpar = _construct_gpar(reg, reg.vs, reg.m, reg.p) | (reg.x, reg.y, reg.w)
    with torch.no_grad():
        mean, _ = gpar._moments(torch.as_tensor(xs), _default_weights(xs.shape[0], reg.p), True)
    return to_np(mean).copy()


@pytest.mark.parametrize("per", (False, True))
def test_hyper_jacobian_against_central_differences(hip, per):
    """n = 40, n* = 7, p = 3, nonlinear=True (the cross-layer chain rule), replace=False: the training inputs are data, so a plain
    re-conditioning at shifted values is the central difference with the training inputs frozen.

    The data.  The reference resolves a column only down to its own error: the re-conditioned means carry rounding of about eps times
    the condition number of K times |mean|, which the difference divides by 2 h.  A bound of 1e-6 of the COLUMN therefore needs every
    column to reach about 1e-3 of |mean|.  With unit-scale outputs the default linear term over the previous outputs (length scale 100)
    weighs 1e-4 of the others and its scale's column is too small for that; so the outputs have amplitude 20 and are not normalised -
    the order of magnitude a length scale of 100 is a prior for, and still small enough that the nonlinear term over the outputs
    (length scale 1) couples neighbouring rows: every term of the default kernel is a live part of the model (DESIGN 3.25 has the
    figures)."""
    from gpar_amd import GPARRegressor
    from gpar_amd.regression import _construct_gpar

    x, y = _series(40, 3)
    y = 20.0 * y
    xs = np.random.default_rng(5).uniform(0, 1, (7, 1))
    reg = GPARRegressor(replace=False, nonlinear=True, per=per, per_period=0.7, noise=0.05, normalise_y=False)
    reg.condition(x, y)
    objectives = reg._layer_chains()
    names = [n for obj in objectives for n in obj.names]
    u0 = reg.vs.get_vector(names)
    chains = [obj.chain_matrix(reg.vs.get_vector(obj.names)) for obj in objectives]
    gpar = _construct_gpar(reg, reg.vs, reg.m, reg.p) | (reg.x, reg.y, reg.w)
    jac = [to_np(J) for J in gpar.hyper_jacobian(hip.tensor(xs), chains)]
    P = u0.size
    names_flat = [f"{name}[{j}]" for obj in objectives for name, _, _, _, sl, _ in obj.layout for j in range(sl.stop - sl.start)]
    assert all(J.shape == (7, P) for J in jac) and P == sum(obj.size for obj in objectives)
    h = 1e-5
    fd = np.zeros((3, 7, P))
    for k in range(P):
        for sign in (1.0, -1.0):
            u = u0.copy()
            u[k] += sign * h
            reg.vs.set_vector(u, names)
            fd[:, :, k] += sign * _plug_in_means(reg, xs).T / (2 * h)
    reg.vs.set_vector(u0, names)
    misses = []
    for i in range(3):
        scale = np.abs(fd[i]).max(axis=0)
        err = np.abs(jac[i] - fd[i]).max(axis=0)
        for k in np.flatnonzero(scale > 0):
            print(f"output {i} {names_flat[k]}: column magnitude {scale[k]:.3e}, error {err[k]:.3e}, relative {err[k] / scale[k]:.3e}")
        misses += [(i, names_flat[k], float(scale[k]), float(err[k])) for k in np.flatnonzero(err > 1e-6 * scale)]
    assert not misses, misses
    # later layers do depend on earlier layers' variables, earlier ones not on later ones
    first = objectives[0].size
    assert np.abs(jac[2][:, :first]).max() > 0 and np.all(jac[0][:, first:] == 0.0)


def test_hessian_against_second_differences_of_the_values(hip):
    from gpar_amd import GPARRegressor

    x, y = _series(30, 1)
    reg = GPARRegressor(replace=True, nonlinear=True, noise=0.05)
    reg.condition(x, y)
    obj, _ = reg._layer_objectives()[0]
    u = reg.vs.get_vector(obj.names)
    H = obj.hessian(u)
    assert np.array_equal(H, H.T)
    P, h = u.size, 1e-3
    f = lambda v: obj.fg(v)[0]
    ref = np.zeros((P, P))
    for i in range(P):
        for j in range(i, P):
            ei, ej = np.eye(P)[i] * h, np.eye(P)[j] * h
            ref[i, j] = ref[j, i] = (f(u + ei + ej) - f(u + ei - ej) - f(u - ei + ej) + f(u - ei - ej)) / (4 * h * h)
    print(f"largest entry {np.abs(ref).max():.3e}, largest difference {np.abs(H - ref).max():.3e}")
    assert np.abs(H - ref).max() <= 1e-4 * np.abs(ref).max()


def test_public_behaviour(hip):
    from gpar_amd import GPARRegressor

    x, y = _series(40, 2, seed=3)
    xs = np.linspace(0, 1, 9)[:, None]
    reg = GPARRegressor(replace=True, nonlinear=True, noise=0.05)
    reg.fit(x, y, iters=30)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hp = reg.laplace(x, y)
    trained = [n for n in reg.get_variables() if n.split("/")[0] in ("0", "1")]
    assert len(hp.names) == len(trained) and set(hp.names) == set(trained)
    assert [n.split("/")[0] for n in hp.names] == sorted(n.split("/")[0] for n in hp.names)   # (layer by layer)
    values = reg.get_variables()
    for name, value, sd, sl in zip(hp.names, hp.value, hp.stderr, hp.slices):
        np.testing.assert_allclose(value, values[name], rtol=1e-12)
        var = reg.vs._vars[name]
        u = var.latent.detach().numpy().reshape(-1)
        s = 1.0 / (1.0 + np.exp(-u))
        slope = (var.upper - var.lower) * s * (1 - s) if var.kind == "bnd" else (np.exp(u) if var.kind == "pos" else np.ones_like(u))
        expect = np.abs(slope) * np.sqrt(np.diag(hp.cov)[sl])
        finite = np.isfinite(np.asarray(sd).reshape(-1))
        np.testing.assert_allclose(np.asarray(sd).reshape(-1)[finite], expect[finite], rtol=1e-10)
    mean, var, extra = reg.predict_moments_hyper(xs, hp)
    m0, v0 = reg.predict_moments(xs)
    assert np.array_equal(mean, m0) and np.array_equal(var, v0)
    assert extra.shape == mean.shape and np.all(extra >= 0.0) and np.all(np.isfinite(extra))
    if not any(hp.flat):
        assert np.all(extra > 0.0)
    # every direction of every layer flat: nothing to add
    nothing = hp._replace(cov=np.zeros_like(hp.cov))
    assert np.all(reg.predict_moments_hyper(xs, nothing)[2] == 0.0)
    with pytest.raises(ValueError, match="does not belong"):
        reg.predict_moments_hyper(xs, hp._replace(names=hp.names[:-1]))


def test_a_variable_pinned_at_its_bound_is_flat(hip):
    from gpar_amd import GPARRegressor

    x, y = _series(40, 2, seed=3)
    xs = np.linspace(0, 1, 9)[:, None]
    reg = GPARRegressor(replace=True, nonlinear=True, noise=0.05)
    reg.fit(x, y, iters=10)
    pinned = "1/output/lin/scales"   # (a linear term with an enormous length scale: the model stays well conditioned)
    assert reg.vs._vars[pinned].kind == "bnd"
    with torch.no_grad():
        reg.vs._vars[pinned].latent.fill_(60.0)   # sigmoid(60) = 1 to the last bit: the value sits on its upper bound
    with pytest.warns(UserWarning, match="flat") as caught:
        hp = reg.laplace(x, y)
    assert len([w for w in caught if "flat" in str(w.message)]) == 1
    assert hp.flat[1] >= 1
    assert np.all(np.isinf(np.asarray(hp.stderr[hp.names.index(pinned)])))
    extra = reg.predict_moments_hyper(xs, hp)[2]
    assert np.all(np.isfinite(extra)) and np.all(extra >= 0.0)


def test_matern12_single_output_is_served(hip):
    """`matern=0.5` with one output: the Jacobian of the only layer (the r = 0 multiplier is 0, as in training) against the central
    difference of `predict_moments(latent=True)`, h = 1e-5, 1e-6 of the column as above (amplitude 1: no linear term over outputs)."""
    from gpar_amd import GPARRegressor
    from gpar_amd.regression import _construct_gpar

    x, y = _series(40, 1)
    xs = np.random.default_rng(5).uniform(0, 1, (7, 1))
    reg = GPARRegressor(replace=True, nonlinear=True, matern=0.5, noise=0.05, normalise_y=False)
    reg.condition(x, y)
    chains = reg._layer_chains()
    names = list(chains[0].names)
    u0 = reg.vs.get_vector(names)
    gpar = _construct_gpar(reg, reg.vs, reg.m, reg.p) | (reg.x, reg.y, reg.w)
    jac = to_np(gpar.hyper_jacobian(hip.tensor(xs), [c.chain_matrix(u0) for c in chains])[0])
    h, fd = 1e-5, np.zeros((7, u0.size))
    for k in range(u0.size):
        for sign in (1.0, -1.0):
            u = u0.copy()
            u[k] += sign * h
            reg.vs.set_vector(u, names)
            fd[:, k] += sign * reg.predict_moments(xs, latent=True)[0][:, 0] / (2 * h)
    reg.vs.set_vector(u0, names)
    scale, err = np.abs(fd).max(axis=0), np.abs(jac - fd).max(axis=0)
    print("columns", scale, "errors", err)
    assert np.all(scale > 0) and np.all(err <= 1e-6 * scale), (err, scale)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hp = reg.laplace(x, y)
    extra = reg.predict_moments_hyper(xs, hp)[2]
    assert extra.shape == (7, 1) and np.all(np.isfinite(extra)) and np.all(extra >= 0.0)


def test_layers_above_the_one_call_row_limit_are_served(hip, monkeypatch):
    """GPAR_ONE_CALL_GRAD_ROWS=0 ("never"): no layer has a prepared objective.  The Hessian then differences the general route's
    back-propagated gradient - the same device sums, chained by autograd instead of numpy, so the gradients agree to rounding (1e-13
    of their size) and their differences over 2 h ~ 1.2e-5 to about 1e-8: asserted at 1e-6 of the largest entry.  The chain rule of
    `predict_moments_hyper` never touches the objective: with the same `hp` it returns the same bits."""
    from gpar_amd import GPARRegressor
    from gpar_amd.fastfit import DenseLayerObjective, hessian_of

    x, y = _series(40, 2, seed=3)
    xs = np.linspace(0, 1, 9)[:, None]
    reg = GPARRegressor(replace=True, nonlinear=True, noise=0.05)
    reg.fit(x, y, iters=10)

    def hessians():
        out = []
        for obj, fg in reg._layer_objectives():
            u = reg.vs.get_vector(obj.names)
            out.append((type(obj), hessian_of(fg, u)))
            reg.vs.set_vector(u, obj.names)
        return out

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        prepared = hessians()
        hp = reg.laplace(x, y)
        want = reg.predict_moments_hyper(xs, hp)
        monkeypatch.setenv("GPAR_ONE_CALL_GRAD_ROWS", "0")
        general = hessians()
        hp_general = reg.laplace(x, y)
        got = reg.predict_moments_hyper(xs, hp)
    assert all(issubclass(t, DenseLayerObjective) for t, _ in prepared) and not any(issubclass(t, DenseLayerObjective) for t, _ in general)
    for (_, a), (_, b) in zip(prepared, general):
        print(f"largest entry {np.abs(a).max():.3e}, largest difference between the routes {np.abs(a - b).max():.3e}")
        assert np.abs(a - b).max() <= 1e-6 * np.abs(a).max()
    assert hp_general.names == hp.names and hp_general.flat == hp.flat
    assert all(np.array_equal(g, w_) for g, w_ in zip(got, want))
