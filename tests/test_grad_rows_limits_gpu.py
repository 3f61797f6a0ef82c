"""gpar_gram_grad_rows (csrc/gram_grad_rows.h) at the limits of the kernel specification and of its dynamic LDS, against a reference that
shares nothing with it: tests/grad_rows_reference.py, closed forms in long double written from the kernels' definitions (checked against
50-digit central differences in tests/test_grad_rows_limits.py).  A device row is pushed through the host chain rule
`HipEngine._grads_from_moments(ck, row, 1.0)` and compared per NATURAL parameter - every coefficient, length scale, period and RQ alpha -
so that the kernel's formulas and the host map are tested together against truth.

The rule, per row a and parameter theta:   |device - reference| <= 1e-11 S_a,   S_a = sum_b |v_b| |d k_theta(x1_a, x2_b) / d theta|
- the project's rule for a fused weighted Gram product (1e-11 sum |k| |v| for gpar_gram_apply_groups, tests/test_pathwise_gpu.py) and the
1e-11 of the existing kernel parity (tests/test_laplace_gpu.py).

The LDS arithmetic (grad_rows_reference.rows_lds_doubles; 48 KB = 6144 doubles, 160 KB = 20480; a launch opts in to large LDS when its
doubles EXCEED 6144, the entry refuses when they EXCEED 20480), with nused = terms + RQ factors + dims under a factor (+ dims under a
stationary factor with zd):
  wide_eq         no zd, nused 1 + dz    200 dz + 238     dz 29: 6038   dz 30: 6238 >      dz 96: 19438 fits
  wide_mixed      no zd, nused 2 + dz    200 dz + 302     dz 29: 6102   dz 30: 6302 >
  wide_periodic   zd, nused 1 + 2 dz     400 dz + 238     dz 14: 5838   dz 16: 6638 >      dz 50: 20238 fits   dz 52: 21038 refused
  twelve_rq       no zd, nused 20 + dz   200 dz + 1454                                     dz 95: 20454 fits   dz 96: 20654 refused
  twelve_rq + zd  nused 20 + 2 dz        400 dz + 1454                                     dz 47: 20254 fits   dz 48: 20654 refused
  twelve_factors  zd, nused 10 + dz + the dims under its seven stationary factors
                                                          dz 14: 6094   dz 15: 6494 >      dz 52: 20334 fits   dz 53: 20734 refused
twelve_rq is the worst case: every slot kind at its maximum.  Without zd it fits up to dz 95; given zd (which the entry permits for a
structure without periodic dims: every dim under a stationary factor then has a P slot) up to dz 47 - the two figures of the header.
tests/test_grad_rows_limits.py checks this table against `rows_lds_doubles`, `slots_used` and the sources, and runs `every_reference()`
where no GPU is, so that a vacuous case fails there.

Sizes: (n1, n2) = (65, 130) and (129, 65), alternating: two and three row blocks with a ragged last one, three and two column tiles with a
ragged last one.  The worst err / (1e-11 S) of every case is printed; profiles/grad_rows_limits.txt records them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from . import grad_rows_reference as gr
from . import test_laplace_gpu as tl
from . import test_posterior_limits_gpu as lim
from .conftest import to_np
from .test_laplace_gpu import hip  # noqa: F401  (the fixture: the HIP engine installed for one test)

pytestmark = pytest.mark.gpu

RULE = 1e-11
SENTINEL = tl.SENTINEL
VACUITY = 1e-3

#: (structure, dz): both sides of every edge of the table, the largest shapes that fit, three linear factors on shifted inputs
EDGE_CASES = (("wide_eq", 29), ("wide_eq", 30), ("wide_eq", 96), ("wide_mixed", 29), ("wide_mixed", 30), ("wide_mixed", 31),
              ("wide_periodic", 14), ("wide_periodic", 16), ("wide_periodic", 50), ("twelve_rq", 95),
              ("twelve_factors", 14), ("twelve_factors", 15), ("twelve_factors", 52), ("lin3_eq", 29))
#: (structure, dz, zd given): the first refused dz of each 160 KB edge
REFUSED_CASES = (("twelve_rq", 96, False), ("wide_periodic", 52, True), ("twelve_factors", 53, True), ("twelve_rq", 48, True))
SHARED_CASES = (("wide_mixed", 31), ("twelve_factors", 15))   # the first 40 rows of x1 are rows of x2
SPLIT_CASE = ("wide_periodic", 16)                            # above 48 KB
ZD_WITHOUT_PERIODS = (("wide_mixed", 30), ("twelve_rq", 47))  # zd given to structures with no periodic dims
#: the 48 KB edges (structure, zd, largest dz at or below, smallest above) and the 160 KB edges (structure, zd, largest that fits, first refused)
EDGES_48K = (("wide_eq", False, 29, 30), ("wide_mixed", False, 29, 30), ("wide_periodic", True, 14, 16), ("twelve_factors", True, 14, 15))
EDGES_160K = (("wide_eq", False, 96, None), ("wide_periodic", True, 50, 52), ("twelve_rq", False, 95, 96), ("twelve_rq", True, 47, 48),
              ("twelve_factors", True, 52, 53))


def sizes(i):
    """(n1, n2): 65 rows against 130 columns, or 129 against 65."""
    return ((65, 130), (129, 65))[i % 2]


# ---- the structures: those of tests/test_posterior_limits_gpu.py and the worst case of the slot plan ------------------------------------------
def structure(name, dz):
    """(kernel, width, shift) as `test_posterior_limits_gpu.structure`, and
    twelve_rq   8 terms and 12 RQ factors (4 + 2 + 6 x 1) over dz dims dealt round the factors: every C_t and every Al_f slot in use."""
    from gpar_amd.kernels import RQ, Kernel

    if name != "twelve_rq":
        return lim.structure(name, dz)
    assert dz >= 12
    nd = [dz // 12 + (i < dz % 12) for i in range(12)]
    width = max(nd) + 3
    cols = [[(2 * i + j) % width for j in range(nd[i])] for i in range(12)]
    groups = [[0, 1, 2, 3], [4, 5]] + [[i] for i in range(6, 12)]
    terms = []
    for t, group in enumerate(groups):
        total = sum(nd[i] for i in group)
        k = None
        for i in group:
            factor = RQ(0.7 + 0.2 * i).stretch(lim._ell(total) * lim._vary(nd[i], i)).select(cols[i])
            k = factor if k is None else k * factor
        terms.append((1.0 - 0.08 * t) * k)
    return Kernel([t for k in terms for t in k.terms]), width, 0.0


def has_periods(spec):
    return any(f.get("periods") is not None for t in spec["terms"] for f in t["factors"])


def inputs(name, dz, n1, n2, shared=0):
    """(kernel, width, x1, x2, v): inputs uniform on [-1, 1] + the structure's shift, standard-normal weights; the first `shared` rows of
    x1 are rows of x2 (r = 0 pairs)."""
    kernel, width, shift = structure(name, dz)
    assert lim.feature_dims(kernel) == dz and len(kernel.terms) <= 8 and sum(len(t.factors) for t in kernel.terms) <= 12
    rng = np.random.default_rng([sum(map(ord, name)), dz, n1, n2, shared])
    x1, x2 = shift + rng.uniform(-1, 1, (n1, width)), shift + rng.uniform(-1, 1, (n2, width))
    x1[:shared] = x2[:shared]
    return kernel, width, x1, x2, rng.standard_normal(n2)


def assert_not_vacuous(grads, mags, what):
    """Every parameter's column has something to compare: max_a |d g_a / d theta| >= 1e-3 max_a S_a (about 0.1 is expected of
    standard-normal weights over 65 to 130 columns)."""
    assert set(grads) == set(mags) and grads
    for key in grads:
        g, s = float(np.abs(grads[key]).max()), float(mags[key].max())
        assert s > 0.0 and g >= VACUITY * s, (what, key, g, s)


@functools.lru_cache(maxsize=None)
def reference(name, dz, n1, n2, shared=0):
    """(kernel, width, x1, x2, v, spec, {name: d g_a / d theta}, {name: S_a}) - computed once per case, non-vacuous in every parameter."""
    kernel, width, x1, x2, v = inputs(name, dz, n1, n2, shared)
    spec = lim.spec_of(kernel)
    grads, mags = gr.row_gradients(spec, x1, x2, v)
    assert_not_vacuous(grads, mags, f"{name} dz={dz} n1={n1} n2={n2} shared={shared}")
    return kernel, width, x1, x2, v, spec, grads, mags


def every_reference():
    """The arguments of every `reference` the device tests below compare against: tests/test_grad_rows_limits.py runs them on the CPU."""
    out = [(name, dz, *sizes(i)) for i, (name, dz) in enumerate(EDGE_CASES)]
    out += [(name, dz, 65, 130, 40) for name, dz in SHARED_CASES]
    out += [(*SPLIT_CASE, 5, 300), (*SPLIT_CASE, 65, 300)]
    out += [(name, dz, *sizes(i)) for i, (name, dz) in enumerate(ZD_WITHOUT_PERIODS)]
    return out


# ---- the device side -------------------------------------------------------------------------------------------------------------------------------
def _padded(t):
    """A view of a copy of `t` in a buffer with an odd leading dimension of at least three more doubles, the padding NaN (a read of it
    would show in every sum)."""
    rows, cols = int(t.shape[0]), int(t.shape[1])
    ld = cols + 3 + (cols % 2)
    buf = torch.full((rows, ld), float("nan"), dtype=torch.float64, device=t.device)
    buf[:, :cols] = t
    assert ld % 2 == 1 and int(buf.stride(0)) == ld
    return buf[:, :cols]


def features(hip, case, zd=None):
    """(ck, z1, zd1, z2, zd2, v) on the device for a `reference` case; zd: given when the structure has periodic dims, or as asked."""
    kernel, width, x1, x2, v, spec = case[:6]
    ck = hip.compile(kernel, width)
    assert lim.spec_of(ck.kernel) == spec
    t1, t2 = hip.tensor(x1), hip.tensor(x2)
    z1, z2 = _padded(hip.features(ck, t1)), _padded(hip.features(ck, t2))
    zd1 = zd2 = None
    if has_periods(spec) if zd is None else zd:
        zd1, zd2 = _padded(hip.featurize_dfreq(ck, t1)), _padded(hip.featurize_dfreq(ck, t2))
        assert hip._periodic(ck) == has_periods(spec)
    return ck, z1, zd1, z2, zd2, hip.tensor(v)


def natural(hip, ck, raw):
    """{name: n1 values} from raw rows through `_grads_from_moments(ck, row, 1.0)`, named as the restatement names them."""
    out = {}
    for a in range(raw.shape[0]):
        g = hip._grads_from_moments(ck, raw[a], 1.0)
        flat = {f"coef/{t}": c for t, c in enumerate(g["coef"])}
        for t, factors in enumerate(g["factors"]):
            for f, fg in enumerate(factors):
                flat.update({f"scales/{t}/{f}/{q}": s for q, s in enumerate(np.asarray(fg["scales"]).reshape(-1))})
                if fg["periods"] is not None:
                    flat.update({f"periods/{t}/{f}/{c}": s for c, s in enumerate(np.asarray(fg["periods"]).reshape(-1))})
                if fg["alpha"] is not None:
                    flat[f"alpha/{t}/{f}"] = fg["alpha"]
        for key, value in flat.items():
            out.setdefault(key, np.zeros(raw.shape[0]))[a] = float(value)
    return out


def worst_ratio(got, grads, mags):
    """max over parameters and rows of err / (1e-11 S) and where; every parameter of the restatement must be there, and no other."""
    assert set(got) == set(grads), set(got) ^ set(grads)
    worst, where = 0.0, None
    for key, want in grads.items():
        err = np.abs(np.asarray(got[key], dtype=gr.LD) - want)
        bound = RULE * mags[key]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
        a = int(np.argmax(ratio))
        if float(ratio[a]) >= worst:
            worst, where = float(ratio[a]), (key, a)
    return worst, where


def lds_of(ck, zd):
    used = gr.slots_used(ck.kspec, zd)
    return used, gr.rows_lds_doubles(ck.dz, zd, len(used))


def check(hip, case, what, zd=None, ws_doubles=None, rows=None):
    """One call through the raw entry into a sentinel-filled buffer with a padded `ldo`: padding untouched, unused raw slots exactly 0,
    every natural parameter within the rule.  Returns (raw rows, worst ratio, ck, the features)."""
    ck, z1, zd1, z2, zd2, v = feats = features(hip, case, zd)
    grads, mags = case[6], case[7]
    if rows is not None:
        z1, zd1 = z1[rows], (None if zd1 is None else zd1[rows])
        grads, mags = {k: g[rows] for k, g in grads.items()}, {k: s[rows] for k, s in mags.items()}
    _, buf = tl._rows(hip, ck, z1, zd1, z2, zd2, v, ws_doubles=ws_doubles)
    nacc = gr.GRAD_NACC
    assert np.all(buf[:, nacc:] == SENTINEL), what
    raw = buf[:, :nacc]
    used, doubles = lds_of(ck, zd1 is not None)
    assert doubles <= gr.LDS_160K
    unused = [s for s in range(nacc) if s not in used]
    assert np.all(raw[:, unused] == 0.0) and np.all(np.isfinite(raw)), what
    ratio, where = worst_ratio(natural(hip, ck, raw), grads, mags)
    print(f"grad_rows_limits: {what}: {len(used)} slots, {doubles} doubles, large LDS {'yes' if doubles > gr.LDS_48K else 'no'}, "
          f"worst err / (1e-11 S) = {ratio:.3e} at {where}")
    assert ratio <= 1.0, (what, ratio, where)
    return raw, ratio, ck, feats


@pytest.mark.parametrize("i", range(len(EDGE_CASES)))
def test_rows_on_both_sides_of_every_lds_edge_against_the_restatement(hip, i):
    name, dz = EDGE_CASES[i]
    n1, n2 = sizes(i)
    check(hip, reference(name, dz, n1, n2), f"{name} dz={dz} n1={n1} n2={n2}")


@pytest.mark.parametrize("name,dz,zd", REFUSED_CASES)
def test_a_structure_over_the_lds_limit_is_an_argument_error_that_touches_nothing(hip, name, dz, zd):
    """GPAR_ARG_ERROR(10) = -1010 at the first dz past each 160 KB edge; `out` and the workspace stay as they were."""
    from gpar_amd import _lib, hip as hipmod

    lib = _lib.load()
    n1, n2 = 5, 64
    kernel, width, x1, x2, v = inputs(name, dz, n1, n2)
    case = (kernel, width, x1, x2, v, lim.spec_of(kernel))
    ck, z1, zd1, z2, zd2, vt = features(hip, case, zd)
    assert (zd1 is not None) == zd
    used, doubles = lds_of(ck, zd)
    assert doubles > gr.LDS_160K
    nws = int(lib.gpar_workspace_doubles(_lib.WS_GRAM_GRAD_ROWS, n2, n1, 0))
    ws = torch.full((nws,), SENTINEL, dtype=torch.float64, device=hip.device)
    out = torch.full((n1, gr.GRAD_NACC + 3), SENTINEL, dtype=torch.float64, device=hip.device)
    rc = lib.gpar_gram_grad_rows(ctypes.byref(ck.kspec), z1.data_ptr(), None if zd1 is None else zd1.data_ptr(), n1, tl._ld(z1), z2.data_ptr(),
                                 None if zd2 is None else zd2.data_ptr(), n2, tl._ld(z2), ck.dz, vt.data_ptr(), out.data_ptr(), gr.GRAD_NACC + 3,
                                 ws.data_ptr(), nws, hipmod.stream_ptr(hip.device))
    assert rc == -1010
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())
    print(f"grad_rows_limits: {name} dz={dz}{' zd' if zd else ''}: {len(used)} slots, {doubles} doubles, refused")
    with pytest.raises(_lib.HipLibraryError, match="gpar_gram_grad_rows failed with status -1010.*160 KiB of LDS"):
        hipmod.gram_grad_rows(ck, z1, z2, vt, zd1=zd1, zd2=zd2)


@pytest.mark.parametrize("name,dz", SHARED_CASES)
def test_rows_of_x2_among_x1_at_width(hip, name, dz):
    """r = 0 pairs in the first 40 rows: everything finite (asserted in `check`), the rule as everywhere."""
    case = reference(name, dz, 65, 130, 40)
    assert np.array_equal(case[2][:40], case[3][:40])
    check(hip, case, f"{name} dz={dz} shared=40")


def test_splits_between_one_and_all_above_48k(hip):
    """wide_periodic at dz 16 (6638 doubles), n1 = 5, n2 = 300 (five column tiles): the recommended workspace gives five splits, one of
    exactly 2 n1 GRAD_NACC doubles two (split 0 walks tiles 0, 2, 4), the least one.  All within the rule; the same bits twice."""
    from gpar_amd import _lib

    name, dz = SPLIT_CASE
    n1, n2 = 5, 300
    case = reference(name, dz, n1, n2)
    recommended = int(_lib.load().gpar_workspace_doubles(_lib.WS_GRAM_GRAD_ROWS, n2, n1, 0))
    assert recommended == 5 * n1 * gr.GRAD_NACC
    for splits in (5, 2, 1):
        raw, _, ck, _ = check(hip, case, f"{name} dz={dz} n1={n1} n2={n2} splits={splits}", ws_doubles=splits * n1 * gr.GRAD_NACC)
        again = check(hip, case, f"{name} dz={dz} n1={n1} n2={n2} splits={splits} again", ws_doubles=splits * n1 * gr.GRAD_NACC)[0]
        assert np.array_equal(raw, again)
        assert lds_of(ck, True)[1] > gr.LDS_48K


def test_a_row_alone_has_the_bits_it_has_among_the_others_above_48k(hip):
    """n1 = 65 (rows 0 and 63 in the first row block, 64 alone in the second), n2 = 300, two splits in every call (a workspace of exactly
    two splits' partial sums): row a alone has the bits it has among the 65."""
    name, dz = SPLIT_CASE
    n1, n2 = 65, 300
    case = reference(name, dz, n1, n2)
    whole = check(hip, case, f"{name} dz={dz} n1={n1} n2={n2} splits=2", ws_doubles=2 * n1 * gr.GRAD_NACC)[0]
    for a in (0, 63, 64):
        alone = check(hip, case, f"{name} dz={dz} row {a} alone", ws_doubles=2 * gr.GRAD_NACC, rows=slice(a, a + 1))[0]
        assert np.array_equal(alone[0], whole[a]), a


@pytest.mark.parametrize("i", range(len(ZD_WITHOUT_PERIODS)))
def test_zd_given_to_a_structure_without_periodic_dims(hip, i):
    """include/gpar_hip.h: zd1 / zd2 both NULL or both given - the entry does not ask whether a dim is periodic.  Given zd (all zero: no
    feature depends on a frequency) every dim under a stationary factor gets a P slot, whose sums are exactly 0; the rest is within the
    rule.  wide_mixed at dz 30 is above 48 KB either way; twelve_rq at dz 47 is the widest the worst case fits with zd."""
    name, dz = ZD_WITHOUT_PERIODS[i]
    n1, n2 = sizes(i)
    case = reference(name, dz, n1, n2)
    assert not has_periods(case[5])
    raw, _, ck, feats = check(hip, case, f"{name} dz={dz} n1={n1} n2={n2} zd", zd=True)
    assert bool((feats[2] == 0.0).all()) and bool((feats[4] == 0.0).all())
    p0 = gr.MAX_TERMS + gr.MAX_FACTORS + gr.MAX_DIMS
    with_p = [s for s in gr.slots_used(ck.kspec, True) if s >= p0]
    assert len(with_p) == len(gr.slots_used(ck.kspec, True)) - len(gr.slots_used(ck.kspec, False)) > 0
    assert np.all(raw[:, p0:] == 0.0)
    plain = check(hip, case, f"{name} dz={dz} n1={n1} n2={n2}")[0]
    assert np.array_equal(raw, plain)   # (the same sums in the same order: the P slots add nothing to the others)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------------
def _jacobian_model():
    """A conditioned model of WIDE_MODELS["input_linear"]'s shape (40 input columns; layers of 80, 82, 84 feature dims) whose Jacobian a
    central difference can resolve to 1e-6 of every column (test_laplace_gpu.test_hyper_jacobian_against_central_differences has the
    error budget): complete data and replace=False, so that re-conditioning at shifted variables IS the difference with the training
    inputs held as given; outputs of amplitude 20, not normalised, for the linear term over the outputs (length scale 100); every
    output a function of every input column, and the linear term over the inputs at the length scale sqrt(m / 3) at which it is O(1)
    on [0, 1] (at the default 100 it weighs 1e-3 of the others and its 40 columns drown in the difference's rounding)."""
    from gpar_amd import GPARRegressor

    m, config, dims = lim.WIDE_MODELS["input_linear"]
    rng = np.random.default_rng(m)
    x = rng.uniform(0, 1, (lim.N, m))
    s = (x - 0.5) @ (rng.standard_normal((m, 3)) * np.sqrt(3.0 / m))
    y = 20.0 * (np.stack([np.sin(3 * s[:, 0]), np.cos(2 * s[:, 1]) * s[:, 0], s[:, 2] - s[:, 0] ** 2], axis=1) + 0.05 * rng.standard_normal((lim.N, 3)))
    xs = rng.uniform(0.05, 0.95, (lim.NS, m))
    reg = GPARRegressor(replace=False, normalise_y=False, noise=0.05, scale=0.5 * lim._ell(m), input_linear_scale=float(np.sqrt(m / 3.0)), **config)
    reg.condition(x, y)
    return reg, xs, dims


def test_wide_regressor_hyper_jacobian_against_central_differences(hip):
    """Layers of 80, 82, 84 feature dims without zd (16238 to 17038 doubles of LDS): the total Jacobian against central differences of
    the plug-in means, h = 1e-5 and 1e-6 of the column's largest magnitude, as test_hyper_jacobian_against_central_differences.  The
    layers have 260 variables between them and a column costs two re-conditionings of the model, so the columns compared are every
    scalar variable and the first, middle and last entry of every vector of 40 or more - every kind of variable of every layer."""
    from gpar_amd.regression import _construct_gpar
    from oracle import gpar_ref

    reg, xs, dims = _jacobian_model()
    objectives = reg._layer_chains()
    names = [n for obj in objectives for n in obj.names]
    u0 = reg.vs.get_vector(names)
    chains = [obj.chain_matrix(reg.vs.get_vector(obj.names)) for obj in objectives]
    gpar = _construct_gpar(reg, reg.vs, reg.m, reg.p) | (reg.x, reg.y, reg.w)
    jac = [to_np(J) for J in gpar.hyper_jacobian(hip.tensor(xs), chains)]
    m = xs.shape[1]   # (the layers' feature dims, read off the variables - which exist once the layers have been built)
    got = tuple(sum(len(f["scales"]) for t in gpar_ref.layer_spec(reg.get_variables(), m, i, reg.model_config)[0]["terms"] for f in t["factors"])
                for i in range(lim.P))
    assert got == dims, got
    P = u0.size
    assert all(J.shape == (lim.NS, P) for J in jac) and P == sum(obj.size for obj in objectives)
    columns, at = {}, 0
    for obj in objectives:
        for name, _, _, _, sl, _ in obj.layout:
            size = sl.stop - sl.start
            for j in sorted({0, size // 2, size - 1} if size >= 40 else set(range(size))):
                columns[at + sl.start + j] = f"{name}[{j}]"
        at += obj.size
    h = 1e-5
    fd = {k: np.zeros((lim.P, lim.NS)) for k in columns}
    for k in columns:
        for sign in (1.0, -1.0):
            u = u0.copy()
            u[k] += sign * h
            reg.vs.set_vector(u, names)
            fd[k] += sign * tl._plug_in_means(reg, xs).T / (2 * h)
    reg.vs.set_vector(u0, names)
    misses, worst = [], 0.0
    first = objectives[0].size
    for i in range(lim.P):
        for k, what in columns.items():
            scale, err = np.abs(fd[k][i]).max(), np.abs(jac[i][:, k] - fd[k][i]).max()
            if scale > 0:
                print(f"output {i} {what}: column magnitude {scale:.3e}, error {err:.3e}, relative {err / scale:.3e}")
                worst = max(worst, err / scale)
            if err > 1e-6 * scale:
                misses.append((i, what, float(scale), float(err)))
    print(f"grad_rows_limits: input_linear dz=80..84: {len(columns)} of {P} columns, worst column error {worst:.3e} of the column")
    assert not misses, misses
    assert np.abs(jac[2][:, :first]).max() > 0 and np.all(jac[0][:, first:] == 0.0)


def test_a_model_over_the_lds_limit_is_refused_by_name(hip):
    """WIDE_MODELS["per"] (92 to 94 feature dims with periodic dims: 4 x 92 x 68 doubles of tiles alone exceed 160 KB): the other posterior
    passes serve it, per-row gradient sums cannot.  `hyper_jacobian` and `predict_moments_hyper` raise, naming the entry and the limit;
    `predict_moments` goes on working."""
    from gpar_amd import _lib
    from gpar_amd.regression import _construct_gpar

    reg, _, _, xs, _ = lim._wide_model("per", True)
    objectives = reg._layer_chains()
    chains = [obj.chain_matrix(reg.vs.get_vector(obj.names)) for obj in objectives]
    size = sum(obj.size for obj in objectives)
    hp = _Hyper(names=tuple(n for obj in objectives for n in obj.names), cov=np.eye(size))
    message = "gpar_gram_grad_rows failed with status -1010.*160 KiB of LDS"
    gpar = _construct_gpar(reg, reg.vs, reg.m, reg.p) | (reg.x, reg.y, reg.w)
    with pytest.raises(_lib.HipLibraryError, match=message):
        gpar.hyper_jacobian(hip.tensor(xs), chains)
    result = None
    with pytest.raises(_lib.HipLibraryError, match=message):
        result = reg.predict_moments_hyper(xs, hp)
    assert result is None
    mean, var = reg.predict_moments(xs)
    assert mean.shape == var.shape == (lim.NS, lim.P) and np.all(np.isfinite(mean)) and np.all(var > 0)
    lim._assert_wide(reg, "per")   # (92, 93, 94 feature dims; the variables it reads exist once the layers have been built)


class _Hyper:
    """What `predict_moments_hyper` reads of a `laplace` result: the variables' names and their covariance."""

    def __init__(self, names, cov):
        self.names, self.cov = names, cov
