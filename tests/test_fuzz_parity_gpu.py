"""Seeded random differential test of the public API: HIP path (through the C ABI) against

  (1) `oracle.gpar_ref.gpar_logpdf` - the restatement that shares nothing with the product - for the prior log-density, and
  (2) the product's host algebra on the CPU oracle engine for posterior log-density and replace-mode predictions,

over randomly drawn model options (every kernel switch of gpar/regression.py:264-286, markov orders, tied scales, inducing
points with each approximation), ragged sizes (n = 2 .. 160, m = 1 .. 3, p = 1 .. 4), random missing patterns (including a
fully observed and a nearly empty output) and random weights.  The cases are fixed by their seeds; what the parametrised parity
tests cover by design, this covers by accident.

Seeds from MATERN_FIRST on are the same draws with `matern` = 0.5 / 1.5 / 2.5 set in addition (which excludes rq): the Matern
kernels under missing data, weights, markov orders, tied scales, the three inducing-point approximations, impute / replace and
posterior samples on the shared stream, at the tolerances of every other case.  tests/test_fuzz_cases.py (CPU) checks what the
block contains.  The tests print their error / tolerance ratios for these seeds (pytest -s).

Seeds from SPECTRAL_FIRST on are, again, the same draws, with `spectral` = 1 / 2 components set in addition (periods 0.5, 1.0 or the
pair (0.7, 0.31) against inputs in [0, 1]; every other seed a short envelope, `spectral_scale` = 0.8): the cosine factor under
everything the Matern block lists.  Three seeds of four force the EQ model beside the spectral terms; the fourth keeps a drawn
rq=True or else takes a Matern smoothness by seed, so that RQ and Matern factors are evaluated next to the cosine.  Q <= 2 always
fits the device's eight terms (1 + per + 2 input_linear + linear + nonlinear + Q)."""
import numpy as np
import pytest

from .conftest import make_engine, to_np

pytestmark = pytest.mark.gpu


MATERN_FIRST = 1000                                   # first seed of the Matern block (the seeds below it keep their cases)
MATERN_SEEDS = list(range(MATERN_FIRST, MATERN_FIRST + 48))
MATERN_GRADIENT_SEEDS = list(range(MATERN_FIRST + 100, MATERN_FIRST + 115))
MATERN_MID_SEEDS = list(range(MATERN_FIRST, MATERN_FIRST + 6))


SPECTRAL_FIRST = 2000                                 # first seed of the spectral block (the seeds below it keep their cases)
SPECTRAL_SEEDS = list(range(SPECTRAL_FIRST, SPECTRAL_FIRST + 36))
SPECTRAL_GRADIENT_SEEDS = list(range(SPECTRAL_FIRST + 100, SPECTRAL_FIRST + 112))
# (chosen: the numpy engine forms every derivative matrix explicitly, which takes minutes for dense `replace` at n = 2475 - seed 2001 - and
# at n = 1536 - seed 2006; these six hold both Q, inducing points with a periodic term, an RQ and a Matern factor beside the cosine)
SPECTRAL_MID_SEEDS = [SPECTRAL_FIRST + k for k in (0, 2, 3, 4, 5, 7)]


def _matern(seed):
    """Smoothness of a seed of the Matern block (each value every third seed), None below the block; in the spectral block the
    smoothness every fourth seed takes unless it drew rq=True, None for the others."""
    if seed >= SPECTRAL_FIRST:
        k = seed - SPECTRAL_FIRST
        return [0.5, 1.5, 2.5][(k // 4) % 3] if k % 4 == 3 else None
    return None if seed < MATERN_FIRST else [0.5, 1.5, 2.5][(seed - MATERN_FIRST) % 3]


def _spectral(seed):
    """The spectral keywords of a seed of the spectral block, None below it."""
    if seed < SPECTRAL_FIRST:
        return None
    k = seed - SPECTRAL_FIRST
    q = [1, 2][k % 2]
    period = [0.5, 1.0, (0.7, 0.31)][k % 3]
    out = dict(spectral=q, spectral_period=period if q == 2 or not isinstance(period, tuple) else 0.5)
    if (k // 2) % 2:   # every other pair of seeds (so that both Q meet it): an envelope that is not flat over [0, 1]
        out["spectral_scale"] = 0.8
    return out


def _block_kernel_switches(seed, kw):
    """`matern` / `rq` / `spectral*` of the seed's block, set into the drawn keywords (nothing is drawn for them: the stream is that
    of every other seed)."""
    if seed >= SPECTRAL_FIRST:
        if (seed - SPECTRAL_FIRST) % 4 != 3:
            kw["rq"] = False                       # the EQ model beside the spectral terms
        elif not kw["rq"]:
            kw["matern"] = _matern(seed)           # a drawn rq=True stays; else the Matern kernel of the seed
        kw.update(_spectral(seed))
    elif _matern(seed) is not None:
        kw["matern"], kw["rq"] = _matern(seed), False


def _report(label, seed, ratios, kw=None):
    if seed >= SPECTRAL_FIRST:
        sp = _spectral(seed)
        print(f"[spectral] {label} seed={seed} Q={sp['spectral']} T={sp['spectral_period']} matern={(kw or {}).get('matern')} "
              f"rq={(kw or {}).get('rq')}: error / tolerance = " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    elif seed >= MATERN_FIRST:
        print(f"[matern] {label} seed={seed} nu={_matern(seed)}: error / tolerance = " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))


def _case(seed):
    rng = np.random.default_rng(1000 + seed)
    n, m, p = int(rng.integers(2, 161)), int(rng.integers(1, 4)), int(rng.integers(1, 5))
    kw = dict(
        scale=float(rng.uniform(0.2, 1.5)), noise=float(rng.uniform(0.02, 0.5)), normalise_y=False,
        linear=bool(rng.integers(2)), nonlinear=bool(rng.integers(2)), input_linear=bool(rng.integers(2)), rq=bool(rng.integers(2)),
        per=bool(rng.integers(3) == 0), scale_tie=bool(rng.integers(4) == 0),
        markov=[None, None, 0, 1, 2][int(rng.integers(5))],
        impute=bool(rng.integers(2)), replace=bool(rng.integers(3) == 0),
    )
    _block_kernel_switches(seed, kw)   # (nothing is drawn for them: the stream below is that of every other seed)
    if kw["per"]:
        kw["per_period"] = float(rng.uniform(0.3, 1.2))
    if rng.integers(3) == 0 and n >= 6:
        kw["x_ind"] = rng.uniform(0, 1, (int(rng.integers(2, min(n, 14))), m))
        kw["sparse_method"] = ["vfe", "vfe", "fitc", "dtc"][int(rng.integers(4))]
    x = rng.uniform(0, 1, (n, m))
    cols = []
    for i in range(p):
        base = np.sin(2 * np.pi * (x @ rng.uniform(0.5, 1.5, m)) + i)
        if cols:
            base = base + 0.4 * cols[-1]
        cols.append(base + 0.1 * rng.standard_normal(n))
    y = np.stack(cols, axis=1)
    mode = int(rng.integers(4))
    if mode == 1:
        y[rng.random(y.shape) < 0.25] = np.nan
    elif mode == 2 and p > 1:
        j = int(rng.integers(p))
        y[rng.random(n) < 0.9, j] = np.nan      # a nearly empty output
        y[0, j] = 0.1
    elif mode == 3:
        y[rng.random(y.shape) < 0.1] = np.nan
        y[int(rng.integers(n))] = np.nan          # a row with nothing observed
    if np.isnan(y).all(axis=0).any():             # every output keeps at least one observation
        y[0] = 0.3
    w = None if rng.integers(2) else rng.uniform(0.5, 2.0, (n, p))
    xs = rng.uniform(0, 1, (int(rng.integers(1, 30)), m))
    return kw, x, y, w, xs


def _run(kind, kw, x, y, w, xs):
    from gpar_amd.engine import set_engine
    from gpar_amd.regression import GPARRegressor

    eng = make_engine(kind, seed=5)
    previous = set_engine(eng)
    try:
        reg = GPARRegressor(**kw)
        prior = float(reg.logpdf(x, y, w))
        reg.condition(x, y, w)
        post = float(reg.logpdf(x, y, w, posterior=True))
        # one latent posterior sample on the engines' shared Philox stream (same seed, same draws)
        sample = to_np(reg.sample(xs, num_samples=1, latent=True, posterior=True)[0])
        return prior, post, sample, reg.get_variables(), reg.model_config
    finally:
        set_engine(previous)


@pytest.mark.parametrize("seed", [-s - 1 for s in range(24)] + list(range(96)) + MATERN_SEEDS + [-s - 1 for s in MATERN_SEEDS[:12]]
                         + SPECTRAL_SEEDS + [-s - 1 for s in SPECTRAL_SEEDS[:8]])
def test_random_configuration(seed, monkeypatch):
    """(negative seeds: case -seed - 1 once more with GPAR_HOST_MASKS=0 - boolean device masks computed layer by layer, the
    path every engine but the HIP one still takes - so that both ways through the missing-data bookkeeping stay covered)"""
    from oracle import gpar_ref

    if seed < 0:
        monkeypatch.setenv("GPAR_HOST_MASKS", "0")
        seed = -seed - 1
    kw, x, y, w, xs = _case(seed)
    sparse = "x_ind" in kw
    prior, post, sample, hypers, config = _run("hip", kw, x, y, w, xs)
    o_prior, o_post, o_sample, _, _ = _run("oracle", kw, x, y, w, xs)
    # inducing-point chains go through K_zz^-1 with a 1e-12 jitter: conditioning-limited, everything else to rounding
    tol = 1e-6 if sparse else 1e-9
    scale = max(abs(o_prior), 1.0)
    ratios = {"prior": abs(prior - o_prior) / (tol * scale), "posterior": abs(post - o_post) / (tol * max(abs(o_post), 1.0)),
              "sample": float(np.max(np.abs(sample - o_sample))) / ((1e-4 if sparse else 1e-7) * max(1.0, np.abs(o_sample).max()))}
    want = None
    if kw.get("sparse_method", "vfe") == "vfe":   # the independent restatement implements the reference's default approximation
        want = gpar_ref.gpar_logpdf(x, y, w, hypers, config, impute=kw["impute"], replace=kw["replace"], x_ind=kw.get("x_ind"))
        ratios["restatement"] = abs(prior - want) / (tol * max(abs(want), 1.0))
    _report("fuzz", seed, ratios, kw)
    assert config.get("matern") == kw.get("matern") and (seed >= SPECTRAL_FIRST or kw.get("matern") == _matern(seed))
    assert config.get("spectral") == kw.get("spectral") == (_spectral(seed) or {}).get("spectral")
    assert abs(prior - o_prior) <= tol * scale, (kw, prior, o_prior)
    assert abs(post - o_post) <= tol * max(abs(o_post), 1.0), (kw, post, o_post)
    np.testing.assert_allclose(sample, o_sample, rtol=0, atol=(1e-4 if sparse else 1e-7) * max(1.0, np.abs(o_sample).max()))
    if want is not None:
        assert abs(prior - want) <= tol * max(abs(want), 1.0), (kw, prior, want)


def _grads(kind, kw, x, y, w):
    import torch

    from gpar_amd.engine import set_engine
    from gpar_amd.regression import GPARRegressor

    eng = make_engine(kind, seed=5)
    previous = set_engine(eng)
    try:
        reg = GPARRegressor(**kw)
        with torch.no_grad():
            reg.logpdf(x, y, w)
        reg.vs.requires_grad(True)
        args = [torch.tensor(x), torch.tensor(y)] + ([] if w is None else [torch.tensor(w)])
        value = reg.logpdf(*args)
        value.backward()
        names = [v for v in reg.vs.get_vars()]
        return float(value.detach()), np.concatenate([(v.grad if v.grad is not None else torch.zeros_like(v)).numpy().reshape(-1) for v in names])
    finally:
        set_engine(previous)


def _gradient_ratios(sparse, value, o_value, got, ref):
    big = max(np.max(np.abs(ref)), 1e-3)
    rtol, atol = (1e-4, 1e-5 * big) if sparse else (1e-6, 1e-7 * big)
    return {"value": abs(value - o_value) / ((1e-6 if sparse else 1e-9) * max(abs(o_value), 1.0)),
            "gradient": float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref))))}


@pytest.mark.parametrize("seed", list(range(32)) + MATERN_GRADIENT_SEEDS + SPECTRAL_GRADIENT_SEEDS)
def test_random_configuration_gradient(seed):
    """d logpdf / d(every hyper-parameter) - the joint objective of fit(fix=False), through imputed / replaced columns and
    extended inducing inputs where the drawn configuration has them - HIP kernels against the numpy engine."""
    kw, x, y, w, _ = _case(seed if seed >= MATERN_FIRST else 200 + seed)   # (the Matern block's seeds are taken as they are)
    sparse = "x_ind" in kw
    value, got = _grads("hip", kw, x, y, w)
    o_value, ref = _grads("oracle", kw, x, y, w)
    _report("fuzz gradient", seed, _gradient_ratios(sparse, value, o_value, got, ref), kw)
    assert abs(value - o_value) <= (1e-6 if sparse else 1e-9) * max(abs(o_value), 1.0)
    big = max(np.max(np.abs(ref)), 1e-3)
    np.testing.assert_allclose(got, ref, rtol=1e-4 if sparse else 1e-6, atol=(1e-5 if sparse else 1e-7) * big, err_msg=str(kw))


def _mid_case(seed):
    """Sizes at which the blocked device paths run: fused 512-column panels, look-ahead, the recursive inverse (n a multiple of
    512) and its fallback (ragged n after missing rows are dropped), generated kernels (the session's thresholds), M up to 320."""
    rng = np.random.default_rng(5000 + seed)
    n = int(rng.choice([1024, 1536, 2048, int(rng.integers(600, 2600))]))
    m, p = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    kw = dict(scale=float(rng.uniform(0.3, 1.0)), noise=float(rng.uniform(0.05, 0.3)), normalise_y=False, linear=True,
              nonlinear=bool(rng.integers(2)), rq=bool(rng.integers(2)), per=bool(rng.integers(4) == 0),
              markov=[None, 1, 2][int(rng.integers(3))], impute=bool(rng.integers(2)), replace=bool(rng.integers(4) == 0))
    _block_kernel_switches(seed, kw)
    if rng.integers(3) == 0:
        kw["x_ind"] = rng.uniform(0, 1, (int(rng.integers(40, 321)), m))
    x = rng.uniform(0, 1, (n, m))
    cols = []
    for i in range(p):
        base = np.sin(2 * np.pi * (x @ rng.uniform(0.5, 1.5, m)) + i)
        if cols:
            base = base + 0.4 * cols[-1]
        cols.append(base + 0.1 * rng.standard_normal(n))
    y = np.stack(cols, axis=1)
    if rng.integers(2):
        y[rng.random(y.shape) < 0.07] = np.nan
        y[0] = 0.2
    w = None if rng.integers(2) else rng.uniform(0.5, 2.0, (n, p))
    return kw, x, y, w


@pytest.mark.parametrize("seed", list(range(20)) + MATERN_MID_SEEDS + SPECTRAL_MID_SEEDS)
def test_random_configuration_at_blocked_sizes(seed):
    kw, x, y, w = _mid_case(seed)
    sparse = "x_ind" in kw
    value, got = _grads("hip", kw, x, y, w)
    o_value, ref = _grads("oracle", kw, x, y, w)
    _report("fuzz blocked sizes", seed, _gradient_ratios(sparse, value, o_value, got, ref), kw)
    assert abs(value - o_value) <= (1e-6 if sparse else 1e-9) * max(abs(o_value), 1.0), (kw, value, o_value)
    big = max(np.max(np.abs(ref)), 1e-3)
    np.testing.assert_allclose(got, ref, rtol=1e-4 if sparse else 1e-6, atol=(1e-5 if sparse else 1e-7) * big, err_msg=str(kw))


@pytest.mark.parametrize("seed", range(10))
@pytest.mark.parametrize("mode", ["joint", "marginal", "replace"])
def test_inducing_point_posterior_sampling_in_batches(seed, mode):
    """Several ancestral samples through inducing-point posteriors: from the second layer on every sample has a design matrix of its
    own, and the HIP engine draws all of them through ONE stacked cross-Gram, two triangular solves, batched rank-M corrections and
    a lock-step factorisation (gp.PseudoObs.posterior_sample_batch / posterior_marginals_batch / posterior_mean_batch) where the
    numpy engine goes sample by sample - same Philox stream, same values."""
    from gpar_amd.engine import set_engine
    from gpar_amd.regression import GPARRegressor

    rng = np.random.default_rng(800 + seed)
    n, m, p, ns, S = int(rng.integers(60, 400)), int(rng.integers(1, 3)), int(rng.integers(2, 4)), int(rng.integers(20, 200)), int(rng.integers(2, 6))
    x = rng.uniform(0, 1, (n, m))
    y = np.stack([np.sin(3 * x[:, 0] + i) + 0.1 * rng.standard_normal(n) for i in range(p)], axis=1)
    xs = rng.uniform(0, 1, (ns, m))
    kw = dict(scale=0.5, linear=True, nonlinear=bool(rng.integers(2)), rq=bool(rng.integers(2)), noise=0.1, normalise_y=False,
              x_ind=rng.uniform(0, 1, (int(rng.integers(8, 40)), m)), sparse_method=["vfe", "fitc", "dtc"][seed % 3], replace=mode == "replace")

    def run(kind):
        previous = set_engine(make_engine(kind, seed=9))
        try:
            reg = GPARRegressor(**kw)
            reg.condition(x, y)
            if mode == "marginal":
                mean, lo, hi = reg.predict(xs, num_samples=S, credible_bounds=True, marginal=True)
                return np.stack([to_np(mean), to_np(lo), to_np(hi)])
            return np.stack([to_np(s_) for s_ in reg.sample(xs, num_samples=S, posterior=True)])
        finally:
            set_engine(previous)

    got, ref = run("hip"), run("oracle")
    # (inducing-point chains go through K_zz^-1 with a 1e-12 jitter: agreement to its conditioning, as everywhere in this file)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-4 * max(1.0, np.abs(ref).max()))


@pytest.mark.parametrize("seed", [507, 516])
def test_inducing_matrix_at_the_edge_of_definiteness(seed):
    """Two cases of the extended sweep (tools/fuzz_more.py, same generator): 216 / 330 inducing inputs on one axis, K_zz + 1e-12 with
    its smallest eigenvalue at 9e-13 against |K| = 440 - the size of any Cholesky's backward error.  numpy's factorisation gets through
    both, the fused panel path through neither (pivots 148 / 193; tools/r04_marginal_potrf.py has the statistics): the non-positive
    pivot is confirmed on the unfused path before it is reported (model._retry_unfused), and the value agrees with the numpy engine to
    the conditioning of K_zz (measured: 9e-9 / 1.6e-7).  The gradient goes through K_zz^-1 once more: at eps * cond(K_zz) ~ 0.05 two
    correct evaluations share one to two digits (measured 2.5e-2 / 6.6e-2 of the largest component), which is all that is asked."""
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("fuzz_more", os.path.join(os.path.dirname(os.path.dirname(__file__)), "tools", "fuzz_more.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    kw, x, y, w, _ = module.case(seed)
    hv, hg = _grads("hip", kw, x, y, w)
    ov, og = _grads("oracle", kw, x, y, w)
    assert abs(hv - ov) <= 1e-5 * abs(ov), (hv, ov)
    assert np.all(np.isfinite(hg)) and np.max(np.abs(hg - og)) <= 0.25 * np.max(np.abs(og)), (hg, og)
