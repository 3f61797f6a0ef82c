"""The generated (per-structure) Gram and gradient kernels - csrc/gram_jit.h, csrc/grad_jit.h - at the edges of their own geometry.

Every Gram build, parameter-gradient pass and input-gradient pass exists twice: the interpreter of csrc/gram.h and the kernel generated
for a layer's structure, which is what runs from n ~ 725 on (archive) or 2^24 / 2^26 entries on (hiprtc).  Here both are driven through
the C ABI at small sizes (`GPAR_GRAM_JIT_MIN_ENTRIES` / `GPAR_GRAD_JIT_MIN_ENTRIES` = -1: interpreter, 0: generated) on operands whose
storage the test lays out itself, so that nothing is re-packed or re-aligned on the way:

* Gram: the strip walk of the narrow kernel (`GPAR_GRAM_JIT_STRIP` forces 1 / 2 / 4 / 8 column tiles per workgroup; the launch clamps it
  to the structure's limit and the wide kernel ignores it) against the interpreter, BIT FOR BIT, over the whole output buffer - padding,
  tail and, in lower builds, the tiles above the diagonal included: a skipped tile, one written twice by neighbouring strips, a store
  past n2 or above the diagonal shows as a changed word.  The cross builds are also compared with the numpy oracle.
* Parameter-gradient passes (gpar_gram_grad, gpar_gram_grad_cross SYM / RECT) and the input-gradient pass (RECT / SYM): 1 .. 130 rows,
  every relation of `nblocks` / `nsplit` to the tile counts, weights whose strict upper triangle (symmetric modes) and padding hold NaN,
  against the interpreter (1e-11 of the largest sum / entry) and the numpy oracle (the tolerances of tests/test_hip_primitives.py).

Storage variants (`_VARIANTS`): "tight" (ld = columns: odd where the column count is odd), "even" (padded, even ld, 16-byte aligned base),
"odd" (padded, odd ld), "offset" (even ld, base moved by one double: 8-byte aligned only).  The 16-byte vector stores of the Gram
kernels and the 16-byte weight loads of the gradient kernels (`vec` / `vecw`) are taken by "even" (and by "tight" at an even column
count); "odd", "offset" and "tight" at an odd column count take the SCALAR store / weight-load paths of all three kernel families - for
the wide Gram kernel its 4-entry scalar path, and at the ragged last column tile the scalar tail of a vector build.

What this file cannot see: a hipModuleLaunchKernel that FAILS makes the launch fall back to the interpreter silently - no counter moves,
and for the Gram kernel the bits are the same by design.  The guards that exist: the failure count of gpar_jit_stats must not move and
the cache must hold the structure after a generated run; and for the gradient kernels, whose sums are formed in another order than the
interpreter's, the number of cases that differ from the interpreter in at least one bit is counted - none differing means the generated
kernel did not run, and is reported as a failure of the test's premise."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

#: (name, GPARRegressor keywords, m, layer), built as tests/test_hip_primitives.py::_jit_cases builds its own.  Feature dims / role:
#: 8 (strip limit 8, three terms) | 12, periodic + RQ (strip limit 4; HAS_ZD gradient kernels) | 23 (the wide Gram kernel; no generated
#: input-gradient kernel) | 7 with two EQ x cosine terms | 10, Matern 1/2 + linear + constant term (strip limit 4) | 0 (no inputs and
#: markov=0: every factor over zero columns, DZ_LOAD == 0).
STRUCTURES = [
    ("eq-lin-eq", dict(scale=0.5, linear=True, nonlinear=True, markov=2), 4, 7),
    ("per-rq", dict(scale=0.5, per=True, rq=True, linear=True, nonlinear=True), 2, 2),
    ("matern52-wide", dict(scale=0.5, linear=True, nonlinear=True, matern=2.5), 1, 11),
    ("spectral2-lin", dict(spectral=2, linear=True), 1, 2),
    ("matern12-inputlinear-const", dict(scale=0.7, input_linear=True, linear=True, nonlinear=True, matern=0.5), 2, 3),
    ("markov0-no-inputs", dict(linear=True, nonlinear=True, markov=0), 0, 2),
]
_DIMS = {"eq-lin-eq": 8, "per-rq": 12, "matern52-wide": 23, "spectral2-lin": 7, "matern12-inputlinear-const": 10, "markov0-no-inputs": 0}
_NAMES = [s[0] for s in STRUCTURES]

SENTINEL = -7.25          # finite, and no kernel value: what every output buffer holds before a launch
TAIL = 9                  # doubles behind the last row of every buffer
STRIPS = (1, 2, 4, 8)
_VARIANTS = ("tight", "even", "odd", "offset")


@functools.lru_cache(maxsize=None)
def structures():
    """[(name, kernel, width)] of STRUCTURES (host-side model objects only: needs no GPU)."""
    from gpar_amd.engine import set_engine
    from gpar_amd.regression import GPARRegressor, _construct_gpar
    from oracle.engine import OracleEngine

    previous = set_engine(OracleEngine())   # (only to instantiate the hyper-parameters of the host-side model objects)
    try:
        out = []
        for name, kw, m, layer in STRUCTURES:
            reg = GPARRegressor(**kw)
            f, _ = _construct_gpar(reg, reg.vs, m, layer + 1).layers[layer]()
            out.append((name, f.kernel, m + layer))
        return out
    finally:
        set_engine(previous)


class _Gpu:
    def __init__(self):
        import torch

        from gpar_amd import _lib
        from gpar_amd import hip as H

        assert torch.cuda.is_available()
        self.torch, self.H, self._lib = torch, H, _lib
        self.dev = torch.device("cuda:0")
        self.lib = _lib.load()
        self.stream = H.stream_ptr(self.dev)

    def stats(self):
        """(compiled, failures, cached) of gpar_jit_stats."""
        cs = [ctypes.c_int(), ctypes.c_int(), ctypes.c_int()]
        assert self.lib.gpar_jit_stats(*[ctypes.byref(c) for c in cs]) == 0
        return tuple(c.value for c in cs)

    def assert_cached(self, ck, kinds, what):
        """The generated kernels of `kinds` (include/gpar_hip.h: 0 Gram; 1 / 11 parameter gradients SYM / RECT, + 20 with frequency
        derivatives; 2 / 12 input gradients SYM / RECT) are in the cache for THIS structure: gpar_jit_prepare finds them ready and neither
        compiles nor loads anything."""
        for kind in kinds:
            before = self.stats()
            assert self.lib.gpar_jit_prepare(kind, ctypes.byref(ck.kspec), ck.dz, self.stream) == 0, (what, kind)
            assert self.stats() == before, (what, kind, "the generated runs left no kernel of this kind in the cache: they did not use one")

    def upload(self, a):
        return self.torch.tensor(np.ascontiguousarray(a), dtype=self.torch.float64, device=self.dev)

    def filled(self, count, value=SENTINEL):
        buf = self.torch.full((count,), value, dtype=self.torch.float64, device=self.dev)
        assert buf.data_ptr() % 16 == 0
        return buf

    def compiled_kernel(self, case):
        from gpar_amd.kernels import compile_kernel

        name, kernel, width = structures()[case]
        ck = compile_kernel(kernel, width)
        assert ck.dz == _DIMS[name], (name, ck.dz)
        return name, kernel, width, ck

    def features(self, ck, x):
        """(z, zd or None): features of the rows of x and, for periodic structures, their frequency derivatives (one leading dimension)."""
        xd = self.upload(x)
        z = self.H.featurize(ck, xd)
        periodic = any(f.periods is not None for t in ck.kernel.terms for f in t.factors)
        zd = self.H.featurize_dfreq(ck, xd) if periodic else None
        assert zd is None or int(zd.stride(0)) == int(z.stride(0))
        return z, zd


@pytest.fixture(scope="module")
def gpu():
    return _Gpu()


def _layout(cols, variant):
    """(leading dimension, offset of the base in doubles) of a matrix with `cols` columns in storage `variant`."""
    even = cols + 2 + (cols & 1)
    return {"tight": (cols, 0), "even": (even, 0), "odd": (even + 1, 0), "offset": (even, 1)}[variant]


def _positions(off, rows, cols, ld, keep=None):
    """Flat indices of the entries (r, c) of a rows x cols matrix at offset `off` with leading dimension `ld` (where `keep` holds)."""
    idx = off + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]
    return idx.reshape(-1) if keep is None else idx[keep]


def _lower_tiles(n):
    """Entries of the 64 x 64 tiles on and below the diagonal tiles: what a lower build writes."""
    t = np.arange(n) // 64
    return t[None, :] <= t[:, None]


def _ptr(buf, off=0):
    return buf.data_ptr() + 8 * off


def _ratio(got, ref, rtol, atol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref)))) if ref.size else 0.0


# ---- 1. Gram: forced strips against the interpreter, bit for bit ------------------------------------------------------------------------
#: lower-triangular builds: 130 - 3 tile rows (strip 8: full = 0, rest = 3); 300 - 5 (strip 2: full = 2, rest = 1); 513 - 9 (strip 4:
#: full = 2, rest = 1; strip 8: full = 1, rest = 1); 674 - 11 (rest = 3 at strips 4 and 8; last tile of 34 rows)
SYM_N = (1, 2, 63, 64, 65, 130, 300, 513, 674)
CROSS = ((130, 674), (674, 65), (1, 600), (65, 1), (64, 64))
BATCH, BATCH_N = 3, 130


def _gram_jobs(g, case):
    """The launches of one structure: [(label, launch(buffer), buffer doubles, flat indices the build must write, oracle or None, rows x
    cols view parameters)].  Two storage variants per case - one of ("tight", "odd"), one of ("even", "offset") - cycling over the cases."""
    from oracle import kernels as ok

    name, kernel, width, ck = g.compiled_kernel(case)
    rng = np.random.default_rng(100 + case)
    X1, X2 = rng.standard_normal((max(SYM_N), width)), rng.standard_normal((max(SYM_N), width))
    noise, rs = rng.uniform(0.01, 1.0, max(SYM_N)), rng.uniform(0.5, 1.5, max(SYM_N))
    z1, _ = g.features(ck, X1)
    z2, _ = g.features(ck, X2)
    ldz = int(z1.stride(0))
    assert int(z2.stride(0)) == ldz and z1.data_ptr() != z2.data_ptr()
    noise_d, rs_d = g.upload(noise), g.upload(rs)
    spec = ok.spec_to_dict(kernel.resolve(width))
    ks = ctypes.byref(ck.kspec)
    keep = [z1, z2, noise_d, rs_d, ck]
    jobs = []

    def variants(i):
        return (_VARIANTS[2 * (i & 1)], _VARIANTS[1 + 2 * ((i >> 1) & 1)])   # (tight | odd, even | offset)

    for i, n in enumerate(SYM_N):
        for variant in variants(i + case):
            ld, off = _layout(n, variant)

            def launch(buf, n=n, ld=ld, off=off):
                return g.lib.gpar_gram(ks, z1.data_ptr(), n, ldz, z1.data_ptr(), n, ldz, ck.dz, _ptr(buf, off), ld, g._lib.GRAM_LOWER,
                                       noise_d.data_ptr(), 1e-12, None, g.stream)

            jobs.append((f"sym n={n} {variant}", launch, off + n * ld + TAIL, _positions(off, n, n, ld, _lower_tiles(n)), None, None))
    for i, (n1, n2) in enumerate(CROSS):
        want = ok.gram(spec, X1[:n1], X2[:n2]) * rs[:n1, None]
        for variant in variants(i + case + 1):
            ld, off = _layout(n2, variant)

            def launch(buf, n1=n1, n2=n2, ld=ld, off=off):
                return g.lib.gpar_gram(ks, z1.data_ptr(), n1, ldz, z2.data_ptr(), n2, ldz, ck.dz, _ptr(buf, off), ld, 0, None, 0.0,
                                       rs_d.data_ptr(), g.stream)

            jobs.append((f"cross {n1}x{n2} {variant}", launch, off + n1 * ld + TAIL, _positions(off, n1, n2, ld), want, (off, n1, n2, ld)))
    # batch: three members whose strides carry padding - the odd output stride puts member 1 on an 8-byte-only aligned base (scalar
    # stores) between two members on the vector path; the gaps between the members are part of the compared buffer
    n = BATCH_N
    stride_z = n * ldz + 5
    zb = g.filled(BATCH * stride_z + TAIL, 0.0)
    for b in range(BATCH):
        zb[b * stride_z : b * stride_z + n * ldz].view(n, ldz)[:, : max(ck.dz, 1)] = z1[b * n : (b + 1) * n]
    keep.append(zb)
    ld, off = _layout(n, "even")
    stride_k = n * ld + 7
    written = np.concatenate([_positions(off + b * stride_k, n, n, ld, _lower_tiles(n)) for b in range(BATCH)])

    def launch_batch(buf):
        return g.lib.gpar_gram_batch(ks, zb.data_ptr(), n, ldz, stride_z, ck.dz, _ptr(buf, off), ld, stride_k, g._lib.GRAM_LOWER, None, 0.1,
                                     BATCH, g.stream)

    jobs.append((f"batch {BATCH}x{n}", launch_batch, off + BATCH * stride_k + TAIL, written, None, None))
    return name, ck, jobs, keep


@pytest.mark.parametrize("case", range(len(STRUCTURES)), ids=_NAMES)
def test_gram_strips_write_the_interpreters_bits_and_nothing_else(gpu, case, monkeypatch):
    """Symmetric lower builds with noise diagonal and jitter, cross builds with row scaling and a batch, at strips 1 / 2 / 4 / 8 (the
    batch at 2 and 8): the whole buffer of every generated run equals the interpreter's in bits; padding, tail, gaps between batch
    members and - in lower builds - every tile above the diagonal tiles keep their sentinel; the cross builds agree with the numpy
    oracle at rtol 1e-13 / atol 1e-15 (tests/test_hip_primitives.py::test_generated_gram_kernel_is_bit_identical_to_the_interpreter)."""
    g, torch = gpu, gpu.torch
    name, ck, jobs, keep = _gram_jobs(g, case)
    monkeypatch.delenv("GPAR_GRAM_JIT_STRIP", raising=False)

    def run(launch, count):
        buf = g.filled(count)
        assert launch(buf) == 0
        return buf

    monkeypatch.setenv("GPAR_GRAM_JIT_MIN_ENTRIES", "-1")   # never: the interpreter
    refs = [run(launch, count) for _, launch, count, _, _, _ in jobs]
    torch.cuda.synchronize()
    for (label, _, count, written, _, _), ref in zip(jobs, refs):
        flat = ref.cpu().numpy()
        mask = np.zeros(count, dtype=bool)
        mask[written] = True
        assert (flat[~mask] == SENTINEL).all(), (name, label, "the interpreter wrote outside the matrix")
        assert (flat[mask] != SENTINEL).all() and np.isfinite(flat[mask]).all(), (name, label, "the interpreter left entries unwritten")
    before = g.stats()
    monkeypatch.setenv("GPAR_GRAM_JIT_MIN_ENTRIES", "0")    # always: the generated kernel
    worst = 0.0
    for strip in STRIPS:
        monkeypatch.setenv("GPAR_GRAM_JIT_STRIP", str(strip))   # (clamped to the structure's limit; the wide kernel takes one tile whatever it says)
        for (label, launch, count, written, want, view), ref in zip(jobs, refs):
            if label.startswith("batch") and strip not in (2, 8):
                continue
            got = run(launch, count)
            if not torch.equal(got, ref):
                bad = torch.nonzero(got != ref).reshape(-1).cpu().numpy()
                inside = np.isin(bad, written)
                raise AssertionError(f"{name} {label} strip {strip}: {bad.size} words differ from the interpreter's buffer ({int((~inside).sum())} of them "
                                     f"outside the matrix), first at flat index {int(bad[0])}")
            if want is not None:
                off, n1, n2, ld = view
                mat = got[off : off + n1 * ld].cpu().numpy().reshape(n1, ld)[:, :n2]
                worst = max(worst, _ratio(mat, want, 1e-13, 1e-15))
                np.testing.assert_allclose(mat, want, rtol=1e-13, atol=1e-15, err_msg=f"{name} {label} strip {strip}")
    after = g.stats()
    assert after[1] == before[1], "a generated Gram kernel failed to compile"
    assert after[2] >= 1, "no generated kernel is cached after the generated runs"
    g.assert_cached(ck, [0], name)
    print(f"[generated gram] {name}: worst error / tolerance against the oracle = {worst:.3g}")


# ---- 2. / 3. gradient passes --------------------------------------------------------------------------------------------------------------
GRAD_N = (1, 2, 63, 64, 65, 129, 130)
#: rectangular weights: every n with a smaller (or, at 1, an equal) and a larger (at 130: an equal) n2
RECT_N2 = {1: (1, 7), 2: (1, 7), 63: (7, 64), 64: (7, 65), 65: (64, 130), 129: (65, 130), 130: (64, 130)}
GRAD_MAX = 130


def _tiles(n):
    return (n + 63) // 64


def _block_counts(ntiles):
    """nblocks: 1, the tile count, a value in between that does not divide it (where there is one), and one workgroup more than tiles."""
    between = [k for k in range(2, ntiles) if ntiles % k]
    return sorted({1, ntiles, ntiles + 1} | set(between[-1:]))


def _weights(g, W, variant, lower):
    """Device copy of the weights W in storage `variant`: NaN in the padding, before the base, behind the last row and - `lower`: a
    symmetric matrix given by its lower triangle - in the strict upper triangle: none of it may be read."""
    rows, cols = W.shape
    ld, off = _layout(cols, variant)
    host = np.full(off + rows * ld + TAIL, np.nan)
    keep = np.tril(np.ones((rows, cols), dtype=bool)) if lower else np.ones((rows, cols), dtype=bool)
    host[_positions(off, rows, cols, ld, keep)] = W[keep]
    buf = g.upload(host)
    assert buf.data_ptr() % 16 == 0
    return buf, _ptr(buf, off), ld


def _check_parameter_gradients(got, ref, scale, what):
    """The assertions of tests/test_hip_primitives.py::test_kernel_gradients_match_oracle (and of the cross passes' test): coefficients to
    1e-12 of the summed weights, scales / periods / alphas at rtol 1e-10, atol 1e-12 of the summed weights.  Returns the worst ratio."""
    worst = 0.0
    for t in range(len(ref["coef"])):
        worst = max(worst, abs(got["coef"][t] - ref["coef"][t]) / (1e-12 * scale))
        assert abs(got["coef"][t] - ref["coef"][t]) <= 1e-12 * scale, (what, "coef", t)
        for fi, (gf, rf) in enumerate(zip(got["factors"][t], ref["factors"][t])):
            for key in ("scales", "periods", "alpha"):
                if rf[key] is None:
                    continue
                worst = max(worst, _ratio(gf[key], rf[key], 1e-10, 1e-12 * scale))
                assert np.allclose(gf[key], rf[key], rtol=1e-10, atol=1e-12 * scale), (what, key, t, fi)
    return worst


@pytest.mark.parametrize("case", range(len(STRUCTURES)), ids=_NAMES)
def test_parameter_gradient_passes_at_every_size_and_weight_storage(gpu, case, monkeypatch):
    """gpar_gram_grad and gpar_gram_grad_cross (SYM, RECT) on both routes: generated against interpreter at 1e-11 of the largest sum, both
    against the numpy oracle, two generated runs of one call in bits."""
    from gpar_amd.engine import HipEngine
    from oracle import kernels as ok
    from oracle.engine import OracleEngine

    g, torch = gpu, gpu.torch
    name, kernel, width, ck = g.compiled_kernel(case)
    rng = np.random.default_rng(200 + case)
    X1, X2 = rng.standard_normal((GRAD_MAX, width)), rng.standard_normal((GRAD_MAX, width))
    Ws = rng.standard_normal((GRAD_MAX, GRAD_MAX))
    Ws = Ws + Ws.T
    Wr = rng.standard_normal((GRAD_MAX, GRAD_MAX))
    z1, zd1 = g.features(ck, X1)
    z2, zd2 = g.features(ck, X2)
    ldz = int(z1.stride(0))
    assert int(z2.stride(0)) == ldz
    zdp1, zdp2 = (None, None) if zd1 is None else (zd1.data_ptr(), zd2.data_ptr())
    ks = ctypes.byref(ck.kspec)
    nacc = g._lib.GRAD_NACC
    spec = ok.spec_to_dict(kernel.resolve(width))
    ora = OracleEngine()
    ock = ora.compile(kernel, width)

    # (kind, n, n2) -> (oracle gradients, factor of the moment sums, summed weights): computed once, shared by every storage / nblocks
    oracle = {}
    for n in GRAD_N:
        half = ok.kernel_grads(spec, X1[:n], Ws[:n, :n])
        full = {"coef": [2.0 * c for c in half["coef"]],
                "factors": [[{k: (None if v is None else 2.0 * np.asarray(v)) for k, v in f.items()} for f in fs] for fs in half["factors"]]}
        oracle["grad", n, n] = (half, 0.5, np.abs(Ws[:n, :n]).sum())
        oracle["sym", n, n] = (full, 1.0, np.abs(Ws[:n, :n]).sum())
        for n2 in RECT_N2[n]:
            ref = ora.kernel_grads_weighted(ock, torch.tensor(X1[:n]), torch.tensor(X2[:n2]), torch.tensor(Wr[:n, :n2].copy()))
            oracle["rect", n, n2] = (ref, 1.0, np.abs(Wr[:n, :n2]).sum())

    configs, held = [], []
    for kind, n, n2 in oracle:
        W = Wr[:n, :n2] if kind == "rect" else Ws[:n, :n]
        ntiles = _tiles(n) * _tiles(n2) if kind == "rect" else _tiles(n) * (_tiles(n) + 1) // 2
        for variant in _VARIANTS:
            buf, wptr, ldw = _weights(g, W, variant, lower=kind != "rect")
            held.append(buf)
            for nblocks in _block_counts(ntiles):
                configs.append((kind, n, n2, variant, wptr, ldw, nblocks))

    def run(kind, n, n2, variant, wptr, ldw, nblocks):
        work = g.filled(nblocks * nacc + TAIL)
        out = g.filled(nacc + TAIL)
        if kind == "grad":
            rc = g.lib.gpar_gram_grad(ks, z1.data_ptr(), zdp1, n, ldz, ck.dz, wptr, ldw, work.data_ptr(), nblocks, out.data_ptr(), g.stream)
        elif kind == "sym":
            rc = g.lib.gpar_gram_grad_cross(ks, z1.data_ptr(), zdp1, n, ldz, z1.data_ptr(), zdp1, n, ldz, ck.dz, wptr, ldw, g.H.GRAD_SYM,
                                            work.data_ptr(), nblocks, out.data_ptr(), g.stream)
        else:
            rc = g.lib.gpar_gram_grad_cross(ks, z1.data_ptr(), zdp1, n, ldz, z2.data_ptr(), zdp2, n2, ldz, ck.dz, wptr, ldw, g.H.GRAD_RECT,
                                            work.data_ptr(), nblocks, out.data_ptr(), g.stream)
        assert rc == 0, (name, kind, n, n2, variant, nblocks, rc)
        flat, wflat = out.cpu().numpy(), work.cpu().numpy()
        assert (flat[nacc:] == SENTINEL).all() and (wflat[nblocks * nacc :] == SENTINEL).all(), (name, kind, n, n2, variant, nblocks, "wrote past its output")
        return flat[:nacc]

    monkeypatch.setenv("GPAR_GRAD_JIT_MIN_ENTRIES", "-1")
    refs = [run(*c) for c in configs]
    before = g.stats()
    monkeypatch.setenv("GPAR_GRAD_JIT_MIN_ENTRIES", "0")
    differing, worst_routes, worst_oracle = 0, 0.0, 0.0
    for c, ref in zip(configs, refs):
        kind, n, n2 = c[:3]
        what = (name,) + c[:4] + c[5:]
        got, again = run(*c), run(*c)
        assert np.array_equal(got, again), (what, "the reduction is ordered (fixed tile walk per workgroup, fixed order over waves and workgroups): "
                                                  "two runs of one call must agree in every bit")
        assert np.isfinite(ref).all() and np.isfinite(got).all(), (what, "a NaN weight (strict upper triangle or padding) was read")
        scale = float(np.abs(ref).max()) + 1e-300
        worst_routes = max(worst_routes, float(np.abs(got - ref).max()) / (1e-11 * scale))
        assert float(np.abs(got - ref).max()) <= 1e-11 * scale, (what, float(np.abs(got - ref).max()), scale)
        differing += not np.array_equal(got, ref)
        want, factor, wsum = oracle[kind, n, n2]
        for route, raw in (("interpreter", ref), ("generated", got)):
            worst_oracle = max(worst_oracle, _check_parameter_gradients(HipEngine._grads_from_moments(ck, raw, factor), want, wsum, what + (route,)))
    after = g.stats()
    assert after[1] == before[1], "a generated gradient kernel failed to compile"
    assert after[2] >= 1, "no generated kernel is cached after the generated runs"
    g.assert_cached(ck, [21, 31] if zd1 is not None else [1, 11], name)
    print(f"[generated parameter gradients] {name}: {len(configs)} cases, {differing} differ from the interpreter in at least one bit; worst error / "
          f"tolerance: between the routes {worst_routes:.3g}, against the oracle {worst_oracle:.3g}")
    assert differing > 0, (name, "premise: the generated kernel sums in another order than the interpreter, so some case must differ in a bit - "
                                 "none does: the generated kernel did not run (a failed launch falls back silently)")


def _to_columns(ck, gz, x1, lib):
    """Host chain from feature space back to design-matrix columns, as HipEngine.kernel_input_grads applies it."""
    out = np.zeros((x1.shape[0], ck.width))
    fs = ck.fspec
    for q in range(ck.dz):
        c, inv, freq, embed = int(fs.col[q]), float(fs.inv_scale[q]), float(fs.freq[q]), int(fs.embed[q])
        if embed == lib.EMBED_SIN:
            d = inv * freq * np.cos(freq * x1[:, c])
        elif embed == lib.EMBED_COS:
            d = -inv * freq * np.sin(freq * x1[:, c])
        else:
            d = inv
        out[:, c] += gz[:, q] * d
    return out


@pytest.mark.parametrize("case", range(len(STRUCTURES)), ids=_NAMES)
def test_input_gradient_pass_at_every_size_split_and_weight_storage(gpu, case, monkeypatch):
    """gpar_gram_input_grad (RECT, SYM) on both routes with nsplit 1, 2, the number of column tiles and one more (the entry point
    accepts it: the idle split contributes zeros): generated against interpreter at 1e-11 of the largest entry, both against the numpy
    oracle (doubled for SYM) at 1e-11 of max(1, largest entry); output rows past n1 and the output's padding keep their sentinel.
    Structures outside 1 .. 20 feature dims have no generated kernel: 23 dims fall back to the interpreter (nothing compiled, nothing
    cached, the same bits), 0 dims leave the output untouched."""
    from oracle import kernels as ok

    g = gpu
    name, kernel, width, ck = g.compiled_kernel(case)
    rng = np.random.default_rng(300 + case)
    X1, X2 = rng.uniform(-1, 1, (GRAD_MAX, width)), rng.uniform(-1, 1, (GRAD_MAX, width))
    Ws = rng.standard_normal((GRAD_MAX, GRAD_MAX))
    Ws = Ws + Ws.T
    Wr = rng.standard_normal((GRAD_MAX, GRAD_MAX))
    z1, _ = g.features(ck, X1)
    z2, _ = g.features(ck, X2)
    ldz = int(z1.stride(0))
    assert int(z2.stride(0)) == ldz
    ks = ctypes.byref(ck.kspec)
    spec = ok.spec_to_dict(kernel.resolve(width))
    dzc = max(ck.dz, 1)
    ldo, extra_rows = dzc + 3, 2
    generated = 1 <= ck.dz <= 20

    oracle = {}
    for n in GRAD_N:
        oracle["sym", n, n] = 2.0 * ok.kernel_input_grads(spec, X1[:n], X1[:n], Ws[:n, :n]) if ck.dz else None
        for n2 in RECT_N2[n]:
            oracle["rect", n, n2] = ok.kernel_input_grads(spec, X1[:n], X2[:n2], Wr[:n, :n2]) if ck.dz else None

    configs, held = [], []
    for kind, n, n2 in oracle:
        W = Wr[:n, :n2] if kind == "rect" else Ws[:n, :n]
        for variant in _VARIANTS:
            buf, wptr, ldw = _weights(g, W, variant, lower=kind == "sym")
            held.append(buf)
            for nsplit in sorted({1, 2, _tiles(n2), _tiles(n2) + 1}):
                configs.append((kind, n, n2, variant, wptr, ldw, nsplit))

    def run(kind, n, n2, variant, wptr, ldw, nsplit):
        doubles = g.lib.gpar_workspace_doubles(g._lib.WS_INPUT_GRAD, n, ck.dz, nsplit)
        assert doubles == n * ck.dz * nsplit
        work = g.filled(doubles + TAIL)
        out = g.filled((n + extra_rows) * ldo + TAIL)
        zb, mode = (z1, g.H.GRAD_SYM) if kind == "sym" else (z2, g.H.GRAD_RECT)
        rc = g.lib.gpar_gram_input_grad(ks, z1.data_ptr(), n, ldz, zb.data_ptr(), n2, ldz, ck.dz, wptr, ldw, mode, nsplit, work.data_ptr(),
                                        out.data_ptr(), ldo, g.stream)
        assert rc == 0, (name, kind, n, n2, variant, nsplit, rc)
        flat, wflat = out.cpu().numpy(), work.cpu().numpy()
        assert (wflat[doubles:] == SENTINEL).all(), (name, kind, n, n2, variant, nsplit, "wrote past its workspace")
        mat = flat[: (n + extra_rows) * ldo].reshape(n + extra_rows, ldo)
        assert (mat[n:] == SENTINEL).all() and (mat[:, ck.dz :] == SENTINEL).all() and (flat[(n + extra_rows) * ldo :] == SENTINEL).all(), \
            (name, kind, n, n2, variant, nsplit, "rows past n1 or the padding of the output were written")
        return mat[:n, : ck.dz].copy()

    monkeypatch.setenv("GPAR_GRAD_JIT_MIN_ENTRIES", "-1")
    refs = [run(*c) for c in configs]
    before = g.stats()
    monkeypatch.setenv("GPAR_GRAD_JIT_MIN_ENTRIES", "0")
    differing, worst_routes, worst_oracle = 0, 0.0, 0.0
    for c, ref in zip(configs, refs):
        kind, n, n2 = c[:3]
        what = (name,) + c[:4] + c[5:]
        got = run(*c)
        if ck.dz == 0:   # (nothing to differentiate: the entry point returns before it touches the output - `run` saw the sentinel everywhere)
            assert got.size == 0
            continue
        assert np.isfinite(ref).all() and np.isfinite(got).all(), (what, "a NaN weight (strict upper triangle or padding) was read")
        scale = float(np.abs(ref).max()) + 1e-300
        worst_routes = max(worst_routes, float(np.abs(got - ref).max()) / (1e-11 * scale))
        assert float(np.abs(got - ref).max()) <= 1e-11 * scale, (what, float(np.abs(got - ref).max()), scale)
        same = np.array_equal(got, ref)
        differing += not same
        assert generated or same, (what, "no generated kernel serves this structure: the interpreter ran twice and must repeat its bits")
        want = oracle[kind, n, n2]
        bound = 1e-11 * max(1.0, float(np.max(np.abs(want))))
        for route, raw in (("interpreter", ref), ("generated", got)):
            cols = _to_columns(ck, raw, X1[:n], g._lib) * (2.0 if kind == "sym" else 1.0)
            worst_oracle = max(worst_oracle, float(np.max(np.abs(cols - want))) / bound)
            assert np.max(np.abs(cols - want)) <= bound, (what, route, float(np.max(np.abs(cols - want))), bound)
    after = g.stats()
    assert after[1] == before[1], "a generated input-gradient kernel failed to compile"
    print(f"[generated input gradients] {name}: {len(configs)} cases, {differing} differ from the interpreter in at least one bit; worst error / "
          f"tolerance: between the routes {worst_routes:.3g}, against the oracle {worst_oracle:.3g}")
    if generated:
        assert after[2] >= 1, "no generated kernel is cached after the generated runs"
        g.assert_cached(ck, [2, 12], name)
        assert differing > 0, (name, "premise: the generated kernel sums in another order than the interpreter, so some case must differ in a bit - "
                                     "none does: the generated kernel did not run (a failed launch falls back silently)")
    else:
        assert after[0] == before[0] and after[2] == before[2], (name, "a structure outside 1 .. 20 feature dims must stay on the interpreter", before, after)
