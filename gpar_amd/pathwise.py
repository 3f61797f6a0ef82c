"""Pathwise posterior sampling: the basis (Matheron's rule; Wilson et al., "Efficiently sampling functions from Gaussian process
posteriors", ICML 2020).

A posterior draw is a prior draw corrected by one exact data-dependent update,

    f*_s(.) = f_s(.) + k(., X) (K + D)^-1 (y - f_s(X) - eps_s),        eps_s ~ N(0, D),

and the prior draw f_s = Phi(.) theta_s, theta_s ~ N(0, I), comes from a finite basis Phi with Phi(z) Phi(z')^T ~ k(z, z'): random
Fourier features for the stationary product terms, exact finite feature maps for the linear and the constant ones.  This module builds
the basis from the `Kernel` object alone (`CompiledKernel.kernel`, which the device and the oracle compiled forms both carry) - numpy and
torch only; the update and the device passes live in `gp.Obs.pathwise_sample_batch`.

Everything here works in the FEATURE space of the kernel, z = stretch(periodic(select(x))) in the factor order of `compile_kernel`'s
layout (`feature_map`): every factor but `linear` is stationary there - EQ, RQ and the Matern kernels are functions of |z - z'| over their
dims, the cosine factor of sum_d (z_d - z'_d), and `periodic()` is an embedding in front of such a factor.
"""
import math

import numpy as np
import torch

__all__ = ["Basis", "feature_map", "draw_basis"]

STATIONARY = ("eq", "rq", "matern12", "matern32", "matern52", "cos")
_MATERN_2NU = {"matern12": 1, "matern32": 3, "matern52": 5}


def _factors(kernel):
    """(term index, factor index, offset, nd, factor) in the order `compile_kernel` lays the features out, and the total width dz."""
    out, dz = [], 0
    for ti, term in enumerate(kernel.terms):
        for fi, f in enumerate(term.factors):
            nd = f.num_features()
            out.append((ti, fi, dz, nd, f))
            dz += nd
    return out, dz


def feature_map(kernel, x):
    """rows x dz: the featurised coordinates of the rows of x under `kernel`, in the factor order of `compile_kernel`'s layout -
    x[col] / scale for a plain dim, sin | cos(2 pi x[col] / period) / scale for a periodic one.  The arithmetic is the device feature
    map's (v * (2 pi / period), then sin / cos, then * (1 / scale)), so that on the HIP engine the result is `eng.features(ck, x)` up to
    the last bit of sin and cos.  x: a torch tensor (any device; the result lives with it) or an array (a numpy array comes back)."""
    as_numpy = not isinstance(x, torch.Tensor)
    xt = torch.as_tensor(np.asarray(x, dtype=np.float64)) if as_numpy else x
    if xt.dim() == 1:
        xt = xt[:, None]
    kernel = kernel.resolve(int(xt.shape[1]))
    blocks = []
    for _, _, _, _, f in _factors(kernel)[0]:
        cols = torch.as_tensor(list(f.cols), dtype=torch.long, device=xt.device)
        v = xt.index_select(1, cols)
        inv_scale = torch.as_tensor(1.0 / f.scales_value(), dtype=torch.float64, device=xt.device)
        if f.periods is None:
            blocks.append(v * inv_scale)
        else:
            arg = v * torch.as_tensor(2.0 * math.pi / f.periods_value(), dtype=torch.float64, device=xt.device)
            blocks.append(torch.cat([torch.sin(arg), torch.cos(arg)], dim=1) * inv_scale)
    z = torch.cat(blocks, dim=1) if blocks else torch.zeros(xt.shape[0], 0, dtype=torch.float64, device=xt.device)
    return z.numpy() if as_numpy else z


class Basis:
    """A finite basis Phi of one layer kernel, Phi(z) Phi(z')^T ~ k(z, z'), over the features z of `feature_map`:

        omega      F_tot x dz   frequencies in cycles per unit of z (zero outside their term's dims)
        amp        F_tot        amplitudes sqrt(c_t / F_t): the features are the PAIRS amp cos(2 pi omega . (z - shift)), amp sin(...)
        lin_idx, lin_amp        exact features lin_amp[i] * z[lin_idx[i]] (linear terms; they use z itself, not z - shift)
        const_amp               exact features const_amp[i] (additive constants)
        shift_dims              the dims a shift applies to: the non-periodic dims of stationary factors
        shift      dz           what is subtracted from z before the phase is formed (None until `with_shift`): the column means of the
                                training features on `shift_dims`, zero elsewhere.  Stationary kernels do not see it; like the Gram
                                kernels, which form differences first, the phase then keeps its digits for time stamps like 1e6.

    A weight vector theta has `num_weights` entries, ordered [cos | sin | linear | constant]; f = Phi theta."""

    def __init__(self, omega, amp, lin_idx, lin_amp, const_amp, shift_dims, shift=None):
        self.omega = np.ascontiguousarray(omega, dtype=np.float64)
        self.amp = np.asarray(amp, dtype=np.float64)
        self.lin_idx = np.asarray(lin_idx, dtype=np.int64)
        self.lin_amp = np.asarray(lin_amp, dtype=np.float64)
        self.const_amp = np.asarray(const_amp, dtype=np.float64)
        self.shift_dims = np.asarray(shift_dims, dtype=bool)
        self.shift = None if shift is None else np.asarray(shift, dtype=np.float64)
        self.dz = int(self.omega.shape[1])
        self._on = {}

    @property
    def num_frequencies(self):
        return int(self.omega.shape[0])

    @property
    def num_weights(self):
        return 2 * self.num_frequencies + int(self.lin_idx.size) + int(self.const_amp.size)

    def with_shift(self, z_train):
        """The same basis with `shift` taken from the training features (rows x dz, torch or numpy)."""
        shift = np.zeros(self.dz)
        if z_train is not None and z_train.shape[0] > 0 and self.shift_dims.any():
            zt = z_train.detach().cpu().numpy() if isinstance(z_train, torch.Tensor) else np.asarray(z_train)
            shift[self.shift_dims] = zt[:, : self.dz].mean(axis=0)[self.shift_dims]
        return Basis(self.omega, self.amp, self.lin_idx, self.lin_amp, self.const_amp, self.shift_dims, shift)

    def on(self, like):
        """omega, amp, shift, lin_idx, lin_amp, const_amp as tensors on the device of `like` (kept)."""
        key = str(like.device)
        if key not in self._on:
            def t(a, dtype=torch.float64):
                return torch.as_tensor(a, dtype=dtype).to(like.device)
            shift = self.shift if self.shift is not None else np.zeros(self.dz)
            self._on[key] = (t(self.omega), t(self.amp), t(shift), t(self.lin_idx, torch.long), t(self.lin_amp), t(self.const_amp))
        return self._on[key]

    def exact_phi(self, z):
        """rows x (linear + constant features): the exact part of Phi."""
        _, _, _, lin_idx, lin_amp, const_amp = self.on(z)
        return torch.cat([z.index_select(1, lin_idx) * lin_amp, const_amp.expand(z.shape[0], -1)], dim=1)

    def phi(self, z):
        """Phi(z), rows x num_weights, for a torch tensor of features (or an array: a numpy array comes back)."""
        as_numpy = not isinstance(z, torch.Tensor)
        zt = torch.as_tensor(np.asarray(z, dtype=np.float64)) if as_numpy else z
        omega, amp, shift, _, _, _ = self.on(zt)
        phase = (2.0 * math.pi) * ((zt[:, : self.dz] - shift) @ omega.T)
        out = torch.cat([torch.cos(phase) * amp, torch.sin(phase) * amp, self.exact_phi(zt)], dim=1)
        return out.numpy() if as_numpy else out


def _describe(ti, term):
    return f"term {ti}" + (f" ({term.label})" if term.label else "")


def draw_basis(kernel, features=2048, rng=None):
    """A `Basis` for `kernel` (resolved: every factor bound to its columns, as `CompiledKernel.kernel` is) with `features` frequency
    vectors per stationary product term, drawn from `rng` (a numpy Generator).  Per product term t with coefficient c_t:

      every factor stationary   `features` frequencies, zero outside the term's dims; every factor fills its own dims (factors own
                                disjoint feature dims, so the frequency of a product is the concatenation):
                                    EQ,  exp(-r^2 / 2)            omega = g / 2 pi,                   g ~ N(0, I)
                                    RQ,  (1 + r^2 / 2 a)^-a       omega = sqrt(tau) g / 2 pi,         tau ~ Gamma(shape a, rate a)
                                    Matern nu                     omega = g / (2 pi sqrt(u / 2 nu)),  u ~ chi^2(2 nu)
                                    Cos, cos(2 pi sum_d dz_d)     omega = 1 on each of its dims
                                a term whose factors are all Cos needs ONE pair and is then exact
      one Linear factor alone   the exact features sqrt(c_t) z_d over its dims
      no factor                 the exact feature sqrt(c_t)

    anything else (Linear times another factor, c_t <= 0) raises ValueError naming the term."""
    if int(features) < 1:
        raise ValueError(f"features must be at least 1 (got {features})")
    features = int(features)
    rng = np.random.default_rng() if rng is None else rng
    layout, dz = _factors(kernel)
    omegas, amps, lin_idx, lin_amp, const_amp = [], [], [], [], []
    shift_dims = np.zeros(dz, dtype=bool)
    for ti, term in enumerate(kernel.terms):
        coef = term.coef_value()
        if not coef > 0.0:
            raise ValueError(f"pathwise sampling needs positive coefficients: {_describe(ti, term)} has {coef}")
        mine = [(off, nd, f) for tj, _, off, nd, f in layout if tj == ti]
        types = [f.type for _, _, f in mine]
        if not mine:
            const_amp.append(math.sqrt(coef))
        elif types == ["linear"]:
            off, nd, _ = mine[0]
            lin_idx += list(range(off, off + nd))
            lin_amp += [math.sqrt(coef)] * nd
        elif all(t in STATIONARY for t in types):
            count = 1 if all(t == "cos" for t in types) else features
            om = np.zeros((count, dz))
            for off, nd, f in mine:
                if f.type == "cos":
                    om[:, off : off + nd] = 1.0
                    if f.periods is None:
                        shift_dims[off : off + nd] = True
                    continue
                g = rng.standard_normal((count, nd))
                if f.type == "rq":
                    alpha = f.alpha_value()
                    g *= np.sqrt(rng.gamma(alpha, 1.0 / alpha, size=(count, 1)))
                elif f.type in _MATERN_2NU:
                    two_nu = _MATERN_2NU[f.type]
                    u = np.sum(rng.standard_normal((count, two_nu)) ** 2, axis=1, keepdims=True)
                    g /= np.sqrt(u / two_nu)
                om[:, off : off + nd] = g / (2.0 * math.pi)
                if f.periods is None:
                    shift_dims[off : off + nd] = True
            omegas.append(om)
            amps.append(np.full(count, math.sqrt(coef / count)))
        else:
            raise ValueError(f"pathwise sampling has no basis for {_describe(ti, term)}: a product of factors {types} "
                             "(a linear factor must stand alone in its term)")
    omega = np.concatenate(omegas, axis=0) if omegas else np.zeros((0, dz))
    amp = np.concatenate(amps) if amps else np.zeros(0)
    return Basis(omega, amp, lin_idx, lin_amp, const_amp, shift_dims)
