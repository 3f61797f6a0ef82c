// Posterior derivatives (ABI v21): mean and latent variance of DIRECTIONAL DERIVATIVES of one conditioned dense layer.  The derivative of a
// Gaussian process is a Gaussian process (Rasmussen & Williams 9.4): with K = k(X, X) + D + eps I = L L^T and alpha = K^-1 y (what
// conditioning holds), at a test feature row zs_a and for a feature-space direction J[c][a] (the caller's d z / d x applied to a direction of
// the design space, by the convention of gpar_gram_input_grad),
//     d_c,a[b]    = J[c][a] . grad_z k(zs_a, z_b)                                      (the cross-covariance of the derivative with f(X))
//     dmean[c][a] = sum_b d_c,a[b] alpha[b]
//     dvar[c][a]  = J[c][a]^T H(zs_a) J[c][a] - |L^-1 d_c,a|^2,      H = grad_z grad_z'^T k at z = z' = zs_a      (latent)
// - the shape of gpar_posterior_terms (gram_terms.h) with "components" replaced by "directions": the means are one fused pass that writes no
// n* x n matrix, the variances ONE triangular solve over the stacked rows d of a chunk of test rows.
//
// Per pair and product term the factor values phi_f and the multipliers of their gradients are evaluated ONCE (deriv_term_weights8); every
// direction's dot product is formed from them by the product rule (deriv_term_dir8):
//     J . grad_z (c_t prod_f phi_f) = sum_f w_f u_f,    w_f = c_t prod_{g != f} phi_g * m_f,
//     EQ / RQ / Matern  m_f = 2 d phi / d r2    u_f = sum_d J_d (z_d - z'_d)         cosine  m_f = -2 pi sin(2 pi sigma)    u_f = sum_d J_d
//     linear            m_f = 1                 u_f = sum_d J_d z'_d
// The mean kernel and the stack kernel share both helpers: a pair has the same arithmetic in either.  The factor values use libm's exp / log1p
// (gram_nonlin, as the input-gradient interpreter does), not the Gram kernels' tables.  No floating-point atomics: partial sums are reduced
// in a fixed order, a call returns the same bits every time.  At most GRAD_MAXF factors per product term, as in the gradient passes.
#pragma once
#include "gram_terms.h"

namespace gpar {

// Where each term's factors begin (the walk of gram_kernel: factors in term order), by value.
struct DerivPlan {
    int f0[GPAR_MAX_TERMS + 1];
};

// Argument checks of the kernel specification, made before anything is launched or written.
static inline int deriv_check(const gpar_kspec_t* ks, int ndir, int dz, DerivPlan& pl) {
    if (!ks || ks->nterms < 0 || ks->nterms > GPAR_MAX_TERMS || ks->nfactors < 0 || ks->nfactors > GPAR_MAX_FACTORS) return GPAR_ARG_ERROR(1);
    if (!kspec_cos_ok(ks)) return GPAR_ARG_ERROR(1);
    if (ndir < 1 || ndir > GPAR_MAX_TERMS) return GPAR_ARG_ERROR(3);
    if (dz < 0 || dz > GPAR_MAX_DIMS) return GPAR_ARG_ERROR(4);
    for (int f = 0; f < ks->nfactors; ++f) {
        const gpar_factor_t& fa = ks->factor[f];
        if (fa.off < 0 || fa.nd < 0 || fa.off + fa.nd > dz) return GPAR_ARG_ERROR(1);
        if (fa.type == GPAR_K_MATERN12) return GPAR_ARG_ERROR(2);   // not mean-square differentiable: its process has no derivative
    }
    int f = 0;
    for (int t = 0; t < GPAR_MAX_TERMS; ++t) {
        pl.f0[t] = f;
        if (t >= ks->nterms) continue;
        while (f < ks->nfactors && ks->factor[f].term == t) ++f;
        if (f - pl.f0[t] > GRAD_MAXF) return GPAR_ARG_ERROR(1);
    }
    pl.f0[GPAR_MAX_TERMS] = f;
    return 0;
}

// w[ff][e] = c_t prod_{g != ff} phi_g * m_ff over a thread's 4 x 2 micro-tile (entry (i, j) at 2 i + j) for the nf <= GRAD_MAXF factors of
// one term from factor f0 on; factors beyond nf get weight 0.
__device__ __forceinline__ void deriv_term_weights8(const gpar_kspec_t& ks, int term, int f0, int nf, const double* __restrict__ Za,
                                                    const double* __restrict__ Zb, int ty, int cb, double (&w)[GRAD_MAXF][8]) {
    double phi[GRAD_MAXF][8];
#pragma unroll
    for (int ff = 0; ff < GRAD_MAXF; ++ff) {
        if (ff < nf) {
            const int type = ks.factor[f0 + ff].type, off = ks.factor[f0 + ff].off, nd = ks.factor[f0 + ff].nd;
            const double alpha = ks.factor[f0 + ff].alpha;
            double s[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] = 0.0;
            if (type == GPAR_K_LINEAR) {
                gram_accum_dims<true>(Za, Zb, off, nd, ty, cb, s);
#pragma unroll
                for (int e = 0; e < 8; ++e) { phi[ff][e] = s[e]; w[ff][e] = 1.0; }
            } else if (type == GPAR_K_COS) {
                gram_accum_diff_dims(Za, Zb, off, nd, ty, cb, s);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    double sn, cs;
                    sincospi(2.0 * s[e], &sn, &cs);
                    phi[ff][e] = cs;
                    w[ff][e] = -GRAM_2PI * sn;
                }
            } else {
                gram_accum_dims<false>(Za, Zb, off, nd, ty, cb, s);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const double v = gram_nonlin(type, s[e], alpha);
                    phi[ff][e] = v;
                    if (type == GPAR_K_EQ) w[ff][e] = -v;
                    else if (type == GPAR_K_RQ) w[ff][e] = -v / (1.0 + s[e] / (2.0 * alpha));
                    else w[ff][e] = 2.0 * gram_matern_dkds(type, s[e]);
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) { phi[ff][e] = 1.0; w[ff][e] = 0.0; }
        }
    }
    const double coef = ks.coef[term];
#pragma unroll
    for (int ff = 0; ff < GRAD_MAXF; ++ff)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            double rest = coef;
#pragma unroll
            for (int f2 = 0; f2 < GRAD_MAXF; ++f2)
                if (f2 != ff) rest *= phi[f2][e];
            w[ff][e] *= rest;
        }
}

// d[e] += sum_ff w[ff][e] u_ff for ONE direction, whose rows are staged like the features: Jc[dim * GRAM_LD + row of the tile].
__device__ __forceinline__ void deriv_term_dir8(const gpar_kspec_t& ks, int f0, int nf, const double* __restrict__ Za, const double* __restrict__ Zb,
                                                const double* __restrict__ Jc, int ty, int cb, const double (&w)[GRAD_MAXF][8], double (&d)[8]) {
#pragma unroll
    for (int ff = 0; ff < GRAD_MAXF; ++ff) {
        if (ff >= nf) continue;
        const int type = ks.factor[f0 + ff].type, off = ks.factor[f0 + ff].off, nd = ks.factor[f0 + ff].nd;
        double u[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) u[e] = 0.0;
        for (int q = off; q < off + nd; ++q) {
            const g_d4 ja = *reinterpret_cast<const g_d4*>(&Jc[q * GRAM_LD + 4 * ty]);
            if (type == GPAR_K_COS) {
#pragma unroll
                for (int i = 0; i < 4; ++i) { u[2 * i] += ja[i]; u[2 * i + 1] += ja[i]; }
            } else {
                const g_d2 zb = *reinterpret_cast<const g_d2*>(&Zb[q * GRAM_LD + cb]);
                if (type == GPAR_K_LINEAR) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) { u[2 * i] = fma(ja[i], zb[0], u[2 * i]); u[2 * i + 1] = fma(ja[i], zb[1], u[2 * i + 1]); }
                } else {
                    const g_d4 za = *reinterpret_cast<const g_d4*>(&Za[q * GRAM_LD + 4 * ty]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        u[2 * i] = fma(ja[i], za[i] - zb[0], u[2 * i]);
                        u[2 * i + 1] = fma(ja[i], za[i] - zb[1], u[2 * i + 1]);
                    }
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) d[e] = fma(w[ff][e], u[e], d[e]);
    }
}

// Stage 64 rows of the test features and of every direction field, transposed ([dim][GRAM_LD]); rows past `rows` are zero.
__device__ __forceinline__ void deriv_stage_rows(const double* __restrict__ zs, int ldzs, const double* __restrict__ J, int ldj, long long stride_j,
                                                 int ndir, int row0, int rows, int dz, int dzl, double* __restrict__ Za, double* __restrict__ Ja,
                                                 int t) {
    for (int idx = t; idx < GRAM_T * dz; idx += 256) {
        const int r = idx / dz, q = idx - r * dz;
        const bool in = row0 + r < rows;
        Za[q * GRAM_LD + r] = in ? zs[(size_t)(row0 + r) * ldzs + q] : 0.0;
        for (int c = 0; c < ndir; ++c)
            Ja[((size_t)c * dzl + q) * GRAM_LD + r] = in ? J[(size_t)c * stride_j + (size_t)(row0 + r) * ldj + q] : 0.0;
    }
}

// ---- the means: a fused pass in the mould of posterior_terms_mean_kernel (gram_terms.h) -----------------------------------------------------
// One workgroup per (64 test rows, split of the training rows): it walks the 64-column tiles bn = split, split + nsplit, ... of its split.
// Per tile and pass a thread evaluates the weights of its 4 x 2 pairs term by term, forms every direction's d from them, multiplies into
// alpha and keeps the sums of its rows in registers; after the terms they are reduced over the 16 lanes that share the rows (a fixed
// butterfly) and added to the direction's 64 accumulators in LDS by the one lane that owns the row.  partial[(split * ndir + c) * ns + row];
// the splits are summed in order by posterior_terms_mean_reduce_kernel.  Columns past n carry alpha = 0 (their pairs are finite).
__global__ __launch_bounds__(256) void posterior_deriv_mean_kernel(gpar_kspec_t ks, DerivPlan pl, const double* __restrict__ zs, int ns, int ldzs,
                                                                   const double* __restrict__ J, int ldj, long long stride_j, int ndir,
                                                                   const double* __restrict__ z, int n, int ldz, int dz,
                                                                   const double* __restrict__ alpha, int nsplit, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(32))) double gsm[];
    const int dzl = dz > 0 ? dz : 1;
    double* Za = gsm;
    double* Zb = Za + (size_t)dzl * GRAM_LD;
    double* Ja = Zb + (size_t)dzl * GRAM_LD;          // [ndir][dzl][GRAM_LD]
    double* al = Ja + (size_t)ndir * dzl * GRAM_LD;   // alpha of the tile's columns
    double* macc = al + GRAM_LD;                      // [ndir][64]
    const int t = threadIdx.x;
    const int tx = t & 15, ty = t >> 4;
    const int row0 = blockIdx.x * GRAM_T, split = blockIdx.y;
    const int nt2 = (n + GRAM_T - 1) / GRAM_T;
    for (int i = t; i < ndir * GRAM_T; i += 256) macc[i] = 0.0;
    deriv_stage_rows(zs, ldzs, J, ldj, stride_j, ndir, row0, ns, dz, dzl, Za, Ja, t);
    for (int bn = split; bn < nt2; bn += nsplit) {
        const int col0 = bn * GRAM_T;
        __syncthreads();
        for (int idx = t; idx < GRAM_T * dz; idx += 256) {
            const int r = idx / dz, q = idx - r * dz;
            Zb[q * GRAM_LD + r] = (col0 + r < n) ? z[(size_t)(col0 + r) * ldz + q] : 0.0;
        }
        if (t < GRAM_T) al[t] = (col0 + t < n) ? alpha[col0 + t] : 0.0;
        __syncthreads();
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            const int cb = 32 * h + 2 * tx;
            const double a0 = al[cb], a1 = al[cb + 1];
            double racc[GPAR_MAX_TERMS][4];
#pragma unroll
            for (int c = 0; c < GPAR_MAX_TERMS; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) racc[c][i] = 0.0;
#pragma unroll 1
            for (int term = 0; term < ks.nterms; ++term) {
                const int f0 = pl.f0[term], nf = pl.f0[term + 1] - f0;
                if (nf == 0) continue;   // (a constant term has no gradient)
                double w[GRAD_MAXF][8];
                deriv_term_weights8(ks, term, f0, nf, Za, Zb, ty, cb, w);
#pragma unroll
                for (int c = 0; c < GPAR_MAX_TERMS; ++c) {
                    if (c >= ndir) continue;
                    double d[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) d[e] = 0.0;
                    deriv_term_dir8(ks, f0, nf, Za, Zb, Ja + (size_t)c * dzl * GRAM_LD, ty, cb, w, d);
#pragma unroll
                    for (int i = 0; i < 4; ++i) racc[c][i] += fma(d[2 * i + 1], a1, d[2 * i] * a0);
                }
            }
#pragma unroll
            for (int c = 0; c < GPAR_MAX_TERMS; ++c) {
                if (c >= ndir) continue;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    double p = racc[c][i];
#pragma unroll
                    for (int off = 8; off > 0; off >>= 1) p += __shfl_xor(p, off, 16);   // tx = 0 .. 15 of one ty are consecutive lanes
                    if (tx == 0) macc[c * GRAM_T + 4 * ty + i] += p;
                }
            }
        }
    }
    __syncthreads();
    for (int i = t; i < ndir * GRAM_T; i += 256) {
        const int c = i / GRAM_T, r = i - c * GRAM_T;
        if (row0 + r < ns) partial[((size_t)split * ndir + c) * ns + row0 + r] = macc[i];
    }
}

// ---- the stack of a chunk of `rows` test rows: S[(c * rows + a) * lds_ + b] = d_c,a[b], the pairs by the helpers of the mean kernel ----------
__global__ __launch_bounds__(256) void posterior_deriv_stack_kernel(gpar_kspec_t ks, DerivPlan pl, const double* __restrict__ zs, int rows, int ldzs,
                                                                    const double* __restrict__ J, int ldj, long long stride_j, int ndir,
                                                                    const double* __restrict__ z, int n, int ldz, int dz, double* __restrict__ S,
                                                                    int lds_) {
    extern __shared__ __attribute__((aligned(32))) double gsm[];
    const int dzl = dz > 0 ? dz : 1;
    double* Za = gsm;
    double* Zb = Za + (size_t)dzl * GRAM_LD;
    double* Ja = Zb + (size_t)dzl * GRAM_LD;
    const int t = threadIdx.x;
    const int tx = t & 15, ty = t >> 4;
    const int row0 = blockIdx.y * GRAM_T, col0 = blockIdx.x * GRAM_T;
    deriv_stage_rows(zs, ldzs, J, ldj, stride_j, ndir, row0, rows, dz, dzl, Za, Ja, t);
    for (int idx = t; idx < GRAM_T * dz; idx += 256) {
        const int r = idx / dz, q = idx - r * dz;
        Zb[q * GRAM_LD + r] = (col0 + r < n) ? z[(size_t)(col0 + r) * ldz + q] : 0.0;
    }
    __syncthreads();
    const bool vec = ((lds_ & 1) == 0) && gpar_aligned16(S);
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
        const int cb = 32 * h + 2 * tx;
        double d[GPAR_MAX_TERMS][8];
#pragma unroll
        for (int c = 0; c < GPAR_MAX_TERMS; ++c)
#pragma unroll
            for (int e = 0; e < 8; ++e) d[c][e] = 0.0;
#pragma unroll 1
        for (int term = 0; term < ks.nterms; ++term) {
            const int f0 = pl.f0[term], nf = pl.f0[term + 1] - f0;
            if (nf == 0) continue;
            double w[GRAD_MAXF][8];
            deriv_term_weights8(ks, term, f0, nf, Za, Zb, ty, cb, w);
#pragma unroll
            for (int c = 0; c < GPAR_MAX_TERMS; ++c)
                if (c < ndir) deriv_term_dir8(ks, f0, nf, Za, Zb, Ja + (size_t)c * dzl * GRAM_LD, ty, cb, w, d[c]);
        }
#pragma unroll
        for (int c = 0; c < GPAR_MAX_TERMS; ++c) {
            if (c >= ndir) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = row0 + 4 * ty + i, col = col0 + cb;
                if (row >= rows) continue;
                double* out = S + ((size_t)c * rows + row) * lds_ + col;
                if (vec && col + 1 < n) {
                    *reinterpret_cast<g_d2*>(out) = g_d2{d[c][2 * i], d[c][2 * i + 1]};
                } else {
                    if (col < n) out[0] = d[c][2 * i];
                    if (col + 1 < n) out[1] = d[c][2 * i + 1];
                }
            }
        }
    }
}

// ---- the prior term J^T H J of one (direction, test row), minus sub[c * ldsub + a] where given (the last step of the variances) --------------
// On the diagonal z = z' every stationary and cosine factor has value 1 and no gradient; a linear factor has value |z|^2 and both gradients
// equal to z.  Per factor: H_f = -2 phi'(0) I on its dims (EQ 1, RQ 1, Matern 3/2 3, Matern 5/2 5/3), 4 pi^2 1 1^T (cosine), I (linear); per
// term  c_t [sum_f (J^T H_f J) prod_{g != f} v_g + sum_{f != g} (J . grad phi_f)(J . grad' phi_g) prod_{h != f, g} v_h] - the cross terms
// live between two linear factors of one term only.
__global__ __launch_bounds__(256) void posterior_deriv_prior_kernel(gpar_kspec_t ks, DerivPlan pl, const double* __restrict__ zs, int ns, int ldzs,
                                                                    const double* __restrict__ J, int ldj, long long stride_j, int ndir,
                                                                    double* __restrict__ out, int ldo, const double* __restrict__ sub, int ldsub) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)ndir * ns) return;
    const int c = (int)(idx / ns), r = (int)(idx - (long long)c * ns);
    const double* zr = zs + (size_t)r * ldzs;
    const double* jr = J + (size_t)c * stride_j + (size_t)r * ldj;
    double total = 0.0;
    for (int term = 0; term < ks.nterms; ++term) {
        const int f0 = pl.f0[term], nf = pl.f0[term + 1] - f0;
        double v[GRAD_MAXF], q[GRAD_MAXF], l[GRAD_MAXF];
#pragma unroll
        for (int ff = 0; ff < GRAD_MAXF; ++ff) {
            v[ff] = 1.0;
            q[ff] = 0.0;
            l[ff] = 0.0;
            if (ff >= nf) continue;
            const int type = ks.factor[f0 + ff].type, off = ks.factor[f0 + ff].off, nd = ks.factor[f0 + ff].nd;
            double jj = 0.0, js = 0.0, jz = 0.0, zz = 0.0;
            for (int d = off; d < off + nd; ++d) {
                const double jv = jr[d], zv = zr[d];
                jj = fma(jv, jv, jj);
                js += jv;
                jz = fma(jv, zv, jz);
                zz = fma(zv, zv, zz);
            }
            if (type == GPAR_K_LINEAR) {
                v[ff] = zz;
                q[ff] = jj;
                l[ff] = jz;
            } else if (type == GPAR_K_COS) {
                q[ff] = (GRAM_2PI * GRAM_2PI) * (js * js);
            } else {
                q[ff] = (type == GPAR_K_MATERN32 ? 3.0 : (type == GPAR_K_MATERN52 ? GRAM_5_3 : 1.0)) * jj;
            }
        }
        double sum = 0.0;
#pragma unroll
        for (int f = 0; f < GRAD_MAXF; ++f) {
            double rest = 1.0;
#pragma unroll
            for (int g = 0; g < GRAD_MAXF; ++g)
                if (g != f) rest *= v[g];
            sum = fma(q[f], rest, sum);
#pragma unroll
            for (int g = 0; g < GRAD_MAXF; ++g) {
                if (g == f) continue;
                double rest2 = 1.0;
#pragma unroll
                for (int hh = 0; hh < GRAD_MAXF; ++hh)
                    if (hh != f && hh != g) rest2 *= v[hh];
                sum = fma(l[f] * l[g], rest2, sum);
            }
        }
        total = fma(ks.coef[term], sum, total);
    }
    out[(size_t)c * ldo + r] = sub ? total - sub[(size_t)c * ldsub + r] : total;
}

// Splits of the training rows for the mean pass and the workspace: the shapes of gpar_posterior_terms with the directions in the place of the
// components (pt_nsplit, pt_row_doubles, pt_workspace_doubles, gram_terms.h).  The target of 1024 workgroups there is a GUESS, and nothing
// here has been tuned either: tools/time_derivative.py times the call as it stands.
static inline size_t pd_lds_bytes(int dz, int ndir, bool mean) {
    const size_t dzl = dz > 0 ? dz : 1;
    return ((size_t)(2 + ndir) * dzl * GRAM_LD + (mean ? GRAM_LD + (size_t)ndir * GRAM_T : 0)) * sizeof(double);
}
constexpr size_t PD_MAX_LDS = 160 * 1024;

static int posterior_deriv_prior_launch(const gpar_kspec_t* ks, const DerivPlan& pl, const double* zs, int ns, int ldzs, const double* J, int ldj,
                                        long long stride_j, int ndir, double* out, int ldo, const double* sub, int ldsub, hipStream_t stream) {
    const long long total = (long long)ndir * ns;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(posterior_deriv_prior_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, *ks, pl, zs, ns, ldzs, J, ldj,
                       stride_j, ndir, out, ldo, sub, ldsub);
    GPAR_LAUNCH_CHECK();
    return 0;
}

static int posterior_deriv_run(const gpar_kspec_t* ks, const DerivPlan& pl, const double* zs, int ns, int ldzs, const double* J, int ldj,
                               long long stride_j, int ndir, const double* z, int n, int ldz, int dz, const double* alpha, const double* L, int ldl,
                               double* mean, int ldm, double* var, int ldv, double* ws, long long ws_doubles, hipStream_t stream) {
    // ---- means
    int nsplit = 0;   // (n = 0: the reduce kernel sums nothing and writes zeros)
    if (n > 0) {
        nsplit = pt_nsplit(n, ns);
        const long long fit = ws_doubles / ((long long)ndir * ns);
        if (fit < nsplit) nsplit = (int)fit;
        const size_t lds = pd_lds_bytes(dz, ndir, true);
        if (lds > 48 * 1024) GPAR_HIP_TRY(gpar_set_max_lds(reinterpret_cast<const void*>(&posterior_deriv_mean_kernel), (int)PD_MAX_LDS));
        hipLaunchKernelGGL(posterior_deriv_mean_kernel, dim3(gpar_ceil_div(ns, GRAM_T), nsplit), dim3(256), lds, stream, *ks, pl, zs, ns, ldzs, J, ldj,
                           stride_j, ndir, z, n, ldz, dz, alpha, nsplit, ws);
    }
    const long long total = (long long)ndir * ns;
    hipLaunchKernelGGL(posterior_terms_mean_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const double*)ws, nsplit,
                       ndir, ns, mean, ldm);
    GPAR_LAUNCH_CHECK();
    if (!var) return 0;
    // ---- variances: J^T H J - |row of d L^-T|^2, a chunk of test rows at a time
    if (n <= 0) return posterior_deriv_prior_launch(ks, pl, zs, ns, ldzs, J, ldj, stride_j, ndir, var, ldv, nullptr, 0, stream);
    const int ldn = (int)pt_ldn(n);
    long long c = ws_doubles / pt_row_doubles(n, ndir);
    if (c > ns) c = ns;
    const size_t lds = pd_lds_bytes(dz, ndir, false);
    if (lds > 48 * 1024) GPAR_HIP_TRY(gpar_set_max_lds(reinterpret_cast<const void*>(&posterior_deriv_stack_kernel), (int)PD_MAX_LDS));
    for (int c0 = 0; c0 < ns; c0 += (int)c) {
        const int cc = (ns - c0 < c) ? ns - c0 : (int)c;
        double* S = ws;                                 // (ndir * cc) x n, direction c's rows from c * cc
        double* rn = ws + (size_t)ndir * cc * ldn;      // their squared norms
        const double* zc = zs + (size_t)c0 * ldzs;
        const double* Jc = J + (size_t)c0 * ldj;
        hipLaunchKernelGGL(posterior_deriv_stack_kernel, dim3(gpar_ceil_div(n, GRAM_T), gpar_ceil_div(cc, GRAM_T)), dim3(256), lds, stream, *ks, pl,
                           zc, cc, ldzs, Jc, ldj, stride_j, ndir, z, n, ldz, dz, S, ldn);
        GPAR_LAUNCH_CHECK();
        int rc = trsm_rlt_run(L, n, ldl, S, ndir * cc, ldn, stream);   // ONE solve with ndir * cc right-hand sides
        if (rc) return rc;
        hipLaunchKernelGGL(rownorm2_kernel, dim3((unsigned)((ndir * cc + 3) / 4)), dim3(256), 0, stream, (const double*)S, ndir * cc, n, ldn, rn);
        GPAR_LAUNCH_CHECK();
        rc = posterior_deriv_prior_launch(ks, pl, zc, cc, ldzs, Jc, ldj, stride_j, ndir, var + c0, ldv, rn, cc, stream);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace gpar
