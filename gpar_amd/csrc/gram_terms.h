// Posterior decomposition by kernel component (ABI v18): Gram matrices, prior variances and posterior moments of the GROUPS of product
// terms of one layer kernel k = sum_t c_t k_t.  A grouping comp[t] in {-1, 0 .. G - 1} sends term t to component g = comp[t] (-1: to none);
// k_g = sum_{comp[t] = g} c_t k_t.  With K = k(X, X) + D + eps I = L L^T and alpha = K^-1 y (what conditioning holds), at test inputs x*:
//     mean_g(x*) = k_g(x*, X) alpha,        var_g(x*) = k_g(x*, x*) - |L^-1 k_g(X, x*)|^2        (latent: the noise belongs to no component)
// - the additive decomposition of Rasmussen & Williams 5.4.3.  Over a grouping that uses every term once the means sum to the layer's
// posterior mean; one component holding every term has the layer's posterior variance.
//
// The kernels are interpreters that take the specification by value, like gram_kernel (gram.h), and evaluate a term with its helpers in its
// order: a term has the same bits here as there, and a component holding every term is gram_kernel's sum, bit for bit.  What differs is the
// accumulator and the store: one pass over the pairs serves every component - the feature rows of a tile are staged once.  No
// floating-point atomics: partial sums are reduced in a fixed order, a call returns the same bits every time.
#pragma once
#include "gram.h"

namespace gpar {

// The grouping by value: comp[t] as given, f0[t] the first factor of term t (gram_kernel walks the factor list once, in term order; the
// kernels here visit the terms of one component at a time and so need to know where a term's factors begin).
struct TermGroups {
    int ncomp;
    int comp[GPAR_MAX_TERMS];
    int f0[GPAR_MAX_TERMS + 1];
};

// Argument checks shared by the three entry points, made before anything is launched or written.
static inline int term_groups_check(const gpar_kspec_t* ks, const int* comp, int ncomp, int dz, TermGroups& tg) {
    if (!ks || ks->nterms < 0 || ks->nterms > GPAR_MAX_TERMS || ks->nfactors < 0 || ks->nfactors > GPAR_MAX_FACTORS) return GPAR_ARG_ERROR(1);
    if (!kspec_cos_ok(ks)) return GPAR_ARG_ERROR(1);
    if (ncomp < 1 || ncomp > GPAR_MAX_TERMS) return GPAR_ARG_ERROR(3);
    if (!comp && ks->nterms > 0) return GPAR_ARG_ERROR(2);
    if (dz < 0 || dz > GPAR_MAX_DIMS) return GPAR_ARG_ERROR(4);
    for (int f = 0; f < ks->nfactors; ++f)
        if (ks->factor[f].off < 0 || ks->factor[f].nd < 0 || ks->factor[f].off + ks->factor[f].nd > (dz > 0 ? dz : 0)) return GPAR_ARG_ERROR(1);
    tg.ncomp = ncomp;
    int f = 0;
    for (int t = 0; t < GPAR_MAX_TERMS; ++t) {
        tg.comp[t] = -1;
        tg.f0[t] = f;
        if (t >= ks->nterms) continue;
        if (comp[t] < -1 || comp[t] >= ncomp) return GPAR_ARG_ERROR(2);
        tg.comp[t] = comp[t];
        while (f < ks->nfactors && ks->factor[f].term == t) ++f;   // (the walk of gram_kernel: factors out of term order belong to nothing)
    }
    tg.f0[GPAR_MAX_TERMS] = f;
    return 0;
}

// total += c_t k_t over a thread's 4 x 2 micro-tile: the body of gram_kernel's term loop (same helpers, same order: same bits).
__device__ __forceinline__ void gram_term_add8(const gpar_kspec_t& ks, int term, int f, const double* __restrict__ Za,
                                               const double* __restrict__ Zb, const double* __restrict__ tab, int ty, int cb, double (&total)[8]) {
    double expo[8], lin[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { expo[e] = 0.0; lin[e] = ks.coef[term]; }
    bool any_exp = false;
    while (f < ks.nfactors && ks.factor[f].term == term) {
        const int type = ks.factor[f].type, off = ks.factor[f].off, nd = ks.factor[f].nd;
        double s[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = 0.0;
        if (type == GPAR_K_LINEAR) {
            gram_accum_dims<true>(Za, Zb, off, nd, ty, cb, s);
#pragma unroll
            for (int e = 0; e < 8; ++e) lin[e] *= s[e];
        } else if (type == GPAR_K_COS) {
            gram_accum_diff_dims(Za, Zb, off, nd, ty, cb, s);
            gram_cosh8(s, lin);
        } else {
            gram_accum_dims<false>(Za, Zb, off, nd, ty, cb, s);
            any_exp = true;
            if (type == GPAR_K_EQ) {
#pragma unroll
                for (int e = 0; e < 8; ++e) expo[e] += s[e];
            } else if (type == GPAR_K_RQ) {
                gram_rqh8(s, ks.factor[f].alpha, expo, tab);
            } else if (type == GPAR_K_MATERN12) {
                gram_maternh8<1>(s, expo, lin);
            } else if (type == GPAR_K_MATERN32) {
                gram_maternh8<3>(s, expo, lin);
            } else {
                gram_maternh8<5>(s, expo, lin);
            }
        }
        ++f;
    }
    if (any_exp) {
        gram_exph8(expo, tab);
#pragma unroll
        for (int e = 0; e < 8; ++e) total[e] = fma(lin[e], expo[e], total[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) total[e] += lin[e];
    }
}

// k_g over the micro-tile: its terms in term order, from zero (an empty component is zero).
__device__ __forceinline__ void gram_component8(const gpar_kspec_t& ks, const TermGroups& tg, int g, const double* __restrict__ Za,
                                                const double* __restrict__ Zb, const double* __restrict__ tab, int ty, int cb, double (&total)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) total[e] = 0.0;
    for (int term = 0; term < ks.nterms; ++term)
        if (tg.comp[term] == g) gram_term_add8(ks, term, tg.f0[term], Za, Zb, tab, ty, cb, total);
}

// ---- gpar_gram_terms: the G matrices k_g(z1, z2), component g at K + g * stride_k -----------------------------------------------------
// gram_kernel's tiling (64 x 64 outputs per workgroup, two passes of a 4 x 2 micro-tile per thread); per pass the components one after the
// other, each stored as it is finished.
__global__ __launch_bounds__(256) void gram_terms_kernel(gpar_kspec_t ks, TermGroups tg, const double* __restrict__ z1, int n1, int ldz1,
                                                         const double* __restrict__ z2, int n2, int ldz2, int dz, double* __restrict__ K, int ldk,
                                                         long long stride_k) {
    extern __shared__ __attribute__((aligned(32))) double gsm[];
    const double* tab = gsm;
    double* Za = gsm + GRAM_TAB_DOUBLES;
    double* Zb = Za + (size_t)(dz > 0 ? dz : 1) * GRAM_LD;
    const int t = threadIdx.x;
    const int row0 = blockIdx.y * GRAM_T, col0 = blockIdx.x * GRAM_T;
    gram_load_tables(gsm, t);
    for (int idx = t; idx < GRAM_T * dz; idx += 256) {
        const int r = idx / dz, d = idx - r * dz;
        Za[d * GRAM_LD + r] = (row0 + r < n1) ? z1[(size_t)(row0 + r) * ldz1 + d] : 0.0;
        Zb[d * GRAM_LD + r] = (col0 + r < n2) ? z2[(size_t)(col0 + r) * ldz2 + d] : 0.0;
    }
    __syncthreads();
    const int tx = t & 15, ty = t >> 4;
    const bool vec = ((ldk & 1) == 0) && ((stride_k & 1) == 0) && gpar_aligned16(K);
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
        const int cb = 32 * h + 2 * tx;
#pragma unroll 1
        for (int g = 0; g < tg.ncomp; ++g) {
            double total[8];
            gram_component8(ks, tg, g, Za, Zb, tab, ty, cb, total);
            double* Kg = K + (size_t)g * stride_k;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = row0 + 4 * ty + i;
                if (row >= n1) continue;
                const int col = col0 + cb;
                double* out = Kg + (size_t)row * ldk + col;
                if (vec && col + 1 < n2) {
                    *reinterpret_cast<g_d2*>(out) = g_d2{total[2 * i], total[2 * i + 1]};
                } else {
                    if (col < n2) out[0] = total[2 * i];
                    if (col + 1 < n2) out[1] = total[2 * i + 1];
                }
            }
        }
    }
}

static int gram_terms_launch(const gpar_kspec_t* ks, const TermGroups& tg, const double* z1, int n1, int ldz1, const double* z2, int n2, int ldz2,
                             int dz, double* K, int ldk, long long stride_k, hipStream_t stream) {
    if (n1 <= 0 || n2 <= 0) return 0;
    const size_t lds = ((size_t)2 * (dz > 0 ? dz : 1) * GRAM_LD + GRAM_TAB_DOUBLES) * sizeof(double);
    if (lds > 48 * 1024) GPAR_HIP_TRY(gpar_set_max_lds(reinterpret_cast<const void*>(&gram_terms_kernel), 160 * 1024));
    hipLaunchKernelGGL(gram_terms_kernel, dim3(gpar_ceil_div(n2, GRAM_T), gpar_ceil_div(n1, GRAM_T)), dim3(256), lds, stream, *ks, tg, z1, n1, ldz1,
                       z2, n2, ldz2, dz, K, ldk, stride_k);
    GPAR_LAUNCH_CHECK();
    return 0;
}

// ---- gpar_gram_terms_diag: out[g][a] = k_g(z_a, z_a) (- sub[g][a]: the last step of the posterior variances) ------------------------------
// c_t k_t(z, z) of one feature row: the inner loop of gram_diag_value (gram.h), one term at a time.
__device__ __forceinline__ double gram_diag_term(const gpar_kspec_t& ks, int term, int f, const double* __restrict__ zr) {
    double prod = ks.coef[term];
    while (f < ks.nfactors && ks.factor[f].term == term) {
        double s = 0.0;
        if (ks.factor[f].type == GPAR_K_COS) { ++f; continue; }   // cos(0) = 1 exactly
        if (ks.factor[f].type == GPAR_K_LINEAR) {
            for (int d = ks.factor[f].off; d < ks.factor[f].off + ks.factor[f].nd; ++d) {
                const double v = zr[d];
                s = fma(v, v, s);
            }
        }
        prod *= gram_nonlin(ks.factor[f].type, s, ks.factor[f].alpha);
        ++f;
    }
    return prod;
}

__global__ __launch_bounds__(256) void gram_terms_diag_kernel(gpar_kspec_t ks, TermGroups tg, const double* __restrict__ z, int n, int ldz,
                                                              double* __restrict__ out, int ldo, const double* __restrict__ sub, int lds_) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const double* zr = z + (size_t)r * ldz;
    for (int g = 0; g < tg.ncomp; ++g) {
        double total = 0.0;
        for (int term = 0; term < ks.nterms; ++term)
            if (tg.comp[term] == g) total += gram_diag_term(ks, term, tg.f0[term], zr);
        out[(size_t)g * ldo + r] = sub ? total - sub[(size_t)g * lds_ + r] : total;
    }
}

static int gram_terms_diag_launch(const gpar_kspec_t* ks, const TermGroups& tg, const double* z, int n, int ldz, double* out, int ldo,
                                  const double* sub, int ldsub, hipStream_t stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(gram_terms_diag_kernel, dim3(gpar_ceil_div(n, 256)), dim3(256), 0, stream, *ks, tg, z, n, ldz, out, ldo, sub, ldsub);
    GPAR_LAUNCH_CHECK();
    return 0;
}

// ---- gpar_posterior_terms: the means, a fused Gram-times-vector pass -----------------------------------------------------------------------
// One workgroup per (64 test rows, split of the training rows): it walks the 64-column tiles bn = split, split + nsplit, ... of its split;
// per tile and pass every thread evaluates its 4 x 2 pairs of component g and multiplies them into alpha, the row sums are reduced over the
// 16 lanes that share the rows (a fixed butterfly) and added to the component's 64 accumulators in LDS by the one lane that owns the row.
// No n* x n matrix is written.  partial[(split * G + g) * ns + row]; the splits are summed in order by the reduce kernel.
__global__ __launch_bounds__(256) void posterior_terms_mean_kernel(gpar_kspec_t ks, TermGroups tg, const double* __restrict__ zs, int ns, int ldzs,
                                                                   const double* __restrict__ z, int n, int ldz, int dz,
                                                                   const double* __restrict__ alpha, int nsplit, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(32))) double gsm[];
    const int dzl = dz > 0 ? dz : 1;
    const double* tab = gsm;
    double* Za = gsm + GRAM_TAB_DOUBLES;
    double* Zb = Za + (size_t)dzl * GRAM_LD;
    double* al = Zb + (size_t)dzl * GRAM_LD;   // alpha of the tile's columns (GRAM_LD doubles: the accumulators stay 32-byte aligned)
    double* macc = al + GRAM_LD;               // [ncomp][64]
    const int t = threadIdx.x;
    const int tx = t & 15, ty = t >> 4;
    const int row0 = blockIdx.x * GRAM_T, split = blockIdx.y;
    const int nt2 = (n + GRAM_T - 1) / GRAM_T;
    gram_load_tables(gsm, t);
    for (int i = t; i < tg.ncomp * GRAM_T; i += 256) macc[i] = 0.0;
    for (int idx = t; idx < GRAM_T * dz; idx += 256) {
        const int r = idx / dz, d = idx - r * dz;
        Za[d * GRAM_LD + r] = (row0 + r < ns) ? zs[(size_t)(row0 + r) * ldzs + d] : 0.0;
    }
    for (int bn = split; bn < nt2; bn += nsplit) {
        const int col0 = bn * GRAM_T;
        __syncthreads();
        for (int idx = t; idx < GRAM_T * dz; idx += 256) {
            const int r = idx / dz, d = idx - r * dz;
            Zb[d * GRAM_LD + r] = (col0 + r < n) ? z[(size_t)(col0 + r) * ldz + d] : 0.0;
        }
        if (t < GRAM_T) al[t] = (col0 + t < n) ? alpha[col0 + t] : 0.0;   // (columns past n: weight zero)
        __syncthreads();
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            const int cb = 32 * h + 2 * tx;
            const double a0 = al[cb], a1 = al[cb + 1];
#pragma unroll 1
            for (int g = 0; g < tg.ncomp; ++g) {
                double total[8];
                gram_component8(ks, tg, g, Za, Zb, tab, ty, cb, total);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    double p = fma(total[2 * i + 1], a1, total[2 * i] * a0);
#pragma unroll
                    for (int off = 8; off > 0; off >>= 1) p += __shfl_xor(p, off, 16);   // tx = 0 .. 15 of one ty are consecutive lanes
                    if (tx == 0) macc[g * GRAM_T + 4 * ty + i] += p;
                }
            }
        }
    }
    __syncthreads();
    for (int i = t; i < tg.ncomp * GRAM_T; i += 256) {
        const int g = i / GRAM_T, r = i - g * GRAM_T;
        if (row0 + r < ns) partial[((size_t)split * tg.ncomp + g) * ns + row0 + r] = macc[i];
    }
}

__global__ __launch_bounds__(256) void posterior_terms_mean_reduce_kernel(const double* __restrict__ partial, int nsplit, int ncomp, int ns,
                                                                          double* __restrict__ mean, int ldm) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)ncomp * ns) return;
    const int g = (int)(i / ns), r = (int)(i - (long long)g * ns);
    double s = 0.0;
    for (int q = 0; q < nsplit; ++q) s += partial[((size_t)q * ncomp + g) * ns + r];
    mean[(size_t)g * ldm + r] = s;
}

// Splits of the training rows for the mean pass: enough workgroups to fill the device when n* is small, never more than there are column
// tiles.  The target of 1024 workgroups (four per compute unit of an MI355X) is a GUESS that has not been tuned: tools/time_decompose.py
// times the pass as it stands.
constexpr int PT_TARGET_WORKGROUPS = 1024;
static inline int pt_nsplit(int n, int ns) {
    const int row_blocks = gpar_ceil_div(ns > 0 ? ns : 1, GRAM_T), col_tiles = gpar_ceil_div(n > 0 ? n : 1, GRAM_T);
    int s = PT_TARGET_WORKGROUPS / row_blocks;
    if (s > col_tiles) s = col_tiles;
    return s < 1 ? 1 : s;
}

// Workspace of gpar_posterior_terms.  The means need nsplit * G * n* partial sums; the variances a stack of G * c rows of ldn = n rounded up
// to even doubles and G * c squared norms, for a chunk of c test rows - c as large as keeps the stack within 2^27 doubles (1 GiB) is what
// gpar_workspace_doubles recommends; the call takes any workspace that holds the partial sums of ONE split and the stack of ONE test row, and
// sizes its splits and chunks by what it is given.
static inline long long pt_ldn(int n) { return ((long long)(n > 0 ? n : 1) + 1) & ~1LL; }
static inline long long pt_row_doubles(int n, int ncomp) { return (long long)ncomp * (pt_ldn(n) + 1); }
static inline long long pt_workspace_doubles(int n, int ns, int ncomp) {
    if (n < 0 || ns < 0 || ncomp < 1 || ncomp > GPAR_MAX_TERMS) return -1;
    const long long means = (long long)pt_nsplit(n, ns) * ncomp * ns;
    long long c = (1LL << 27) / pt_row_doubles(n, ncomp);
    if (c < 1) c = 1;
    if (c > ns) c = ns;
    const long long stack = c * pt_row_doubles(n, ncomp);
    const long long w = means > stack ? means : stack;
    return w > 1 ? w : 1;
}

static int posterior_terms_run(const gpar_kspec_t* ks, const TermGroups& tg, const double* zs, int ns, int ldzs, const double* z, int n, int ldz,
                               int dz, const double* alpha, const double* L, int ldl, double* mean, int ldm, double* var, int ldv, double* ws,
                               long long ws_doubles, hipStream_t stream) {
    const int G = tg.ncomp;
    // ---- means
    int nsplit = 0;   // (n = 0: the reduce kernel sums nothing and writes zeros)
    if (n > 0) {
        nsplit = pt_nsplit(n, ns);
        const long long fit = ws_doubles / ((long long)G * ns);
        if (fit < nsplit) nsplit = (int)fit;
        const size_t lds = ((size_t)2 * (dz > 0 ? dz : 1) * GRAM_LD + GRAM_TAB_DOUBLES + GRAM_LD + (size_t)G * GRAM_T) * sizeof(double);
        if (lds > 48 * 1024) GPAR_HIP_TRY(gpar_set_max_lds(reinterpret_cast<const void*>(&posterior_terms_mean_kernel), 160 * 1024));
        hipLaunchKernelGGL(posterior_terms_mean_kernel, dim3(gpar_ceil_div(ns, GRAM_T), nsplit), dim3(256), lds, stream, *ks, tg, zs, ns, ldzs, z, n,
                           ldz, dz, alpha, nsplit, ws);
    }
    const long long total = (long long)G * ns;
    hipLaunchKernelGGL(posterior_terms_mean_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const double*)ws, nsplit, G,
                       ns, mean, ldm);
    GPAR_LAUNCH_CHECK();
    if (!var) return 0;
    // ---- variances: k_g(x*, x*) - |row of k_g(x*, X) L^-T|^2, a chunk of test rows at a time
    if (n <= 0) return gram_terms_diag_launch(ks, tg, zs, ns, ldzs, var, ldv, nullptr, 0, stream);
    const int ldn = (int)pt_ldn(n);
    long long c = ws_doubles / pt_row_doubles(n, G);
    if (c > ns) c = ns;
    for (int c0 = 0; c0 < ns; c0 += (int)c) {
        const int cc = (ns - c0 < c) ? ns - c0 : (int)c;
        double* S = ws;                              // (G * cc) x n, component g's rows from g * cc
        double* rn = ws + (size_t)G * cc * ldn;      // their squared norms
        int rc = gram_terms_launch(ks, tg, zs + (size_t)c0 * ldzs, cc, ldzs, z, n, ldz, dz, S, ldn, (long long)cc * ldn, stream);
        if (!rc) rc = trsm_rlt_run(L, n, ldl, S, G * cc, ldn, stream);   // ONE solve with G * cc right-hand sides
        if (rc) return rc;
        hipLaunchKernelGGL(rownorm2_kernel, dim3((unsigned)((G * cc + 3) / 4)), dim3(256), 0, stream, (const double*)S, G * cc, n, ldn, rn);
        GPAR_LAUNCH_CHECK();
        rc = gram_terms_diag_launch(ks, tg, zs + (size_t)c0 * ldzs, cc, ldzs, var + c0, ldv, rn, cc, stream);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace gpar
