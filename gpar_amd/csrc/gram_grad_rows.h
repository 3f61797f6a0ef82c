// Per-row gradient moment sums (gpar_gram_grad_rows): the sums of gram_grad_kernel (gram.h) with the ROW index left unreduced,
//     out[a][s] = sum_b v[b] * (moment s of the pair (z1_a, z2_b)),      s over C_t, Al_f, A_q, P_q  (GRAD_OFF_*, gram.h)
// so that row a is what gpar_gram_grad_cross(GPAR_GRAD_RECT) returns for n1 = 1, z1 = z1[a], W = v^T.  With v = alpha = K^-1 y these are
// the sums behind d mean(x*_a) / d theta of a conditioned layer (sensitivity of the posterior mean to the hyperparameters), which the
// pair-reduced passes cannot give without one call per test row.
//
// The shape of the mean pass of gram_terms.h / gram_deriv.h: one workgroup per (64 rows of z1, split of the rows of z2); it walks the
// 64-column tiles bn = split, split + nsplit, ... of its split, every thread a 4 x 2 patch of pairs, twice per tile.  The per-pair
// arithmetic is gram_grad_kernel's (gram_nonlin, gram_matern_dkds, the same expressions for g, Al, A and P).  Per slot a thread sums its
// two columns, the 16 lanes that share the rows are reduced by a fixed butterfly and the one lane that owns the row adds to the slot's 64
// accumulators in LDS.  Only the slots the structure uses have accumulators (RowsPlan): nterms + RQ factors + dims under a factor (+ the
// dims under a stationary factor again when zd is given); the others are written as 0.  partial[(split * n1 + a) * GRAD_NACC + s]; the
// splits are summed in order by gram_grad_rows_reduce_kernel.  No atomics: a call returns the same bits every time, and a row's bits
// depend on its own features, the columns and the number of splits only - not on the other rows of the call.
//
// LDS: (2 or 4) * dz * GRAM_LD doubles of staged features (4 with zd), GRAM_LD weights, GRAD_NACC map entries and 64 doubles per used
// slot; the call refuses a structure that needs more than 160 KiB (without zd dz <= 95 always fits, with zd dz <= 47; wider ones
// fit when they use fewer slots).  Nothing here has been tuned: tools/time_laplace.py times the call as it stands.
#pragma once
#include "gram_terms.h"

namespace gpar {

// Where each term's factors begin, and the accumulator of every raw slot (-1: the structure does not use it), by value.
struct RowsPlan {
    int f0[GPAR_MAX_TERMS + 1];
    short slot[GRAD_NACC];
    int nused;
};

// Argument checks of the kernel specification, made before anything is launched or written.
static inline int rows_check(const gpar_kspec_t* ks, int dz, bool has_zd, RowsPlan& pl) {
    if (!ks || ks->nterms < 0 || ks->nterms > GPAR_MAX_TERMS || ks->nfactors < 0 || ks->nfactors > GPAR_MAX_FACTORS) return GPAR_ARG_ERROR(1);
    if (!kspec_cos_ok(ks)) return GPAR_ARG_ERROR(1);
    if (dz < 0 || dz > GPAR_MAX_DIMS) return GPAR_ARG_ERROR(4);
    for (int s = 0; s < GRAD_NACC; ++s) pl.slot[s] = -1;
    bool used[GRAD_NACC] = {false};
    for (int f = 0; f < ks->nfactors; ++f) {
        const gpar_factor_t& fa = ks->factor[f];
        if (fa.term < 0 || fa.term >= ks->nterms || (f > 0 && fa.term < ks->factor[f - 1].term)) return GPAR_ARG_ERROR(1);
        if (fa.off < 0 || fa.nd < 0 || fa.off + fa.nd > dz) return GPAR_ARG_ERROR(4);
        if (fa.type == GPAR_K_RQ) used[GRAD_OFF_AL + f] = true;
        for (int d = fa.off; d < fa.off + fa.nd; ++d) {
            used[GRAD_OFF_A + d] = true;
            if (has_zd && fa.type != GPAR_K_LINEAR && fa.type != GPAR_K_COS) used[GRAD_OFF_P + d] = true;
        }
    }
    int f = 0;
    for (int t = 0; t < GPAR_MAX_TERMS; ++t) {
        pl.f0[t] = f;
        if (t >= ks->nterms) continue;
        used[GRAD_OFF_C + t] = true;
        while (f < ks->nfactors && ks->factor[f].term == t) ++f;
        if (f - pl.f0[t] > GRAD_MAXF) return GPAR_ARG_ERROR(6);
    }
    pl.f0[GPAR_MAX_TERMS] = f;
    pl.nused = 0;
    for (int s = 0; s < GRAD_NACC; ++s)
        if (used[s]) pl.slot[s] = (short)pl.nused++;
    return 0;
}

static inline size_t rows_lds_bytes(int dz, bool has_zd, int nused) {
    const size_t dzl = dz > 0 ? dz : 1;
    return ((size_t)(has_zd ? 4 : 2) * dzl * GRAM_LD + GRAM_LD + (size_t)nused * GRAM_T) * sizeof(double) + GRAD_NACC * sizeof(int);
}
constexpr size_t ROWS_MAX_LDS = 160 * 1024;

// acc[k][row] += the sum over the 2 x 16 columns of the 16 lanes that share the thread's 4 rows (val: entry (i, j) at 2 i + j).
__device__ __forceinline__ void rows_add8(double* __restrict__ acc, int k, int tx, int ty, const double (&val)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double p = val[2 * i] + val[2 * i + 1];
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) p += __shfl_xor(p, off, 16);   // tx = 0 .. 15 of one ty are consecutive lanes
        if (tx == 0) acc[k * GRAM_T + 4 * ty + i] += p;
    }
}

__global__ __launch_bounds__(256) void gram_grad_rows_kernel(gpar_kspec_t ks, RowsPlan pl, const double* __restrict__ z1,
                                                             const double* __restrict__ zd1, int n1, int ldz1, const double* __restrict__ z2,
                                                             const double* __restrict__ zd2, int n2, int ldz2, int dz,
                                                             const double* __restrict__ v, int nsplit, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(32))) double gsm[];
    const int dzl = dz > 0 ? dz : 1;
    const bool has_zd = zd1 != nullptr;
    double* Za = gsm;
    double* Zb = Za + (size_t)dzl * GRAM_LD;
    double* Zda = Zb + (size_t)dzl * GRAM_LD;
    double* Zdb = Zda + (has_zd ? (size_t)dzl * GRAM_LD : 0);
    double* vv = Zdb + (has_zd ? (size_t)dzl * GRAM_LD : 0);   // v of the tile's columns
    double* acc = vv + GRAM_LD;                                // [nused][64]
    int* smap = reinterpret_cast<int*>(acc + (size_t)pl.nused * GRAM_T);   // raw slot -> accumulator
    const int t = threadIdx.x;
    const int tx = t & 15, ty = t >> 4;
    const int row0 = blockIdx.x * GRAM_T, split = blockIdx.y;
    const int nt2 = (n2 + GRAM_T - 1) / GRAM_T;
    for (int i = t; i < pl.nused * GRAM_T; i += 256) acc[i] = 0.0;
    if (t < GRAD_NACC) smap[t] = pl.slot[t];
    static_assert(GRAD_NACC <= 256, "one thread per slot fills the map");
    for (int idx = t; idx < GRAM_T * dz; idx += 256) {
        const int r = idx / dz, q = idx - r * dz;
        const bool in = row0 + r < n1;
        Za[q * GRAM_LD + r] = in ? z1[(size_t)(row0 + r) * ldz1 + q] : 0.0;
        if (has_zd) Zda[q * GRAM_LD + r] = in ? zd1[(size_t)(row0 + r) * ldz1 + q] : 0.0;
    }
    for (int bn = split; bn < nt2; bn += nsplit) {
        const int col0 = bn * GRAM_T;
        __syncthreads();
        for (int idx = t; idx < GRAM_T * dz; idx += 256) {
            const int r = idx / dz, q = idx - r * dz;
            const bool in = col0 + r < n2;
            Zb[q * GRAM_LD + r] = in ? z2[(size_t)(col0 + r) * ldz2 + q] : 0.0;
            if (has_zd) Zdb[q * GRAM_LD + r] = in ? zd2[(size_t)(col0 + r) * ldz2 + q] : 0.0;
        }
        if (t < GRAM_T) vv[t] = (col0 + t < n2) ? v[col0 + t] : 0.0;   // columns past n2 carry weight 0 (their pairs are finite)
        __syncthreads();
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            const int cb = 32 * h + 2 * tx;
            double w[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) { w[2 * i] = vv[cb]; w[2 * i + 1] = vv[cb + 1]; }
#pragma unroll 1
            for (int term = 0; term < ks.nterms; ++term) {
                const int f0 = pl.f0[term], nf = pl.f0[term + 1] - f0;
                const double coef = ks.coef[term];
                double phi[GRAD_MAXF][8], sv[GRAD_MAXF][8];
#pragma unroll
                for (int ff = 0; ff < GRAD_MAXF; ++ff) {
                    if (ff < nf) {
                        const int type = ks.factor[f0 + ff].type, off = ks.factor[f0 + ff].off, nd = ks.factor[f0 + ff].nd;
                        const double alpha = ks.factor[f0 + ff].alpha;
                        double s[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) s[e] = 0.0;
                        if (type == GPAR_K_LINEAR) gram_accum_dims<true>(Za, Zb, off, nd, ty, cb, s);
                        else if (type == GPAR_K_COS) gram_accum_diff_dims(Za, Zb, off, nd, ty, cb, s);
                        else gram_accum_dims<false>(Za, Zb, off, nd, ty, cb, s);
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            if (type == GPAR_K_COS) {   // value and d phi / d sigma = -2 pi sin(2 pi sigma) (kept where the others keep s)
                                double sn, cs;
                                sincospi(2.0 * s[e], &sn, &cs);
                                sv[ff][e] = -GRAM_2PI * sn;
                                phi[ff][e] = cs;
                            } else {
                                sv[ff][e] = s[e];
                                phi[ff][e] = gram_nonlin(type, s[e], alpha);
                            }
                        }
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e) { sv[ff][e] = 0.0; phi[ff][e] = 1.0; }
                    }
                }
                {   // coefficient
                    double val[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) val[e] = w[e] * (phi[0][e] * phi[1][e] * phi[2][e] * phi[3][e]);
                    rows_add8(acc, smap[GRAD_OFF_C + term], tx, ty, val);
                }
#pragma unroll
                for (int ff = 0; ff < GRAD_MAXF; ++ff) {
                    if (ff >= nf) continue;
                    const int type = ks.factor[f0 + ff].type, off = ks.factor[f0 + ff].off, nd = ks.factor[f0 + ff].nd;
                    const double alpha = ks.factor[f0 + ff].alpha;
                    double g[8], al[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        double rest = coef;
#pragma unroll
                        for (int f2 = 0; f2 < GRAD_MAXF; ++f2)
                            if (f2 != ff) rest *= phi[f2][e];
                        al[e] = 0.0;
                        if (type == GPAR_K_EQ) g[e] = w[e] * rest * (-0.5 * phi[ff][e]);
                        else if (type == GPAR_K_RQ) {
                            const double tq = sv[ff][e] / (2.0 * alpha), base = 1.0 + tq;
                            g[e] = w[e] * rest * (-0.5 * phi[ff][e] / base);
                            al[e] = (w[e] * rest * phi[ff][e]) * (tq / base - log1p(tq));
                        } else if (gram_is_matern(type)) g[e] = w[e] * rest * gram_matern_dkds(type, sv[ff][e]);
                        else if (type == GPAR_K_COS) g[e] = w[e] * rest * sv[ff][e];
                        else g[e] = w[e] * rest;
                    }
                    if (type == GPAR_K_RQ) rows_add8(acc, smap[GRAD_OFF_AL + f0 + ff], tx, ty, al);
                    const bool with_p = has_zd && type != GPAR_K_LINEAR && type != GPAR_K_COS;
                    for (int d = off; d < off + nd; ++d) {
                        const g_d4 za = *reinterpret_cast<const g_d4*>(&Za[d * GRAM_LD + 4 * ty]);
                        const g_d2 zb = *reinterpret_cast<const g_d2*>(&Zb[d * GRAM_LD + cb]);
                        double a[8];
                        if (type == GPAR_K_LINEAR) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) a[e] = g[e] * (za[e >> 1] * zb[e & 1]);
                        } else if (type == GPAR_K_COS) {   // half the first difference: the host's -2 A / scale is the cosine's rule too
#pragma unroll
                            for (int e = 0; e < 8; ++e) a[e] = g[e] * (0.5 * (za[e >> 1] - zb[e & 1]));
                        } else {
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                const double df = za[e >> 1] - zb[e & 1];
                                a[e] = g[e] * (df * df);
                            }
                        }
                        rows_add8(acc, smap[GRAD_OFF_A + d], tx, ty, a);
                        if (with_p) {
                            const g_d4 zda = *reinterpret_cast<const g_d4*>(&Zda[d * GRAM_LD + 4 * ty]);
                            const g_d2 zdb = *reinterpret_cast<const g_d2*>(&Zdb[d * GRAM_LD + cb]);
                            double pp[8];
#pragma unroll
                            for (int e = 0; e < 8; ++e) pp[e] = g[e] * ((za[e >> 1] - zb[e & 1]) * (zda[e >> 1] - zdb[e & 1]));
                            rows_add8(acc, smap[GRAD_OFF_P + d], tx, ty, pp);
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int i = t; i < GRAM_T * GRAD_NACC; i += 256) {
        const int r = i / GRAD_NACC, s = i - r * GRAD_NACC;
        const int k = smap[s];
        if (k >= 0 && row0 + r < n1) partial[((size_t)split * n1 + row0 + r) * GRAD_NACC + s] = acc[k * GRAM_T + r];
    }
}

// out[a][s] = the splits' partial sums in order; 0 for a slot the structure does not use (and for every slot when there are no splits).
__global__ __launch_bounds__(256) void gram_grad_rows_reduce_kernel(RowsPlan pl, const double* __restrict__ partial, int nsplit, int n1,
                                                                    double* __restrict__ out, int ldo) {
    __shared__ int smap[GRAD_NACC];
    if (threadIdx.x < GRAD_NACC) smap[threadIdx.x] = pl.slot[threadIdx.x];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n1 * GRAD_NACC) return;
    const int a = (int)(i / GRAD_NACC), s = (int)(i - (long long)a * GRAD_NACC);
    double sum = 0.0;
    if (smap[s] >= 0)
        for (int q = 0; q < nsplit; ++q) sum += partial[((size_t)q * n1 + a) * GRAD_NACC + s];
    out[(size_t)a * ldo + s] = sum;
}

// Splits of the rows of z2 (pt_nsplit: enough workgroups to fill the device when n1 is small) within what the workspace holds: a split
// keeps n1 * GRAD_NACC doubles.
static inline long long rows_workspace_doubles(int n2, int n1) {
    if (n2 < 0 || n1 < 0) return -1;
    const long long w = (long long)pt_nsplit(n2, n1) * n1 * GRAD_NACC;
    return w > 1 ? w : 1;
}

static int gram_grad_rows_run(const gpar_kspec_t* ks, const RowsPlan& pl, const double* z1, const double* zd1, int n1, int ldz1, const double* z2,
                              const double* zd2, int n2, int ldz2, int dz, const double* v, double* out, int ldo, double* ws, long long ws_doubles,
                              hipStream_t stream) {
    int nsplit = 0;   // (n2 = 0: the reduce kernel sums nothing and writes zeros)
    if (n2 > 0) {
        nsplit = pt_nsplit(n2, n1);
        const long long fit = ws_doubles / ((long long)n1 * GRAD_NACC);
        if (fit < nsplit) nsplit = (int)fit;
        const size_t lds = rows_lds_bytes(dz, zd1 != nullptr, pl.nused);
        if (lds > 48 * 1024) GPAR_HIP_TRY(gpar_set_max_lds(reinterpret_cast<const void*>(&gram_grad_rows_kernel), (int)ROWS_MAX_LDS));
        hipLaunchKernelGGL(gram_grad_rows_kernel, dim3(gpar_ceil_div(n1, GRAM_T), nsplit), dim3(256), lds, stream, *ks, pl, z1, zd1, n1, ldz1, z2,
                           zd2, n2, ldz2, dz, v, nsplit, ws);
    }
    const long long total = (long long)n1 * GRAD_NACC;
    hipLaunchKernelGGL(gram_grad_rows_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, pl, (const double*)ws, nsplit, n1,
                       out, ldo);
    GPAR_LAUNCH_CHECK();
    return 0;
}

}  // namespace gpar
