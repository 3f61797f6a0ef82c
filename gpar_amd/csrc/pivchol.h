// Greedy (partially pivoted) Cholesky of k(Z, Z): the selection of inducing points by largest conditional variance
// (Fine & Scheinberg 2001; Burt et al. 2019).  Step j picks p = argmax_i d_i of the residual diagonal d, forms column j of the factor
//   c_i = k(z_i, z_p) - sum_{t<j} Lt[t][i] Lt[t][p],   Lt[j][i] = c_i / sqrt(d_p),   d_i <- d_i - Lt[j][i]^2
// and stops when d_p <= floor, when the residual trace sum_i d_i has fallen to tol * trace_0, or when d_p is not finite.
//
// Launch structure: nothing waits on anything.  One plain launch per step on the caller's stream (plus one that produces d and one
// that closes the trace sequence); no atomics, no hand-off words inside a launch, no host synchronisation.  Every workgroup of step j
// opens by reducing, in a fixed order, the per-workgroup partials {max d, its row, sum d} the previous launch left - so every workgroup
// knows p, d_p and the trace, and takes the stop decision itself; workgroup 0 alone records it.  The partials and the stop word live in
// two slots used alternately: a launch reads one and writes the other, so nothing a launch reads is written by that launch.
//
// The factor is stored TRANSPOSED (Lt: step x row), so that the thread of row i reads Lt[t][i], t < j, coalesced along i.
// Traffic: step j reads j n doubles of Lt: 8 n M^2 / 2 bytes in all; the kernel entry itself is one scalar interpreter evaluation per
// row and step (gram_nonlin: libm exp, not the Gram kernels' tables).
#pragma once
#include <limits.h>
#include "gram.h"

namespace gpar {

constexpr int PC_T = 256;            // rows (threads) per workgroup
constexpr int PC_MAX_RANK = 4096;    // Lt[0:j][p] is staged in LDS: 32 KB at the last step

// Order of the argmax: larger d wins, ties go to the smaller row, a NaN ranks above every number (it must surface as the pivot).
__device__ __forceinline__ bool pc_better(double a, int ia, double b, int ib) {
    const bool an = a != a, bn = b != b;
    if (an || bn) return an && (!bn || ia < ib);
    return a > b || (a == b && ia < ib);
}

// Fixed-order tree over the workgroup's PC_T candidates {value, row} and partial sums: the result lands in slot 0.
__device__ __forceinline__ void pc_reduce(double* sv, int* si, double* ss, int tid) {
    for (int s = PC_T / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) {
            if (pc_better(sv[tid + s], si[tid + s], sv[tid], si[tid])) {
                sv[tid] = sv[tid + s];
                si[tid] = si[tid + s];
            }
            ss[tid] += ss[tid + s];
        }
    }
    __syncthreads();
}

// k(zi, zp): the scalar interpreter loop of gram_diag_kernel for a pair (squared distances and inner products by fma over the dims
// in order, gram_nonlin per factor, product per term, sum over terms).
__device__ __forceinline__ double pc_kernel_entry(const gpar_kspec_t& ks, const double* __restrict__ zi, const double* zp) {
    double total = 0.0;
    int f = 0;
    for (int term = 0; term < ks.nterms; ++term) {
        double prod = ks.coef[term];
        while (f < ks.nfactors && ks.factor[f].term == term) {
            const int off = ks.factor[f].off, end = off + ks.factor[f].nd;
            double s = 0.0;
            if (ks.factor[f].type == GPAR_K_LINEAR) {
                for (int d = off; d < end; ++d) s = fma(zi[d], zp[d], s);
            } else if (ks.factor[f].type == GPAR_K_COS) {   // cos(2 pi sum of the differences, in dim order)
                for (int d = off; d < end; ++d) s += zi[d] - zp[d];
                prod *= cospi(2.0 * s);
                ++f;
                continue;
            } else {
                for (int d = off; d < end; ++d) {
                    const double diff = zi[d] - zp[d];
                    s = fma(diff, diff, s);
                }
            }
            prod *= gram_nonlin(ks.factor[f].type, s, ks.factor[f].alpha);
            ++f;
        }
        total += prod;
    }
    return total;
}

// Workspace (doubles): d[n]; two slots of partials {max[nwg], sum[nwg], row[nwg]}; one double holding the two stop words (ints).
__host__ __device__ static inline size_t pc_slot(int n, int nwg, int slot) { return (size_t)n + (size_t)slot * 3 * nwg; }
static inline long long pc_workspace_doubles(int n) {
    const long long nwg = n > 0 ? (n + PC_T - 1) / PC_T : 0;
    return (n > 0 ? n : 0) + 6 * nwg + 1;
}

// LDS of one launch: candidates and sums of the tree, the pivot's features, Lt[0:j][p], the candidates' rows
__host__ __device__ static inline size_t pc_lds_bytes(int j) {
    return ((size_t)2 * PC_T + GPAR_MAX_DIMS + (size_t)((j + 1) & ~1)) * sizeof(double) + PC_T * sizeof(int);
}

// d0 = diag k(Z, Z) (the arithmetic of gram_diag_kernel), the first partials, and the words of a run zeroed.
__global__ __launch_bounds__(PC_T) void pivchol_init_kernel(gpar_kspec_t ks, const double* __restrict__ z, int n, int ldz,
                                                            double* __restrict__ ws, int nwg, int* __restrict__ rank,
                                                            int* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) double pc_lds[];
    double* sv = pc_lds;
    double* ss = sv + PC_T;
    int* si = reinterpret_cast<int*>(ss + PC_T + GPAR_MAX_DIMS);
    const int tid = threadIdx.x, i = blockIdx.x * PC_T + tid;
    double v = -INFINITY;
    if (i < n) {
        v = gram_diag_value(ks, z + (size_t)i * ldz);
        ws[i] = v;
    }
    sv[tid] = v;
    si[tid] = i < n ? i : INT_MAX;
    ss[tid] = i < n ? v : 0.0;
    pc_reduce(sv, si, ss, tid);
    if (tid == 0) {
        double* pout = ws + pc_slot(n, nwg, 0);
        pout[blockIdx.x] = sv[0];
        pout[nwg + blockIdx.x] = ss[0];
        pout[2 * nwg + blockIdx.x] = (double)si[0];
        if (blockIdx.x == 0) {
            int* flag = reinterpret_cast<int*>(ws + pc_slot(n, nwg, 2));
            flag[0] = 0;
            flag[1] = 0;
            *rank = 0;
            *info = 0;
        }
    }
}

// Step j < max_rank (grid: nwg workgroups), or j == max_rank: the closing launch (one workgroup) that only reduces the last partials
// into trace[max_rank] and, where no step stopped, rank = max_rank.
__global__ __launch_bounds__(PC_T) void pivchol_step_kernel(gpar_kspec_t ks, const double* __restrict__ z, int n, int ldz, int dz, int j,
                                                            int max_rank, double tol_trace, double floor_, double* __restrict__ Lt, int ldl,
                                                            int* __restrict__ piv, double* __restrict__ trace, int* __restrict__ rank,
                                                            int* __restrict__ info, double* __restrict__ ws, int nwg) {
    extern __shared__ __attribute__((aligned(16))) double pc_lds[];
    double* sv = pc_lds;
    double* ss = sv + PC_T;
    double* zp = ss + PC_T;
    double* ltp = zp + GPAR_MAX_DIMS;
    int* si = reinterpret_cast<int*>(ltp + ((j + 1) & ~1));
    const int tid = threadIdx.x, i = blockIdx.x * PC_T + tid;
    const bool last = j == max_rank;
    const int* flag_in = reinterpret_cast<const int*>(ws + pc_slot(n, nwg, 2)) + (j & 1);
    int* flag_out = reinterpret_cast<int*>(ws + pc_slot(n, nwg, 2)) + ((j + 1) & 1);
    if (*flag_in) {
        // an earlier step stopped: this launch only leaves its row of the outputs empty
        if (!last && i < n) Lt[(size_t)j * ldl + i] = 0.0;
        if (blockIdx.x == 0 && tid == 0) {
            *flag_out = 1;
            trace[j] = 0.0;
            if (!last) piv[j] = -1;
        }
        return;
    }

    // the pivot and the residual trace from the partials of the previous launch: workgroup w's partial in ascending w per thread, then the tree
    const double* pin = ws + pc_slot(n, nwg, j & 1);
    double bv = -INFINITY, bs = 0.0;
    int bi = INT_MAX;
    for (int w = tid; w < nwg; w += PC_T) {
        const double v = pin[w];
        const int vi = (int)pin[2 * nwg + w];
        if (pc_better(v, vi, bv, bi)) {
            bv = v;
            bi = vi;
        }
        bs += pin[nwg + w];
    }
    sv[tid] = bv;
    si[tid] = bi;
    ss[tid] = bs;
    pc_reduce(sv, si, ss, tid);
    const int p = si[0];
    const double dp = sv[0], tr = ss[0];
    const double tr0 = j == 0 ? tr : trace[0];
    const bool finite = __builtin_isfinite(dp);
    const bool stop = last || dp <= floor_ || tr <= tol_trace * tr0 || !finite;
    if (blockIdx.x == 0 && tid == 0) {
        trace[j] = tr;
        *flag_out = stop ? 1 : 0;
        if (stop) *rank = j;
        if (!last) piv[j] = stop ? -1 : p;
        if (!last && !finite) *info = p + 1;
    }
    if (stop) {
        if (!last && i < n) Lt[(size_t)j * ldl + i] = 0.0;
        return;
    }

    // the pivot's features and its row of the factor so far, once per workgroup
    for (int q = tid; q < dz; q += PC_T) zp[q] = z[(size_t)p * ldz + q];
    for (int t = tid; t < j; t += PC_T) ltp[t] = Lt[(size_t)t * ldl + p];
    __syncthreads();   // (also: every thread has read slot 0 of the tree before it is written again below)

    double dn = -INFINITY;
    if (i < n) {
        double c = pc_kernel_entry(ks, z + (size_t)i * ldz, zp);
        const double* col = Lt + i;
        int t = 0;
        for (; t + 8 <= j; t += 8) {   // eight coalesced loads in flight, the sum itself in the order of t
            double a[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] = col[(size_t)(t + u) * ldl];
#pragma unroll
            for (int u = 0; u < 8; ++u) c = fma(-a[u], ltp[t + u], c);
        }
        for (; t < j; ++t) c = fma(-col[(size_t)t * ldl], ltp[t], c);
        const double r = sqrt(dp);
        double v = c / r;
        if (i == p) {
            v = r;
            dn = 0.0;
        } else {
            dn = fma(-v, v, ws[i]);
        }
        Lt[(size_t)j * ldl + i] = v;
        ws[i] = dn;
    }
    sv[tid] = dn;
    si[tid] = i < n ? i : INT_MAX;
    ss[tid] = i < n ? dn : 0.0;
    pc_reduce(sv, si, ss, tid);
    if (tid == 0) {
        double* pout = ws + pc_slot(n, nwg, (j + 1) & 1);
        pout[blockIdx.x] = sv[0];
        pout[nwg + blockIdx.x] = ss[0];
        pout[2 * nwg + blockIdx.x] = (double)si[0];
    }
}

static int pivoted_chol_run(const gpar_kspec_t* ks, const double* z, int n, int ldz, int dz, int max_rank, double tol_trace, double floor_,
                            double* Lt, int ldl, int* piv, double* trace, int* rank, int* info, double* ws, hipStream_t stream) {
    if (!ks || ks->nterms < 0 || ks->nterms > GPAR_MAX_TERMS || ks->nfactors < 0 || ks->nfactors > GPAR_MAX_FACTORS) return GPAR_ARG_ERROR(3);
    if (dz < 0 || dz > GPAR_MAX_DIMS) return GPAR_ARG_ERROR(4);
    for (int f = 0; f < ks->nfactors; ++f)   // the kernels index the pivot's LDS copy by these
        if (ks->factor[f].off < 0 || ks->factor[f].nd < 0 || ks->factor[f].off + ks->factor[f].nd > dz) return GPAR_ARG_ERROR(3);
    if (!kspec_cos_ok(ks)) return GPAR_ARG_ERROR(3);
    if (n < 1 || n > INT_MAX - PC_T || max_rank < 1 || max_rank > PC_MAX_RANK || ldz < dz || ldl < n) return GPAR_ARG_ERROR(1);
    if (!(floor_ >= 0.0) || !(tol_trace >= 0.0)) return GPAR_ARG_ERROR(2);   // (a picked row holds d = 0: never above a floor >= 0)
    if (!Lt || !piv || !trace || !rank || !info || !ws || (dz > 0 && !z)) return GPAR_ARG_ERROR(5);
    const int nwg = gpar_ceil_div(n, PC_T);
    hipLaunchKernelGGL(pivchol_init_kernel, dim3(nwg), dim3(PC_T), pc_lds_bytes(0), stream, *ks, z, n, ldz, ws, nwg, rank, info);
    for (int j = 0; j <= max_rank; ++j)
        hipLaunchKernelGGL(pivchol_step_kernel, dim3(j < max_rank ? nwg : 1), dim3(PC_T), pc_lds_bytes(j), stream, *ks, z, n, ldz, dz, j, max_rank,
                           tol_trace, floor_, Lt, ldl, piv, trace, rank, info, ws, nwg);
    GPAR_LAUNCH_CHECK();
    return 0;
}

}  // namespace gpar
