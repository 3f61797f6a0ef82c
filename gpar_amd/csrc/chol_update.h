// Rank-k Cholesky UPDATE of an augmented factor: forgetting the k leading observations of a conditioned layer.
//
// With L = [[L11, 0], [L21, L22]] the factor of S and z = L^-1 y in the augmented row, the factor of S[k:, k:] satisfies
//   L22' L22'^T = L22 L22^T + L21 L21^T,
// a positive rank-k update of L22 by the k columns of L21 - never a downdate, so plane rotations with c^2 + s^2 = 1 serve and the result
// is backward stable whatever the conditioning.  The algorithm is LINPACK's dchud, one rotation per (column, update vector), blocked in
// panels of CU_W columns.  The augmented row takes part as row m = n - k of every update vector and of the factor: v_t[m] = z1[t], and on
// exit row m of `out` holds z2' with L22' z2' = y2 (the rotations are orthogonal maps of [L22 | L21] and of [z2^T | z1^T] alike).
//
// Exact operation order.  For column j = 0 .. m-1 ascending and, inside it, update vector t = 0 .. k-1 ascending, with a = L_jj as the
// vectors t' < t have left it and b = v_t[j] as the columns j' < j have left it:
//   r = sqrt(fma(a, a, b * b));   c = a / r;   s = b / r;   L_jj <- r;
//   for every row i > j, the augmented row included:   L_ij' = fma(c, L_ij, s * v_t[i]);   v_t[i]' = fma(c, v_t[i], -(s * L_ij))
// (both from the old L_ij and v_t[i]).  Operation (j, t) needs (j, t - 1) and (j - 1, t) and nothing else: the kernels walk this graph in
// other loop orders (slabs of t outermost), which leaves every operand of every operation - and so every bit of the result - as above.
//   corner = -(fma chain over j ascending of z2'_j^2, starting from 0);   logdet = 2 * (sum over j ascending of log L_jj', panel by panel).
//
// Launch structure: two plain launches per panel on the caller's stream and nothing else - no waiting inside a launch, no atomics, no
// host synchronisation, vector stores only.
//   diagonal kernel  one workgroup of one wave: the CU_W x CU_W diagonal block and the panel's CU_W rows of V in LDS (V in slabs of
//                    CU_SLAB vectors); lane i owns row i; writes the block to `out`, the panel's (c, s) table (CU_W x k pairs) to the
//                    workspace, adds the panel's share of the log-determinant, and reports a non-finite r (1-based column) in `info`;
//   row kernel       one thread per row below the block plus the augmented row; the row's CU_W entries stay in registers while the k
//                    vectors pass in chunks of CU_TS; reads the (c, s) table at wave-uniform addresses; writes L' to `out`, V' to the
//                    workspace, and (the augmented row's thread) the running corner.
// A row of V is dead once its own panel is done, so the diagonal kernel writes none back.  Panel 0 reads V from the input (L21 and z1
// in place: the augmented row of the input follows L21's last row), later panels from the workspace.
//
// Traffic: every entry of the lower triangle of L22 is read and written once - 8 n^2 bytes per drop for n ~ m - plus 16 (m - j) k bytes of
// V per panel.  The chain r -> c, s -> next r of the diagonal kernel is m k sequential sqrt / divide steps: that latency, not the
// 3 k m^2 flops of the row kernel, bounds the update for all but the smallest k.
#pragma once
#include "common.h"

namespace gpar {

constexpr int CU_W = 64;      // columns per panel = rows of the diagonal block = lanes of its wave
constexpr int CU_SLAB = 64;   // update vectors the diagonal kernel holds in LDS at once (CU_W x CU_SLAB + the block: 64 KB)
constexpr int CU_TS = 8;      // update vectors a thread of the row kernel holds in registers at once

static inline int cu_kp(int k) { return (k + 1) & ~1; }   // row stride of V in the workspace (even: 16-byte aligned rows)
static inline long long cu_workspace_doubles(int n, int k) {
    if (n < 2 || k < 1 || k >= n || k > GPAR_CHOL_UPDATE_MAX_RANK) return -1;
    return (long long)(n - k + 1) * cu_kp(k) + 2LL * CU_W * k;   // V: (m + 1) x kp, then the (c, s) table of one panel
}

// One rotation applied to a pair (entry of the factor, entry of the update vector): the same expression in both kernels.
__device__ __forceinline__ void cu_rotate(double c, double s, double& l, double& v) {
    const double nl = fma(c, l, s * v);
    const double nv = fma(c, v, -(s * l));
    l = nl;
    v = nv;
}

__global__ __launch_bounds__(CU_W) void chol_update_diag_kernel(const double* __restrict__ A, int lda, int k, int j0, int w,
                                                                const double* __restrict__ Vsrc, int ldv, double* __restrict__ out,
                                                                int ldo, double* __restrict__ cs, double* __restrict__ logdet,
                                                                int* __restrict__ info) {
    __shared__ double Ld[CU_W][CU_W];      // the block, row-major (touched once per column: its bank conflicts do not matter)
    __shared__ double Vs[CU_SLAB][CU_W];   // the slab TRANSPOSED: Vs[t][row], lane = row is conflict-free
    const int i = threadIdx.x;
    for (int r = i; r < w; ++r) Ld[r][i] = A[(size_t)(k + j0 + r) * lda + k + j0 + i];   // lane = column: coalesced, lower triangle only
    int bad = 0;
    for (int t0 = 0; t0 < k; t0 += CU_SLAB) {
        const int ts = min(CU_SLAB, k - t0);
        __syncthreads();
        if (i < ts)
            for (int r = 0; r < w; ++r) Vs[i][r] = Vsrc[(size_t)(j0 + r) * ldv + t0 + i];   // lane = vector: coalesced
        __syncthreads();
        for (int j = 0; j < w; ++j) {
            const bool live = i > j && i < w;
            double a = Ld[j][j];
            double l = live ? Ld[i][j] : 0.0;
            double b = Vs[0][j];
            double v = live ? Vs[0][i] : 0.0;
            for (int t = 0; t < ts; ++t) {
                // the operands of (j, t + 1) were final when column j - 1 ended: fetched ahead of the chain below
                const double bn = t + 1 < ts ? Vs[t + 1][j] : 0.0;
                const double vn = live && t + 1 < ts ? Vs[t + 1][i] : 0.0;
                const double r = sqrt(fma(a, a, b * b));
                const double c = a / r, s = b / r;
                if (!__builtin_isfinite(r) && !bad) bad = j0 + j + 1;
                if (live) {
                    cu_rotate(c, s, l, v);
                    Vs[t][i] = v;
                }
                if (i == 0) {
                    cs[((size_t)j * k + t0 + t) * 2] = c;
                    cs[((size_t)j * k + t0 + t) * 2 + 1] = s;
                }
                a = r;
                b = bn;
                v = vn;
            }
            if (live) Ld[i][j] = l;
            if (i == j) Ld[j][j] = a;
            __syncthreads();
        }
    }
    for (int r = i; r < w; ++r) out[(size_t)(j0 + r) * ldo + j0 + i] = Ld[r][i];
    if (i == 0) {
        if (logdet) {
            double sum = 0.0;
            for (int j = 0; j < w; ++j) sum += log(Ld[j][j]);
            *logdet = (j0 == 0 ? 0.0 : *logdet) + 2.0 * sum;
        }
        if (info && bad && *info == 0) *info = bad;
    }
}

__global__ __launch_bounds__(CU_W) void chol_update_rows_kernel(const double* __restrict__ A, int lda, int m, int k, int j0, int w,
                                                                const double* Vsrc, int ldv, double* __restrict__ out, int ldo,
                                                                double* V, int kp, const double* __restrict__ cs, int vec_in,
                                                                int vec_out) {
    const int i = j0 + w + blockIdx.x * CU_W + threadIdx.x;   // rows below the block; i == m: the augmented row
    if (i > m) return;
    const double* src = A + (size_t)(k + i) * lda + k + j0;    // (row k + m = n of the input is its augmented row)
    double L[CU_W];
    if (w == CU_W && vec_in) {
#pragma unroll
        for (int j = 0; j < CU_W; j += 2) {
            const double2 q = *reinterpret_cast<const double2*>(src + j);
            L[j] = q.x;
            L[j + 1] = q.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < CU_W; ++j) L[j] = j < w ? src[j] : 0.0;
    }
    const double* vin = Vsrc + (size_t)i * ldv;
    double* vout = V + (size_t)i * kp;   // (from panel 1 on vin == vout: a thread reads its chunk before it writes it)
    for (int t0 = 0; t0 < k; t0 += CU_TS) {
        double v[CU_TS];
#pragma unroll
        for (int u = 0; u < CU_TS; ++u) v[u] = t0 + u < k ? vin[t0 + u] : 0.0;
#pragma unroll
        for (int j = 0; j < CU_W; ++j) {
            if (j < w) {
                const double* pair = cs + ((size_t)j * k + t0) * 2;   // wave-uniform: scalar loads
#pragma unroll
                for (int u = 0; u < CU_TS; ++u)
                    if (t0 + u < k) cu_rotate(pair[2 * u], pair[2 * u + 1], L[j], v[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < CU_TS; ++u)
            if (t0 + u < k) vout[t0 + u] = v[u];
    }
    double* dst = out + (size_t)i * ldo + j0;
    if (w == CU_W && vec_out) {
#pragma unroll
        for (int j = 0; j < CU_W; j += 2) *reinterpret_cast<double2*>(dst + j) = make_double2(L[j], L[j + 1]);
    } else {
#pragma unroll
        for (int j = 0; j < CU_W; ++j)
            if (j < w) dst[j] = L[j];
    }
    if (i == m) {
        double* corner = out + (size_t)m * ldo + m;
        double acc = j0 == 0 ? 0.0 : -*corner;
#pragma unroll
        for (int j = 0; j < CU_W; ++j)
            if (j < w) acc = fma(L[j], L[j], acc);
        *corner = -acc;
    }
}

// A: the (n + 1) x (n + 1) augmented factor (lda); out: (n - k + 1) x (n - k + 1) (ldo), must not overlap A; ws: cu_workspace_doubles.
static int chol_drop_leading_run(const double* A, int n, int k, int lda, double* out, int ldo, double* ws, double* logdet, int* info,
                                 hipStream_t stream) {
    if (n < 2 || k < 1 || k >= n || k > GPAR_CHOL_UPDATE_MAX_RANK) return GPAR_ARG_ERROR(1);
    const int m = n - k;
    if (lda < n + 1 || ldo < m + 1) return GPAR_ARG_ERROR(2);
    if (!A || !out || !ws) return GPAR_ARG_ERROR(3);
    const int kp = cu_kp(k);
    double* V = ws;
    double* cs = ws + (size_t)(m + 1) * kp;
    const int vec_in = gpar_aligned16(A) && lda % 2 == 0 && k % 2 == 0;
    const int vec_out = gpar_aligned16(out) && ldo % 2 == 0;
    for (int j0 = 0; j0 < m; j0 += CU_W) {
        const int w = m - j0 < CU_W ? m - j0 : CU_W;
        const double* Vsrc = j0 == 0 ? A + (size_t)k * lda : V;
        const int ldv = j0 == 0 ? lda : kp;
        hipLaunchKernelGGL(chol_update_diag_kernel, dim3(1), dim3(CU_W), 0, stream, A, lda, k, j0, w, Vsrc, ldv, out, ldo, cs, logdet, info);
        const int rows = m - (j0 + w) + 1;   // below the block, plus the augmented row
        hipLaunchKernelGGL(chol_update_rows_kernel, dim3(gpar_ceil_div(rows, CU_W)), dim3(CU_W), 0, stream, A, lda, m, k, j0, w, Vsrc, ldv, out,
                           ldo, V, kp, cs, vec_in, vec_out);
    }
    GPAR_LAUNCH_CHECK();
    return 0;
}

}  // namespace gpar
