// Rolling-origin forecast scoring of one dense layer (ABI v12): the kernels between the factorisation and the two products with X = L^-T.
// With K + D + eps I = L L^T, a = L^-1 y (row n of the augmented factor) and the rows in the order given, the prediction of row r from rows
// 0 ... o_r - 1 (o_r = origin[r]; -1: the row is not scored) has
//     e_r = y_r - mean_r = sum_{c = o_r .. r} L_rc a_c,      v_r = var_r = sum_{c = o_r .. r} L_rc^2
// - the factor of a leading block is the leading block of the factor -, and
//     value = sum_scored term(e_r, v_r),      dvalue/dtheta = 1/2 sum_ab W_ab dK_ab/dtheta,
//     q_r = -dterm/de_r,  s_r = -dterm/dv_r   (zero on unscored rows; the scoring rule decides all three: score.h - for the log score
//     term = -1/2 [log 2 pi + log v_r + e_r^2 / v_r],  q_r = e_r / v_r,  s_r = 1/2 (1 / v_r - q_r^2)),
//     B_rc = -q_r a_c - 2 s_r L_rc  (o_r <= c <= r),      abar_c = -sum_{r >= c, o_r <= c} q_r L_rc,
//     P = Phi(L^T B - abar a^T),      W = X (P + P^T) X^T.
// Four launches: ahead_check_kernel (the origins' range, the smallest origin of every 32 rows), ahead_rows_kernel (e, v, q, s, the value
// terms), ahead_abar_kernel, ahead_band_kernel (P + P^T as a full matrix).  Every kernel behind the check returns at once when the info
// word is set - by the factorisation, by the check, by a non-positive v_r -, so a failed call leaves the value, the means, the variances
// and the gradient outputs as they were.  No workgroup waits on another one; every sum has a fixed order.
#pragma once

namespace gpar {

constexpr int AH_T = 32;                 // tile edge of ahead_abar_kernel and ahead_band_kernel, rows per entry of `cmin`
constexpr int AH_NONE = 0x7fffffff;      // "no origin": an unscored row, a chunk without scored rows

// `vec` of the gradient forms: q, s, value terms, abar (n each), cmin (ceil(n / AH_T) ints in n doubles), then the n x ah_ldt(n) matrix of
// the first product at an even offset; of the value-only form: the n value terms.
inline int ah_ldt(int n) { return n + (n & 1); }
inline long long ah_off_t(int n) { return 5LL * n + (n & 1); }
inline long long ah_workspace_doubles(int n, int grad) {
    if (n <= 0) return 0;
    return grad ? ah_off_t(n) + (long long)n * ah_ldt(n) : n;
}

// One workgroup.  An origin outside -1 ... r: n + 1 + r of the first such row into info (the first to report stays) and nothing else;
// otherwise cmin[k] = the smallest origin among the scored rows of chunk k (AH_NONE when it has none).
__global__ __launch_bounds__(256) void ahead_check_kernel(const int* __restrict__ origin, int n, int* __restrict__ cmin, int* __restrict__ info) {
    __shared__ int sm[256];
    const int t = threadIdx.x;
    int bad = AH_NONE;
    for (int r = t; r < n; r += 256) {
        const int o = origin[r];
        if ((o < -1 || o > r) && bad == AH_NONE) bad = r;
    }
    sm[t] = bad;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) sm[t] = min(sm[t], sm[t + off]);
        __syncthreads();
    }
    if (sm[0] != AH_NONE) {
        if (t == 0) atomicCAS(info, 0, n + 1 + sm[0]);
        return;
    }
    if (!cmin) return;
    const int nchunks = (n + AH_T - 1) / AH_T;
    for (int k = t; k < nchunks; k += 256) {
        int m = AH_NONE;
        for (int r = k * AH_T; r < min(n, (k + 1) * AH_T); ++r) {
            const int o = origin[r];
            if (o >= 0) m = min(m, o);
        }
        cmin[k] = m;
    }
}

// One wave per row: lanes stride the row of L from o_r to r, two wave sums; the scoring rule `rule` turns (e_r, v_r) into the value term,
// q_r and s_r (score_row).  q, s null: the value-only form.  A non-positive v_r: the 1-based row into info, nothing written for it.
__global__ __launch_bounds__(256) void ahead_rows_kernel(const double* __restrict__ L, int ldl, int n, const double* __restrict__ a,
                                                         const double* __restrict__ y, long incy, const int* __restrict__ origin,
                                                         double* __restrict__ mean, double* __restrict__ var, double* __restrict__ q,
                                                         double* __restrict__ s, double* __restrict__ term, int rule, int* __restrict__ info) {
    if (info[0] != 0) return;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int o = origin[row];
    if (o < 0) {
        if (lane == 0) {
            mean[row] = var[row] = __builtin_nan("");
            term[row] = 0.0;
            if (q) q[row] = s[row] = 0.0;
        }
        return;
    }
    const double* Lr = L + (size_t)row * ldl;
    double e0 = 0.0, e1 = 0.0, v0 = 0.0, v1 = 0.0;
    int j = o + lane;
    for (; j + 64 <= row; j += 128) {
        const double l0 = Lr[j], l1 = Lr[j + 64];
        e0 = fma(l0, a[j], e0); v0 = fma(l0, l0, v0);
        e1 = fma(l1, a[j + 64], e1); v1 = fma(l1, l1, v1);
    }
    if (j <= row) { const double l0 = Lr[j]; e0 = fma(l0, a[j], e0); v0 = fma(l0, l0, v0); }
    const double e = wave_sum(e0 + e1), v = wave_sum(v0 + v1);
    if (lane != 0) return;
    if (!(v > 0.0)) {
        atomicCAS(info, 0, row + 1);
        return;
    }
    double tr, qr, sr;
    score_row(rule, e, v, tr, qr, sr);
    mean[row] = y[(size_t)row * incy] - e;
    var[row] = v;
    term[row] = tr;
    if (q) {
        q[row] = qr;
        s[row] = sr;
    }
}

// abar_c = -sum_{r >= c, o_r <= c} q_r L_rc for the AH_T columns of one workgroup: thread (ty, tx) takes rows c0 + ty, c0 + ty + 8, ... of
// column c0 + tx - the 32 threads of a row group read along a row of L - and the 8 partial sums of a column meet in LDS, summed in order.
// LDS: 8 x 33 doubles (2112 bytes).
__global__ __launch_bounds__(256) void ahead_abar_kernel(const double* __restrict__ L, int ldl, int n, const double* __restrict__ q,
                                                         const int* __restrict__ origin, double* __restrict__ abar,
                                                         const int* __restrict__ info) {
    __shared__ double part[8][AH_T + 1];
    if (info[0] != 0) return;
    const int tx = threadIdx.x & (AH_T - 1), ty = threadIdx.x / AH_T;
    const int c0 = blockIdx.x * AH_T, c = c0 + tx;
    double acc = 0.0;
    if (c < n) {
#pragma unroll 4
        for (int r = c0 + ty; r < n; r += 8) {
            const int o = origin[r];
            if (r >= c && o >= 0 && o <= c) acc = fma(q[r], L[(size_t)r * ldl + c], acc);
        }
    }
    part[ty][tx] = acc;
    __syncthreads();
    if (ty == 0 && c < n) {
        double sum = 0.0;
        for (int k = 0; k < 8; ++k) sum += part[k][tx];
        abar[c] = -sum;
    }
}

// Tile (bj, bc), bc <= bj, of  P + P^T  (its lower triangle:  (L^T B)_jc - abar_j a_c,  (L^T B)_jc = -sum_{r >= j, o_r <= c} L_rj (q_r a_c +
// 2 s_r L_rc)),  written at (bj, bc) and, transposed, at (bc, bj): a full symmetric matrix for the product with X, both stores along rows.
// The rows r come through LDS in chunks of AH_T (both column slabs of L read along rows; L_rj stored as zero for r < j, the origin of an
// unscored row as AH_NONE); a chunk whose smallest origin lies right of the tile's columns is skipped, which makes the cost follow the
// band (sum_j sum_{i >= j} #{r >= i: o_r <= j} multiply-adds up to the tile granularity).  Thread (ty, tx): column c0 + tx, rows j0 + ty + 8 k.
// LDS: two 32 x 33 tiles of doubles, q, s and the origins of a chunk: 2 * 8448 + 2 * 256 + 128 = 17536 bytes.
__global__ __launch_bounds__(256) void ahead_band_kernel(const double* __restrict__ L, int ldl, int n, const double* __restrict__ a,
                                                         const double* __restrict__ q, const double* __restrict__ s,
                                                         const double* __restrict__ abar, const int* __restrict__ origin,
                                                         const int* __restrict__ cmin, double* __restrict__ S, int lds,
                                                         const int* __restrict__ info) {
    __shared__ double Lj[AH_T][AH_T + 1];
    __shared__ double Lc[AH_T][AH_T + 1];
    __shared__ double qs[AH_T], ss[AH_T];
    __shared__ int os[AH_T];
    const int bc = blockIdx.x, bj = blockIdx.y;
    if (bc > bj || info[0] != 0) return;
    const int t = threadIdx.x, tx = t & (AH_T - 1), ty = t / AH_T;
    const int j0 = bj * AH_T, c0 = bc * AH_T, gc = c0 + tx;
    const int nchunks = (n + AH_T - 1) / AH_T;
    const double ac = gc < n ? a[gc] : 0.0;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = bj; k < nchunks; ++k) {
        if (cmin[k] > c0 + AH_T - 1) continue;   // (the same verdict in every thread)
        const int r0 = k * AH_T;
        __syncthreads();
        for (int rr = ty; rr < AH_T; rr += 8) {
            const int gr = r0 + rr;
            Lj[rr][tx] = (gr < n && j0 + tx <= gr) ? L[(size_t)gr * ldl + j0 + tx] : 0.0;
            Lc[rr][tx] = (gr < n && gc <= gr) ? L[(size_t)gr * ldl + gc] : 0.0;
        }
        if (t < AH_T) {
            const int gr = r0 + t;
            const int o = gr < n ? origin[gr] : -1;
            qs[t] = o >= 0 ? q[gr] : 0.0;
            ss[t] = o >= 0 ? s[gr] : 0.0;
            os[t] = o >= 0 ? o : AH_NONE;
        }
        __syncthreads();
#pragma unroll 8
        for (int rr = 0; rr < AH_T; ++rr) {
            const double wv = os[rr] <= gc ? fma(2.0 * ss[rr], Lc[rr][tx], qs[rr] * ac) : 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = fma(Lj[rr][ty + 8 * i], wv, acc[i]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gj = j0 + ty + 8 * i;
        Lj[ty + 8 * i][tx] = gj < n ? -acc[i] - abar[gj] * ac : 0.0;
    }
    __syncthreads();
    const bool diag = bj == bc;
    for (int r = ty; r < AH_T; r += 8) {
        const int gr = j0 + r;
        if (gr < n && gc < n) S[(size_t)gr * lds + gc] = (diag && tx > r) ? Lj[tx][r] : Lj[r][tx];
        const int mr = c0 + r, mc = j0 + tx;
        if (!diag && mr < n && mc < n) S[(size_t)mr * lds + mc] = Lj[tx][r];
    }
}

// the value-only form's last launch, and the last block of the gradient forms' epilogue: the sum of the value terms in loo_sum_terms' order
__global__ __launch_bounds__(256) void ahead_value_kernel(const double* __restrict__ term, int n, double* __restrict__ out,
                                                          const int* __restrict__ info) {
    __shared__ double sm[256];
    if (info[0] != 0) return;
    const double v = loo_sum_terms(term, n, sm);
    if (threadIdx.x == 0) out[0] = v;
}

__global__ __launch_bounds__(256) void ahead_grad_epilogue_kernel(const double* __restrict__ partial, int nblocks, double* __restrict__ out,
                                                                  const double* __restrict__ W, int ldw, int n, double* __restrict__ half_diag,
                                                                  const double* __restrict__ term, const int* __restrict__ info) {
    __shared__ double sm[256];
    if (info[0] != 0) return;
    if (grad_epilogue_sums(partial, nblocks, out, W, ldw, n, half_diag)) return;
    const double v = loo_sum_terms(term, n, sm);
    if (threadIdx.x == 0) out[0] = v;
}

// check + rows: everything of the value-only form behind the factor, the head of the weight stage.  q, s, cmin null: value only.
static void ahead_rows_run(const double* A, int lda, int n, const double* y, long incy, const int* origin, double* mean, double* var, double* q,
                           double* s, double* term, int* cmin, int rule, int* info, hipStream_t st) {
    hipLaunchKernelGGL(ahead_check_kernel, dim3(1), dim3(256), 0, st, origin, n, cmin, info);
    hipLaunchKernelGGL(ahead_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, A, lda, n, A + (size_t)n * lda, y, incy, origin, mean, var,
                       q, s, term, rule, info);
}

// The weight stage of the gradient forms: W <- X (P + P^T) X^T on its lower triangle (X = L^-T in its upper triangle, whatever lies below
// its diagonal blocks unread: both products start their K range at the tile's first row).
static int ahead_weights_run(const double* A, int lda, int n, const double* y, long incy, const int* origin, double* mean, double* var, double* vec,
                             const double* X, int ldx, double* W, int ldw, int rule, int* info, hipStream_t st) {
    double *q = vec, *s = vec + n, *term = vec + 2 * (size_t)n, *abar = vec + 3 * (size_t)n, *T = vec + ah_off_t(n);
    int* cmin = reinterpret_cast<int*>(vec + 4 * (size_t)n);
    const int ldt = ah_ldt(n), nt = gpar_ceil_div(n, AH_T);
    const double* a = A + (size_t)n * lda;
    ahead_rows_run(A, lda, n, y, incy, origin, mean, var, q, s, term, cmin, rule, info, st);
    hipLaunchKernelGGL(ahead_abar_kernel, dim3((unsigned)nt), dim3(256), 0, st, A, lda, n, (const double*)q, origin, abar, (const int*)info);
    hipLaunchKernelGGL(ahead_band_kernel, dim3((unsigned)nt, (unsigned)nt), dim3(256), 0, st, A, lda, n, a, (const double*)q, (const double*)s,
                       (const double*)abar, origin, (const int*)cmin, W, ldw, (const int*)info);
    int rc = gemm_launch(0, 1, n, n, n, 1.0, X, ldx, W, ldw, 0.0, T, ldt, GPAR_GEMM_K_FROM_ROW, st);
    if (!rc) rc = gemm_launch(0, 1, n, n, n, 1.0, X, ldx, T, ldt, 0.0, W, ldw, GPAR_GEMM_C_LOWER | GPAR_GEMM_K_FROM_ROW, st);
    return rc;
}

// ---- several horizons in one pass (ABI v15) -------------------------------------------------------------------------------------------
// K = nh origin arrays (origins[k n + r] = o_k[r]) and weights w_k > 0 over ONE factor:
//     e_kr = sum_{c = o_k[r] .. r} L_rc a_c,   v_kr = sum_{c = o_k[r] .. r} L_rc^2,   value_k = sum_r term(e_kr, v_kr),   value = sum_k w_k value_k,
//     Q_r(c) = sum_k w_k q_kr [o_k[r] <= c],   S_r(c) = sum_k w_k s_kr [o_k[r] <= c]      (step functions of c, one step per horizon),
//     B_rc = -Q_r(c) a_c - 2 S_r(c) L_rc,   abar_c = -sum_{r >= c} Q_r(c) L_rc,   P, W as above.
// The row kernel stores w_k q_kr and w_k s_kr, so the kernels behind it take no weights.  A row's K sums come from ONE walk along its row
// of L, from its smallest scored origin.  The band kernel folds the steps into the column slab of a chunk once - Lc[rr][tx] becomes
// Q_r(c) a_c + 2 S_r(c) L_rc, K compares per (r, c) - and its inner loop over the 32 rows j of the tile is the single-horizon one without
// the compare.  LDS: the two 32 x 33 tiles (16896 bytes) + K x 32 x (8 + 8 + 4) bytes of steps: 17536 bytes at K = 1 (the single-horizon
// kernel's), 18816 at K = 3, 22016 at K = 8.  With one horizon and weight 1 every kernel here forms the single-horizon kernels' bits.
struct AheadWeights { double w[GPAR_AHEAD_MAX_HORIZONS]; };

// `vec` of the gradient forms: w q, w s, value terms (K x n each), abar (n), cmin (ceil(n / AH_T) ints in n doubles), then the n x ah_ldt(n)
// matrix of the first product at an even offset; of the value-only form: the K x n value terms.
inline long long ahm_off_t(int n, int nh) {
    const long long o = 3LL * nh * n + 2LL * n;
    return o + (o & 1);
}
inline long long ahm_workspace_doubles(int n, int grad, int nh) {
    if (n <= 0 || nh <= 0) return 0;
    return grad ? ahm_off_t(n, nh) + (long long)n * ah_ldt(n) : (long long)nh * n;
}
inline size_t ahm_band_lds_bytes(int nh) { return (size_t)nh * AH_T * (2 * sizeof(double) + sizeof(int)); }

// ahead_check_kernel over the K arrays: n + 1 + r of the smallest r with an origin outside -1 ... r in any of them; cmin[chunk] = the smallest
// scored origin of the chunk's rows over all horizons.
__global__ __launch_bounds__(256) void ahead_multi_check_kernel(const int* __restrict__ origins, int n, int nh, int* __restrict__ cmin,
                                                                int* __restrict__ info) {
    __shared__ int sm[256];
    const int t = threadIdx.x;
    int bad = AH_NONE;
    for (int r = t; r < n && bad == AH_NONE; r += 256)
        for (int k = 0; k < nh; ++k) {
            const int o = origins[(size_t)k * n + r];
            if (o < -1 || o > r) bad = r;
        }
    sm[t] = bad;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) sm[t] = min(sm[t], sm[t + off]);
        __syncthreads();
    }
    if (sm[0] != AH_NONE) {
        if (t == 0) atomicCAS(info, 0, n + 1 + sm[0]);
        return;
    }
    if (!cmin) return;
    const int nchunks = (n + AH_T - 1) / AH_T;
    for (int c = t; c < nchunks; c += 256) {
        int m = AH_NONE;
        for (int k = 0; k < nh; ++k)
            for (int r = c * AH_T; r < min(n, (c + 1) * AH_T); ++r) {
                const int o = origins[(size_t)k * n + r];
                if (o >= 0) m = min(m, o);
            }
        cmin[c] = m;
    }
}

// One wave per row, one walk: lanes stride the row of L from the row's smallest scored origin to r, and an element at column j enters the
// sums of every horizon with o_k[r] <= j.  q, s null: the value-only form.  A non-positive v_kr: the 1-based row into info, nothing written
// for the row.  NH: the number of horizons (the sums live in registers; C++ linkage: this header is included among the C entries).
extern "C++" {
template <int NH>
__global__ __launch_bounds__(256) void ahead_multi_rows_kernel(const double* __restrict__ L, int ldl, int n, const double* __restrict__ a,
                                                               const double* __restrict__ y, long incy, const int* __restrict__ origins,
                                                               AheadWeights wt, double* __restrict__ mean, double* __restrict__ var,
                                                               double* __restrict__ q, double* __restrict__ s, double* __restrict__ term, int rule,
                                                               int* __restrict__ info) {
    if (info[0] != 0) return;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    int o[NH], omin = AH_NONE;
    double e[NH], v[NH];
#pragma unroll
    for (int k = 0; k < NH; ++k) {
        const int ok = origins[(size_t)k * n + row];
        o[k] = ok >= 0 ? ok : AH_NONE;
        omin = min(omin, o[k]);
        e[k] = v[k] = 0.0;
    }
    if (omin != AH_NONE) {
        const double* Lr = L + (size_t)row * ldl;
#pragma unroll 2
        for (int j = omin + lane; j <= row; j += 64) {
            const double l = Lr[j], aj = a[j];
#pragma unroll
            for (int k = 0; k < NH; ++k)
                if (j >= o[k]) {
                    e[k] = fma(l, aj, e[k]);
                    v[k] = fma(l, l, v[k]);
                }
        }
#pragma unroll
        for (int k = 0; k < NH; ++k) {
            e[k] = wave_sum(e[k]);
            v[k] = wave_sum(v[k]);
        }
    }
    if (lane != 0) return;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < NH; ++k) ok = ok && (o[k] == AH_NONE || v[k] > 0.0);
    if (!ok) {
        atomicCAS(info, 0, row + 1);
        return;
    }
    const double yr = y[(size_t)row * incy];
#pragma unroll
    for (int k = 0; k < NH; ++k) {
        const size_t at = (size_t)k * n + row;
        double tr = 0.0, qr = 0.0, sr = 0.0;
        if (o[k] == AH_NONE) {
            mean[at] = var[at] = __builtin_nan("");
        } else {
            score_row(rule, e[k], v[k], tr, qr, sr);
            mean[at] = yr - e[k];
            var[at] = v[k];
        }
        term[at] = tr;
        if (q) {
            q[at] = wt.w[k] * qr;
            s[at] = wt.w[k] * sr;
        }
    }
}
}  // extern "C++"

// ahead_abar_kernel with the step weight Q_r(c) in the place of q_r [o_r <= c] (`q` holds w_k q_kr)
__global__ __launch_bounds__(256) void ahead_multi_abar_kernel(const double* __restrict__ L, int ldl, int n, const double* __restrict__ q,
                                                               const int* __restrict__ origins, int nh, double* __restrict__ abar,
                                                               const int* __restrict__ info) {
    __shared__ double part[8][AH_T + 1];
    if (info[0] != 0) return;
    const int tx = threadIdx.x & (AH_T - 1), ty = threadIdx.x / AH_T;
    const int c0 = blockIdx.x * AH_T, c = c0 + tx;
    double acc = 0.0;
    if (c < n) {
        for (int r = c0 + ty; r < n; r += 8) {
            if (r < c) continue;
            double Q = 0.0;
            for (int k = 0; k < nh; ++k) {
                const int o = origins[(size_t)k * n + r];
                if (o >= 0 && o <= c) Q += q[(size_t)k * n + r];
            }
            acc = fma(Q, L[(size_t)r * ldl + c], acc);
        }
    }
    part[ty][tx] = acc;
    __syncthreads();
    if (ty == 0 && c < n) {
        double sum = 0.0;
        for (int k = 0; k < 8; ++k) sum += part[k][tx];
        abar[c] = -sum;
    }
}

// ahead_band_kernel for K horizons: per chunk the steps (w q, 2 w s, origins; AH_NONE on unscored (k, r)) go to LDS, every thread folds
// them into its four entries of the column slab - Lc[rr][tx] = Q_r(c) a_c + 2 S_r(c) L_rc -, and the inner loop multiplies the two tiles.
// Dynamic LDS: ahm_band_lds_bytes(nh) behind the two static tiles.
__global__ __launch_bounds__(256) void ahead_multi_band_kernel(const double* __restrict__ L, int ldl, int n, const double* __restrict__ a,
                                                               const double* __restrict__ q, const double* __restrict__ s,
                                                               const double* __restrict__ abar, const int* __restrict__ origins, int nh,
                                                               const int* __restrict__ cmin, double* __restrict__ S, int lds,
                                                               const int* __restrict__ info) {
    __shared__ double Lj[AH_T][AH_T + 1];
    __shared__ double Lc[AH_T][AH_T + 1];
    extern __shared__ double ahm_steps[];
    double *qs = ahm_steps, *ss = ahm_steps + nh * AH_T;
    int* os = reinterpret_cast<int*>(ahm_steps + 2 * nh * AH_T);
    const int bc = blockIdx.x, bj = blockIdx.y;
    if (bc > bj || info[0] != 0) return;
    const int t = threadIdx.x, tx = t & (AH_T - 1), ty = t / AH_T;
    const int j0 = bj * AH_T, c0 = bc * AH_T, gc = c0 + tx;
    const int nchunks = (n + AH_T - 1) / AH_T;
    const double ac = gc < n ? a[gc] : 0.0;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = bj; k < nchunks; ++k) {
        if (cmin[k] > c0 + AH_T - 1) continue;   // (the same verdict in every thread)
        const int r0 = k * AH_T;
        __syncthreads();
        for (int idx = t; idx < nh * AH_T; idx += 256) {
            const int h = idx / AH_T, gr = r0 + (idx & (AH_T - 1));
            const int o = gr < n ? origins[(size_t)h * n + gr] : -1;
            qs[idx] = o >= 0 ? q[(size_t)h * n + gr] : 0.0;
            ss[idx] = o >= 0 ? 2.0 * s[(size_t)h * n + gr] : 0.0;
            os[idx] = o >= 0 ? o : AH_NONE;
        }
        double lc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rr = ty + 8 * i, gr = r0 + rr;
            Lj[rr][tx] = (gr < n && j0 + tx <= gr) ? L[(size_t)gr * ldl + j0 + tx] : 0.0;
            lc[i] = (gr < n && gc <= gr) ? L[(size_t)gr * ldl + gc] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rr = ty + 8 * i;
            double Q = 0.0, S2 = 0.0;
            for (int h = 0; h < nh; ++h)
                if (os[h * AH_T + rr] <= gc) {
                    Q += qs[h * AH_T + rr];
                    S2 += ss[h * AH_T + rr];
                }
            Lc[rr][tx] = fma(S2, lc[i], Q * ac);
        }
        __syncthreads();
#pragma unroll 8
        for (int rr = 0; rr < AH_T; ++rr) {
            const double wv = Lc[rr][tx];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = fma(Lj[rr][ty + 8 * i], wv, acc[i]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gj = j0 + ty + 8 * i;
        Lj[ty + 8 * i][tx] = gj < n ? -acc[i] - abar[gj] * ac : 0.0;
    }
    __syncthreads();
    const bool diag = bj == bc;
    for (int r = ty; r < AH_T; r += 8) {
        const int gr = j0 + r;
        if (gr < n && gc < n) S[(size_t)gr * lds + gc] = (diag && tx > r) ? Lj[tx][r] : Lj[r][tx];
        const int mr = c0 + r, mc = j0 + tx;
        if (!diag && mr < n && mc < n) S[(size_t)mr * lds + mc] = Lj[tx][r];
    }
}

// values[k] = the sum of horizon k's terms in loo_sum_terms' order; out[0] = sum_k w_k values[k], added in the order of k (one workgroup)
__device__ __forceinline__ void ahead_multi_sum_values(const double* __restrict__ term, int n, int nh, const AheadWeights& wt,
                                                       double* __restrict__ values, double* __restrict__ out, double* sm) {
    double total = 0.0;
    for (int k = 0; k < nh; ++k) {
        const double v = loo_sum_terms(term + (size_t)k * n, n, sm);
        __syncthreads();   // (every thread has read sm[0] before the next sum writes it)
        if (threadIdx.x == 0) values[k] = v;
        total += wt.w[k] * v;
    }
    if (threadIdx.x == 0) out[0] = total;
}

__global__ __launch_bounds__(256) void ahead_multi_value_kernel(const double* __restrict__ term, int n, int nh, AheadWeights wt,
                                                                double* __restrict__ values, double* __restrict__ out,
                                                                const int* __restrict__ info) {
    __shared__ double sm[256];
    if (info[0] != 0) return;
    ahead_multi_sum_values(term, n, nh, wt, values, out, sm);
}

__global__ __launch_bounds__(256) void ahead_multi_grad_epilogue_kernel(const double* __restrict__ partial, int nblocks, double* __restrict__ out,
                                                                        const double* __restrict__ W, int ldw, int n, double* __restrict__ half_diag,
                                                                        const double* __restrict__ term, int nh, AheadWeights wt,
                                                                        double* __restrict__ values, const int* __restrict__ info) {
    __shared__ double sm[256];
    if (info[0] != 0) return;
    if (grad_epilogue_sums(partial, nblocks, out, W, ldw, n, half_diag)) return;
    ahead_multi_sum_values(term, n, nh, wt, values, out, sm);
}

// check + rows for K horizons.  q, s, cmin null: value only.
static void ahead_multi_rows_run(const double* A, int lda, int n, const double* y, long incy, const int* origins, int nh, const AheadWeights& wt,
                                 double* mean, double* var, double* q, double* s, double* term, int* cmin, int rule, int* info, hipStream_t st) {
    hipLaunchKernelGGL(ahead_multi_check_kernel, dim3(1), dim3(256), 0, st, origins, n, nh, cmin, info);
    const dim3 grid((unsigned)((n + 3) / 4));
    const double* a = A + (size_t)n * lda;
#define GPAR_AHM_ROWS(NH)                                                                                                                    \
    case NH:                                                                                                                                 \
        hipLaunchKernelGGL(ahead_multi_rows_kernel<NH>, grid, dim3(256), 0, st, A, lda, n, a, y, incy, origins, wt, mean, var, q, s, term, rule, \
                           info);                                                                                                            \
        break;
    switch (nh) {
        GPAR_AHM_ROWS(1) GPAR_AHM_ROWS(2) GPAR_AHM_ROWS(3) GPAR_AHM_ROWS(4) GPAR_AHM_ROWS(5) GPAR_AHM_ROWS(6) GPAR_AHM_ROWS(7) GPAR_AHM_ROWS(8)
    }
#undef GPAR_AHM_ROWS
}

// ahead_weights_run for K horizons: the same launches with the multi-horizon kernels, the two products unchanged
static int ahead_multi_weights_run(const double* A, int lda, int n, const double* y, long incy, const int* origins, int nh, const AheadWeights& wt,
                                   double* mean, double* var, double* vec, const double* X, int ldx, double* W, int ldw, int rule, int* info,
                                   hipStream_t st) {
    const size_t kn = (size_t)nh * n;
    double *q = vec, *s = vec + kn, *term = vec + 2 * kn, *abar = vec + 3 * kn, *T = vec + ahm_off_t(n, nh);
    int* cmin = reinterpret_cast<int*>(vec + 3 * kn + n);
    const int ldt = ah_ldt(n), nt = gpar_ceil_div(n, AH_T);
    const double* a = A + (size_t)n * lda;
    ahead_multi_rows_run(A, lda, n, y, incy, origins, nh, wt, mean, var, q, s, term, cmin, rule, info, st);
    hipLaunchKernelGGL(ahead_multi_abar_kernel, dim3((unsigned)nt), dim3(256), 0, st, A, lda, n, (const double*)q, origins, nh, abar,
                       (const int*)info);
    hipLaunchKernelGGL(ahead_multi_band_kernel, dim3((unsigned)nt, (unsigned)nt), dim3(256), ahm_band_lds_bytes(nh), st, A, lda, n, a,
                       (const double*)q, (const double*)s, (const double*)abar, origins, nh, (const int*)cmin, W, ldw, (const int*)info);
    int rc = gemm_launch(0, 1, n, n, n, 1.0, X, ldx, W, ldw, 0.0, T, ldt, GPAR_GEMM_K_FROM_ROW, st);
    if (!rc) rc = gemm_launch(0, 1, n, n, n, 1.0, X, ldx, T, ldt, 0.0, W, ldw, GPAR_GEMM_C_LOWER | GPAR_GEMM_K_FROM_ROW, st);
    return rc;
}

}  // namespace gpar
