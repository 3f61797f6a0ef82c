// Purged (hv-block) blocked cross-validation of one dense layer (ABI v14): the kernels between K^-1 and the product W <- -2 P (C P).
// Fold f scores the rows F = [fold_start[f], fold_start[f + 1]) and is predicted from the rows outside H = [hold_lo[f], hold_hi[f]), H
// containing F: the rows G = H \ F on either side of the fold - the purge - are neither scored nor conditioned on.  With P = S^-1,
// alpha = P y and the block P_HH ordered (G left, G right, F) and factored, P_HH = L L^T, N = L^-1, w = N alpha_H:
//   - the leading |G| pivots factor P_GG, the trailing ones the Schur complement Dt = P_FF - P_FG P_GG^-1 P_GF, and w_F = L_Dt^-1 alphat;
//   - e = Sigma alpha_H = N^T w (Sigma = P_HH^-1), whose F rows are bt = Dt^-1 alphat:  y_F | rows outside H ~ N(y_F - e_F, N_FF^T N_FF),
//     term = sum_F log L_ii - 1/2 |w_F|^2;
//   - b_H = Sigma[:, F] alphat = N_F^T w_F (N_F: the |F| trailing rows of N), g = e - b_H = N_G^T w_G (zero on F), and
//     C_H = Sigma Sm Sigma + 1/2 (e b_H^T + b_H e^T) = 1/2 (N_F^T N_F + e e^T - g g^T)        (Sm = 1/2 (Dt - alphat alphat^T) on F):
//     symmetric, indefinite through - g g^T, and equal to cv's 1/2 (D_F^-1 + b_F b_F^T) when G is empty.
// The blocks H of neighbouring folds overlap, so C = sum_f E_H C_H E_H^T is a band matrix of half-bandwidth < max_hold.  The fold kernel
// stores the factors of C_H - row k of N_F with the scored row k, e and g with the fold's first row, each over the columns of H in the
// order of the layer - and cvg_assemble_kernel sums them into the band image Cb (n x (2 max_hold - 1), entry (r, j) at column
// j - r + max_hold - 1) and into b = sum_f E_H b_H: one thread per entry, ascending rows k (ascending folds), no atomics.  Then
// Pf = P as a full matrix (cvg_mirror_kernel), T = C Pf (cvg_band_kernel, 2 max_hold n^2 multiply-adds on the vector ALU), and the chain
// goes on with gpar_gemm.  Every kernel behind the fold kernel returns at once when the info word is set: what it would read may be
// missing.  No workgroup waits on another one; every sum has a fixed order.
#pragma once

namespace gpar {

constexpr int CVG_R = 16;   // rows of T per workgroup of cvg_band_kernel
constexpr int CVG_T = 32;   // tile edge of cvg_mirror_kernel
// two max_hold x CV_LD tiles (L, N) and four vectors (alpha_H, w, e, g): 1 KiB above cv_folds_kernel's claim, 68,608 B at max_hold = 64
constexpr int cvg_lds_bytes(int max_hold) { return (2 * max_hold * CV_LD + 4 * GPAR_CV_MAX_FOLD) * (int)sizeof(double); }

// `vec` of the gradient forms: b, value terms, u (n each), the rows' block extents (3 n ints in 2 n doubles: first row of H, one past its
// last row, "first row of its fold"), N_F, e, g (n max_hold each), the band image, then Pf (n x cvg_ldp(n)) at an even offset; of the
// value-only form: the n value terms.
inline int cvg_ldp(int n) { return n + (n & 1); }
inline long long cvg_off_n(int n) { return 5LL * n; }
inline long long cvg_off_band(int n, int mh) { return cvg_off_n(n) + 3LL * n * mh; }
inline long long cvg_off_p(int n, int mh) {
    const long long o = cvg_off_band(n, mh) + (long long)n * (2 * mh - 1);
    return o + (o & 1);
}
inline long long cvg_workspace_doubles(int n, int grad, int mh) {
    if (mh < 1 || mh > GPAR_CV_MAX_FOLD) return -1;
    if (n <= 0) return 0;
    return grad ? cvg_off_p(n, mh) + (long long)n * cvg_ldp(n) : n;
}

// fold f's extents when they are well-formed - the scored rows as cv_fold_extent wants them (a partition of [0, n) into non-empty runs),
// 0 <= lo <= start, end <= hi <= n, hi - lo <= max_hold <= GPAR_CV_MAX_FOLD, lo and hi not decreasing in f: |H|; otherwise 0
__device__ __forceinline__ int cvg_extent(const int* __restrict__ fold_start, const int* __restrict__ hold_lo, const int* __restrict__ hold_hi,
                                          int nfolds, int max_hold, int n, int f, int& start, int& end, int& lo) {
    start = fold_start[f];
    end = fold_start[f + 1];
    lo = hold_lo[f];
    const int hi = hold_hi[f];
    bool ok = start >= 0 && end <= n && end > start && (f > 0 || start == 0) && (f < nfolds - 1 || end == n) && lo >= 0 && hi <= n &&
              lo <= start && hi >= end && hi - lo <= max_hold && max_hold >= 1 && max_hold <= GPAR_CV_MAX_FOLD;
    if (ok && f > 0) ok = hold_lo[f - 1] <= lo && hold_hi[f - 1] <= hi;
    return ok ? hi - lo : 0;
}

// One workgroup per fold, everything in LDS.  Position p of the block's order (G left, G right, F) is row_of(p) of the layer.  alpha_H as
// trmv_upper_kernel forms it (one wave per row; the scored rows write theirs to `alpha`); P_HH = L L^T in place (cv_chol_lower: the
// leading pivots are P_GG's, the trailing ones Dt's); N = L^-1 column by column into the second tile; w = N alpha_H; e, g, the means,
// the marginal variances, the fold's value term (wave 0, a fixed butterfly) at the fold's first row of `term` and zeros behind it.  With
// Nrow: the factors of C_H and the rows' block extents (file comment).  A non-positive pivot: the 1-based row of the layer it belongs to
// into info (the first to report stays); malformed extents: n + 1 + fold, with nothing else touched.
__global__ __launch_bounds__(256) void cvg_folds_kernel(const double* __restrict__ P, int ldp, int n, const double* __restrict__ X, int ldx,
                                                        const double* __restrict__ zrow, const double* __restrict__ y, long incy,
                                                        const int* __restrict__ fold_start, const int* __restrict__ hold_lo,
                                                        const int* __restrict__ hold_hi, int nfolds, int max_hold, double* __restrict__ alpha,
                                                        double* __restrict__ mean, double* __restrict__ var, double* __restrict__ term,
                                                        double* __restrict__ Nrow, double* __restrict__ EF, double* __restrict__ GF,
                                                        int* __restrict__ meta, int* __restrict__ info) {
    extern __shared__ double cvg_sm[];
    const int f = blockIdx.x, t = threadIdx.x, lane = t & 63;
    int s, e, lo;
    const int mh = cvg_extent(fold_start, hold_lo, hold_hi, nfolds, max_hold, n, f, s, e, lo);
    if (mh == 0) {
        if (t == 0) atomicCAS(info, 0, n + 1 + f);
        return;
    }
    const int m = e - s, gl = s - lo, g = mh - m;
    auto row_of = [&](int p) { return p < gl ? lo + p : p < g ? e + (p - gl) : s + (p - g); };
    double* TA = cvg_sm;
    double* TB = TA + max_hold * CV_LD;
    double* al = TB + max_hold * CV_LD;
    double* wv = al + GPAR_CV_MAX_FOLD;
    double* ev = wv + GPAR_CV_MAX_FOLD;
    double* gv = ev + GPAR_CV_MAX_FOLD;
    for (int i = t >> 6; i < mh; i += 4) {
        const int r = row_of(i);
        const double a = trmv_upper_row(X, n, ldx, zrow, 1, r, lane);
        if (lane == 0) {
            al[i] = a;
            if (alpha && i >= g) alpha[r] = a;
        }
    }
    for (int idx = t; idx < mh * mh; idx += 256) {
        const int i = idx / mh, j = idx - i * mh;
        if (j > i) continue;
        const int ri = row_of(i), rj = row_of(j);   // (P is given by its lower triangle)
        TA[i * CV_LD + j] = ri >= rj ? P[(size_t)ri * ldp + rj] : P[(size_t)rj * ldp + ri];
    }
    if (t < m) term[s + t] = 0.0;
    __syncthreads();
    const int bad = cv_chol_lower(TA, mh, t);
    if (bad) {
        if (t == 0) atomicCAS(info, 0, row_of(bad - 1) + 1);
        return;
    }
    const double log_g = (t >= g && t < mh) ? log(TA[t * CV_LD + t]) : 0.0;   // 1/2 log|Dt| = sum_F log L_ii
    if (t < mh) {   // column t of N = L^-1 by forward substitution (below the diagonal; nothing above it is read)
        for (int i = t; i < mh; ++i) {
            double acc = i == t ? 1.0 : 0.0;
            for (int k = t; k < i; ++k) acc = fma(-TA[i * CV_LD + k], TB[k * CV_LD + t], acc);
            TB[i * CV_LD + t] = acc / TA[i * CV_LD + i];
        }
    }
    __syncthreads();
    if (t < mh) {
        double acc = 0.0;
        for (int k = 0; k <= t; ++k) acc = fma(TB[t * CV_LD + k], al[k], acc);
        wv[t] = acc;
    }
    __syncthreads();
    double w2 = 0.0;
    if (t < mh) {   // column t of N against w: its G rows give g_t, its F rows (b_H)_t and, squared, the variance
        double gg = 0.0, bb = 0.0, vv = 0.0;
        for (int k = t; k < g; ++k) gg = fma(TB[k * CV_LD + t], wv[k], gg);
        for (int k = t > g ? t : g; k < mh; ++k) {
            const double nk = TB[k * CV_LD + t];
            bb = fma(nk, wv[k], bb);
            vv = fma(nk, nk, vv);
        }
        ev[t] = gg + bb;
        gv[t] = gg;
        if (t >= g) {
            const int r = s + (t - g);
            mean[r] = y[(size_t)r * incy] - bb;
            var[r] = vv;
            w2 = wv[t] * wv[t];
        }
    }
    if (t < 64) {
        const double v = wave_sum(log_g - 0.5 * w2);
        if (t == 0) term[s] = v;
    }
    if (!Nrow) return;
    __syncthreads();
    // column c of H in the order of the layer is position pos(c) of the block's order
    auto pos = [&](int c) { return c < gl ? c : c < gl + m ? g + (c - gl) : gl + (c - gl - m); };
    for (int idx = t; idx < m * mh; idx += 256) {
        const int i = idx / mh, c = idx - i * mh;
        const int p = pos(c);
        Nrow[(size_t)(s + i) * max_hold + c] = p <= g + i ? TB[(g + i) * CV_LD + p] : 0.0;
    }
    if (t < mh) {
        const int p = pos(t);
        EF[(size_t)s * max_hold + t] = ev[p];
        GF[(size_t)s * max_hold + t] = gv[p];
    }
    if (t < m) {
        meta[3 * (s + t)] = lo;
        meta[3 * (s + t) + 1] = lo + mh;
        meta[3 * (s + t) + 2] = t == 0;
    }
}

// One wave per row r, lane d for the entry (r, j = r - d) of the band, d < max_hold:
//   C_rj = 1/2 sum_k [N_kr N_kj + first(k) (e_r e_j - g_r g_j)]  over the scored rows k whose block holds r and j (all lie in
// [r - max_hold + 1, j + max_hold - 1]), ascending; stored at (r, j) and (j, r).  Lane 0 also sums b_r = sum (e_r - g_r) over the same folds.
__global__ __launch_bounds__(256) void cvg_assemble_kernel(int n, int max_hold, const double* __restrict__ Nrow, const double* __restrict__ EF,
                                                           const double* __restrict__ GF, const int* __restrict__ meta, double* __restrict__ Cb,
                                                           double* __restrict__ bvec, const int* __restrict__ info) {
    if (info[0] != 0) return;
    const int d = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int j = r - d;
    if (r >= n || d >= max_hold || j < 0) return;
    const int k0 = r - (max_hold - 1) > 0 ? r - (max_hold - 1) : 0;
    const int k1 = j + max_hold - 1 < n - 1 ? j + max_hold - 1 : n - 1;
    double acc = 0.0, bs = 0.0;
    for (int k = k0; k <= k1; ++k) {
        const int lo = meta[3 * k], hi = meta[3 * k + 1];
        if (lo > j || r >= hi) continue;
        const size_t at = (size_t)k * max_hold;
        const int cr = r - lo, cj = j - lo;
        acc = fma(Nrow[at + cr], Nrow[at + cj], acc);
        if (meta[3 * k + 2]) {
            acc = fma(EF[at + cr], EF[at + cj], acc);
            acc = fma(-GF[at + cr], GF[at + cj], acc);
            if (d == 0) bs += EF[at + cr] - GF[at + cr];
        }
    }
    const int bw = 2 * max_hold - 1;
    Cb[(size_t)r * bw + (max_hold - 1 - d)] = 0.5 * acc;
    Cb[(size_t)j * bw + (max_hold - 1 + d)] = 0.5 * acc;
    if (d == 0) bvec[r] = bs;
}

// blocks [0, nt^2), nt = ceil(n / 32): tile (bi, bj), bj <= bi, of the lower triangle of P through LDS to (bi, bj) and, transposed, to
// (bj, bi) of the full matrix Pf, both stores along rows; the blocks behind them: u = P b (sym_lower_matvec_rows).
__global__ __launch_bounds__(256) void cvg_mirror_kernel(const double* __restrict__ P, int ldp, int n, const double* __restrict__ bvec,
                                                         double* __restrict__ u, double* __restrict__ Pf, int ldf, const int* __restrict__ info) {
    __shared__ double tile[CVG_T][CVG_T + 1];
    if (info[0] != 0) return;
    const int nt = (n + CVG_T - 1) / CVG_T;
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= nt * nt) {
        sym_lower_matvec_rows(P, ldp, n, bvec, u, b - nt * nt, t);
        return;
    }
    const int bi = b / nt, bj = b - bi * nt;
    if (bj > bi) return;
    const int tx = t & 31, ty = t >> 5;
    const int r0 = bi * CVG_T, c0 = bj * CVG_T;
    for (int r = ty; r < CVG_T; r += 8) {
        const int gr = r0 + r, gc = c0 + tx;
        tile[r][tx] = (gr < n && gc <= gr) ? P[(size_t)gr * ldp + gc] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < CVG_T; r += 8) {
        const int gr = r0 + r, gc = c0 + tx;
        if (gr < n && gc < n) Pf[(size_t)gr * ldf + gc] = (bi == bj && tx > r) ? tile[tx][r] : tile[r][tx];
        const int mr = c0 + r, mc = r0 + tx;
        if (bi != bj && mr < n && mc < n) Pf[(size_t)mr * ldf + mc] = tile[tx][r];
    }
}

// T = C Pf for the band image Cb of C: workgroup (bx, by) forms rows [16 by, 16 by + 16) of T at columns [256 bx, 256 bx + 256), one
// column per thread.  The rows' band entries meet in LDS, laid out by the column j they multiply (zero outside the band and the matrix);
// every row j of Pf the band reaches is read once, along the row, and used 16 times.
__global__ __launch_bounds__(256) void cvg_band_kernel(const double* __restrict__ Cb, int n, int max_hold, const double* __restrict__ Pf, int ldf,
                                                       double* __restrict__ T, int ldt, const int* __restrict__ info) {
    __shared__ double cs[CVG_R][2 * GPAR_CV_MAX_FOLD - 2 + CVG_R];
    if (info[0] != 0) return;
    const int t = threadIdx.x;
    const int r0 = blockIdx.y * CVG_R, c = blockIdx.x * 256 + t;
    const int bw = 2 * max_hold - 1, wd = bw - 1 + CVG_R, jlo = r0 - (max_hold - 1);
    for (int idx = t; idx < CVG_R * wd; idx += 256) {
        const int i = idx / wd, jj = idx - i * wd;
        const int r = r0 + i, j = jlo + jj, bc = jj - i;   // (bc = j - r + max_hold - 1)
        cs[i][jj] = (r < n && j >= 0 && j < n && bc >= 0 && bc < bw) ? Cb[(size_t)r * bw + bc] : 0.0;
    }
    __syncthreads();
    if (c >= n) return;
    double acc[CVG_R];
#pragma unroll
    for (int i = 0; i < CVG_R; ++i) acc[i] = 0.0;
    const int j0 = jlo > 0 ? jlo : 0, j1 = jlo + wd < n ? jlo + wd : n;
    for (int j = j0; j < j1; ++j) {
        const double p = Pf[(size_t)j * ldf + c];
#pragma unroll
        for (int i = 0; i < CVG_R; ++i) acc[i] = fma(cs[i][j - jlo], p, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < CVG_R; ++i)
        if (r0 + i < n) T[(size_t)(r0 + i) * ldt + c] = acc[i];
}

struct CvHold {
    const int *lo, *hi;   // nfolds extents of the blocks H (device)
    int max_hold;
};

static int cvg_folds_launch(const double* P, int ldp, int n, const double* X, int ldx, const double* zrow, const double* y, long incy,
                            const int* fold_start, int nfolds, const CvHold& hold, double* alpha, double* mean, double* var, double* term,
                            double* Nrow, double* EF, double* GF, int* meta, int* info, hipStream_t st) {
    GPAR_HIP_TRY(gpar_set_max_lds(reinterpret_cast<const void*>(&cvg_folds_kernel), cvg_lds_bytes(GPAR_CV_MAX_FOLD)));
    hipLaunchKernelGGL(cvg_folds_kernel, dim3((unsigned)nfolds), dim3(256), (size_t)cvg_lds_bytes(hold.max_hold), st, P, ldp, n, X, ldx, zrow, y,
                       incy, fold_start, hold.lo, hold.hi, nfolds, hold.max_hold, alpha, mean, var, term, Nrow, EF, GF, meta, info);
    return 0;
}

// The weight stage of the gradient forms up to T: W holds P on its lower triangle and X = L^-T on entry; on return `vec` holds b, the
// value terms and u, X holds T = C P and Pf (in `vec`) P as a full matrix - the caller forms W <- -2 Pf T on the lower triangle.
static int cvg_weights_run(const double* W, int ldw, int n, double* X, int ldx, const double* zrow, const double* y, long incy,
                           const int* fold_start, int nfolds, const CvHold& hold, double* alpha, double* mean, double* var, double* vec, int* info,
                           hipStream_t st) {
    const int mh = hold.max_hold;
    double *bvec = vec, *term = vec + n, *u = vec + 2 * (size_t)n;
    int* meta = reinterpret_cast<int*>(vec + 3 * (size_t)n);
    double *Nrow = vec + cvg_off_n(n), *EF = Nrow + (size_t)n * mh, *GF = EF + (size_t)n * mh;
    double *Cb = vec + cvg_off_band(n, mh), *Pf = vec + cvg_off_p(n, mh);
    const int ldf = cvg_ldp(n);
    const int rc = cvg_folds_launch(W, ldw, n, X, ldx, zrow, y, incy, fold_start, nfolds, hold, alpha, mean, var, term, Nrow, EF, GF, meta, info, st);
    if (rc) return rc;
    hipLaunchKernelGGL(cvg_assemble_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, n, mh, (const double*)Nrow, (const double*)EF,
                       (const double*)GF, (const int*)meta, Cb, bvec, (const int*)info);
    const int nt = gpar_ceil_div(n, CVG_T);
    hipLaunchKernelGGL(cvg_mirror_kernel, dim3((unsigned)(nt * nt + (n + 3) / 4)), dim3(256), 0, st, W, ldw, n, (const double*)bvec, u, Pf, ldf,
                       (const int*)info);
    hipLaunchKernelGGL(cvg_band_kernel, dim3(gpar_ceil_div(n, 256), gpar_ceil_div(n, CVG_R)), dim3(256), 0, st, (const double*)Cb, n, mh,
                       (const double*)Pf, ldf, X, ldx, (const int*)info);
    return 0;
}

}  // namespace gpar
