// Sliding-window forecast scoring of one dense layer (ABI v16): rolling-origin forecasts from a WINDOW of rows instead of every earlier row.
// With K = k + diag(noise / w) + eps I as the expanding form builds it and the rows in the order given, the scored row t = r is predicted
// from the run S = lo[r] ... origin[r] - 1 alone (origin[r] = -1: not scored; lo[r] = origin[r]: from the prior; at most
// GPAR_AHEAD_WINDOW_MAX rows).  On J = S u {t}, t last, K_JJ = G G^T:
//     z = G^-1 y_J,   e_r = y_t - mean_r = G_tt z_t,   v_r = var_r = G_tt^2          (the identity of ahead.h on the block J),
//     c = [-K_SS^-1 k_St; 1] = G_tt G^-T e_t,   p = [K_SS^-1 y_S; 0] = [G_SS^-T z_S; 0],   e = c^T y_J,  v = c^T K_JJ c,
//     value = sum_scored term(e_r, v_r),   dvalue/dtheta = 1/2 sum_ab W_ab dK_ab/dtheta,   W = sum_r scatter_J(W^r),
//     W^r = -2 s_r c c^T + q_r (p c^T + c p^T)      (q_r = -dterm/de, s_r = -dterm/dv: score.h)
// - no n x n factorisation, no X = L^-T, no n^3 product: n factorisations of at most 65 rows behind the Gram build.  With lo = 0, horizon 1,
// every row scored and the log rule, W = alpha alpha^T - K^-1.
// Three launches behind the Gram build: ahead_window_check_kernel (the ranges and the order of lo and origin), ahead_window_rows_kernel (one
// workgroup per row: e, v, the value term, q, s, and c, p compactly), ahead_window_gather_kernel (W on its lower triangle, every entry the
// sum of the rows whose blocks hold it, in increasing r).  Every kernel behind the check returns at once when the info word is set: a
// call the check fails leaves the value, the means, the variances and the gradient outputs as they were; after a non-positive pivot the
// value and the gradient outputs are, and the rows whose own blocks were sound have written their means and variances.  No workgroup
// waits on another one and no sum uses an atomic: every sum has a fixed order.
#pragma once

namespace gpar {

// (AW_LD = GPAR_AHEAD_WINDOW_MAX + 1, AW_VEC and AW_LDS_BYTES - the tile and three vectors: y_J -> z and the two right-hand sides - stand
// beside the kernel's declaration ahead of gpar_init, which registers the kernel's dynamic LDS)
constexpr int AW_CP = 2 * AW_LD;                   // doubles of a row's c and p in the workspace
constexpr int AW_T = 32;                           // tile edge of ahead_window_gather_kernel
static_assert(AW_LD == CV_LD, "ahead_window_rows_kernel factors its tile with cv_chol_lower");

// `vec` of the gradient form: value terms, q, s (n each), then c and p of row r in the AW_CP doubles at 3 n + r AW_CP; of the value-only
// form: the n value terms.
inline long long aw_workspace_doubles(int n, int grad) {
    if (n <= 0) return 0;
    return grad ? (3LL + AW_CP) * n : n;
}

// One workgroup.  A scored row r is well-formed when 0 <= lo[r] <= origin[r] <= r, origin[r] - lo[r] <= GPAR_AHEAD_WINDOW_MAX and neither
// lo[r] nor origin[r] lies below that of an earlier scored row.  n + 1 + r of the first row that is not into info (the first to report
// stays), and nothing else.  Thread t walks the rows [t len, (t + 1) len): the largest lo and origin of its scored rows, an exclusive
// running maximum over the threads in LDS, then the walk again with what lies before it.
__global__ __launch_bounds__(256) void ahead_window_check_kernel(const int* __restrict__ lo, const int* __restrict__ origin, int n,
                                                                 int* __restrict__ info) {
    __shared__ int ml[256], mo[256], sm[256];
    const int t = threadIdx.x;
    const int len = (n + 255) / 256, r0 = min(n, t * len), r1 = min(n, r0 + len);
    int top_l = -1, top_o = -1;
    for (int r = r0; r < r1; ++r) {
        const int o = origin[r];
        if (o < 0) continue;
        top_l = max(top_l, lo[r]);
        top_o = max(top_o, o);
    }
    ml[t] = top_l;
    mo[t] = top_o;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {   // inclusive running maxima
        const int a = t >= off ? ml[t - off] : -1, b = t >= off ? mo[t - off] : -1;
        __syncthreads();
        ml[t] = max(ml[t], a);
        mo[t] = max(mo[t], b);
        __syncthreads();
    }
    int before_l = t > 0 ? ml[t - 1] : -1, before_o = t > 0 ? mo[t - 1] : -1;
    int bad = AH_NONE;
    for (int r = r0; r < r1 && bad == AH_NONE; ++r) {
        const int o = origin[r];
        if (o == -1) continue;
        const int l = lo[r];
        if (o < -1 || o > r || l < 0 || l > o || o - l > GPAR_AHEAD_WINDOW_MAX || l < before_l || o < before_o) bad = r;
        before_l = l;
        before_o = o;
    }
    sm[t] = bad;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) sm[t] = min(sm[t], sm[t + off]);
        __syncthreads();
    }
    if (t == 0 && sm[0] != AH_NONE) atomicCAS(info, 0, n + 1 + sm[0]);
}

// One workgroup per row, everything in dynamic LDS (AW_LDS_BYTES).  The lower triangle of K_JJ comes from the lower triangle of K, is
// factored in place, right-looking (cv_chol_lower), and y_J is taken through the forward substitution behind it; thread 0 turns (e, v)
// into the value term, q and s (score_row) and writes the mean and the variance.  With `cp` (the gradient form) two backward
// substitutions run side by side - G^T c' = G_tt e_t over the block, G_SS^T p_S = z_S over its leading rows -, thread k storing entry k.
// A non-positive pivot: the 1-based row of K into info, nothing written for the row.  An unscored row: NaN in its mean and variance.
__global__ __launch_bounds__(256) void ahead_window_rows_kernel(const double* __restrict__ K, int ldk, int n, const double* __restrict__ y,
                                                                long incy, const int* __restrict__ lo, const int* __restrict__ origin,
                                                                double* __restrict__ mean, double* __restrict__ var, double* __restrict__ q,
                                                                double* __restrict__ s, double* __restrict__ term, double* __restrict__ cp,
                                                                int rule, int* __restrict__ info) {
    extern __shared__ double aw_sm[];
    if (info[0] != 0) return;
    const int r = blockIdx.x, t = threadIdx.x;
    const int hi = origin[r];
    if (hi < 0) {
        if (t == 0) {
            mean[r] = var[r] = __builtin_nan("");
            term[r] = 0.0;
            if (q) q[r] = s[r] = 0.0;
        }
        return;
    }
    const int l = lo[r], m = hi - l, m1 = m + 1;   // (the check has passed: 0 <= m <= GPAR_AHEAD_WINDOW_MAX, l + m <= r < n)
    double* T = aw_sm;
    double* yv = T + AW_LD * AW_LD;
    double* bc = yv + AW_VEC;
    double* bp = bc + AW_VEC;
    for (int idx = t; idx < m1 * m1; idx += 256) {
        const int i = idx / m1, j = idx - i * m1;
        if (j <= i) T[i * AW_LD + j] = K[(size_t)(i < m ? l + i : r) * ldk + (j < m ? l + j : r)];
    }
    if (t < m1) yv[t] = y[(size_t)(t < m ? l + t : r) * incy];
    __syncthreads();
    const int bad = cv_chol_lower(T, m1, t);
    if (bad) {
        if (t == 0) atomicCAS(info, 0, (bad <= m ? l + bad - 1 : r) + 1);
        return;
    }
    for (int k = 0; k < m1; ++k) {   // z = G^-1 y_J, column by column
        const double zk = yv[k] / T[k * AW_LD + k];
        __syncthreads();
        if (t == k) yv[k] = zk;
        else if (t > k && t < m1) yv[t] = fma(-T[t * AW_LD + k], zk, yv[t]);
        __syncthreads();
    }
    const double gtt = T[m * AW_LD + m];
    if (t == 0) {
        const double e = gtt * yv[m], v = gtt * gtt;
        double tr, qr, sr;
        score_row(rule, e, v, tr, qr, sr);
        mean[r] = y[(size_t)r * incy] - e;
        var[r] = v;
        term[r] = tr;
        if (q) {
            q[r] = qr;
            s[r] = sr;
        }
    }
    if (!cp) return;
    if (t < m1) {
        bc[t] = t == m ? gtt : 0.0;
        bp[t] = t < m ? yv[t] : 0.0;
    }
    __syncthreads();
    double* cr = cp + (size_t)r * AW_CP;
    double* pr = cr + AW_LD;
    for (int k = m; k >= 0; --k) {   // row k of G holds column k of G^T: the threads left of the diagonal read along it
        const double d = T[k * AW_LD + k];
        const double xc = bc[k] / d, xp = bp[k] / d;
        if (t == k) {
            cr[k] = xc;
            pr[k] = xp;
        } else if (t < k) {
            const double g = T[k * AW_LD + t];
            bc[t] = fma(-g, xc, bc[t]);
            bp[t] = fma(-g, xp, bp[t]);
        }
        __syncthreads();
    }
}

// Tile (bi, bj), bj <= bi, of the lower triangle of W.  Entry (a, b), a >= b, lies in the block of row r when a and b both lie in
// lo[r] ... origin[r] - 1 or are r itself: r = a (its own row of the block), or r > a with lo[r] <= b and origin[r] > a - a run of rows,
// because lo and origin do not decrease.  The workgroup first finds the first and the last row whose block meets the tile (a scan of lo
// and origin from the tile's first row on, min and max through LDS), then every thread walks that run in increasing r for its four
// entries: thread (ty, tx) holds column j0 + tx and rows i0 + ty + 8 k.  A tile no block meets is written as zeros.  c and p are read
// where the rows kernel left them (130 doubles a row, shared by the whole workgroup).
__global__ __launch_bounds__(256) void ahead_window_gather_kernel(const double* __restrict__ cp, const double* __restrict__ q,
                                                                  const double* __restrict__ s, const int* __restrict__ lo,
                                                                  const int* __restrict__ origin, int n, double* __restrict__ W, int ldw,
                                                                  const int* __restrict__ info) {
    __shared__ int first[256], last[256];
    const int bj = blockIdx.x, bi = blockIdx.y;
    if (bj > bi || info[0] != 0) return;
    const int t = threadIdx.x, tx = t & (AW_T - 1), ty = t / AW_T;
    const int i0 = bi * AW_T, j0 = bj * AW_T, i1 = min(n, i0 + AW_T) - 1, j1 = min(n, j0 + AW_T) - 1;
    int rmin = AH_NONE, rmax = -1;
    for (int r = i0 + t; r < n; r += 256) {   // (a block holds no row behind its own: rows before the tile's first add nothing to it)
        const int o = origin[r];
        if (o < 0) continue;
        const int l = lo[r];
        if (l > j1) break;   // (lo does not decrease: nor does any later block reach the tile's columns)
        if (r <= i1 || (o > i0 && o > j0)) {
            rmin = min(rmin, r);
            rmax = max(rmax, r);
        }
    }
    first[t] = rmin;
    last[t] = rmax;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
            first[t] = min(first[t], first[t + off]);
            last[t] = max(last[t], last[t + off]);
        }
        __syncthreads();
    }
    rmin = first[0];
    rmax = last[0];
    const int b = j0 + tx;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = rmin; r <= rmax; ++r) {
        const int o = origin[r];
        if (o < 0) continue;
        const int l = lo[r], m = o - l;
        const int jb = b == r ? m : (b >= l && b < o ? b - l : -1);
        if (jb < 0) continue;
        const double* c = cp + (size_t)r * AW_CP;
        const double* p = c + AW_LD;
        const double qr = q[r], s2 = -2.0 * s[r];
        const double cb = c[jb], pb = p[jb];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int a = i0 + ty + 8 * k;
            const int ia = a == r ? m : (a >= l && a < o ? a - l : -1);
            if (ia < 0 || a < b) continue;
            const double ca = c[ia], pa = p[ia];
            acc[k] += fma(s2 * ca, cb, qr * fma(pa, cb, ca * pb));
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int a = i0 + ty + 8 * k;
        if (a < n && b < n && a >= b) W[(size_t)a * ldw + b] = acc[k];
    }
}

static int aw_check_args(const int* lo, const int* origin, int score) {
    if (!lo || !origin) return GPAR_ARG_ERROR(1);
    if (!score_known(score)) return GPAR_ARG_ERROR(14);
    return 0;
}

// features, observations and the Gram matrix as dense_factor_run opens (the prep kernel clears the info word and the log-determinant
// word, which stays 0: nothing is factored whole), then the check and the rows.  q, s, cp null: the value-only form.
static int ahead_window_rows_run(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                                 const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* logdet,
                                 const int* lo, const int* origin, double* mean, double* var, double* q, double* s, double* term, double* cp,
                                 int rule, int* info, hipStream_t st) {
    if (fs->dz < 0 || fs->dz > GPAR_MAX_DIMS) return GPAR_ARG_ERROR(2);
    if (ks->nfactors < 0 || ks->nfactors > GPAR_MAX_FACTORS || !kspec_cos_embed_ok(fs, ks)) return GPAR_ARG_ERROR(3);
    const long total = (long)n * fs->dz > (long)n + 1 ? (long)n * fs->dz : (long)n + 1;
    hipLaunchKernelGGL(dense_grad_prep_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, *fs, x, n, ldx, z, zd, ldz, y, incy, A, lda,
                       logdet, info);
    const int rc = gram_launch(ks, z, n, ldz, z, n, ldz, fs->dz, A, lda, GPAR_GRAM_LOWER, noise_diag, jitter, nullptr, st);
    if (rc) return rc;
    GPAR_HIP_TRY(gpar_set_max_lds(reinterpret_cast<const void*>(&ahead_window_rows_kernel), AW_LDS_BYTES));
    hipLaunchKernelGGL(ahead_window_check_kernel, dim3(1), dim3(256), 0, st, lo, origin, n, info);
    hipLaunchKernelGGL(ahead_window_rows_kernel, dim3((unsigned)n), dim3(256), (size_t)AW_LDS_BYTES, st, (const double*)A, lda, n, y, incy, lo, origin,
                       mean, var, q, s, term, cp, rule, info);
    return 0;
}

}  // namespace gpar
