// libgpar_hip.so — C ABI (include/gpar_hip.h) over the gfx950 kernels.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC gpar_hip.hip -o ../libgpar_hip.so
#include <mutex>
#include <string.h>
#include "common.h"
#include "gemm_f64.h"
#include "potrf.h"
#include "panel.h"
#include "panel2.h"
#include "gram.h"
#include "gram_jit.h"
#include "grad_jit.h"
#include "blas1.h"
#include "pivchol.h"
#include "chol_update.h"
#include "score.h"   // the scoring rules of the held-out objectives
#include "periodogram.h"   // generalised Lomb-Scargle periodogram (gpar_periodogram)
#include "gram_terms.h"   // posterior decomposition by kernel component: its kernels and the chain of gpar_posterior_terms
#include "gram_deriv.h"   // posterior derivatives: the kernels and the chain of gpar_posterior_deriv
#include "pathwise.h"   // pathwise posterior sampling: gpar_rff_apply, gpar_gram_apply_groups
#include "gram_grad_rows.h"   // per-row gradient moment sums: the kernels and the chain of gpar_gram_grad_rows

namespace gpar {

// Philox-4x32-10 (Salmon et al. 2011).  counter = (pair index lo, hi, offset lo, hi), key = seed.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&r)[4]) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += W0; k1 += W1;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

__global__ __launch_bounds__(256) void randn_kernel(uint64_t seed, uint64_t offset, double* __restrict__ out, int rows,
                                                    int cols, int ldo) {
    const size_t total = (size_t)rows * cols;
    const size_t pair = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pair * 2 >= total) return;
    uint32_t r[4];
    philox4x32_10((uint32_t)pair, (uint32_t)(pair >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed,
                  (uint32_t)(seed >> 32), r);
    const uint64_t a = ((uint64_t)r[1] << 32) | r[0], b = ((uint64_t)r[3] << 32) | r[2];
    const double u1 = ((double)(a >> 11) + 0.5) * 1.1102230246251565404e-16;  // (0, 1)
    const double u2 = ((double)(b >> 11) + 0.5) * 1.1102230246251565404e-16;
    const double rad = sqrt(-2.0 * log(u1));
    const double ang = 6.283185307179586476925286766559 * u2;
    const double zv[2] = {rad * cos(ang), rad * sin(ang)};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const size_t idx = pair * 2 + e;
        if (idx < total) {
            const size_t rr = idx / cols, cc = idx - rr * cols;
            out[rr * ldo + cc] = zv[e];
        }
    }
}

}  // namespace gpar

using namespace gpar;

// ---- y = L x for a lower-triangular L and one vector: one wave per row, lanes stride the row (coalesced), wave reduce
__global__ __launch_bounds__(256) void trmv_lower_kernel(const double* __restrict__ L, int n, int ldl, const double* __restrict__ x,
                                                         int incx, double* __restrict__ y, int incy) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const double* Lr = L + (size_t)row * ldl;
    double a0 = 0.0, a1 = 0.0;
    int j = lane;
    for (; j + 64 <= row; j += 128) {
        a0 = fma(Lr[j], x[(size_t)j * incx], a0);
        a1 = fma(Lr[j + 64], x[(size_t)(j + 64) * incx], a1);
    }
    if (j <= row) a0 = fma(Lr[j], x[(size_t)j * incx], a0);
    double s = a0 + a1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) y[(size_t)row * incy] = s;
}

// ---- y = U x for an UPPER-triangular U (row i: columns i .. n - 1; the strict lower triangle is never read) and one vector:
// one wave per row, lanes stride the row, wave reduce.  alpha = (L L^T)^-1 y = L^-T (L^-1 y) = X z with X = L^-T, which the
// inverse of the gradient pass has just formed: n^2 / 2 multiply-adds at memory speed instead of a backward substitution's chain of
// n / 512 block kernels with an update each (n = 4096: 8 x 31 + 7 x 8 us -> ~15 us).
__device__ __forceinline__ double trmv_upper_row(const double* __restrict__ U, int n, int ldu, const double* __restrict__ x, int incx, int row,
                                                 int lane) {
    const double* Ur = U + (size_t)row * ldu;
    double a0 = 0.0, a1 = 0.0;
    int j = row + lane;
    for (; j + 64 < n; j += 128) {
        a0 = fma(Ur[j], x[(size_t)j * incx], a0);
        a1 = fma(Ur[j + 64], x[(size_t)(j + 64) * incx], a1);
    }
    if (j < n) a0 = fma(Ur[j], x[(size_t)j * incx], a0);
    double s = a0 + a1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}
__global__ __launch_bounds__(256) void trmv_upper_kernel(const double* __restrict__ U, int n, int ldu, const double* __restrict__ x,
                                                         int incx, double* __restrict__ y, int incy) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const double s = trmv_upper_row(U, n, ldu, x, incx, row, lane);
    if (lane == 0) y[(size_t)row * incy] = s;
}

// ---- y = alpha A x for a general row-major A and one vector: one wave per row (coalesced along the row), wave reduce.  A 128-wide
// GEMM tile for ONE column is a K-long chain of stages for nothing (M = 1024: 99 us; this: ~6 us)
__global__ __launch_bounds__(256) void gemv_n_kernel(const double* __restrict__ A, int rows, int cols, int lda, const double* __restrict__ x, int incx,
                                                     double alpha, double* __restrict__ y, int incy) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const double* Ar = A + (size_t)row * lda;
    double a0 = 0.0, a1 = 0.0;
    int j = lane;
    for (; j + 64 < cols; j += 128) {
        a0 = fma(Ar[j], x[(size_t)j * incx], a0);
        a1 = fma(Ar[j + 64], x[(size_t)(j + 64) * incx], a1);
    }
    if (j < cols) a0 = fma(Ar[j], x[(size_t)j * incx], a0);
    double s = a0 + a1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) y[(size_t)row * incy] = alpha * s;
}

// ---- the same for `batch` matrices and one vector each (gridDim.y = batch): y_b = L_b x_b (+ add_b)
__global__ __launch_bounds__(256) void trmv_lower_batch_kernel(const double* __restrict__ L, long long stride_l, int n, int ldl,
                                                               const double* __restrict__ x, int incx, long long stride_x,
                                                               const double* __restrict__ add, int inca, long long stride_add,
                                                               double* __restrict__ y, int incy, long long stride_y) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const size_t b = blockIdx.y;
    const double* Lr = L + b * stride_l + (size_t)row * ldl;
    const double* xb = x + b * stride_x;
    double a0 = 0.0, a1 = 0.0;
    int j = lane;
    for (; j + 64 <= row; j += 128) {
        a0 = fma(Lr[j], xb[(size_t)j * incx], a0);
        a1 = fma(Lr[j + 64], xb[(size_t)(j + 64) * incx], a1);
    }
    if (j <= row) a0 = fma(Lr[j], xb[(size_t)j * incx], a0);
    double s = a0 + a1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) y[b * stride_y + (size_t)row * incy] = add ? s + add[b * stride_add + (size_t)row * inca] : s;
}

// ---- Monte-Carlo reduction over posterior samples (reference regression.py:589-595)
__device__ __forceinline__ double np_lerp(double a, double b, double t) {
    // numpy's _lerp: a + (b - a) t, replaced by b - (b - a)(1 - t) when t >= 0.5; numpy rounds the product and the
    // sum separately, so no fused multiply-add here
#pragma clang fp contract(off)
    const double d = b - a;
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

__global__ __launch_bounds__(256) void sample_stats_kernel(const double* __restrict__ x, int S, long long count, long long stride,
                                                           int k_lo, double g_lo, int k_hi, double g_hi, double* __restrict__ mean,
                                                           double* __restrict__ lo, double* __restrict__ hi) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    const double* col = x + e;
    double sum = 0.0;
    bool has_nan = false;
    for (int s = 0; s < S; ++s) {
        const double v = col[(long long)s * stride];
        has_nan |= (v != v);
        sum += v;
    }
    mean[e] = sum / (double)S;
    if (!lo && !hi) return;
    if (has_nan) {
        // np.percentile of a column that holds a NaN is NaN (NaN sorts last and poisons the interpolation); rank counting
        // with < and == would silently mis-rank instead
        if (lo) lo[e] = __builtin_nan("");
        if (hi) hi[e] = __builtin_nan("");
        return;
    }
    const int k_lo1 = min(k_lo + 1, S - 1), k_hi1 = min(k_hi + 1, S - 1);
    double a0 = 0.0, b0 = 0.0, a1 = 0.0, b1 = 0.0;
    for (int s = 0; s < S; ++s) {
        const double v = col[(long long)s * stride];
        int rank = 0;   // position of sample s in the stable ascending order
        for (int t = 0; t < S; ++t) {
            const double u = col[(long long)t * stride];
            rank += (u < v || (u == v && t < s)) ? 1 : 0;
        }
        if (rank == k_lo) a0 = v;
        if (rank == k_lo1) b0 = v;
        if (rank == k_hi) a1 = v;
        if (rank == k_hi1) b1 = v;
    }
    if (lo) lo[e] = np_lerp(a0, b0, g_lo);
    if (hi) hi[e] = np_lerp(a1, b1, g_hi);
}

// The library keeps process-global state (look-ahead side streams and events, the profile hook, one-time kernel
// attributes).  Entry points only ENQUEUE work, so serialising them costs nothing measurable and makes the library safe
// to call from several host threads (GPARRegressor.fit trains independent layers from two threads, each on its stream).
static std::mutex g_api_mutex;
// Every entry point also makes the device of the caller's stream current for its duration (and restores the previous one):
// the auxiliary streams and events the library creates must live on that device, whatever the calling thread's current
// device happens to be (a fresh host thread starts on device 0).
struct GparDeviceGuard {
    int prev = -1, dev = -1;
    explicit GparDeviceGuard(void* stream) {
        hipDevice_t d;
        // (a null stream is the current device's default stream: nothing to switch, and per-device state is looked up by
        // the current device)
        if (stream && hipGetDevice(&prev) == hipSuccess && hipStreamGetDevice(static_cast<hipStream_t>(stream), &d) == hipSuccess) {
            dev = (int)d;
            if (dev != prev) GPAR_HIP_IGNORE(hipSetDevice(dev));   // a failure shows up in the launch that follows
        }
    }
    ~GparDeviceGuard() {
        if (dev >= 0 && dev != prev) GPAR_HIP_IGNORE(hipSetDevice(prev));
    }
};
#define GPAR_API_GUARD                                         \
    std::lock_guard<std::mutex> gpar_api_guard(g_api_mutex);   \
    GparDeviceGuard gpar_device_guard(stream)
#define GPAR_API_GUARD_NOSTREAM std::lock_guard<std::mutex> gpar_api_guard(g_api_mutex)

static int featurize_launch(const gpar_fspec_t* fs, const double* x, int n, int ldx, double* z, int ldz, hipStream_t stream) {
    if (!fs || fs->dz < 0 || fs->dz > GPAR_MAX_DIMS) return GPAR_ARG_ERROR(2);
    if (n <= 0 || fs->dz == 0) return 0;
    const long total = (long)n * fs->dz;
    hipLaunchKernelGGL(featurize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, *fs, x, n, ldx, z, ldz);
    GPAR_LAUNCH_CHECK();
    return 0;
}

static int gram_launch(const gpar_kspec_t* ks, const double* z1, int n1, int ldz1, const double* z2, int n2, int ldz2, int dz, double* K,
                       int ldk, int flags, const double* diag_add, double diag_const, const double* row_scale, hipStream_t stream,
                       int batch = 1, long long batch_z = 0, long long batch_k = 0) {
    if (!ks || ks->nterms < 0 || ks->nterms > GPAR_MAX_TERMS || ks->nfactors < 0 || ks->nfactors > GPAR_MAX_FACTORS)
        return GPAR_ARG_ERROR(3);
    if (!kspec_cos_ok(ks)) return GPAR_ARG_ERROR(3);
    if (dz < 0 || dz > GPAR_MAX_DIMS) return GPAR_ARG_ERROR(4);
    if (n1 <= 0 || n2 <= 0) return 0;
    const int sym = (z1 == z2 && n1 == n2) ? 1 : 0;
    if ((flags & GPAR_GRAM_LOWER) && !sym) return GPAR_ARG_ERROR(5);
    const size_t lds = ((size_t)2 * (dz > 0 ? dz : 1) * GRAM_LD + GRAM_TAB_DOUBLES) * sizeof(double);
    const int nt1 = gpar_ceil_div(n1, GRAM_T), nt2 = gpar_ceil_div(n2, GRAM_T);
    dim3 grid(nt2, nt1, batch);
    if (flags & GPAR_GRAM_LOWER) grid = dim3((unsigned)((long long)nt1 * (nt1 + 1) / 2), 1, batch);
    // per-specification kernel (gram_jit.h) for problems large enough to repay its compilation; the interpreter otherwise
    if (gram_jit_launch(ks, z1, n1, ldz1, z2, n2, ldz2, dz, K, ldk, flags, diag_add, diag_const, row_scale, sym, grid, stream, batch_z, batch_k))
        return 0;
    hipLaunchKernelGGL(gram_kernel, grid, dim3(256), lds, stream, *ks, z1, n1, ldz1, z2, n2, ldz2, dz, K, ldk, flags, diag_add,
                       diag_const, row_scale, sym, batch_z, batch_k);
    GPAR_LAUNCH_CHECK();
    return 0;
}

// row n of the augmented matrix <- observations, corner / log-determinant / info word <- 0
__global__ __launch_bounds__(256) void logpdf_prepare_kernel(const double* __restrict__ y, long incy, int n, double* __restrict__ A, int lda,
                                                             double* __restrict__ logdet, int* __restrict__ info) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) A[(size_t)n * lda + i] = y[(size_t)i * incy];
    if (i == n) {
        A[(size_t)n * lda + n] = 0.0;
        logdet[0] = 0.0;
        info[0] = 0;
    }
}

__global__ void logpdf_value_kernel(const double* __restrict__ A, int lda, int n, double n_log_2pi, const double* __restrict__ logdet,
                                    double* __restrict__ value, long long batch_a = 0) {
    A += (size_t)blockIdx.x * batch_a;   // batched: one block per matrix, its words at logdet[b] / value[b]
    logdet += blockIdx.x;
    value += blockIdx.x;
    // the corner holds -|L^-1 y|^2 (potrf.h: the augmented row's Schur complement).  Two additions and an exact scaling, the
    // product n log 2 pi formed on the host: the same roundings as the host-side expression this replaces (a multiply next to
    // an add would be contracted into a fused multiply-add here), so that the fused and the separate paths return the same bits.
    value[0] = -0.5 * ((logdet[0] + n_log_2pi) - A[(size_t)n * lda + n]);
}


// ---- one call for a whole lock-step evaluation (gpar_logpdf_lockstep) ---------------------------------------------------------
// observation-noise variance and observed column of up to LOCKSTEP_CHUNK layers, by value
constexpr int LOCKSTEP_CHUNK = 64;
struct LockstepCols {
    double noise[LOCKSTEP_CHUNK];
    int ycol[LOCKSTEP_CHUNK];
};

// For layer b = blockIdx.y of the chunk: row n of its augmented matrix <- its observations, its noise diagonal noise_b / w (an IEEE
// division, as the host-side tensor expression it replaces) when weights are given, corner / log-determinant / info word <- 0.
__global__ __launch_bounds__(256) void lockstep_prepare_kernel(LockstepCols lc, const double* __restrict__ y, int ldy, const double* __restrict__ w,
                                                               int ldw, int n, double* __restrict__ nd, double* __restrict__ A, int lda,
                                                               long long stride_a, double* __restrict__ logdet, int* __restrict__ info) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    double* Ab = A + (size_t)b * stride_a;
    const int col = lc.ycol[b];
    if (i < n) {
        Ab[(size_t)n * lda + i] = y[(size_t)i * ldy + col];
        if (nd) nd[(size_t)b * n + i] = lc.noise[b] / w[(size_t)i * ldw + col];
    }
    if (i == n) {
        Ab[(size_t)n * lda + n] = 0.0;
        logdet[b] = 0.0;
        info[b] = 0;
    }
}

// value[b] as logpdf_value_kernel computes it, then total = ((0 + value[0]) + value[1]) + ... in layer order (the host-side sum it replaces)
__global__ __launch_bounds__(64) void lockstep_finish_kernel(const double* __restrict__ A, int lda, long long stride_a, int n, double n_log_2pi,
                                                             const double* __restrict__ logdet, double* __restrict__ value, int batch,
                                                             double* __restrict__ total) {
    for (int b = threadIdx.x; b < batch; b += 64) {
        const double* Ab = A + (size_t)b * stride_a;
        value[b] = -0.5 * ((logdet[b] + n_log_2pi) - Ab[(size_t)n * lda + n]);
    }
    __syncthreads();
    if (threadIdx.x == 0 && total) {
        double t = 0.0;
        for (int b = 0; b < batch; ++b) t = t + value[b];
        total[0] = t;
    }
}

// row n of the augmented factor -> a contiguous vector (alpha before its backward solve); 1/2 diag(W) -> a vector
__global__ __launch_bounds__(256) void copy_row_kernel(const double* __restrict__ src, double* __restrict__ dst, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
__global__ __launch_bounds__(256) void half_diag_kernel(const double* __restrict__ W, int ldw, int n, double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = 0.5 * W[(size_t)i * ldw + i];
}

// ---- the scalar side of the inducing-point bound (gpar_vfe_assemble / gpar_vfe_value) ------------------------------------------
// A <- [[G + diag_add I (lower triangle), .], [c^T, 0]], log-determinant and info words zeroed: one launch instead of six tensor operations
__global__ __launch_bounds__(256) void vfe_assemble_kernel(const double* __restrict__ G, int M, int ldg, const double* __restrict__ c, double diag_add,
                                                           double* __restrict__ A, int lda, double* __restrict__ logdet, int* __restrict__ info) {
    const int r = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (r < M) {
        if (j <= r) A[(size_t)r * lda + j] = G[(size_t)r * ldg + j] + (j == r ? diag_add : 0.0);
    } else {
        if (j < M) A[(size_t)M * lda + j] = c[j];
        if (j == M) {
            A[(size_t)M * lda + M] = 0.0;
            logdet[0] = 0.0;
            info[0] = 0;
        }
    }
}
// Partial sums of  ys^2, kdiag / d, log d  (n terms each) and of the diagonal of G (M terms): VFE_PARTS workgroups, block b writes
// scal[4 b .. 4 b + 3]; vfe_value_kernel adds the parts in order (a fixed summation order; one workgroup over 65536 terms with a
// logarithm and a division each took 67 us)
constexpr int VFE_PARTS = 64;
__global__ __launch_bounds__(256) void vfe_sums_kernel(const double* __restrict__ ys, const double* __restrict__ kdiag, const double* __restrict__ d, int n,
                                                       const double* __restrict__ G, int M, int ldg, double* __restrict__ scal) {
    __shared__ double sm[4][256];
    const int t = threadIdx.x, b = blockIdx.x;
    const int per_n = (n + VFE_PARTS - 1) / VFE_PARTS, per_m = (M + VFE_PARTS - 1) / VFE_PARTS;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int i = b * per_n + t; i < min(n, (b + 1) * per_n); i += 256) {
        const double y = ys[i], di = d[i];
        a0 = fma(y, y, a0);
        a1 += kdiag[i] / di;
        a2 += log(di);
    }
    for (int i = b * per_m + t; i < min(M, (b + 1) * per_m); i += 256) a3 += G[(size_t)i * ldg + i];
    sm[0][t] = a0; sm[1][t] = a1; sm[2][t] = a2; sm[3][t] = a3;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int q = 0; q < 4; ++q) sm[q][t] += sm[q][t + off];
        }
        __syncthreads();
    }
    if (t < 4) scal[4 * b + t] = sm[t][0];
}
// the bound from its pieces: -1/2 (trace + sum log d + n log 2 pi + log|A| + y^T D^-1 y - |L_A^-1 c|^2)
__global__ void vfe_value_kernel(const double* __restrict__ scal, const double* __restrict__ logdet, const double* __restrict__ A, int lda, int M,
                                 double n_log_2pi, int with_trace, double* __restrict__ out) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < VFE_PARTS; ++b)
        for (int q = 0; q < 4; ++q) s[q] += scal[4 * b + q];
    const double quad = -A[(size_t)M * lda + M];
    const double trace = with_trace ? s[1] - s[3] : 0.0;
    out[0] = -0.5 * (trace + s[2] + n_log_2pi + logdet[0] + s[0] - quad);
}

extern "C" {

int gpar_abi_version(void) { return GPAR_ABI_VERSION; }
size_t gpar_sizeof_fspec(void) { return sizeof(gpar_fspec_t); }
size_t gpar_sizeof_kspec(void) { return sizeof(gpar_kspec_t); }
size_t gpar_sizeof_layer(void) { return sizeof(gpar_layer_t); }

// The fold kernel of the blocked cross-validation (defined with its entry points below) and its dynamic LDS: two max_fold x CV_LD tiles
// and two vectors.
constexpr int CV_LD = GPAR_CV_MAX_FOLD + 1;   // (odd leading dimension: columns of a tile fall into distinct LDS banks)
constexpr int cv_lds_bytes(int max_fold) { return (2 * max_fold * CV_LD + 2 * GPAR_CV_MAX_FOLD) * (int)sizeof(double); }
constexpr int CV_LDS_BYTES = cv_lds_bytes(GPAR_CV_MAX_FOLD);   // 67,584 B of the 160 KiB a workgroup may claim on gfx950
__global__ void cv_folds_kernel(const double* __restrict__ P, int ldp, int n, const double* __restrict__ X, int ldx, const double* __restrict__ zrow,
                                const double* __restrict__ y, long incy, const int* __restrict__ fold_start, int nfolds, int max_fold,
                                double* __restrict__ alpha, double* __restrict__ mean, double* __restrict__ var, double* __restrict__ bvec,
                                double* __restrict__ term, double* __restrict__ Rm, int* __restrict__ info);

// The rows kernel of the sliding-window forecast scoring (ahead_window.h, with its entry points below) and its dynamic LDS: the tile of
// the largest block - GPAR_AHEAD_WINDOW_MAX rows and the scored one - and three vectors.
namespace gpar {
constexpr int AW_LD = GPAR_AHEAD_WINDOW_MAX + 1;   // rows of the largest block, and the (odd) leading dimension of its tile
constexpr int AW_VEC = AW_LD + 1;                  // doubles between the vectors behind the tile
constexpr int AW_LDS_BYTES = (AW_LD * AW_LD + 3 * AW_VEC) * (int)sizeof(double);   // 35,384 B: four workgroups share a compute unit's 160 KiB
__global__ void ahead_window_rows_kernel(const double* __restrict__ K, int ldk, int n, const double* __restrict__ y, long incy,
                                         const int* __restrict__ lo, const int* __restrict__ origin, double* __restrict__ mean,
                                         double* __restrict__ var, double* __restrict__ q, double* __restrict__ s, double* __restrict__ term,
                                         double* __restrict__ cp, int rule, int* __restrict__ info);
}  // namespace gpar

// Everything the library creates lazily, created now: the look-ahead side stream paired with `stream`, the event ring and
// every kernel's dynamic-LDS attribute on the device that owns `stream`.  After it, entry points called
// on `stream` make no HIP object-creation call - the precondition of capturing them into a hipGraph (the run-time compiled
// kernels excepted: a structure is compiled at its first large launch, which must therefore happen once outside the capture).
int gpar_init(void* stream) {
    GPAR_API_GUARD;
    if (!la_init()) return -(int)hipErrorOutOfMemory;
    if (!la_side((hipStream_t)stream)) return -(int)hipErrorOutOfMemory;
    if (!spin_chain_init()) return -(int)hipErrorOutOfMemory;
    const void* big[] = {reinterpret_cast<const void*>(&gemm_f64_kernel<false, false, 0>), reinterpret_cast<const void*>(&gemm_f64_kernel<false, true, 0>),
                         reinterpret_cast<const void*>(&gemm_f64_kernel<true, false, 0>), reinterpret_cast<const void*>(&gemm_f64_kernel<true, true, 0>),
                         reinterpret_cast<const void*>(&gemm_f64_kernel<false, true, 1>), reinterpret_cast<const void*>(&gemm_f64_kernel<false, true, 0, 64>),
                         reinterpret_cast<const void*>(&gemm_f64_kernel<false, true, 1, 64>), reinterpret_cast<const void*>(&gram_grad_kernel),
                         reinterpret_cast<const void*>(&gram_input_grad_kernel)};
    for (const void* fn : big) GPAR_HIP_TRY(gpar_set_max_lds(fn, 160 * 1024));
    const void* p2[] = {reinterpret_cast<const void*>(&potrf_panel2_kernel), reinterpret_cast<const void*>(&trsm_block2_kernel),
                        reinterpret_cast<const void*>(&trsm_block2_back_kernel), reinterpret_cast<const void*>(&trinv_blocks2_kernel)};
    for (const void* fn : p2) GPAR_HIP_TRY(gpar_set_max_lds(fn, P2_LDS_BYTES));
    GPAR_HIP_TRY(gpar_set_max_lds(reinterpret_cast<const void*>(&cv_folds_kernel), CV_LDS_BYTES));
    GPAR_HIP_TRY(gpar_set_max_lds(reinterpret_cast<const void*>(&ahead_window_rows_kernel), AW_LDS_BYTES));
    return 0;
}

// ---- run-time specialisation (jit.h) ----------------------------------------------------------------------------------
static bool jit_request(int kind, const gpar_kspec_t& ks, int dz, int& jkind, int& extra, std::string& entry, std::string& source, bool want_source);

int gpar_jit_compile_check(int kind, const gpar_kspec_t* ks, int dz, const char* arch, char* log, int log_len) {
    // (no library lock: nothing shared is touched - source generation and hiprtc only -, and several threads may check at once)
    if (!ks || !arch || ks->nterms < 0 || ks->nterms > GPAR_MAX_TERMS || ks->nfactors < 0 || ks->nfactors > GPAR_MAX_FACTORS || dz < 0 ||
        dz > GPAR_MAX_DIMS || !kspec_cos_ok(ks))
        return GPAR_ARG_ERROR(1);
    std::string source, entry;
    int jkind = 0, extra = 0;
    if (!jit_request(kind, *ks, dz, jkind, extra, entry, source, true)) return GPAR_ARG_ERROR(2);
    std::string code, text;
    const bool ok = jit_compile(source, entry.c_str(), arch, code, text);
    if (log && log_len > 0) {
        const size_t n = text.size() < (size_t)(log_len - 1) ? text.size() : (size_t)(log_len - 1);
        memcpy(log, text.data(), n);
        log[n] = '\0';
    }
    return ok ? (int)code.size() : -1;
}

// Compile the kernel of `kind` for this structure and hand back the code object together with its archive key: the build step
// (gpar_amd/aot.py) collects these into gpar_aot_<arch>.bin.  Needs no GPU.  Returns the code size (> capacity: nothing copied), or -1.
long long gpar_jit_compile(int kind, const gpar_kspec_t* ks, int dz, const char* arch, void* code_out, long long capacity, char* key_out,
                           int key_len, char* log, int log_len) {
    if (!ks || !arch || ks->nterms < 0 || ks->nterms > GPAR_MAX_TERMS || ks->nfactors < 0 || ks->nfactors > GPAR_MAX_FACTORS || dz < 0 ||
        dz > GPAR_MAX_DIMS || !kspec_cos_ok(ks))
        return GPAR_ARG_ERROR(1);
    std::string source, entry;
    int jkind = 0, extra = 0;
    if (!jit_request(kind, *ks, dz, jkind, extra, entry, source, true)) return GPAR_ARG_ERROR(2);
    std::string code, text;
    const bool ok = jit_compile(source, entry.c_str(), arch, code, text);
    if (log && log_len > 0) {
        const size_t n = text.size() < (size_t)(log_len - 1) ? text.size() : (size_t)(log_len - 1);
        memcpy(log, text.data(), n);
        log[n] = '\0';
    }
    if (!ok) return -1;
    const std::string key = aot_key(jkind, *ks, dz, extra);
    if (key_out && key_len > 0) {
        const size_t n = key.size() < (size_t)(key_len - 1) ? key.size() : (size_t)(key_len - 1);
        memcpy(key_out, key.data(), n);
        key_out[n] = '\0';
    }
    if (code_out && (long long)code.size() <= capacity) memcpy(code_out, code.data(), code.size());
    return (long long)code.size();
}

// Fingerprint of the kernel generators: FNV-1a over the sources of every kernel kind for one probe structure that uses every factor
// type (EQ x RQ product, a linear term, a constant term, a product of the three Matern factors, an EQ x cosine product, a cosine
// term without an exponential; thirteen feature dims), + the ABI version.  Pure host code, needs no GPU.
unsigned long long gpar::aot_fingerprint() {
    static unsigned long long cached = 0ull;
    if (cached) return cached;
    gpar_kspec_t ks;
    memset(&ks, 0, sizeof ks);
    ks.nterms = 6;
    ks.nfactors = 9;
    ks.coef[0] = 1.0; ks.coef[1] = 1.0; ks.coef[2] = 1.0; ks.coef[3] = 1.0; ks.coef[4] = 1.0; ks.coef[5] = 1.0;
    ks.factor[0] = gpar_factor_t{GPAR_K_EQ, 0, 0, 2, 0.0};
    ks.factor[1] = gpar_factor_t{GPAR_K_RQ, 0, 2, 2, 0.5};
    ks.factor[2] = gpar_factor_t{GPAR_K_LINEAR, 1, 4, 2, 0.0};
    ks.factor[3] = gpar_factor_t{GPAR_K_MATERN12, 3, 6, 1, 0.0};
    ks.factor[4] = gpar_factor_t{GPAR_K_MATERN32, 3, 7, 1, 0.0};
    ks.factor[5] = gpar_factor_t{GPAR_K_MATERN52, 3, 8, 1, 0.0};
    ks.factor[6] = gpar_factor_t{GPAR_K_EQ, 4, 9, 1, 0.0};
    ks.factor[7] = gpar_factor_t{GPAR_K_COS, 4, 10, 2, 0.0};
    ks.factor[8] = gpar_factor_t{GPAR_K_COS, 5, 12, 1, 0.0};
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&](const std::string& text) {
        for (unsigned char ch : text) h = (h ^ ch) * 1099511628211ull;
        h = (h ^ 0xffu) * 1099511628211ull;
    };
    const int kinds[] = {JIT_GRAM, JIT_GRAD, JIT_GRAD + 10, JIT_GRAD + 20, JIT_GRAD + 30, JIT_INPUT_GRAD, JIT_INPUT_GRAD + 10};
    for (int kind : kinds) {
        std::string source, entry;
        int jkind = 0, extra = 0;
        if (jit_request(kind, ks, 13, jkind, extra, entry, source, true)) mix(entry + "\n" + source);
        else mix("-");
    }
    {   // ... and the wide form of the Gram generator (more than GRAM_JIT_MAX_DZ feature dims): the same factor types over 23 dims
        // (without the cosine term: a wide structure that holds one has no generated Gram kernel)
        gpar_kspec_t wide = ks;
        wide.nterms = 4; wide.nfactors = 6;
        wide.factor[0].nd = 8; wide.factor[1].off = 8; wide.factor[1].nd = 7; wide.factor[2].off = 15; wide.factor[2].nd = 5;
        wide.factor[3].off = 20; wide.factor[4].off = 21; wide.factor[5].off = 22;
        std::string source, entry;
        int jkind = 0, extra = 0;
        if (jit_request(JIT_GRAM, wide, 23, jkind, extra, entry, source, true)) mix(entry + "\n" + source);
        else mix("-");
    }
    mix("abi " + std::to_string(GPAR_ABI_VERSION));
    cached = h ? h : 1ull;
    return cached;
}

unsigned long long gpar_aot_fingerprint(void) { return gpar::aot_fingerprint(); }

int gpar_aot_stats(int* entries, int* loaded) {
    GPAR_API_GUARD_NOSTREAM;
    if (entries) *entries = (int)g_aot.entries.size();
    if (loaded) *loaded = g_aot.loaded;
    return 0;
}

// (kind, structure) -> what the launch paths would ask jit_get for: cache key ingredients, entry point, source
static bool jit_request(int kind, const gpar_kspec_t& ks, int dz, int& jkind, int& extra, std::string& entry, std::string& source, bool want_source) {
    if (kind == JIT_GRAM) {
        const int strip = gram_jit_strip(1 << 20, dz);
        if (strip <= 0) return false;   // wide structure: there is no generated Gram kernel (gram_jit.h)
        if (!gram_jit_serves(ks, dz)) return false;   // ... nor for a cosine factor beside more than GRAM_JIT_MAX_DZ dims
        jkind = JIT_GRAM; extra = 1; entry = "gram_jit";
        if (want_source) source = gram_jit_source(ks, dz, strip);
    } else if (kind == JIT_GRAD || kind == JIT_GRAD + 10 || kind == JIT_GRAD + 20 || kind == JIT_GRAD + 30) {
        const int mode = (kind / 10) & 1, has_zd = kind >= 20;
        jkind = JIT_GRAD; extra = 100 + mode * 2 + has_zd; entry = "gram_grad_jit";
        if (want_source) source = grad_jit_source(ks, dz, mode, has_zd);
    } else if (kind == JIT_INPUT_GRAD || kind == JIT_INPUT_GRAD + 10) {
        jkind = JIT_INPUT_GRAD; extra = 200 + kind / 10; entry = "gram_input_grad_jit";
        if (want_source) source = input_grad_jit_source(ks, dz, kind / 10);
    } else {
        return false;
    }
    return true;
}

// Compile the kernel of `kind` for this structure NOW if it is not cached yet, on the calling thread and OUTSIDE the library's
// mutex: a host that knows which structures a model will need (all layers of a GPARRegressor) calls this from several threads at
// once, so that p structures cost one compilation time instead of p, and no compilation happens inside a timed or pipelined
// evaluation (where it would also hold the mutex every other thread's launches need).  Returns 0 (ready), 1 (compilation failed:
// the interpreter will be used) or an argument error.
int gpar_jit_prepare(int kind, const gpar_kspec_t* ks, int dz, void* stream) {
    if (!ks || ks->nterms < 0 || ks->nterms > GPAR_MAX_TERMS || ks->nfactors < 0 || ks->nfactors > GPAR_MAX_FACTORS || dz < 0 || dz > GPAR_MAX_DIMS ||
        !kspec_cos_ok(ks))
        return GPAR_ARG_ERROR(1);
    int jkind = 0, extra = 0;
    std::string entry, source, key, arch;
    {
        GPAR_API_GUARD;
        if (!jit_request(kind, *ks, dz, jkind, extra, entry, source, false)) return GPAR_ARG_ERROR(2);
        key = jit_key(jkind, *ks, dz, extra);
        if (key.empty()) return -(int)hipErrorInvalidDevice;
        auto it = g_jit.cache.find(key);
        if (it != g_jit.cache.end()) return it->second.failed ? 1 : 0;
        arch = jit_device_arch();
        if (aot_install(jkind, *ks, dz, extra, key, entry.c_str(), arch)) return 0;   // compiled when the library was built
    }
    jit_request(kind, *ks, dz, jkind, extra, entry, source, true);
    std::string code, log;
    const bool ok = !arch.empty() && jit_compile(source, entry.c_str(), arch, code, log);
    {
        GPAR_API_GUARD;
        auto it = g_jit.cache.find(key);   // (another thread may have been faster)
        if (it != g_jit.cache.end()) return it->second.failed ? 1 : 0;
        return jit_install(key, code, entry.c_str(), ok, log) ? 0 : 1;
    }
}

int gpar_jit_stats(int* compiled, int* failures, int* cached) {
    GPAR_API_GUARD_NOSTREAM;
    if (compiled) *compiled = g_jit.compiled;
    if (failures) *failures = g_jit.failures;
    if (cached) *cached = (int)g_jit.cache.size();
    return 0;
}

int gpar_featurize(const gpar_fspec_t* fs, const double* x, int n, int ldx, double* z, int ldz, void* stream) {
    GPAR_API_GUARD;
    return featurize_launch(fs, x, n, ldx, z, ldz, (hipStream_t)stream);
}

int gpar_gram(const gpar_kspec_t* ks, const double* z1, int n1, int ldz1, const double* z2, int n2, int ldz2, int dz,
              double* K, int ldk, int flags, const double* diag_add, double diag_const, const double* row_scale, void* stream) {
    GPAR_API_GUARD;
    return gram_launch(ks, z1, n1, ldz1, z2, n2, ldz2, dz, K, ldk, flags, diag_add, diag_const, row_scale, (hipStream_t)stream);
}

// One dense layer's log marginal likelihood in one call (SURVEY 8(b)'s fused a2-a4; gpar/model.py:226 for a prior process):
// features -> Gram + noise + jitter into the top-left n x n of the (n + 1) x (n + 1) buffer A -> y into row n -> partial
// factorisation -> value = -1/2 (log|K| + n log 2 pi + |L^-1 y|^2).  The same launches the separate entry points make; what
// it saves is the caller's side: a Python host spends ~0.1 ms per layer on the five calls and the small tensor operations
// between them, which at n = 4096 decides when the last of four pipelined layers starts.
int gpar_logpdf_dense(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                      const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* logdet, int* info,
                      double* value, int potrf_flags, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !A || !logdet || !info || !value || (n > 0 && (!x || !y))) return GPAR_ARG_ERROR(1);
    hipStream_t st = (hipStream_t)stream;
    if (ks->nfactors < 0 || ks->nfactors > GPAR_MAX_FACTORS || !kspec_cos_embed_ok(fs, ks)) return GPAR_ARG_ERROR(3);
    int rc = featurize_launch(fs, x, n, ldx, z, ldz, st);
    if (!rc && n > 0) rc = gram_launch(ks, z, n, ldz, z, n, ldz, fs->dz, A, lda, GPAR_GRAM_LOWER, noise_diag, jitter, nullptr, st);
    if (rc) return rc;
    hipLaunchKernelGGL(logpdf_prepare_kernel, dim3(gpar_ceil_div(n + 1, 256)), dim3(256), 0, st, y, incy, n, A, lda, logdet, info);
    if (n > 0) rc = potrf_run(A, n + 1, n, lda, logdet, info, st, potrf_flags);
    if (rc) return rc;
    hipLaunchKernelGGL(logpdf_value_kernel, dim3(1), dim3(1), 0, st, (const double*)A, lda, n, (double)n * 1.8378770664093453,
                       (const double*)logdet, value);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_gram_batch(const gpar_kspec_t* ks, const double* z, int n, int ldz, long long stride_z, int dz, double* K, int ldk,
                    long long stride_k, int flags, const double* diag_add, double diag_const, int batch, void* stream) {
    GPAR_API_GUARD;
    if (batch <= 0) return 0;
    if (stride_z < 0 || stride_k < 0) return GPAR_ARG_ERROR(9);
    return gram_launch(ks, z, n, ldz, z, n, ldz, dz, K, ldk, flags, diag_add, diag_const, nullptr, (hipStream_t)stream, batch, stride_z, stride_k);
}

int gpar_logpdf_dense_build(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                            const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* logdet, int* info,
                            void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !A || !logdet || !info || (n > 0 && (!x || !y))) return GPAR_ARG_ERROR(1);
    hipStream_t st = (hipStream_t)stream;
    if (ks->nfactors < 0 || ks->nfactors > GPAR_MAX_FACTORS || !kspec_cos_embed_ok(fs, ks)) return GPAR_ARG_ERROR(3);
    int rc = featurize_launch(fs, x, n, ldx, z, ldz, st);
    if (!rc && n > 0) rc = gram_launch(ks, z, n, ldz, z, n, ldz, fs->dz, A, lda, GPAR_GRAM_LOWER, noise_diag, jitter, nullptr, st);
    if (rc) return rc;
    hipLaunchKernelGGL(logpdf_prepare_kernel, dim3(gpar_ceil_div(n + 1, 256)), dim3(256), 0, st, y, incy, n, A, lda, logdet, info);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_potrf_batch(double* A, int batch, long long stride_a, int N, int nf, int lda, double* logdet, int* info, int flags, void* stream) {
    GPAR_API_GUARD;
    if (N <= 0 || nf <= 0 || batch <= 0) return 0;
    if (!A || !logdet || !info || stride_a < 0) return GPAR_ARG_ERROR(1);
    return potrf_run_batch(A, batch, stride_a, N, nf, lda, logdet, info, (hipStream_t)stream, flags);
}

int gpar_logpdf_dense_finish(const double* A, int batch, long long stride_a, int n, int lda, const double* logdet, double* value,
                             void* stream) {
    GPAR_API_GUARD;
    if (batch <= 0) return 0;
    if (!A || !logdet || !value || n < 0) return GPAR_ARG_ERROR(1);
    hipLaunchKernelGGL(logpdf_value_kernel, dim3(batch), dim3(1), 0, (hipStream_t)stream, A, lda, n, (double)n * 1.8378770664093453, logdet,
                       value, stride_a);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_logpdf_lockstep(const gpar_layer_t* layers, int batch, const double* x, int n, int ldx, const double* y, int ldy, const double* w,
                         int ldw, double jitter, double* z, int ldz, double* nd, double* A, int lda, long long stride_a, double* logdet,
                         int* info, double* value, double* total, int potrf_flags, void* stream) {
    GPAR_API_GUARD;
    if (batch <= 0) return 0;
    if (!layers || !A || !logdet || !info || !value || stride_a < 0 || (n > 0 && (!x || !y || !z)) || (w && !nd)) return GPAR_ARG_ERROR(1);
    hipStream_t st = (hipStream_t)stream;
    for (int b = 0; b < batch; ++b)
        if (!layers[b].fs || !layers[b].ks || layers[b].y_col < 0) return GPAR_ARG_ERROR(2);
    for (int b = 0; b < batch; ++b) {   // (the fused build below does not pass through gram_launch)
        const gpar_kspec_t* ks = layers[b].ks;
        if (ks->nfactors < 0 || ks->nfactors > GPAR_MAX_FACTORS || !kspec_cos_ok(ks) || !kspec_cos_embed_ok(layers[b].fs, ks)) return GPAR_ARG_ERROR(3);
    }
    // Small evaluations: ONE launch per LS_CHUNK layers builds everything (gram.h: lockstep_build_kernel; same bits as the launches
    // below) - when every feature map fits its compact form and the build is short enough for launch latency to matter.
    bool fused_build = n > 0 && n <= env_int("GPAR_LOCKSTEP_FUSED_BUILD_ROWS", 4096) && w != nullptr;
    for (int b = 0; b < batch && fused_build; ++b) {
        const gpar_fspec_t& fs = *layers[b].fs;
        if (fs.dz < 0 || fs.dz > LS_MAXDZ) fused_build = false;
        for (int q = 0; q < fs.dz && fused_build; ++q)
            if (fs.col[q] < 0 || fs.col[q] > 255) fused_build = false;
    }
    if (fused_build) {
        GPAR_HIP_TRY(gpar_set_max_lds(reinterpret_cast<const void*>(&lockstep_build_kernel), 64 * 1024));
        const int nt = gpar_ceil_div(n, GRAM_T);
        for (int b0 = 0; b0 < batch; b0 += LS_CHUNK) {
            const int cnt = batch - b0 < LS_CHUNK ? batch - b0 : LS_CHUNK;
            LockstepSpecs sp;
            memset(&sp, 0, sizeof(sp));
            int dzmax = 1;
            for (int b = 0; b < cnt; ++b) {
                const gpar_layer_t& L = layers[b0 + b];
                sp.ks[b] = *L.ks;
                sp.fs[b].dz = L.fs->dz;
                for (int q = 0; q < L.fs->dz; ++q) {
                    sp.fs[b].col[q] = (unsigned char)L.fs->col[q];
                    sp.fs[b].embed[q] = (unsigned char)L.fs->embed[q];
                    sp.fs[b].inv_scale[q] = L.fs->inv_scale[q];
                    sp.fs[b].freq[q] = L.fs->freq[q];
                }
                sp.noise[b] = L.noise;
                sp.ycol[b] = L.y_col;
                if (L.fs->dz > dzmax) dzmax = L.fs->dz;
            }
            const size_t lds = ((size_t)2 * dzmax * GRAM_LD + GRAM_TAB_DOUBLES) * sizeof(double);
            hipLaunchKernelGGL(lockstep_build_kernel, dim3((unsigned)((long long)nt * (nt + 1) / 2), 1, cnt), dim3(256), lds, st, sp, x, n, ldx, y, ldy,
                               w, ldw, jitter, A + (size_t)b0 * stride_a, lda, stride_a, logdet + b0, info + b0);
        }
        GPAR_LAUNCH_CHECK();
    } else {
    for (int b0 = 0; b0 < batch; b0 += LOCKSTEP_CHUNK) {
        const int cnt = batch - b0 < LOCKSTEP_CHUNK ? batch - b0 : LOCKSTEP_CHUNK;
        LockstepCols lc;
        for (int b = 0; b < cnt; ++b) { lc.noise[b] = layers[b0 + b].noise; lc.ycol[b] = layers[b0 + b].y_col; }
        hipLaunchKernelGGL(lockstep_prepare_kernel, dim3(gpar_ceil_div(n + 1, 256), cnt), dim3(256), 0, st, lc, y, ldy, w, ldw, n,
                           w ? nd + (size_t)b0 * n : nullptr, A + (size_t)b0 * stride_a, lda, stride_a, logdet + b0, info + b0);
    }
    GPAR_LAUNCH_CHECK();
    for (int b = 0; b < batch && n > 0; ++b) {
        const gpar_layer_t& L = layers[b];
        double* zb = z + (size_t)b * n * ldz;
        int rc = featurize_launch(L.fs, x, n, ldx, zb, ldz, st);
        // unit weights: the diagonal is noise + jitter, added exactly as the kernel adds diag_add[row] + diag_const
        if (!rc) rc = gram_launch(L.ks, zb, n, ldz, zb, n, ldz, L.fs->dz, A + (size_t)b * stride_a, lda, GPAR_GRAM_LOWER, w ? nd + (size_t)b * n : nullptr,
                                  w ? jitter : L.noise + jitter, nullptr, st);
        if (rc) return rc;
    }
    }
    if (n > 0) {
        const int rc = potrf_run_batch(A, batch, stride_a, n + 1, n, lda, logdet, info, st, potrf_flags);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(lockstep_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)A, lda, stride_a, n, (double)n * 1.8378770664093453,
                       (const double*)logdet, value, batch, total);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_gram_diag(const gpar_kspec_t* ks, const double* z, int n, int ldz, int dz, double* out, void* stream) {
    GPAR_API_GUARD;
    (void)dz;
    if (!ks) return GPAR_ARG_ERROR(3);
    if (ks->nfactors < 0 || ks->nfactors > GPAR_MAX_FACTORS || !kspec_cos_ok(ks)) return GPAR_ARG_ERROR(3);
    if (n <= 0) return 0;
    hipLaunchKernelGGL(gram_diag_kernel, dim3(gpar_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, *ks, z, n, ldz, out);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_pivoted_chol(const gpar_kspec_t* ks, const double* z, int n, int ldz, int dz, int max_rank, double tol_trace, double floor, double* Lt,
                      int ldl, int* piv, double* trace, int* rank, int* info, double* ws, void* stream) {
    GPAR_API_GUARD;
    return pivoted_chol_run(ks, z, n, ldz, dz, max_rank, tol_trace, floor, Lt, ldl, piv, trace, rank, info, ws, (hipStream_t)stream);
}

int gpar_featurize_dfreq(const gpar_fspec_t* fs, const double* x, int n, int ldx, double* zd, int ldz, void* stream) {
    GPAR_API_GUARD;
    if (!fs || fs->dz < 0 || fs->dz > GPAR_MAX_DIMS) return GPAR_ARG_ERROR(2);
    if (n <= 0 || fs->dz == 0) return 0;
    const long total = (long)n * fs->dz;
    hipLaunchKernelGGL(featurize_dfreq_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *fs, x,
                       n, ldx, zd, ldz);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_grad_nacc(void) { return GRAD_NACC; }

static int gram_grad_launch(const gpar_kspec_t* ks, const double* z1, const double* zd1, int n1, int ldz1, const double* z2,
                            const double* zd2, int n2, int ldz2, int dz, const double* W, int ldw, int mode, double* workspace,
                            int nblocks, double* out, void* stream, bool reduce = true) {
    if (!ks || ks->nterms < 0 || ks->nterms > GPAR_MAX_TERMS || ks->nfactors < 0 || ks->nfactors > GPAR_MAX_FACTORS)
        return GPAR_ARG_ERROR(3);
    if (!kspec_cos_ok(ks)) return GPAR_ARG_ERROR(3);
    if (dz < 0 || dz > GPAR_MAX_DIMS || nblocks <= 0) return GPAR_ARG_ERROR(4);
    if (mode != GPAR_GRAD_SYM && mode != GPAR_GRAD_RECT && mode != GPAR_GRAD_DIAG) return GPAR_ARG_ERROR(13);
    if (mode != GPAR_GRAD_RECT && (n2 != n1 || z2 != z1)) return GPAR_ARG_ERROR(9);
    if ((zd1 == nullptr) != (zd2 == nullptr)) return GPAR_ARG_ERROR(8);
    {   // the pass handles at most GRAD_MAXF factors per product term
        int cnt[GPAR_MAX_TERMS] = {0};
        for (int f = 0; f < ks->nfactors; ++f) {
            const int t = ks->factor[f].term;
            if (t < 0 || t >= ks->nterms || ++cnt[t] > GRAD_MAXF) return GPAR_ARG_ERROR(6);
        }
    }
    const size_t lds = ((size_t)4 * (dz > 0 ? dz : 1) * GRAM_LD + 4 * GRAD_NACC) * sizeof(double);
    GPAR_HIP_TRY(gpar_set_max_lds(reinterpret_cast<const void*>(&gram_grad_kernel), 160 * 1024));
    if (lds > 160 * 1024) return GPAR_ARG_ERROR(7);
    // per-specification kernel (grad_jit.h) for problems large enough to repay its compilation; the interpreter otherwise
    if (!grad_jit_launch(ks, z1, zd1, n1, ldz1, z2, zd2, n2, ldz2, dz, W, ldw, mode, workspace, nblocks, (hipStream_t)stream))
        hipLaunchKernelGGL(gram_grad_kernel, dim3(nblocks), dim3(256), lds, (hipStream_t)stream, *ks, z1, zd1, n1, ldz1, z2, zd2, n2, ldz2,
                           dz, W, ldw, mode, workspace);
    // (`reduce` false: the caller sums the partials itself - dense_grad_epilogue_kernel, in the same order)
    if (reduce) hipLaunchKernelGGL(gram_grad_reduce_kernel, dim3(GRAD_NACC), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, nblocks, out);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_gram_grad(const gpar_kspec_t* ks, const double* z, const double* zd, int n, int ldz, int dz, const double* W,
                   int ldw, double* workspace, int nblocks, double* out, void* stream) {
    GPAR_API_GUARD;
    return gram_grad_launch(ks, z, zd, n, ldz, z, zd, n, ldz, dz, W, ldw, GPAR_GRAD_SYM, workspace, nblocks, out, stream);
}

int gpar_gram_grad_cross(const gpar_kspec_t* ks, const double* z1, const double* zd1, int n1, int ldz1, const double* z2,
                         const double* zd2, int n2, int ldz2, int dz, const double* W, int ldw, int mode, double* workspace,
                         int nblocks, double* out, void* stream) {
    GPAR_API_GUARD;
    return gram_grad_launch(ks, z1, zd1, n1, ldz1, z2, zd2, n2, ldz2, dz, W, ldw, mode, workspace, nblocks, out, stream);
}

// ---- launches folded together for the one-call training objective (round 6).  Below ~1000 rows an evaluation is a CHAIN of ~23 short
// kernels and every link costs 8-9 us of latency whatever it computes: the element-wise ones are merged - the same expressions per
// element, so the same bits as the separate kernels (featurize_kernel, featurize_dfreq_kernel, logpdf_prepare_kernel; logpdf_value_kernel,
// gram_grad_reduce_kernel, half_diag_kernel).
__global__ __launch_bounds__(256) void dense_grad_prep_kernel(gpar_fspec_t fs, const double* __restrict__ x, int n, int ldx, double* __restrict__ z,
                                                              double* __restrict__ zd, int ldz, const double* __restrict__ y, long incy,
                                                              double* __restrict__ A, int lda, double* __restrict__ logdet, int* __restrict__ info) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int dz = fs.dz;
    if (idx < n * dz) {
        const int r = idx / dz, q = idx - r * dz;
        const double v = x[(size_t)r * ldx + fs.col[q]];
        double e, d = 0.0;
        if (fs.embed[q] == GPAR_EMBED_SIN) { e = sin(v * fs.freq[q]); d = v * cos(v * fs.freq[q]); }
        else if (fs.embed[q] == GPAR_EMBED_COS) { e = cos(v * fs.freq[q]); d = -v * sin(v * fs.freq[q]); }
        else e = v;
        z[(size_t)r * ldz + q] = e * fs.inv_scale[q];
        if (zd) zd[(size_t)r * ldz + q] = d * fs.inv_scale[q];
    }
    if (idx < n) A[(size_t)n * lda + idx] = y[(size_t)idx * incy];
    if (idx == n) {
        A[(size_t)n * lda + n] = 0.0;
        logdet[0] = 0.0;
        info[0] = 0;
    }
}

// What the epilogues of every objective share.  Blocks [0, GRAD_NACC): the gradient pass's partial sums in their fixed order (lanes 0-63,
// as gram_grad_reduce_kernel); blocks [GRAD_NACC, GRAD_NACC + ceil(n / 256)): 1/2 diag W.  False for the one block behind them, which
// forms the objective's value.
__device__ __forceinline__ bool grad_epilogue_sums(const double* __restrict__ partial, int nblocks, double* __restrict__ out,
                                                   const double* __restrict__ W, int ldw, int n, double* __restrict__ half_diag) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b < GRAD_NACC) {
        if (t >= 64) return true;
        double s = 0.0;
        for (int q = t; q < nblocks; q += 64) s += partial[(size_t)q * GRAD_NACC + b];
        s = wave_sum(s);
        if (t == 0) out[2 + b] = s;
        return true;
    }
    const int hb = b - GRAD_NACC, nh = (n + 255) / 256;
    if (hb < nh) {
        const int i = hb * 256 + t;
        if (i < n) half_diag[i] = 0.5 * W[(size_t)i * ldw + i];
        return true;
    }
    return false;
}

// the last block: the value from the corner of the factor and its log-determinant
__global__ __launch_bounds__(256) void dense_grad_epilogue_kernel(const double* __restrict__ partial, int nblocks, double* __restrict__ out,
                                                                  const double* __restrict__ W, int ldw, int n, double* __restrict__ half_diag,
                                                                  const double* __restrict__ A, int lda, double n_log_2pi,
                                                                  const double* __restrict__ logdet) {
    if (grad_epilogue_sums(partial, nblocks, out, W, ldw, n, half_diag)) return;
    if (threadIdx.x == 0) out[0] = -0.5 * ((logdet[0] + n_log_2pi) - A[(size_t)n * lda + n]);
}

// ---- leave-one-out cross-validation of one dense layer (ABI v8; Rasmussen & Williams 5.4.2, Sundararajan & Keerthi 2001) -----------
// With Kinv = (K + D + eps I)^-1, alpha = Kinv y and d = diag Kinv:  mean_-i = y_i - alpha_i / d_i,  var_-i = 1 / d_i,
//     L = sum_i [1/2 log d_i - alpha_i^2 / (2 d_i)] - n/2 log 2 pi,        dL/dtheta = 1/2 sum_ab W_ab dK_ab/dtheta,
//     W = alpha u^T + u alpha^T - 2 S S^T,   b = alpha / d,  c = 1/2 (1 / d + b^2),  S = Kinv diag(sqrt c),  u = Kinv b
// - the shape of weights the weighted-sum pass of the marginal likelihood consumes.  Behind the inverse an evaluation adds three
// launches to that one's chain (rows, {u, S}, the rank-2 term; the product S S^T takes the place of the rank-1 update).
// `vec`: the four n-vectors b, sqrt c, value terms, u (gpar_workspace_doubles(GPAR_WS_LOO, n, 1, 0)).
// Under another scoring rule (ABI v13; score.h) the chain is the same with, for e_i = alpha_i / d_i, v_i = 1 / d_i and the rule's q, s:
//     b_i = q_i v_i,   c_i = q_i e_i v_i + s_i v_i^2      (the log score: b = e, c = 1/2 (v + e^2), written as above - the same bits)
// - c > 0 for the CRPS (sd^3 times a bracket that is 0.117 at z = 0 and grows with |z|), c = 2 e^2 v >= 0 for the squared error - and the
// value is the sum of the rule's terms (the log score keeps its -n/2 log 2 pi in the epilogue: `loo_half_n_log_2pi`).
__device__ __forceinline__ void loo_row_write(int i, double a, double d, double yi, int rule, double* __restrict__ mean, double* __restrict__ var,
                                              double* __restrict__ bvec, double* __restrict__ sc, double* __restrict__ term) {
    const double v = 1.0 / d, b = a / d;   // (b = e, the held-out error, under every rule)
    mean[i] = yi - b;
    var[i] = v;
    if (rule == GPAR_SCORE_LOG) {
        term[i] = 0.5 * log(d) - 0.5 * (a * b);
        if (bvec) bvec[i] = b;
        if (sc) sc[i] = sqrt(0.5 * (v + b * b));
        return;
    }
    double tr, q, s;
    score_row(rule, b, v, tr, q, s);
    term[i] = tr;
    if (bvec) bvec[i] = q * v;
    if (sc) sc[i] = sqrt(q * b * v + s * (v * v));
}
static double loo_half_n_log_2pi(int rule, int n) { return rule == GPAR_SCORE_LOG ? 0.5 * (double)n * 1.8378770664093453 : 0.0; }

// one wave per row: alpha_i as trmv_upper_kernel forms it (same bits), then the row's leave-one-out quantities from Kinv_ii
__global__ __launch_bounds__(256) void loo_rows_kernel(const double* __restrict__ X, int n, int ldx, const double* __restrict__ zrow,
                                                       const double* __restrict__ Kinv, int ldk, const double* __restrict__ y, long incy,
                                                       double* __restrict__ alpha, double* __restrict__ mean, double* __restrict__ var,
                                                       double* __restrict__ vec, int rule) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const double a = trmv_upper_row(X, n, ldx, zrow, 1, row, lane);
    if (lane != 0) return;
    alpha[row] = a;
    loo_row_write(row, a, Kinv[(size_t)row * ldk + row], y[(size_t)row * incy], rule, mean, var, vec, vec + n, vec + 2 * (size_t)n);
}

// the value-only form: alpha_i = sum_j X_ij z_j and d_i = sum_j X_ij^2 over the upper-triangular row i of X = L^-T in one pass
__global__ __launch_bounds__(256) void loo_rows_from_x_kernel(const double* __restrict__ X, int n, int ldx, const double* __restrict__ zrow,
                                                              const double* __restrict__ y, long incy, double* __restrict__ mean,
                                                              double* __restrict__ var, double* __restrict__ term, int rule) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const double* Xr = X + (size_t)row * ldx;
    double a0 = 0.0, a1 = 0.0, d0 = 0.0, d1 = 0.0;
    int j = row + lane;
    for (; j + 64 < n; j += 128) {
        const double x0 = Xr[j], x1 = Xr[j + 64];
        a0 = fma(x0, zrow[j], a0); d0 = fma(x0, x0, d0);
        a1 = fma(x1, zrow[j + 64], a1); d1 = fma(x1, x1, d1);
    }
    if (j < n) { const double x0 = Xr[j]; a0 = fma(x0, zrow[j], a0); d0 = fma(x0, x0, d0); }
    const double a = wave_sum(a0 + a1), d = wave_sum(d0 + d1);
    if (lane == 0) loo_row_write(row, a, d, y[(size_t)row * incy], rule, mean, var, nullptr, nullptr, term);
}

// u = P b for a symmetric P stored in its lower triangle: one wave per row (its row up to the diagonal, its column below it), a fixed
// order.  The tail blocks of loo_weights_kernel and cv_weights_kernel: `blk` counts from the first of them.
__device__ __forceinline__ void sym_lower_matvec_rows(const double* __restrict__ P, int ldp, int n, const double* __restrict__ bvec,
                                                      double* __restrict__ u, int blk, int t) {
    const int lane = t & 63;
    const int row = blk * 4 + (t >> 6);
    if (row >= n) return;
    const double* Pr = P + (size_t)row * ldp;
    double a0 = 0.0, a1 = 0.0;
    for (int j = lane; j <= row; j += 64) a0 = fma(Pr[j], bvec[j], a0);
    for (int j = row + 1 + lane; j < n; j += 64) a1 = fma(P[(size_t)j * ldp + row], bvec[j], a1);
    const double s = wave_sum(a0 + a1);
    if (lane == 0) u[row] = s;
}

// blocks [0, nt^2), nt = ceil(n / 32): tile (bi, bj), bj <= bi, of the LOWER triangle of Kinv through LDS into S = Kinv diag(sqrt c) at
// (bi, bj) and, transposed, at (bj, bi) - a full matrix for the product S S^T, both stores along rows;  the blocks behind them:
// u = Kinv b (sym_lower_matvec_rows).
constexpr int LOO_T = 32;
__global__ __launch_bounds__(256) void loo_weights_kernel(const double* __restrict__ Kinv, int ldk, int n, const double* __restrict__ bvec,
                                                          const double* __restrict__ sc, double* __restrict__ u, double* __restrict__ S, int lds) {
    __shared__ double tile[LOO_T][LOO_T + 1];
    const int nt = (n + LOO_T - 1) / LOO_T;
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= nt * nt) {
        sym_lower_matvec_rows(Kinv, ldk, n, bvec, u, b - nt * nt, t);
        return;
    }
    const int bi = b / nt, bj = b - bi * nt;
    if (bj > bi) return;
    const int tx = t & 31, ty = t >> 5;
    const int r0 = bi * LOO_T, c0 = bj * LOO_T;
    for (int r = ty; r < LOO_T; r += 8) {
        const int gr = r0 + r, gc = c0 + tx;
        tile[r][tx] = (gr < n && gc <= gr) ? Kinv[(size_t)gr * ldk + gc] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < LOO_T; r += 8) {
        const int gr = r0 + r, gc = c0 + tx;
        if (gr < n && gc < n) S[(size_t)gr * lds + gc] = ((bi == bj && tx > r) ? tile[tx][r] : tile[r][tx]) * sc[gc];
        const int mr = c0 + r, mc = r0 + tx;
        if (bi != bj && mr < n && mc < n) S[(size_t)mr * lds + mc] = tile[tx][r] * sc[mc];
    }
}

// W_ij += alpha_i u_j + u_i alpha_j on the lower triangle
__global__ __launch_bounds__(256) void loo_rank2_kernel(double* __restrict__ W, int ldw, int n, const double* __restrict__ alpha,
                                                        const double* __restrict__ u) {
    const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j <= i) W[(size_t)i * ldw + j] += alpha[i] * u[j] + u[i] * alpha[j];
}

// sum of the n value terms in a fixed order (256 strided partial sums, then a tree), by one workgroup
__device__ __forceinline__ double loo_sum_terms(const double* __restrict__ term, int n, double* sm) {
    const int t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < n; i += 256) s += term[i];
    sm[t] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) sm[t] += sm[t + off];
        __syncthreads();
    }
    return sm[0];
}
__global__ __launch_bounds__(256) void loo_value_kernel(const double* __restrict__ term, int n, double half_n_log_2pi, double* __restrict__ out) {
    __shared__ double sm[256];
    const double s = loo_sum_terms(term, n, sm);
    if (threadIdx.x == 0) out[0] = s - half_n_log_2pi;
}

// dense_grad_epilogue_kernel for both cross-validation objectives, leave-one-out (whose name it keeps) and blocked: the last block sums
// the value terms
__global__ __launch_bounds__(256) void loo_grad_epilogue_kernel(const double* __restrict__ partial, int nblocks, double* __restrict__ out,
                                                                const double* __restrict__ W, int ldw, int n, double* __restrict__ half_diag,
                                                                const double* __restrict__ term, double half_n_log_2pi) {
    __shared__ double sm[256];
    if (grad_epilogue_sums(partial, nblocks, out, W, ldw, n, half_diag)) return;
    const double s = loo_sum_terms(term, n, sm);
    if (threadIdx.x == 0) out[0] = s - half_n_log_2pi;
}

// ---- blocked (leave-fold-out) cross-validation of one dense layer (ABI v9) ------------------------------------------------------------
// The folds F partition the rows into contiguous blocks (fold_start: nfolds + 1 ascending offsets, 0 ... n).  With P = (K + D + eps I)^-1
// and alpha = P y, per fold  D_F = P[F, F],  b_F = D_F^-1 alpha_F:  y_F | the other rows ~ N(y_F - b_F, D_F^-1), and
//     L = sum_F [1/2 log|D_F| - 1/2 alpha_F^T b_F] - n/2 log 2 pi,        dL/dtheta = 1/2 sum_ab W_ab dK_ab/dtheta,
//     W = alpha u^T + u alpha^T - 2 S S^T,   C = blockdiag(1/2 (D_F^-1 + b_F b_F^T)) = blockdiag(R_F R_F^T),  S = P blockdiag(R_F),  u = P b
// - leave-one-out's weights with a block-diagonal C in place of the diagonal one, so everything behind S is that chain's.
// `vec`: b, value terms, u (n each), then R_F compactly, row i of its fold in the max_fold doubles at 3 n + i max_fold
// (gpar_workspace_doubles(GPAR_WS_CV, n, 1, max_fold)); the value-only form keeps the n value terms alone.

// T (m x m, lower triangle, leading dimension CV_LD, in LDS) <- its Cholesky factor, in place, by the whole workgroup; 0 or the 1-based
// index of the first non-positive pivot (the same verdict in every thread).  Entered and left behind a barrier.
__device__ __forceinline__ int cv_chol_lower(double* T, int m, int t) {
    for (int k = 0; k < m; ++k) {
        const double d = T[k * CV_LD + k];
        if (!(d > 0.0)) return k + 1;
        const double sd = sqrt(d), rinv = 1.0 / sd;
        __syncthreads();
        if (t == k) T[k * CV_LD + k] = sd;
        else if (t > k && t < m) T[t * CV_LD + k] *= rinv;
        __syncthreads();
        const int w = m - k - 1;
        for (int idx = t; idx < w * w; idx += 256) {
            const int i = k + 1 + idx / w, j = k + 1 + idx % w;
            if (j <= i) T[i * CV_LD + j] = fma(-T[i * CV_LD + k], T[j * CV_LD + k], T[i * CV_LD + j]);
        }
        __syncthreads();
    }
    return 0;
}

// fold f's extent (start, size m) when it is well-formed - inside [0, n), 1 <= m <= max_fold <= GPAR_CV_MAX_FOLD, the first fold starting at
// 0 and the last ending at n - and m = 0 otherwise
__device__ __forceinline__ int cv_fold_extent(const int* __restrict__ fold_start, int nfolds, int max_fold, int n, int f, int& start) {
    start = fold_start[f];
    const int end = fold_start[f + 1], m = end - start;
    const bool ok = start >= 0 && end <= n && m >= 1 && m <= max_fold && max_fold <= GPAR_CV_MAX_FOLD && (f > 0 || start == 0) &&
                    (f < nfolds - 1 || end == n);
    return ok ? m : 0;
}

// One workgroup per fold, everything in LDS (two max_fold x CV_LD tiles and two vectors).  alpha_F as trmv_upper_kernel forms it (one wave per
// row); D_F = G G^T in place; G^-1 column by column into the second tile; D_F^-1 = G^-T G^-1 over the first; b_F, the means, the marginal
// variances, the fold's value term (wave 0, a fixed butterfly) at the fold's first row of `term` and zeros behind it; with Rm, C_F in place
// of D_F^-1, factored in place, its factor stored.  A non-positive pivot of either factorisation: its 1-based row into info (the first
// to report stays, as for the factorisation of K); a malformed fold: n + 1 + fold, with nothing else touched.
__global__ __launch_bounds__(256) void cv_folds_kernel(const double* __restrict__ P, int ldp, int n, const double* __restrict__ X, int ldx,
                                                       const double* __restrict__ zrow, const double* __restrict__ y, long incy,
                                                       const int* __restrict__ fold_start, int nfolds, int max_fold, double* __restrict__ alpha,
                                                       double* __restrict__ mean, double* __restrict__ var, double* __restrict__ bvec,
                                                       double* __restrict__ term, double* __restrict__ Rm, int* __restrict__ info) {
    extern __shared__ double cv_sm[];
    const int f = blockIdx.x, t = threadIdx.x, lane = t & 63;
    int s;
    const int m = cv_fold_extent(fold_start, nfolds, max_fold, n, f, s);
    if (m == 0) {
        if (t == 0) atomicCAS(info, 0, n + 1 + f);
        return;
    }
    double* TA = cv_sm;
    double* TB = TA + max_fold * CV_LD;
    double* al = TB + max_fold * CV_LD;
    double* bv = al + GPAR_CV_MAX_FOLD;
    for (int i = t >> 6; i < m; i += 4) {
        const double a = trmv_upper_row(X, n, ldx, zrow, 1, s + i, lane);
        if (lane == 0) {
            al[i] = a;
            if (alpha) alpha[s + i] = a;
        }
    }
    for (int idx = t; idx < m * m; idx += 256) {
        const int i = idx / m, j = idx - i * m;
        if (j <= i) TA[i * CV_LD + j] = P[(size_t)(s + i) * ldp + s + j];
    }
    if (t < m) term[s + t] = 0.0;
    __syncthreads();
    int bad = cv_chol_lower(TA, m, t);
    if (bad) {
        if (t == 0) atomicCAS(info, 0, s + bad);
        return;
    }
    const double log_g = t < m ? log(TA[t * CV_LD + t]) : 0.0;   // 1/2 log|D_F| = sum_i log G_ii
    if (t < m) {   // column t of G^-1 by forward substitution (below the diagonal; nothing above it is read)
        for (int i = t; i < m; ++i) {
            double acc = i == t ? 1.0 : 0.0;
            for (int k = t; k < i; ++k) acc = fma(-TA[i * CV_LD + k], TB[k * CV_LD + t], acc);
            TB[i * CV_LD + t] = acc / TA[i * CV_LD + i];
        }
    }
    __syncthreads();
    for (int idx = t; idx < m * m; idx += 256) {   // D_F^-1 = G^-T G^-1, lower triangle
        const int i = idx / m, j = idx - i * m;
        if (j > i) continue;
        double acc = 0.0;
        for (int k = i; k < m; ++k) acc = fma(TB[k * CV_LD + i], TB[k * CV_LD + j], acc);
        TA[i * CV_LD + j] = acc;
    }
    __syncthreads();
    double ab = 0.0;
    if (t < m) {
        double acc = 0.0;
        for (int j = 0; j <= t; ++j) acc = fma(TA[t * CV_LD + j], al[j], acc);
        for (int j = t + 1; j < m; ++j) acc = fma(TA[j * CV_LD + t], al[j], acc);
        bv[t] = acc;
        ab = al[t] * acc;
        mean[s + t] = y[(size_t)(s + t) * incy] - acc;
        var[s + t] = TA[t * CV_LD + t];
        if (bvec) bvec[s + t] = acc;
    }
    if (t < 64) {
        const double v = wave_sum(log_g - 0.5 * ab);
        if (t == 0) term[s] = v;
    }
    if (!Rm) return;
    __syncthreads();
    for (int idx = t; idx < m * m; idx += 256) {   // C_F = 1/2 (D_F^-1 + b_F b_F^T)
        const int i = idx / m, j = idx - i * m;
        if (j <= i) TA[i * CV_LD + j] = 0.5 * fma(bv[i], bv[j], TA[i * CV_LD + j]);
    }
    __syncthreads();
    bad = cv_chol_lower(TA, m, t);
    if (bad) {
        if (t == 0) atomicCAS(info, 0, s + bad);
        return;
    }
    for (int idx = t; idx < m * m; idx += 256) {
        const int i = idx / m, j = idx - i * m;
        Rm[(size_t)(s + i) * max_fold + j] = j <= i ? TA[i * CV_LD + j] : 0.0;
    }
}

// blocks [0, nrb * nfolds), nrb = ceil(n / 32): S[rows of block rb, F] = P[rows, F] R_F for fold F = b / nrb, a full matrix for the product
// S S^T.  P is read from its lower triangle alone: element (i, j) with j > i as (j, i), in a second pass whose threads run along row j, so
// both passes read along rows; the tile and R_F meet in LDS.  The blocks behind them: u = P b (sym_lower_matvec_rows).
constexpr int CV_T = 32;
__global__ __launch_bounds__(256) void cv_weights_kernel(const double* __restrict__ P, int ldp, int n, const int* __restrict__ fold_start, int nfolds,
                                                         int max_fold, const double* __restrict__ Rm, const double* __restrict__ bvec,
                                                         double* __restrict__ u, double* __restrict__ S, int lds) {
    __shared__ double Pt[CV_T][CV_LD];
    __shared__ double Rt[GPAR_CV_MAX_FOLD][CV_LD];
    const int nrb = (n + CV_T - 1) / CV_T;
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= nrb * nfolds) {
        sym_lower_matvec_rows(P, ldp, n, bvec, u, b - nrb * nfolds, t);
        return;
    }
    const int f = b / nrb, r0 = (b - f * nrb) * CV_T;
    int s;
    const int m = cv_fold_extent(fold_start, nfolds, max_fold, n, f, s);
    if (m == 0) return;   // (cv_folds_kernel has reported it)
    for (int idx = t; idx < m * m; idx += 256) {
        const int i = idx / m, j = idx - i * m;
        Rt[i][j] = Rm[(size_t)(s + i) * max_fold + j];
    }
    for (int idx = t; idx < CV_T * m; idx += 256) {
        const int r = idx / m, c = idx - r * m;
        const int gr = r0 + r, gc = s + c;
        if (gr < n && gc <= gr) Pt[r][c] = P[(size_t)gr * ldp + gc];
    }
    for (int idx = t; idx < CV_T * m; idx += 256) {
        const int c = idx / CV_T, r = idx - c * CV_T;
        const int gr = r0 + r, gc = s + c;
        if (gr < n && gc > gr) Pt[r][c] = P[(size_t)gc * ldp + gr];
    }
    __syncthreads();
    for (int idx = t; idx < CV_T * m; idx += 256) {
        const int r = idx / m, j = idx - r * m;
        const int gr = r0 + r;
        if (gr >= n) continue;
        double acc = 0.0;
        for (int k = j; k < m; ++k) acc = fma(Pt[r][k], Rt[k][j], acc);
        S[(size_t)gr * lds + s + j] = acc;
    }
}

struct CvFolds {
    const int* start;   // nfolds + 1 ascending row offsets (device)
    int nfolds, max_fold;
};
static int cv_check_folds(const CvFolds& f, int n) {
    if (!f.start) return GPAR_ARG_ERROR(1);
    if (f.max_fold < 1 || f.max_fold > GPAR_CV_MAX_FOLD) return GPAR_ARG_ERROR(3);
    if (f.nfolds < 1 || f.nfolds > n) return GPAR_ARG_ERROR(4);
    return 0;
}

static int cv_folds_launch(const double* P, int ldp, int n, const double* X, int ldx, const double* zrow, const double* y, long incy,
                           const int* fold_start, int nfolds, int max_fold, double* alpha, double* mean, double* var, double* bvec, double* term,
                           double* Rm, int* info, hipStream_t st) {
    GPAR_HIP_TRY(gpar_set_max_lds(reinterpret_cast<const void*>(&cv_folds_kernel), CV_LDS_BYTES));
    hipLaunchKernelGGL(cv_folds_kernel, dim3((unsigned)nfolds), dim3(256), (size_t)cv_lds_bytes(max_fold), st, P, ldp, n, X, ldx, zrow, y, incy,
                       fold_start, nfolds, max_fold, alpha, mean, var, bvec, term, Rm, info);
    return 0;
}

#include "ahead.h"   // rolling-origin forecast scoring: its kernels and weight stage (after loo_sum_terms and grad_epilogue_sums, which it uses)
#include "cv_gap.h"  // purged blocked cross-validation: its kernels and weight stage (after cv_chol_lower and sym_lower_matvec_rows, which it uses)
#include "ahead_window.h"   // sliding-window forecast scoring: its kernels and the head of its chain (after cv_chol_lower, ahead.h and the prep kernel)

// ---- one chain for the dense objectives: marginal likelihood, leave-one-out, blocked cross-validation, rolling-origin forecasts --------
// Every one-call entry is  prologue (features, Gram, factor) -> inverse -> the objective's weights W -> weighted-sum pass -> epilogue;
// the objectives differ in the weight stage and in the last block of the epilogue alone (OBJ_AHEAD also stops the inverse at X = L^-T).
enum DenseObjectiveKind { OBJ_MLL, OBJ_LOO, OBJ_CV, OBJ_AHEAD, OBJ_CV_GAP, OBJ_AHEAD_MULTI };
struct DenseObjective {
    DenseObjectiveKind kind;
    const double* y;            // the observations (the finish form of OBJ_MLL has none: row n of the factor holds all it needs)
    long incy;
    double *vec, *mean, *var;   // OBJ_LOO, OBJ_CV: the vector workspace, held-out means and variances
    CvFolds folds;              // OBJ_CV
    const int* origin;          // OBJ_AHEAD: n origins (device)
    int score;                  // OBJ_LOO, OBJ_AHEAD: the scoring rule (GPAR_SCORE_LOG = 0: what an entry without one scores by)
    CvHold hold;                // OBJ_CV_GAP: the extents of the blocks left out of the conditioning set (`folds`: the scored rows)
    int nh;                     // OBJ_AHEAD_MULTI: the number of horizons (`origin`: nh x n origins; `mean`, `var`: nh x n)
    AheadWeights wt;            // OBJ_AHEAD_MULTI: the horizons' weights
    double* values;             // OBJ_AHEAD_MULTI: the nh unweighted values
};

// What gpar_logpdf_dense does up to the factor: features (+ their frequency derivatives when zd is given; the value-only forms pass null)
// and observations in ONE launch, Gram, the augmented factorisation.  `logdet`: out + 1 of the caller.  `folds`: the blocked entries' folds,
// checked here - between the check of the feature map and the first launch, the order of their error codes -, null for the others.
static int dense_factor_run(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                            const CvFolds* folds, const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda,
                            double* logdet, int* info, int potrf_flags, hipStream_t st) {
    if (fs->dz < 0 || fs->dz > GPAR_MAX_DIMS) return GPAR_ARG_ERROR(2);
    if (ks->nfactors < 0 || ks->nfactors > GPAR_MAX_FACTORS || !kspec_cos_embed_ok(fs, ks)) return GPAR_ARG_ERROR(3);
    int rc = folds ? cv_check_folds(*folds, n) : 0;
    if (rc) return rc;
    const long total = (long)n * fs->dz > (long)n + 1 ? (long)n * fs->dz : (long)n + 1;
    hipLaunchKernelGGL(dense_grad_prep_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, *fs, x, n, ldx, z, zd, ldz, y, incy, A, lda,
                       logdet, info);
    rc = gram_launch(ks, z, n, ldz, z, n, ldz, fs->dz, A, lda, GPAR_GRAM_LOWER, noise_diag, jitter, nullptr, st);
    if (rc) return rc;
    return potrf_run(A, n + 1, n, lda, logdet, info, st, potrf_flags);
}

// Everything of the one-call gradient entries behind the factorisation: K^-1 from L (with X = L^-T), the objective's W on the lower
// triangle, the fused weighted-sum pass, then its partial sums, 1/2 diag W and the value in one epilogue.  `logdet`: the word the
// factorisation left (OBJ_MLL reads it; out[1] holds it in every form).  `info`: where OBJ_CV's fold kernel reports.  `dfreq`: the
// frequency derivatives are still to be formed (the finish forms; the one-call forms' prologue has written them).
static int dense_grad_finish_run(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const DenseObjective& ob, double* z,
                                 double* zd, int ldz, double* A, int lda, const double* logdet, int* info, double* X, int ldxw, double* W, int ldw,
                                 double* alpha, double* workspace, int nblocks, double* out, double* half_diag, void* stream, bool dfreq) {
    hipStream_t st = (hipStream_t)stream;
    if (dfreq && zd && fs->dz > 0) {
        const long total = (long)n * fs->dz;
        hipLaunchKernelGGL(featurize_dfreq_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, *fs, x, n, ldx, zd, ldz);
    }
    const bool ahead = ob.kind == OBJ_AHEAD || ob.kind == OBJ_AHEAD_MULTI;
    int rc = ahead ? trinv_upper_run(A, n, lda, X, ldxw, W, ldw, st) : chol_inverse_run(A, n, lda, X, ldxw, W, ldw, st);
    if (rc) return rc;
    const double* zrow = A + (size_t)n * lda;   // L^-1 y
    double *bvec = ob.vec, *term = nullptr, *u = nullptr;
    switch (ob.kind) {
        case OBJ_MLL:   // alpha = (K + D)^-1 y = X (L^-1 y), then W = alpha alpha^T - K^-1
            hipLaunchKernelGGL(trmv_upper_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, (const double*)X, n, ldxw, zrow, 1, alpha, 1);
            rc = gemm_launch(1, 0, n, n, 1, 1.0, alpha, n, alpha, n, -1.0, W, ldw, GPAR_GEMM_C_LOWER, st);
            break;
        case OBJ_LOO: {   // `vec`: b, sqrt c, value terms, u
            term = ob.vec + 2 * (size_t)n, u = ob.vec + 3 * (size_t)n;
            hipLaunchKernelGGL(loo_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, (const double*)X, n, ldxw, zrow, (const double*)W, ldw,
                               ob.y, ob.incy, alpha, ob.mean, ob.var, ob.vec, ob.score);
            const int nt = gpar_ceil_div(n, LOO_T);
            hipLaunchKernelGGL(loo_weights_kernel, dim3((unsigned)(nt * nt + (n + 3) / 4)), dim3(256), 0, st, (const double*)W, ldw, n,
                               (const double*)bvec, (const double*)(ob.vec + n), u, X, ldxw);
            break;
        }
        case OBJ_CV: {   // `vec`: b, value terms, u, then R_F compactly
            double* Rm = ob.vec + 3 * (size_t)n;
            term = ob.vec + n, u = ob.vec + 2 * (size_t)n;
            rc = cv_folds_launch(W, ldw, n, X, ldxw, zrow, ob.y, ob.incy, ob.folds.start, ob.folds.nfolds, ob.folds.max_fold, alpha, ob.mean, ob.var, bvec, term, Rm,
                                 info, st);
            if (rc) return rc;
            const int nrb = gpar_ceil_div(n, CV_T);
            hipLaunchKernelGGL(cv_weights_kernel, dim3((unsigned)(nrb * ob.folds.nfolds + (n + 3) / 4)), dim3(256), 0, st, (const double*)W, ldw, n,
                               ob.folds.start, ob.folds.nfolds, ob.folds.max_fold, (const double*)Rm, (const double*)bvec, u, X, ldxw);
            break;
        }
        case OBJ_CV_GAP: {   // `vec`: b, value terms, u, the factors of C, its band image, P as a full matrix (cv_gap.h)
            term = ob.vec + n, u = ob.vec + 2 * (size_t)n;
            rc = cvg_weights_run(W, ldw, n, X, ldxw, zrow, ob.y, ob.incy, ob.folds.start, ob.folds.nfolds, ob.hold, alpha, ob.mean, ob.var, ob.vec, info,
                                 st);
            // T = C P (in X) and P whole are formed; C is indefinite, so no S S^T:  W <- -2 P T + alpha u^T + u alpha^T
            if (!rc)
                rc = gemm_launch(0, 0, n, n, n, -2.0, ob.vec + cvg_off_p(n, ob.hold.max_hold), cvg_ldp(n), X, ldxw, 0.0, W, ldw, GPAR_GEMM_C_LOWER, st);
            if (rc) return rc;
            hipLaunchKernelGGL(loo_rank2_kernel, dim3(gpar_ceil_div(n, 256), n), dim3(256), 0, st, W, ldw, n, (const double*)alpha, (const double*)u);
            break;
        }
        case OBJ_AHEAD:   // `vec`: q, s, value terms, abar, chunk origins, the first product;  W = X (P + P^T) X^T whole (no rank-2 tail)
            term = ob.vec + 2 * (size_t)n;
            rc = ahead_weights_run(A, lda, n, ob.y, ob.incy, ob.origin, ob.mean, ob.var, ob.vec, X, ldxw, W, ldw, ob.score, info, st);
            break;
        case OBJ_AHEAD_MULTI:   // `vec`: w q, w s, value terms (nh x n each), abar, chunk origins, the first product
            term = ob.vec + 2 * (size_t)ob.nh * n;
            rc = ahead_multi_weights_run(A, lda, n, ob.y, ob.incy, ob.origin, ob.nh, ob.wt, ob.mean, ob.var, ob.vec, X, ldxw, W, ldw, ob.score, info, st);
            break;
    }
    if (ob.kind == OBJ_LOO || ob.kind == OBJ_CV) {   // u and S (in X: alpha exists, L^-T is no longer needed) are formed: W <- -2 S S^T + alpha u^T + u alpha^T
        rc = gemm_launch(0, 1, n, n, n, -2.0, X, ldxw, X, ldxw, 0.0, W, ldw, GPAR_GEMM_C_LOWER, st);
        if (rc) return rc;
        hipLaunchKernelGGL(loo_rank2_kernel, dim3(gpar_ceil_div(n, 256), n), dim3(256), 0, st, W, ldw, n, (const double*)alpha, (const double*)u);
    }
    if (!rc) rc = gram_grad_launch(ks, z, zd, n, ldz, z, zd, n, ldz, fs->dz, W, ldw, GPAR_GRAD_SYM, workspace, nblocks, out + 2, stream, false);
    if (rc) return rc;
    const dim3 grid((unsigned)(GRAD_NACC + (n + 255) / 256 + 1));
    const double n_log_2pi = (double)n * 1.8378770664093453;
    if (ob.kind == OBJ_MLL)   // (the corner of the factor is untouched since the factorisation)
        hipLaunchKernelGGL(dense_grad_epilogue_kernel, grid, dim3(256), 0, st, (const double*)workspace, nblocks, out, (const double*)W, ldw, n,
                           half_diag, (const double*)A, lda, n_log_2pi, logdet);
    else if (ob.kind == OBJ_AHEAD)
        hipLaunchKernelGGL(ahead_grad_epilogue_kernel, grid, dim3(256), 0, st, (const double*)workspace, nblocks, out, (const double*)W, ldw, n,
                           half_diag, (const double*)term, (const int*)info);
    else if (ob.kind == OBJ_AHEAD_MULTI)
        hipLaunchKernelGGL(ahead_multi_grad_epilogue_kernel, grid, dim3(256), 0, st, (const double*)workspace, nblocks, out, (const double*)W, ldw, n,
                           half_diag, (const double*)term, ob.nh, ob.wt, ob.values, (const int*)info);
    else
        hipLaunchKernelGGL(loo_grad_epilogue_kernel, grid, dim3(256), 0, st, (const double*)workspace, nblocks, out, (const double*)W, ldw, n,
                           half_diag, (const double*)term, ob.kind == OBJ_LOO ? loo_half_n_log_2pi(ob.score, n) : 0.5 * n_log_2pi);
    GPAR_LAUNCH_CHECK();
    return 0;
}

// The finish forms take the words an earlier (batched) factorisation left: the log-determinant into out[1], the info word into info_out.
// The three entries differ in which of `info` / `info_out` may be null, and are kept so (ABI 9): the marginal-likelihood and leave-one-out
// forms accept either as null and then skip the copy; the blocked form requires both, because its fold kernel reports into info_out.
static int finish_carry_words(const double* logdet, const int* info, double* out, int* info_out, hipStream_t st) {
    GPAR_HIP_TRY(hipMemcpyAsync(out + 1, logdet, sizeof(double), hipMemcpyDeviceToDevice, st));
    if (info && info_out) GPAR_HIP_TRY(hipMemcpyAsync(info_out, info, sizeof(int), hipMemcpyDeviceToDevice, st));
    return 0;
}

int gpar_logpdf_dense_grad(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                           const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* X, int ldxw,
                           double* W, int ldw, double* alpha, double* workspace, int nblocks, double* out, double* half_diag, int* info,
                           int potrf_flags, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !X || !W || !alpha || !workspace || !out || !half_diag || !info || n <= 0 || nblocks <= 0)
        return GPAR_ARG_ERROR(1);
    const DenseObjective ob{OBJ_MLL, y, incy};
    const int rc = dense_factor_run(fs, ks, x, n, ldx, y, incy, nullptr, noise_diag, jitter, z, zd, ldz, A, lda, out + 1, info, potrf_flags,
                                    (hipStream_t)stream);
    if (rc) return rc;
    return dense_grad_finish_run(fs, ks, x, n, ldx, ob, z, zd, ldz, A, lda, out + 1, info, X, ldxw, W, ldw, alpha, workspace, nblocks, out, half_diag,
                                 stream, false);
}

int gpar_logpdf_dense_grad_finish(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, double* z, double* zd,
                                  int ldz, double* A, int lda, const double* logdet, const int* info, double* X, int ldxw, double* W, int ldw,
                                  double* alpha, double* workspace, int nblocks, double* out, double* half_diag, int* info_out, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !z || !A || !logdet || !X || !W || !alpha || !workspace || !out || !half_diag || n <= 0 || nblocks <= 0)
        return GPAR_ARG_ERROR(1);
    const int rc = finish_carry_words(logdet, info, out, info_out, (hipStream_t)stream);
    if (rc) return rc;
    return dense_grad_finish_run(fs, ks, x, n, ldx, DenseObjective{OBJ_MLL}, z, zd, ldz, A, lda, logdet, info_out, X, ldxw, W, ldw, alpha, workspace,
                                 nblocks, out, half_diag, stream, true);
}

// (ABI v13: the entries that take a scoring rule do the work; the entries without one forward with GPAR_SCORE_LOG.  An unknown rule is an
// argument error before anything is launched.)
int gpar_loo_dense_grad_score(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                              const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* X, int ldxw,
                              double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                              double* loo_mean, double* loo_var, int score, int* info, int potrf_flags, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !X || !W || !alpha || !vec || !workspace || !out || !half_diag || !loo_mean || !loo_var || !info ||
        n <= 0 || nblocks <= 0)
        return GPAR_ARG_ERROR(1);
    if (!score_known(score)) return GPAR_ARG_ERROR(14);
    const DenseObjective ob{OBJ_LOO, y, incy, vec, loo_mean, loo_var, {}, nullptr, score};
    const int rc = dense_factor_run(fs, ks, x, n, ldx, y, incy, nullptr, noise_diag, jitter, z, zd, ldz, A, lda, out + 1, info, potrf_flags,
                                    (hipStream_t)stream);
    if (rc) return rc;
    return dense_grad_finish_run(fs, ks, x, n, ldx, ob, z, zd, ldz, A, lda, out + 1, info, X, ldxw, W, ldw, alpha, workspace, nblocks, out, half_diag,
                                 stream, false);
}

int gpar_loo_dense_grad(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                        const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* X, int ldxw,
                        double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                        double* loo_mean, double* loo_var, int* info, int potrf_flags, void* stream) {
    return gpar_loo_dense_grad_score(fs, ks, x, n, ldx, y, incy, noise_diag, jitter, z, zd, ldz, A, lda, X, ldxw, W, ldw, alpha, vec, workspace, nblocks,
                                     out, half_diag, loo_mean, loo_var, GPAR_SCORE_LOG, info, potrf_flags, stream);
}

int gpar_loo_dense_grad_finish_score(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                                     double* z, double* zd, int ldz, double* A, int lda, const double* logdet, const int* info, double* X,
                                     int ldxw, double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out,
                                     double* half_diag, double* loo_mean, double* loo_var, int score, int* info_out, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !logdet || !X || !W || !alpha || !vec || !workspace || !out || !half_diag || !loo_mean || !loo_var ||
        n <= 0 || nblocks <= 0)
        return GPAR_ARG_ERROR(1);
    if (!score_known(score)) return GPAR_ARG_ERROR(14);
    const int rc = finish_carry_words(logdet, info, out, info_out, (hipStream_t)stream);
    if (rc) return rc;
    return dense_grad_finish_run(fs, ks, x, n, ldx, DenseObjective{OBJ_LOO, y, incy, vec, loo_mean, loo_var, {}, nullptr, score}, z, zd, ldz, A, lda,
                                 logdet, info_out, X, ldxw, W, ldw, alpha, workspace, nblocks, out, half_diag, stream, true);
}

int gpar_loo_dense_grad_finish(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                               double* z, double* zd, int ldz, double* A, int lda, const double* logdet, const int* info, double* X, int ldxw,
                               double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                               double* loo_mean, double* loo_var, int* info_out, void* stream) {
    return gpar_loo_dense_grad_finish_score(fs, ks, x, n, ldx, y, incy, z, zd, ldz, A, lda, logdet, info, X, ldxw, W, ldw, alpha, vec, workspace,
                                            nblocks, out, half_diag, loo_mean, loo_var, GPAR_SCORE_LOG, info_out, stream);
}

// Value, means and variances alone: no K^-1 is formed - alpha = X (L^-1 y) and d = the squared row norms of X = L^-T come out of one pass
// over X (n^3 / 3 flops for X instead of the inverse's 2 n^3 / 3)
int gpar_loo_dense_score(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                         const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* X, int ldxw, double* T, int ldt,
                         double* vec, double* out, double* loo_mean, double* loo_var, int score, int* info, int potrf_flags, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !X || !T || !vec || !out || !loo_mean || !loo_var || !info || n <= 0) return GPAR_ARG_ERROR(1);
    if (!score_known(score)) return GPAR_ARG_ERROR(14);
    hipStream_t st = (hipStream_t)stream;
    int rc = dense_factor_run(fs, ks, x, n, ldx, y, incy, nullptr, noise_diag, jitter, z, nullptr, ldz, A, lda, out + 1, info, potrf_flags, st);
    if (!rc) rc = trinv_upper_run(A, n, lda, X, ldxw, T, ldt, st);
    if (rc) return rc;
    hipLaunchKernelGGL(loo_rows_from_x_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, (const double*)X, n, ldxw,
                       (const double*)(A + (size_t)n * lda), y, incy, loo_mean, loo_var, vec, score);
    hipLaunchKernelGGL(loo_value_kernel, dim3(1), dim3(256), 0, st, (const double*)vec, n, loo_half_n_log_2pi(score, n), out);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_loo_dense(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                   const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* X, int ldxw, double* T, int ldt,
                   double* vec, double* out, double* loo_mean, double* loo_var, int* info, int potrf_flags, void* stream) {
    return gpar_loo_dense_score(fs, ks, x, n, ldx, y, incy, noise_diag, jitter, z, ldz, A, lda, X, ldxw, T, ldt, vec, out, loo_mean, loo_var,
                                GPAR_SCORE_LOG, info, potrf_flags, stream);
}

int gpar_cv_dense_grad(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                       const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* X, int ldxw,
                       double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                       double* cv_mean, double* cv_var, const int* fold_start, int nfolds, int max_fold, int* info, int potrf_flags,
                       void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !X || !W || !alpha || !vec || !workspace || !out || !half_diag || !cv_mean || !cv_var || !info ||
        n <= 0 || nblocks <= 0)
        return GPAR_ARG_ERROR(1);
    const DenseObjective ob{OBJ_CV, y, incy, vec, cv_mean, cv_var, {fold_start, nfolds, max_fold}};
    const int rc = dense_factor_run(fs, ks, x, n, ldx, y, incy, &ob.folds, noise_diag, jitter, z, zd, ldz, A, lda, out + 1, info, potrf_flags,
                                    (hipStream_t)stream);
    if (rc) return rc;
    return dense_grad_finish_run(fs, ks, x, n, ldx, ob, z, zd, ldz, A, lda, out + 1, info, X, ldxw, W, ldw, alpha, workspace, nblocks, out, half_diag,
                                 stream, false);
}

int gpar_cv_dense_grad_finish(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                              double* z, double* zd, int ldz, double* A, int lda, const double* logdet, const int* info, double* X, int ldxw,
                              double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                              double* cv_mean, double* cv_var, const int* fold_start, int nfolds, int max_fold, int* info_out, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !logdet || !info || !X || !W || !alpha || !vec || !workspace || !out || !half_diag || !cv_mean ||
        !cv_var || !info_out || n <= 0 || nblocks <= 0)
        return GPAR_ARG_ERROR(1);
    const DenseObjective ob{OBJ_CV, y, incy, vec, cv_mean, cv_var, {fold_start, nfolds, max_fold}};
    int rc = cv_check_folds(ob.folds, n);
    if (!rc) rc = finish_carry_words(logdet, info, out, info_out, (hipStream_t)stream);
    if (rc) return rc;
    return dense_grad_finish_run(fs, ks, x, n, ldx, ob, z, zd, ldz, A, lda, logdet, info_out, X, ldxw, W, ldw, alpha, workspace, nblocks, out,
                                 half_diag, stream, true);
}

// Value, means and variances alone.  K^-1 is formed whole (gpar_chol_inverse) and the fold kernel shared; D_F = X_F X_F^T from the row
// slabs of X = L^-T would halve the flops, as gpar_loo_dense does for single rows - a later optimisation.
int gpar_cv_dense(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                  const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* X, int ldxw, double* T, int ldt,
                  double* vec, double* out, double* cv_mean, double* cv_var, const int* fold_start, int nfolds, int max_fold, int* info,
                  int potrf_flags, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !X || !T || !vec || !out || !cv_mean || !cv_var || !info || n <= 0) return GPAR_ARG_ERROR(1);
    hipStream_t st = (hipStream_t)stream;
    const CvFolds folds{fold_start, nfolds, max_fold};
    int rc = dense_factor_run(fs, ks, x, n, ldx, y, incy, &folds, noise_diag, jitter, z, nullptr, ldz, A, lda, out + 1, info, potrf_flags, st);
    if (!rc) rc = chol_inverse_run(A, n, lda, X, ldxw, T, ldt, st);
    if (!rc) rc = cv_folds_launch(T, ldt, n, X, ldxw, A + (size_t)n * lda, y, incy, fold_start, nfolds, max_fold, nullptr, cv_mean, cv_var, nullptr,
                                  vec, nullptr, info, st);
    if (rc) return rc;
    hipLaunchKernelGGL(loo_value_kernel, dim3(1), dim3(256), 0, st, (const double*)vec, n, 0.5 * (double)n * 1.8378770664093453, out);
    GPAR_LAUNCH_CHECK();
    return 0;
}

// ---- purged blocked cross-validation (ABI v14; cv_gap.h) ----------------------------------------------------------------------------------
static int cvg_check(const int* fold_start, const int* hold_lo, const int* hold_hi, int nfolds, int max_hold, int n) {
    if (!hold_lo || !hold_hi) return GPAR_ARG_ERROR(1);
    return cv_check_folds(CvFolds{fold_start, nfolds, max_hold}, n);
}

int gpar_cv_gap_dense_grad(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                           const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* X, int ldxw,
                           double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                           double* cv_mean, double* cv_var, const int* fold_start, const int* hold_lo, const int* hold_hi, int nfolds,
                           int max_hold, int* info, int potrf_flags, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !X || !W || !alpha || !vec || !workspace || !out || !half_diag || !cv_mean || !cv_var || !info ||
        n <= 0 || nblocks <= 0)
        return GPAR_ARG_ERROR(1);
    if (fs->dz < 0 || fs->dz > GPAR_MAX_DIMS) return GPAR_ARG_ERROR(2);
    int rc = cvg_check(fold_start, hold_lo, hold_hi, nfolds, max_hold, n);
    if (rc) return rc;
    const DenseObjective ob{OBJ_CV_GAP, y, incy, vec, cv_mean, cv_var, {fold_start, nfolds, max_hold}, nullptr, GPAR_SCORE_LOG,
                            {hold_lo, hold_hi, max_hold}};
    rc = dense_factor_run(fs, ks, x, n, ldx, y, incy, nullptr, noise_diag, jitter, z, zd, ldz, A, lda, out + 1, info, potrf_flags, (hipStream_t)stream);
    if (rc) return rc;
    return dense_grad_finish_run(fs, ks, x, n, ldx, ob, z, zd, ldz, A, lda, out + 1, info, X, ldxw, W, ldw, alpha, workspace, nblocks, out, half_diag,
                                 stream, false);
}

int gpar_cv_gap_dense_grad_finish(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                                  double* z, double* zd, int ldz, double* A, int lda, const double* logdet, const int* info, double* X, int ldxw,
                                  double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                                  double* cv_mean, double* cv_var, const int* fold_start, const int* hold_lo, const int* hold_hi, int nfolds,
                                  int max_hold, int* info_out, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !logdet || !info || !X || !W || !alpha || !vec || !workspace || !out || !half_diag || !cv_mean ||
        !cv_var || !info_out || n <= 0 || nblocks <= 0)
        return GPAR_ARG_ERROR(1);
    const DenseObjective ob{OBJ_CV_GAP, y, incy, vec, cv_mean, cv_var, {fold_start, nfolds, max_hold}, nullptr, GPAR_SCORE_LOG,
                            {hold_lo, hold_hi, max_hold}};
    int rc = cvg_check(fold_start, hold_lo, hold_hi, nfolds, max_hold, n);
    if (!rc) rc = finish_carry_words(logdet, info, out, info_out, (hipStream_t)stream);
    if (rc) return rc;
    return dense_grad_finish_run(fs, ks, x, n, ldx, ob, z, zd, ldz, A, lda, logdet, info_out, X, ldxw, W, ldw, alpha, workspace, nblocks, out,
                                 half_diag, stream, true);
}

// Value, means and variances alone: K^-1 whole (as gpar_cv_dense forms it), then the purged fold kernel without its gradient outputs.
int gpar_cv_gap_dense(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                      const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* X, int ldxw, double* T, int ldt,
                      double* vec, double* out, double* cv_mean, double* cv_var, const int* fold_start, const int* hold_lo, const int* hold_hi,
                      int nfolds, int max_hold, int* info, int potrf_flags, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !X || !T || !vec || !out || !cv_mean || !cv_var || !info || n <= 0) return GPAR_ARG_ERROR(1);
    if (fs->dz < 0 || fs->dz > GPAR_MAX_DIMS) return GPAR_ARG_ERROR(2);
    hipStream_t st = (hipStream_t)stream;
    int rc = cvg_check(fold_start, hold_lo, hold_hi, nfolds, max_hold, n);
    if (!rc) rc = dense_factor_run(fs, ks, x, n, ldx, y, incy, nullptr, noise_diag, jitter, z, nullptr, ldz, A, lda, out + 1, info, potrf_flags, st);
    if (!rc) rc = chol_inverse_run(A, n, lda, X, ldxw, T, ldt, st);
    if (!rc) rc = cvg_folds_launch(T, ldt, n, X, ldxw, A + (size_t)n * lda, y, incy, fold_start, nfolds, CvHold{hold_lo, hold_hi, max_hold}, nullptr,
                                   cv_mean, cv_var, vec, nullptr, nullptr, nullptr, nullptr, info, st);
    if (rc) return rc;
    hipLaunchKernelGGL(loo_value_kernel, dim3(1), dim3(256), 0, st, (const double*)vec, n, 0.5 * (double)n * 1.8378770664093453, out);
    GPAR_LAUNCH_CHECK();
    return 0;
}

// ---- rolling-origin forecast scoring (ABI v12; ahead.h) ----------------------------------------------------------------------------------
int gpar_ahead_dense_grad_score(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                                const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* X, int ldxw,
                                double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                                double* ahead_mean, double* ahead_var, const int* origin, int score, int* info, int potrf_flags, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !X || !W || !alpha || !vec || !workspace || !out || !half_diag || !ahead_mean || !ahead_var ||
        !origin || !info || n <= 0 || nblocks <= 0)
        return GPAR_ARG_ERROR(1);
    if (!score_known(score)) return GPAR_ARG_ERROR(14);
    const DenseObjective ob{OBJ_AHEAD, y, incy, vec, ahead_mean, ahead_var, {}, origin, score};
    const int rc = dense_factor_run(fs, ks, x, n, ldx, y, incy, nullptr, noise_diag, jitter, z, zd, ldz, A, lda, out + 1, info, potrf_flags,
                                    (hipStream_t)stream);
    if (rc) return rc;
    return dense_grad_finish_run(fs, ks, x, n, ldx, ob, z, zd, ldz, A, lda, out + 1, info, X, ldxw, W, ldw, alpha, workspace, nblocks, out, half_diag,
                                 stream, false);
}

int gpar_ahead_dense_grad(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                          const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* X, int ldxw,
                          double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                          double* ahead_mean, double* ahead_var, const int* origin, int* info, int potrf_flags, void* stream) {
    return gpar_ahead_dense_grad_score(fs, ks, x, n, ldx, y, incy, noise_diag, jitter, z, zd, ldz, A, lda, X, ldxw, W, ldw, alpha, vec, workspace,
                                       nblocks, out, half_diag, ahead_mean, ahead_var, origin, GPAR_SCORE_LOG, info, potrf_flags, stream);
}

// (both info words are required, as for the blocked form: the kernels of the weight stage read and report into info_out)
int gpar_ahead_dense_grad_finish_score(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                                       double* z, double* zd, int ldz, double* A, int lda, const double* logdet, const int* info, double* X,
                                       int ldxw, double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out,
                                       double* half_diag, double* ahead_mean, double* ahead_var, const int* origin, int score, int* info_out,
                                       void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !logdet || !info || !X || !W || !alpha || !vec || !workspace || !out || !half_diag || !ahead_mean ||
        !ahead_var || !origin || !info_out || n <= 0 || nblocks <= 0)
        return GPAR_ARG_ERROR(1);
    if (!score_known(score)) return GPAR_ARG_ERROR(14);
    const int rc = finish_carry_words(logdet, info, out, info_out, (hipStream_t)stream);
    if (rc) return rc;
    return dense_grad_finish_run(fs, ks, x, n, ldx, DenseObjective{OBJ_AHEAD, y, incy, vec, ahead_mean, ahead_var, {}, origin, score}, z, zd, ldz, A, lda,
                                 logdet, info_out, X, ldxw, W, ldw, alpha, workspace, nblocks, out, half_diag, stream, true);
}

int gpar_ahead_dense_grad_finish(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                                 double* z, double* zd, int ldz, double* A, int lda, const double* logdet, const int* info, double* X, int ldxw,
                                 double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                                 double* ahead_mean, double* ahead_var, const int* origin, int* info_out, void* stream) {
    return gpar_ahead_dense_grad_finish_score(fs, ks, x, n, ldx, y, incy, z, zd, ldz, A, lda, logdet, info, X, ldxw, W, ldw, alpha, vec, workspace,
                                              nblocks, out, half_diag, ahead_mean, ahead_var, origin, GPAR_SCORE_LOG, info_out, stream);
}

// Value, means and variances alone: the factor and its augmented row are all it reads - no X, no K^-1
int gpar_ahead_dense_score(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                           const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* vec, double* out,
                           double* ahead_mean, double* ahead_var, const int* origin, int score, int* info, int potrf_flags, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !vec || !out || !ahead_mean || !ahead_var || !origin || !info || n <= 0) return GPAR_ARG_ERROR(1);
    if (!score_known(score)) return GPAR_ARG_ERROR(14);
    hipStream_t st = (hipStream_t)stream;
    const int rc = dense_factor_run(fs, ks, x, n, ldx, y, incy, nullptr, noise_diag, jitter, z, nullptr, ldz, A, lda, out + 1, info, potrf_flags, st);
    if (rc) return rc;
    ahead_rows_run(A, lda, n, y, incy, origin, ahead_mean, ahead_var, nullptr, nullptr, vec, nullptr, score, info, st);
    hipLaunchKernelGGL(ahead_value_kernel, dim3(1), dim3(256), 0, st, (const double*)vec, n, out, (const int*)info);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_ahead_dense(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                     const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* vec, double* out,
                     double* ahead_mean, double* ahead_var, const int* origin, int* info, int potrf_flags, void* stream) {
    return gpar_ahead_dense_score(fs, ks, x, n, ldx, y, incy, noise_diag, jitter, z, ldz, A, lda, vec, out, ahead_mean, ahead_var, origin,
                                  GPAR_SCORE_LOG, info, potrf_flags, stream);
}

// ---- several horizons in one pass (ABI v15; ahead.h) ---------------------------------------------------------------------------------------
// nh outside 1 ... GPAR_AHEAD_MAX_HORIZONS, a weight that is not positive and finite: argument errors before anything is launched
static int ahead_multi_check_args(int nh, const double* weights, AheadWeights& wt) {
    if (nh < 1 || nh > GPAR_AHEAD_MAX_HORIZONS) return GPAR_ARG_ERROR(15);
    for (int k = 0; k < GPAR_AHEAD_MAX_HORIZONS; ++k) {
        if (k < nh && (!(weights[k] > 0.0) || !__builtin_isfinite(weights[k]))) return GPAR_ARG_ERROR(16);
        wt.w[k] = k < nh ? weights[k] : 0.0;
    }
    return 0;
}

int gpar_ahead_multi_dense_grad(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                                const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* X, int ldxw,
                                double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                                double* ahead_mean, double* ahead_var, const int* origins, int nh, const double* weights, double* values, int score,
                                int* info, int potrf_flags, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !X || !W || !alpha || !vec || !workspace || !out || !half_diag || !ahead_mean || !ahead_var ||
        !origins || !weights || !values || !info || n <= 0 || nblocks <= 0)
        return GPAR_ARG_ERROR(1);
    if (!score_known(score)) return GPAR_ARG_ERROR(14);
    DenseObjective ob{OBJ_AHEAD_MULTI, y, incy, vec, ahead_mean, ahead_var, {}, origins, score, {}, nh, {}, values};
    int rc = ahead_multi_check_args(nh, weights, ob.wt);
    if (!rc) rc = dense_factor_run(fs, ks, x, n, ldx, y, incy, nullptr, noise_diag, jitter, z, zd, ldz, A, lda, out + 1, info, potrf_flags,
                                   (hipStream_t)stream);
    if (rc) return rc;
    return dense_grad_finish_run(fs, ks, x, n, ldx, ob, z, zd, ldz, A, lda, out + 1, info, X, ldxw, W, ldw, alpha, workspace, nblocks, out, half_diag,
                                 stream, false);
}

// (both info words are required, as for gpar_ahead_dense_grad_finish)
int gpar_ahead_multi_dense_grad_finish(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                                       double* z, double* zd, int ldz, double* A, int lda, const double* logdet, const int* info, double* X,
                                       int ldxw, double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out,
                                       double* half_diag, double* ahead_mean, double* ahead_var, const int* origins, int nh, const double* weights,
                                       double* values, int score, int* info_out, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !logdet || !info || !X || !W || !alpha || !vec || !workspace || !out || !half_diag || !ahead_mean ||
        !ahead_var || !origins || !weights || !values || !info_out || n <= 0 || nblocks <= 0)
        return GPAR_ARG_ERROR(1);
    if (!score_known(score)) return GPAR_ARG_ERROR(14);
    DenseObjective ob{OBJ_AHEAD_MULTI, y, incy, vec, ahead_mean, ahead_var, {}, origins, score, {}, nh, {}, values};
    int rc = ahead_multi_check_args(nh, weights, ob.wt);
    if (!rc) rc = finish_carry_words(logdet, info, out, info_out, (hipStream_t)stream);
    if (rc) return rc;
    return dense_grad_finish_run(fs, ks, x, n, ldx, ob, z, zd, ldz, A, lda, logdet, info_out, X, ldxw, W, ldw, alpha, workspace, nblocks, out,
                                 half_diag, stream, true);
}

// Values, means and variances alone: the factor and its augmented row are all it reads
int gpar_ahead_multi_dense(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                           const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* vec, double* out,
                           double* ahead_mean, double* ahead_var, const int* origins, int nh, const double* weights, double* values, int score,
                           int* info, int potrf_flags, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !vec || !out || !ahead_mean || !ahead_var || !origins || !weights || !values || !info || n <= 0)
        return GPAR_ARG_ERROR(1);
    if (!score_known(score)) return GPAR_ARG_ERROR(14);
    AheadWeights wt;
    int rc = ahead_multi_check_args(nh, weights, wt);
    hipStream_t st = (hipStream_t)stream;
    if (!rc) rc = dense_factor_run(fs, ks, x, n, ldx, y, incy, nullptr, noise_diag, jitter, z, nullptr, ldz, A, lda, out + 1, info, potrf_flags, st);
    if (rc) return rc;
    ahead_multi_rows_run(A, lda, n, y, incy, origins, nh, wt, ahead_mean, ahead_var, nullptr, nullptr, vec, nullptr, score, info, st);
    hipLaunchKernelGGL(ahead_multi_value_kernel, dim3(1), dim3(256), 0, st, (const double*)vec, n, nh, wt, values, out, (const int*)info);
    GPAR_LAUNCH_CHECK();
    return 0;
}

// ---- sliding-window forecast scoring (ABI v16; ahead_window.h) ------------------------------------------------------------------------------
// No factor of K is formed: out[1], the log-determinant word of the other entries, is 0, and there is no finish form.
int gpar_ahead_window_dense_grad(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                                 const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* W, int ldw,
                                 double* vec, double* workspace, int nblocks, double* out, double* half_diag, double* ahead_mean, double* ahead_var,
                                 const int* lo, const int* origin, int score, int* info, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !W || !vec || !workspace || !out || !half_diag || !ahead_mean || !ahead_var || !info || n <= 0 ||
        nblocks <= 0)
        return GPAR_ARG_ERROR(1);
    int rc = aw_check_args(lo, origin, score);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    double *term = vec, *q = vec + n, *s = vec + 2 * (size_t)n, *cp = vec + 3 * (size_t)n;
    rc = ahead_window_rows_run(fs, ks, x, n, ldx, y, incy, noise_diag, jitter, z, zd, ldz, A, lda, out + 1, lo, origin, ahead_mean, ahead_var, q, s,
                               term, cp, score, info, st);
    if (rc) return rc;
    const int nt = gpar_ceil_div(n, AW_T);
    hipLaunchKernelGGL(ahead_window_gather_kernel, dim3((unsigned)nt, (unsigned)nt), dim3(256), 0, st, (const double*)cp, (const double*)q,
                       (const double*)s, lo, origin, n, W, ldw, (const int*)info);
    rc = gram_grad_launch(ks, z, zd, n, ldz, z, zd, n, ldz, fs->dz, W, ldw, GPAR_GRAD_SYM, workspace, nblocks, out + 2, stream, false);
    if (rc) return rc;
    hipLaunchKernelGGL(ahead_grad_epilogue_kernel, dim3((unsigned)(GRAD_NACC + (n + 255) / 256 + 1)), dim3(256), 0, st, (const double*)workspace,
                       nblocks, out, (const double*)W, ldw, n, half_diag, (const double*)term, (const int*)info);
    GPAR_LAUNCH_CHECK();
    return 0;
}

// Value, means and variances alone: the Gram matrix, the check, the rows, the sum of their terms
int gpar_ahead_window_dense(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                            const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* vec, double* out,
                            double* ahead_mean, double* ahead_var, const int* lo, const int* origin, int score, int* info, void* stream) {
    GPAR_API_GUARD;
    if (!fs || !ks || !x || !y || !z || !A || !vec || !out || !ahead_mean || !ahead_var || !info || n <= 0) return GPAR_ARG_ERROR(1);
    int rc = aw_check_args(lo, origin, score);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = ahead_window_rows_run(fs, ks, x, n, ldx, y, incy, noise_diag, jitter, z, nullptr, ldz, A, lda, out + 1, lo, origin, ahead_mean, ahead_var,
                               nullptr, nullptr, vec, nullptr, score, info, st);
    if (rc) return rc;
    hipLaunchKernelGGL(ahead_value_kernel, dim3(1), dim3(256), 0, st, (const double*)vec, n, out, (const int*)info);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_gram_input_grad(const gpar_kspec_t* ks, const double* z1, int n1, int ldz1, const double* z2, int n2, int ldz2, int dz,
                         const double* W, int ldw, int mode, int nsplit, double* workspace, double* out, int ldo, void* stream) {
    GPAR_API_GUARD;
    if (!ks || ks->nterms < 0 || ks->nterms > GPAR_MAX_TERMS || ks->nfactors < 0 || ks->nfactors > GPAR_MAX_FACTORS)
        return GPAR_ARG_ERROR(3);
    if (!kspec_cos_ok(ks)) return GPAR_ARG_ERROR(3);
    if (dz < 0 || dz > GPAR_MAX_DIMS || nsplit <= 0) return GPAR_ARG_ERROR(4);
    if (mode != GPAR_GRAD_SYM && mode != GPAR_GRAD_RECT) return GPAR_ARG_ERROR(13);
    if (mode == GPAR_GRAD_SYM && (n2 != n1 || z2 != z1)) return GPAR_ARG_ERROR(9);
    {
        int cnt[GPAR_MAX_TERMS] = {0};
        for (int f = 0; f < ks->nfactors; ++f) {
            const int t = ks->factor[f].term;
            if (t < 0 || t >= ks->nterms || ++cnt[t] > GRAD_MAXF) return GPAR_ARG_ERROR(6);
        }
    }
    if (n1 <= 0 || dz == 0) return 0;
    if (n2 <= 0) {
        for (int r = 0; r < n1; ++r) GPAR_HIP_TRY(hipMemsetAsync(out + (size_t)r * ldo, 0, sizeof(double) * dz, (hipStream_t)stream));
        return 0;
    }
    const size_t lds = ((size_t)2 * dz * GRAM_LD + (size_t)GRAM_T * dz) * sizeof(double);
    GPAR_HIP_TRY(gpar_set_max_lds(reinterpret_cast<const void*>(&gram_input_grad_kernel), 160 * 1024));
    if (lds > 160 * 1024) return GPAR_ARG_ERROR(7);
    if (!input_grad_jit_launch(ks, z1, n1, ldz1, z2, n2, ldz2, dz, W, ldw, mode, nsplit, workspace, (hipStream_t)stream))
        hipLaunchKernelGGL(gram_input_grad_kernel, dim3(gpar_ceil_div(n1, GRAM_T), nsplit), dim3(256), lds, (hipStream_t)stream, *ks, z1, n1,
                           ldz1, z2, n2, ldz2, dz, W, ldw, mode, nsplit, workspace);
    const long long total = (long long)n1 * dz;
    hipLaunchKernelGGL(gram_input_grad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const double*)workspace, nsplit, n1, dz, out, ldo);
    GPAR_LAUNCH_CHECK();
    return 0;
}

// ---- posterior decomposition by kernel component (ABI v18; gram_terms.h) ---------------------------------------------------------------------
// Argument errors are found before anything is launched: no output is touched.
int gpar_gram_terms(const gpar_kspec_t* ks, const int* comp, int ncomp, const double* z1, int n1, int ldz1, const double* z2, int n2, int ldz2,
                    int dz, double* K, int ldk, long long stride_k, void* stream) {
    GPAR_API_GUARD;
    TermGroups tg;
    const int rc = term_groups_check(ks, comp, ncomp, dz, tg);
    if (rc) return rc;
    if (n1 < 0 || n2 < 0) return GPAR_ARG_ERROR(5);
    if (n1 == 0 || n2 == 0) return 0;
    if (!z1 || !z2 || !K || ldz1 < dz || ldz2 < dz) return GPAR_ARG_ERROR(6);
    if (ldk < n2 || (ncomp > 1 && stride_k < (long long)(n1 - 1) * ldk + n2)) return GPAR_ARG_ERROR(7);
    return gram_terms_launch(ks, tg, z1, n1, ldz1, z2, n2, ldz2, dz, K, ldk, stride_k, (hipStream_t)stream);
}

int gpar_gram_terms_diag(const gpar_kspec_t* ks, const int* comp, int ncomp, const double* z, int n, int ldz, int dz, double* out, int ldo,
                         void* stream) {
    GPAR_API_GUARD;
    TermGroups tg;
    const int rc = term_groups_check(ks, comp, ncomp, dz, tg);
    if (rc) return rc;
    if (n < 0) return GPAR_ARG_ERROR(5);
    if (n == 0) return 0;
    if (!z || !out || ldz < dz) return GPAR_ARG_ERROR(6);
    if (ldo < n) return GPAR_ARG_ERROR(7);
    return gram_terms_diag_launch(ks, tg, z, n, ldz, out, ldo, nullptr, 0, (hipStream_t)stream);
}

int gpar_posterior_terms(const gpar_kspec_t* ks, const int* comp, int ncomp, const double* zs, int ns, int ldzs, const double* z, int n, int ldz,
                         int dz, const double* alpha, const double* L, int ldl, double* mean, int ldm, double* var, int ldv, double* ws,
                         long long ws_doubles, void* stream) {
    GPAR_API_GUARD;
    TermGroups tg;
    const int rc = term_groups_check(ks, comp, ncomp, dz, tg);
    if (rc) return rc;
    if (n < 0 || ns < 0) return GPAR_ARG_ERROR(5);
    if (ns == 0) return 0;
    if (!zs || !mean || ldzs < dz || (n > 0 && (!z || !alpha || ldz < dz || (var && (!L || ldl < n))))) return GPAR_ARG_ERROR(6);
    if (ldm < ns || (var && ldv < ns)) return GPAR_ARG_ERROR(7);
    if (!ws || ws_doubles < (long long)ncomp * ns || (var && n > 0 && ws_doubles < pt_row_doubles(n, ncomp))) return GPAR_ARG_ERROR(8);
    return posterior_terms_run(ks, tg, zs, ns, ldzs, z, n, ldz, dz, alpha, L, ldl, mean, ldm, var, ldv, ws, ws_doubles, (hipStream_t)stream);
}

// ---- posterior derivatives (ABI v21; gram_deriv.h) ----------------------------------------------------------------------------------------------
// Argument errors are found before anything is launched: no output is touched.
int gpar_posterior_deriv(const gpar_kspec_t* ks, const double* zs, int ns, int ldzs, const double* J, int ldj, long long stride_j, int ndir,
                         const double* z, int n, int ldz, int dz, const double* alpha, const double* L, int ldl, double* mean, int ldm, double* var,
                         int ldv, double* ws, long long ws_doubles, void* stream) {
    GPAR_API_GUARD;
    DerivPlan pl;
    const int rc = deriv_check(ks, ndir, dz, pl);
    if (rc) return rc;
    if (n < 0 || ns < 0) return GPAR_ARG_ERROR(5);
    if (ns == 0) return 0;
    if (!zs || !mean || ldzs < dz || (dz > 0 && (!J || ldj < dz || (ndir > 1 && stride_j < (long long)(ns - 1) * ldj + dz)))) return GPAR_ARG_ERROR(6);
    if (n > 0 && (!z || !alpha || ldz < dz || (var && (!L || ldl < n)))) return GPAR_ARG_ERROR(6);
    if (ldm < ns || (var && ldv < ns)) return GPAR_ARG_ERROR(7);
    if (!ws || ws_doubles < (long long)ndir * ns || (var && n > 0 && ws_doubles < pt_row_doubles(n, ndir))) return GPAR_ARG_ERROR(8);
    if (pd_lds_bytes(dz, ndir, true) > PD_MAX_LDS) return GPAR_ARG_ERROR(9);   // the tiles of features and directions must fit the LDS
    return posterior_deriv_run(ks, pl, zs, ns, ldzs, J, ldj, stride_j, ndir, z, n, ldz, dz, alpha, L, ldl, mean, ldm, var, ldv, ws, ws_doubles,
                               (hipStream_t)stream);
}

// ---- per-row gradient moment sums (gram_grad_rows.h) --------------------------------------------------------------------------------------------
// Argument errors are found before anything is launched: no output is touched.
int gpar_gram_grad_rows(const gpar_kspec_t* ks, const double* z1, const double* zd1, int n1, int ldz1, const double* z2, const double* zd2, int n2,
                        int ldz2, int dz, const double* v, double* out, int ldo, double* ws, long long ws_doubles, void* stream) {
    GPAR_API_GUARD;
    if (n1 < 0 || n2 < 0) return GPAR_ARG_ERROR(5);
    RowsPlan pl;
    const int rc = rows_check(ks, dz, zd1 != nullptr, pl);
    if (rc) return rc;
    if (n1 == 0) return 0;
    // (the rule of gpar_gram_grad_cross: both, for P_q, or neither - where there are rows of z2 to read)
    if (n2 > 0 && (zd1 == nullptr) != (zd2 == nullptr)) return GPAR_ARG_ERROR(8);
    if (ldo < GRAD_NACC || ldz1 < dz || ldz2 < dz) return GPAR_ARG_ERROR(7);
    if (!out || (dz > 0 && !z1) || (n2 > 0 && (!v || (dz > 0 && !z2)))) return GPAR_ARG_ERROR(6);
    if (!ws || ws_doubles < (long long)n1 * GRAD_NACC) return GPAR_ARG_ERROR(9);
    if (rows_lds_bytes(dz, zd1 != nullptr, pl.nused) > ROWS_MAX_LDS) return GPAR_ARG_ERROR(10);   // the tiles and accumulators must fit the LDS
    return gram_grad_rows_run(ks, pl, z1, zd1, n1, ldz1, z2, zd2, n2, ldz2, dz, v, out, ldo, ws, ws_doubles, (hipStream_t)stream);
}

// ---- generalised Lomb-Scargle periodogram (ABI v19; periodogram.h) ------------------------------------------------------------------------------
int gpar_periodogram(const double* t, int n, double t0, const double* y, int ldy, const double* omega, int ldo, int p, const double* freq, int nf,
                     double* power, int ldp, void* stream) {
    GPAR_API_GUARD;
    return periodogram_launch(t, n, t0, y, ldy, omega, ldo, p, freq, nf, power, ldp, (hipStream_t)stream);
}

// ---- pathwise posterior sampling (ABI v20; pathwise.h) --------------------------------------------------------------------------------------------
// Argument errors are found before anything is launched: no output is touched.
int gpar_rff_apply(const double* z, int rows, int ldz, int dz, const double* shift, const double* omega, int ldw, int nfreq, const double* thc,
                   const double* ths, int ldt, int count, int group_rows, double* out, int ldo, void* stream) {
    GPAR_API_GUARD;
    return rff_apply_launch(z, rows, ldz, dz, shift, omega, ldw, nfreq, thc, ths, ldt, count, group_rows, out, ldo, (hipStream_t)stream);
}

int gpar_gram_apply_groups(const gpar_kspec_t* ks, const double* zs, int rows, int ldzs, const double* z, int n, int ldz, int dz, const double* vt,
                           int ldv, int count, int group_rows, double* out, int ldo, double* ws, long long ws_doubles, void* stream) {
    GPAR_API_GUARD;
    TermGroups tg;
    const int every[GPAR_MAX_TERMS] = {0, 0, 0, 0, 0, 0, 0, 0};   // one component holding every term
    static_assert(GPAR_MAX_TERMS == 8, "the grouping above names every term");
    const int rc = term_groups_check(ks, every, 1, dz, tg);
    if (rc) return rc;
    if (n < 0 || rows < 0 || count < 0 || group_rows < 0) return GPAR_ARG_ERROR(5);
    if (group_rows > 0 && (long long)group_rows * count != rows) return GPAR_ARG_ERROR(5);
    if (rows == 0 || count == 0) return 0;
    if (!zs || !out || ldzs < dz || (n > 0 && (!z || !vt || ldz < dz || ldv < n))) return GPAR_ARG_ERROR(6);
    if (group_rows == 0 && ldo < count) return GPAR_ARG_ERROR(7);
    if (!ws || ws_doubles < (long long)rows * (group_rows > 0 ? 1 : count)) return GPAR_ARG_ERROR(8);
    return gram_apply_groups_run(ks, tg, zs, rows, ldzs, z, n, ldz, dz, vt, ldv, count, group_rows, out, group_rows > 0 ? 1 : ldo, ws, ws_doubles,
                                 (hipStream_t)stream);
}

int gpar_potrf(double* A, int N, int nf, int lda, double* logdet, int* info, void* stream) {
    GPAR_API_GUARD;
    if (N <= 0 || nf <= 0) return 0;
    return potrf_run(A, N, nf, lda, logdet, info, (hipStream_t)stream);
}

int gpar_potrf_ex(double* A, int N, int nf, int lda, double* logdet, int* info, int flags, void* stream) {
    GPAR_API_GUARD;
    if (N <= 0 || nf <= 0) return 0;
    return potrf_run(A, N, nf, lda, logdet, info, (hipStream_t)stream, flags);
}

int gpar_trsm_rlt(const double* L, int n, int ldl, double* B, int nrows, int ldb, void* stream) {
    GPAR_API_GUARD;
    return trsm_rlt_run(L, n, ldl, B, nrows, ldb, (hipStream_t)stream);
}

int gpar_trsm_rlt_if(const double* L, int n, int ldl, double* B, int nrows, int ldb, const int* flag, int run_if, void* stream) {
    GPAR_API_GUARD;
    g_pred.flag = flag;
    g_pred.sense = run_if;
    const int rc = trsm_rlt_run(L, n, ldl, B, nrows, ldb, (hipStream_t)stream);
    g_pred.flag = nullptr;
    g_pred.sense = 0;
    return rc;
}

int gpar_vfe_assemble(const double* G, int M, int ldg, const double* c, const double* ys, const double* kdiag, const double* d, int n,
                      double diag_add, double* A, int lda, double* scal, double* logdet, int* info, void* stream) {
    GPAR_API_GUARD;
    if (M <= 0 || n < 0) return 0;
    if (!G || !c || !A || !scal || !logdet || !info || (n > 0 && (!ys || !kdiag || !d))) return GPAR_ARG_ERROR(1);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(vfe_assemble_kernel, dim3(gpar_ceil_div(M + 1, 256), M + 1), dim3(256), 0, st, G, M, ldg, c, diag_add, A, lda, logdet, info);
    hipLaunchKernelGGL(vfe_sums_kernel, dim3(VFE_PARTS), dim3(256), 0, st, ys, kdiag, d, n, G, M, ldg, scal);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_vfe_value(const double* scal, const double* logdet, const double* A, int lda, int M, int n, int with_trace, double* out, void* stream) {
    GPAR_API_GUARD;
    if (!scal || !logdet || !A || !out) return GPAR_ARG_ERROR(1);
    hipLaunchKernelGGL(vfe_value_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, scal, logdet, A, lda, M, (double)n * 1.8378770664093453, with_trace, out);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_chol_spread(const double* L, int n, int ldl, double limit, double* spread, int* flag, void* stream) {
    GPAR_API_GUARD;
    if (n <= 0 || (!spread && !flag)) return 0;
    if (!L) return GPAR_ARG_ERROR(1);
    hipLaunchKernelGGL(chol_spread_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, L, n, ldl, limit, spread, flag);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_trsm_rln(const double* L, int n, int ldl, double* B, int nrows, int ldb, void* stream) {
    GPAR_API_GUARD;
    return trsm_rln_run(L, n, ldl, B, nrows, ldb, (hipStream_t)stream);
}

int gpar_chol_inverse(const double* L, int n, int ldl, double* X, int ldx, double* Kinv, int ldk, void* stream) {
    GPAR_API_GUARD;
    return chol_inverse_run(L, n, ldl, X, ldx, Kinv, ldk, (hipStream_t)stream);
}

int gpar_chol_drop_leading(const double* A, int n, int k, int lda, double* out, int ldo, double* ws, double* logdet, int* info, void* stream) {
    GPAR_API_GUARD;
    return chol_drop_leading_run(A, n, k, lda, out, ldo, ws, logdet, info, (hipStream_t)stream);
}

int gpar_chol_append(double* A, int n0, int k, int lda, double* logdet, int* info, int potrf_flags, void* stream) {
    GPAR_API_GUARD;
    if (n0 < 0 || k < 1 || lda < n0 + k + 1) return GPAR_ARG_ERROR(1);
    if (!A) return GPAR_ARG_ERROR(2);
    hipStream_t st = (hipStream_t)stream;
    const int N = n0 + k + 1;
    double* bottom = A + (size_t)n0 * lda;   // the k + 1 bottom rows; their trailing block starts at column n0
    GPAR_HIP_TRY(hipMemsetAsync(A + (size_t)(N - 1) * lda + (N - 1), 0, sizeof(double), st));
    if (n0 > 0) {
        int rc = trsm_rlt_run(A, n0, lda, bottom, k, lda, st);
        if (rc) return rc;
        rc = gemm_launch(0, 1, k + 1, k + 1, n0, -1.0, bottom, lda, bottom, lda, 1.0, bottom + n0, lda, GPAR_GEMM_C_LOWER, st);
        if (rc) return rc;
    }
    return potrf_run(bottom + n0, k + 1, k, lda, logdet, info, st, potrf_flags);
}

int gpar_gemm(int ta, int tb, int m, int n, int k, double alpha, const double* A, int lda, const double* B, int ldb,
              double beta, double* C, int ldc, int flags, void* stream) {
    GPAR_API_GUARD;
    return gemm_launch(ta, tb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, flags, (hipStream_t)stream);
}

int gpar_gemm_batch(int ta, int tb, int m, int n, int k, double alpha, const double* A, int lda, long long stride_a, const double* B,
                    int ldb, long long stride_b, double beta, double* C, int ldc, long long stride_c, int flags, int batch, void* stream) {
    GPAR_API_GUARD;
    if (batch <= 0) return 0;
    if (stride_a < 0 || stride_b < 0 || stride_c < 0) return GPAR_ARG_ERROR(9);
    return gemm_launch(ta, tb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, flags, (hipStream_t)stream, 0, batch, stride_a, stride_b, stride_c);
}

int gpar_gemm_splitk(int ta, int tb, int m, int n, int k, double alpha, const double* A, int lda, const double* B, int ldb,
                     double beta, double* C, int ldc, int flags, int splits, double* workspace, void* stream) {
    GPAR_API_GUARD;
    return gemm_splitk_launch(ta, tb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, flags, splits, workspace, (hipStream_t)stream);
}

int gpar_dot(const double* x, int incx, const double* y, int incy, int n, double* out, int accumulate, void* stream) {
    GPAR_API_GUARD;
    hipLaunchKernelGGL(dot_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, x, (long)incx, y, (long)incy, n, out, accumulate);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_gemv_t(const double* A, int rows, int cols, int lda, const double* v, double* out, double* workspace, void* stream) {
    GPAR_API_GUARD;
    if (!out || (rows > 0 && cols > 0 && (!A || !v || !workspace))) return GPAR_ARG_ERROR(2);
    return gemv_t_run(A, rows, cols, lda, v, out, workspace, (hipStream_t)stream);
}

int gpar_rownorm2(const double* A, int rows, int cols, int lda, double* out, void* stream) {
    GPAR_API_GUARD;
    if (rows <= 0) return 0;
    if (!A || !out) return GPAR_ARG_ERROR(2);
    hipLaunchKernelGGL(rownorm2_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, A, rows, cols, lda, out);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_pack_lower(const double* A, int n, int lda, double* out, void* stream) {
    GPAR_API_GUARD;
    if (n <= 0) return 0;
    if (!A || !out) return GPAR_ARG_ERROR(2);
    hipLaunchKernelGGL(pack_lower_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, A, n, lda, out);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_unpack_lower(const double* in, int n, double* A, int lda, void* stream) {
    GPAR_API_GUARD;
    if (n <= 0) return 0;
    if (!A || !in) return GPAR_ARG_ERROR(2);
    hipLaunchKernelGGL(unpack_lower_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, in, n, A, lda);
    GPAR_LAUNCH_CHECK();
    return 0;
}

long long gpar_workspace_doubles(int op, int a, int b, int c) {
    switch (op) {
        case GPAR_WS_GEMM_SPLITK: return (long long)a * b * (c > 1 ? c : 1);           /* m, n, splits */
        case GPAR_WS_GEMV_T: return (long long)gemv_t_chunks(a) * (b > 0 ? b : 0);      /* rows, cols */
        case GPAR_WS_GRAM_GRAD: return (long long)(a > 0 ? a : 0) * GRAD_NACC;          /* nblocks */
        case GPAR_WS_CHOL_INVERSE: return (long long)a * b;                             /* n, ldx: the X matrix */
        case GPAR_WS_INPUT_GRAD: return (long long)a * b * (c > 1 ? c : 1);             /* n1, dz, nsplit */
        case GPAR_WS_LOO: return (long long)(a > 0 ? a : 0) * (b ? 4 : 1);              /* n, with gradient */
        case GPAR_WS_CV:                                                                /* n, with gradient, max_fold */
            if (c < 1 || c > GPAR_CV_MAX_FOLD) return -1;
            return (long long)(a > 0 ? a : 0) * (b ? 3 + c : 1);
        case GPAR_WS_AHEAD: return ah_workspace_doubles(a, b);                          /* n, with gradient */
        case GPAR_WS_CV_GAP: return cvg_workspace_doubles(a, b, c);                     /* n, with gradient, max_hold */
        case GPAR_WS_AHEAD_MULTI: return ahm_workspace_doubles(a, b, c);                /* n, with gradient, horizons */
        case GPAR_WS_AHEAD_WINDOW: return aw_workspace_doubles(a, b);                   /* n, with gradient */
        case GPAR_WS_PIVOTED_CHOL: return pc_workspace_doubles(a);                       /* n */
        case GPAR_WS_CHOL_UPDATE: return cu_workspace_doubles(a, b);                     /* n, k */
        case GPAR_WS_POSTERIOR_TERMS: return pt_workspace_doubles(a, b, c);              /* n, ns, ncomp */
        case GPAR_WS_GRAM_APPLY: return ga_workspace_doubles(a, b, c);                   /* n, rows, output columns (1 with groups) */
        case GPAR_WS_POSTERIOR_DERIV: return pt_workspace_doubles(a, b, c);              /* n, ns, ndir */
        case GPAR_WS_GRAM_GRAD_ROWS: return rows_workspace_doubles(a, b);                /* n2, n1 */
        default: return -1;
    }
}

int gpar_randn(uint64_t seed, uint64_t offset, double* out, int rows, int cols, int ldo, void* stream) {
    GPAR_API_GUARD;
    if (rows <= 0 || cols <= 0) return 0;
    const size_t pairs = ((size_t)rows * cols + 1) / 2;
    hipLaunchKernelGGL(randn_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed, offset, out,
                       rows, cols, ldo);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_trmv_lower(const double* L, int n, int ldl, const double* x, int incx, double* y, int incy, void* stream) {
    GPAR_API_GUARD;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(trmv_lower_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, L, n, ldl, x, incx, y, incy);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_trmv_upper(const double* U, int n, int ldu, const double* x, int incx, double* y, int incy, void* stream) {
    GPAR_API_GUARD;
    if (n <= 0) return 0;
    if (!U || !x || !y) return GPAR_ARG_ERROR(2);
    hipLaunchKernelGGL(trmv_upper_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, U, n, ldu, x, incx, y, incy);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_gemv(const double* A, int rows, int cols, int lda, const double* x, int incx, double alpha, double* y, int incy, void* stream) {
    GPAR_API_GUARD;
    if (rows <= 0) return 0;
    if (!A || !y || (cols > 0 && !x)) return GPAR_ARG_ERROR(2);
    hipLaunchKernelGGL(gemv_n_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, A, rows, cols, lda, x, incx, alpha, y, incy);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_trmv_lower_batch(const double* L, int batch, long long stride_l, int n, int ldl, const double* x, int incx, long long stride_x,
                          const double* add, int inca, long long stride_add, double* y, int incy, long long stride_y, void* stream) {
    GPAR_API_GUARD;
    if (n <= 0 || batch <= 0) return 0;
    if (!L || !x || !y) return GPAR_ARG_ERROR(2);
    hipLaunchKernelGGL(trmv_lower_batch_kernel, dim3((unsigned)((n + 3) / 4), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, L, stride_l,
                       n, ldl, x, incx, stride_x, add, inca, stride_add, y, incy, stride_y);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_sample_stats(const double* samples, int S, long long count, long long stride, int k_lo, double g_lo, int k_hi,
                      double g_hi, double* mean, double* lo, double* hi, void* stream) {
    GPAR_API_GUARD;
    if (count <= 0) return 0;
    if (S <= 0 || S > 65536 || !samples || !mean) return GPAR_ARG_ERROR(2);
    if ((lo || hi) && (k_lo < 0 || k_lo >= S || k_hi < 0 || k_hi >= S)) return GPAR_ARG_ERROR(5);
    hipLaunchKernelGGL(sample_stats_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, samples, S,
                       count, stride, k_lo, g_lo, k_hi, g_hi, mean, lo, hi);
    GPAR_LAUNCH_CHECK();
    return 0;
}

int gpar_profile_enable(int on) {
    GPAR_API_GUARD_NOSTREAM;
    g_prof.on = on != 0;
    return 0;
}

int gpar_profile_read(int* launches, double* ms, double* busy_ms, double* flops, int reset) {
    GPAR_API_GUARD_NOSTREAM;
    profile_collect();
    if (launches) *launches = g_prof.launches;
    if (ms) *ms = g_prof.ms_done;
    if (busy_ms) *busy_ms = g_prof.ms_busy;
    if (flops) *flops = g_prof.flops;
    if (reset) { g_prof.launches = 0; g_prof.ms_done = 0.0; g_prof.ms_busy = 0.0; g_prof.flops = 0.0; }
    return 0;
}

}  // extern "C"
