// Generalised Lomb-Scargle periodogram (Zechmeister & Kuerster 2009: floating mean, weights) of the p columns of y on an arbitrary
// frequency grid: gpar_periodogram (ABI v19; include/gpar_hip.h states the formula, the degenerate cases and the argument errors).
//
// Shape.  A workgroup of 256 threads owns PG_FREQS = 64 frequencies - lane l of every wave is frequency 64 * blockIdx.x + l - and its
// PG_SLICES = 4 waves divide the rows: the rows are staged in tiles of 256 (time difference t_i - t0, normalised weight, centred
// observation per output) and wave s takes rows 64 s .. 64 s + 63 of every tile, in ascending order.  One sincospi(2 f (t_i - t0)) per
// (row, frequency) pair serves the PG_CHUNK = 4 outputs of a chunk (8 accumulators each, in registers); more outputs are taken in
// further chunks, which repeat the sincospi.  No recurrence along the grid: every pair's sine and cosine come from its own argument.
//
// Order.  A frequency's sums are the four slices' partial sums - each a serial sum over its rows in ascending order - added as
// ((s0 + s1) + s2) + s3 by wave 0 through LDS.  The division of rows depends on n alone and a lane's arithmetic on nothing but its own
// frequency: the power at a frequency has the same bits alone or inside any grid, and two calls agree in bits.  No atomics.
//
// The frequency-independent sums (total weight, observed rows, weighted mean per output) are formed first, by every workgroup in the
// same fixed order (thread t sums rows t, t + 256, ..., then a tree over the 256 partial sums): every workgroup holds the same bits.
// The observations are centred by that mean before they enter the sums (the power is invariant; the second moment then carries no
// cancellation against the squared mean), and the residual mean of the centred values is still subtracted as the formula asks.
#pragma once
#include "common.h"

namespace gpar {

constexpr int PG_FREQS = 64;    // frequencies per workgroup: one per lane
constexpr int PG_SLICES = 4;    // waves per workgroup: each sums a quarter of every row tile
constexpr int PG_TILE = PG_FREQS * PG_SLICES;   // rows staged at a time, and threads per workgroup
constexpr int PG_CHUNK = 4;     // outputs that share one sincospi (8 fp64 accumulators each)
constexpr int PG_NACC = 8;      // C, S, sum w cos^2, sum w cos sin, sum w y, sum w y^2, sum w y cos, sum w y sin

// The smallness tests, defined once.  The weights are normalised to sum 1, so sum w cos^2 + sum w sin^2 = 1: the trigonometric sums
// are of magnitude 1 and carry a rounding error of about n 2^-53 each.  With tiny = 16 n 2^-52:
//   * fewer than 3 observed rows                          -> 0 (a sinusoid with a floating mean fits any 3 values)
//   * YY <= tiny^2 mean^2  (YY: weighted variance)        -> 0: constant y - centred by a mean that is itself off by up to n 2^-53 mean
//   * D = CC SS - CS^2 <= tiny                            -> 0: sine and cosine are not independent on these time stamps
// and a frequency that is not a positive finite number has power 0.
__device__ __forceinline__ double pg_tiny(int n) { return 16.0 * (double)n * 2.220446049250313e-16; }

__global__ __launch_bounds__(PG_TILE) void periodogram_kernel(const double* __restrict__ t, int n, double t0, const double* __restrict__ y, int ldy,
                                                              const double* __restrict__ omega, int ldo, int p, const double* __restrict__ freq,
                                                              int nf, double* __restrict__ power, int ldp) {
#pragma clang fp contract(off)
    __shared__ double s_dt[PG_TILE];
    __shared__ double s_w[PG_CHUNK][PG_TILE];
    __shared__ double s_y[PG_CHUNK][PG_TILE];
    __shared__ double s_red[PG_SLICES - 1][PG_NACC][PG_FREQS];   // also the 3 x 256 buffer of the first pass
    __shared__ double s_col[PG_CHUNK][3];                        // per output: 1 / total weight, weighted mean, observed rows
    const int tid = threadIdx.x, lane = tid & (PG_FREQS - 1), slice = tid / PG_FREQS;
    const int fi = blockIdx.x * PG_FREQS + lane;
    const double f = fi < nf ? freq[fi] : 0.0;
    const bool f_ok = f > 0.0 && f <= 1.7976931348623157e308;
    const double f2 = 2.0 * f;   // exact
    const double tiny = pg_tiny(n);
    double* red1 = &s_red[0][0][0];   // PG_TILE * 3 doubles <= (PG_SLICES - 1) * PG_NACC * PG_FREQS

    for (int c0 = 0; c0 < p; c0 += PG_CHUNK) {
        const int pc = min(PG_CHUNK, p - c0);
        // ---- first pass: total weight, weighted sum, observed rows of every output of the chunk
        for (int j = 0; j < pc; ++j) {
            double w_sum = 0.0, wy_sum = 0.0, cnt = 0.0;
            for (int i = tid; i < n; i += PG_TILE) {
                const double om = omega[(size_t)i * ldo + c0 + j];
                if (om > 0.0) {
                    w_sum += om;
                    wy_sum = fma(om, y[(size_t)i * ldy + c0 + j], wy_sum);
                    cnt += 1.0;
                }
            }
            __syncthreads();
            red1[tid] = w_sum; red1[PG_TILE + tid] = wy_sum; red1[2 * PG_TILE + tid] = cnt;
            __syncthreads();
            for (int off = PG_TILE / 2; off > 0; off >>= 1) {
                if (tid < off) {
                    red1[tid] += red1[tid + off];
                    red1[PG_TILE + tid] += red1[PG_TILE + tid + off];
                    red1[2 * PG_TILE + tid] += red1[2 * PG_TILE + tid + off];
                }
                __syncthreads();
            }
            if (tid == 0) {
                const double W = red1[0];
                s_col[j][0] = W > 0.0 ? 1.0 / W : 0.0;
                s_col[j][1] = W > 0.0 ? red1[PG_TILE] / W : 0.0;
                s_col[j][2] = red1[2 * PG_TILE];
            }
        }
        __syncthreads();

        // ---- the sums over the rows: this wave's quarter of every tile
        double acc[PG_CHUNK][PG_NACC];
#pragma unroll
        for (int j = 0; j < PG_CHUNK; ++j)
#pragma unroll
            for (int a = 0; a < PG_NACC; ++a) acc[j][a] = 0.0;
        for (int base = 0; base < n; base += PG_TILE) {
            const int i = base + tid;
            s_dt[tid] = i < n ? t[i] - t0 : 0.0;
#pragma unroll
            for (int j = 0; j < PG_CHUNK; ++j) {
                double w = 0.0, yc = 0.0;
                if (i < n && j < pc) {
                    const double om = omega[(size_t)i * ldo + c0 + j];
                    if (om > 0.0) {   // (an unobserved entry's y is never read)
                        w = om * s_col[j][0];
                        yc = y[(size_t)i * ldy + c0 + j] - s_col[j][1];
                    }
                }
                s_w[j][tid] = w;
                s_y[j][tid] = yc;
            }
            __syncthreads();
            const int r_end = min(PG_FREQS, n - base - slice * PG_FREQS);
            for (int r = 0; r < r_end; ++r) {
                const int row = slice * PG_FREQS + r;
                double sn, cs;
                sincospi(f2 * s_dt[row], &sn, &cs);
#pragma unroll
                for (int j = 0; j < PG_CHUNK; ++j) {
                    const double w = s_w[j][row], yc = s_y[j][row];
                    const double wc = w * cs, wy = w * yc;
                    acc[j][0] += wc;
                    acc[j][1] = fma(w, sn, acc[j][1]);
                    acc[j][2] = fma(wc, cs, acc[j][2]);
                    acc[j][3] = fma(wc, sn, acc[j][3]);
                    acc[j][4] += wy;
                    acc[j][5] = fma(wy, yc, acc[j][5]);
                    acc[j][6] = fma(wy, cs, acc[j][6]);
                    acc[j][7] = fma(wy, sn, acc[j][7]);
                }
            }
            __syncthreads();
        }

        // ---- per output: slices 1 .. 3 hand their sums to wave 0, which adds them in order and forms the power
#pragma unroll
        for (int j = 0; j < PG_CHUNK; ++j) {
            if (j < pc) {   // (uniform over the workgroup)
                if (slice > 0) {
#pragma unroll
                    for (int a = 0; a < PG_NACC; ++a) s_red[slice - 1][a][lane] = acc[j][a];
                }
                __syncthreads();
                if (slice == 0 && fi < nf) {
                    double v[PG_NACC];
#pragma unroll
                    for (int a = 0; a < PG_NACC; ++a) v[a] = ((acc[j][a] + s_red[0][a][lane]) + s_red[1][a][lane]) + s_red[2][a][lane];
                    const double C = v[0], S = v[1], Y = v[4];
                    const double YY = v[5] - Y * Y, YC = v[6] - Y * C, YS = v[7] - Y * S;
                    const double CC = v[2] - C * C, SS = (1.0 - v[2]) - S * S, CS = v[3] - C * S;
                    const double D = CC * SS - CS * CS;
                    const double mean = s_col[j][1];
                    double pw = 0.0;
                    if (f_ok && s_col[j][2] >= 3.0 && YY > (tiny * tiny) * (mean * mean) && YY > 0.0 && D > tiny) {
                        pw = (SS * (YC * YC) + CC * (YS * YS) - 2.0 * CS * (YC * YS)) / (YY * D);
                        pw = pw >= 0.0 ? (pw <= 1.0 ? pw : 1.0) : 0.0;   // (rounding may leave 1 + 2^-52; a NaN cannot arise, and would become 0)
                    }
                    power[(size_t)(c0 + j) * ldp + fi] = pw;
                }
                __syncthreads();
            }
        }
    }
}

// Argument errors are found here, before the launch: no output is touched.
static int periodogram_launch(const double* t, int n, double t0, const double* y, int ldy, const double* omega, int ldo, int p, const double* freq,
                              int nf, double* power, int ldp, hipStream_t stream) {
    if (n < 0 || nf < 0) return GPAR_ARG_ERROR(1);
    if (p < 1) return GPAR_ARG_ERROR(2);
    if (ldy < p || ldo < p) return GPAR_ARG_ERROR(3);
    if (nf > 0 && ldp < nf) return GPAR_ARG_ERROR(4);
    if (!(t0 == t0) || t0 - t0 != 0.0) return GPAR_ARG_ERROR(5);   // NaN or infinite
    if (n == 0 || nf == 0) return 0;
    if (!t || !y || !omega || !freq || !power) return GPAR_ARG_ERROR(6);
    hipLaunchKernelGGL(periodogram_kernel, dim3((unsigned)gpar_ceil_div(nf, PG_FREQS)), dim3(PG_TILE), 0, stream, t, n, t0, y, ldy, omega, ldo, p,
                       freq, nf, power, ldp);
    GPAR_LAUNCH_CHECK();
    return 0;
}

}  // namespace gpar
