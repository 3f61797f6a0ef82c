// Pathwise posterior sampling (ABI v20; Matheron's rule - Wilson et al., "Efficiently sampling functions from Gaussian process
// posteriors", ICML 2020): the two device passes of
//     f*_s(.) = f_s(.) + k(., X) (K + D)^-1 (y - f_s(X) - eps_s),     f_s(z) = sum_j thc[j, s] cos(2 pi w_j . (z - shift)) + ths[j, s] sin(...)
// gpar_rff_apply evaluates the random Fourier prior f_s at feature rows, gpar_gram_apply_groups the update k(., X) v_s.  Rows come in
// GROUPS (the S stacked design matrices of ancestral sampling: `group_rows` rows each, group g uses weight column g), or, with
// group_rows = 0, as one set of rows that meets EVERY column (the training rows; a design matrix all samples share).
//
// Both kernels are interpreters in the style of gram_terms.h: 256 threads own 64 rows, the rows' features are staged in LDS, no n* x n
// and no rows x F matrix is written.  No floating-point atomics: every sum has a fixed order that depends on the sizes alone, so a call
// returns the same bits every time, and a row's value depends on its own features, the basis (the training rows) and its own weight
// column alone - it has the same bits whatever other rows, groups or columns the call holds.  (gpar_gram_apply_groups: among calls that
// split the training rows alike - the number of splits follows n, the total number of rows and the workspace, see pt_nsplit.)
#pragma once
#include "gram_terms.h"

namespace gpar {

constexpr int PW_ROWS = 64;     // rows per workgroup: one per lane
constexpr int PW_SLICES = 4;    // waves per workgroup: each takes a quarter of every frequency tile
constexpr int PW_FREQS = 64;    // frequencies staged at a time
constexpr int PW_COLS = 4;      // weight columns that share one sincospi (group_rows = 0; a group has one column)

// Rows, groups and columns of a call: group_rows > 0 - `count` groups of group_rows rows, one column each; group_rows = 0 - one set of
// `rows` rows and `count` columns, taken PW_COLS (rff) or GA_COLS (gram apply) at a time.
struct PwShape {
    int tiles;       // row tiles per group
    int blocks;      // workgroups along x: tiles * (groups | column chunks)
};
static inline PwShape pw_shape(int rows, int count, int group_rows, int cols_per_block) {
    PwShape s;
    if (group_rows > 0) {
        s.tiles = gpar_ceil_div(group_rows, PW_ROWS);
        s.blocks = s.tiles * count;
    } else {
        s.tiles = gpar_ceil_div(rows, PW_ROWS);
        s.blocks = s.tiles * gpar_ceil_div(count, cols_per_block);
    }
    return s;
}

// ---- gpar_rff_apply ---------------------------------------------------------------------------------------------------------------------
// Workgroup (group | column chunk, row tile).  Lane l of every wave is row l of the tile; the tile's features, less the shift, are staged
// transposed ([dz][64]: lanes read consecutive words).  The frequencies are walked in tiles of 64 (omega rows and the weights of the
// workgroup's columns staged; every lane reads the same word: a broadcast); wave q takes frequencies 16 q .. 16 q + 15 of every tile, in
// ascending order, one sincospi(2 w . (z - shift)) per (row, frequency) pair, shared by the columns.  A row's sum is the four waves'
// partial sums added as ((s0 + s1) + s2) + s3 by wave 0 through LDS.
__global__ __launch_bounds__(256) void rff_apply_kernel(const double* __restrict__ z, int rows, int ldz, int dz, const double* __restrict__ shift,
                                                        const double* __restrict__ omega, int ldw, int F, const double* __restrict__ thc,
                                                        const double* __restrict__ ths, int ldt, int count, int group_rows, int tiles,
                                                        double* __restrict__ out, int ldo) {
    extern __shared__ __attribute__((aligned(32))) double psm[];
    const int dzl = dz > 0 ? dz : 1;
    double* Zt = psm;                                   // [dz][PW_ROWS]
    double* Wt = Zt + (size_t)dzl * PW_ROWS;            // [PW_FREQS][dz]
    double* Tc = Wt + (size_t)dzl * PW_FREQS;           // [PW_COLS][PW_FREQS]
    double* Ts = Tc + PW_COLS * PW_FREQS;               // [PW_COLS][PW_FREQS]
    double* red = Ts + PW_COLS * PW_FREQS;              // [PW_SLICES - 1][PW_COLS][PW_ROWS]
    const int t = threadIdx.x, lane = t & (PW_ROWS - 1), slice = t / PW_ROWS;
    const int chunk = blockIdx.x / tiles, tile = blockIdx.x - chunk * tiles;
    // rows of this workgroup: local row index lr < nrow, global row row_base + lr; columns col0 .. col0 + ncol - 1
    const int nrow_all = group_rows > 0 ? group_rows : rows;
    const long long row_base = (group_rows > 0 ? (long long)chunk * group_rows : 0) + (long long)tile * PW_ROWS;
    const int nrow = min(PW_ROWS, nrow_all - tile * PW_ROWS);
    const int col0 = group_rows > 0 ? chunk : chunk * PW_COLS;
    const int ncol = group_rows > 0 ? 1 : min(PW_COLS, count - col0);

    for (int idx = t; idx < PW_ROWS * dz; idx += 256) {
        const int r = idx / dz, d = idx - r * dz;
        Zt[d * PW_ROWS + r] = r < nrow ? z[(size_t)(row_base + r) * ldz + d] - shift[d] : 0.0;
    }
    double acc[PW_COLS];
#pragma unroll
    for (int c = 0; c < PW_COLS; ++c) acc[c] = 0.0;
    for (int j0 = 0; j0 < F; j0 += PW_FREQS) {
        __syncthreads();   // (the previous tile has been read; the first time: nothing yet)
        for (int idx = t; idx < PW_FREQS * dz; idx += 256) {
            const int j = idx / dz, d = idx - j * dz;
            Wt[j * dzl + d] = j0 + j < F ? omega[(size_t)(j0 + j) * ldw + d] : 0.0;
        }
        for (int idx = t; idx < PW_COLS * PW_FREQS; idx += 256) {
            const int c = idx / PW_FREQS, j = idx - c * PW_FREQS;
            const bool in = c < ncol && j0 + j < F;   // (a frequency past F, a column past the chunk: weight zero)
            Tc[idx] = in ? thc[(size_t)(j0 + j) * ldt + col0 + c] : 0.0;
            Ts[idx] = in ? ths[(size_t)(j0 + j) * ldt + col0 + c] : 0.0;
        }
        __syncthreads();
        const int jend = min(PW_FREQS / PW_SLICES, F - j0 - slice * (PW_FREQS / PW_SLICES));
        for (int jj = 0; jj < jend; ++jj) {
            const int j = slice * (PW_FREQS / PW_SLICES) + jj;
            double dot = 0.0;
            for (int d = 0; d < dz; ++d) dot = fma(Wt[j * dzl + d], Zt[d * PW_ROWS + lane], dot);
            double sn, cs;
            sincospi(2.0 * dot, &sn, &cs);
#pragma unroll
            for (int c = 0; c < PW_COLS; ++c) acc[c] = fma(Ts[c * PW_FREQS + j], sn, fma(Tc[c * PW_FREQS + j], cs, acc[c]));
        }
    }
    if (slice > 0) {
#pragma unroll
        for (int c = 0; c < PW_COLS; ++c) red[((slice - 1) * PW_COLS + c) * PW_ROWS + lane] = acc[c];
    }
    __syncthreads();
    if (slice == 0 && lane < nrow) {
        for (int c = 0; c < ncol; ++c) {
            const double v = ((acc[c] + red[(0 * PW_COLS + c) * PW_ROWS + lane]) + red[(1 * PW_COLS + c) * PW_ROWS + lane]) +
                             red[(2 * PW_COLS + c) * PW_ROWS + lane];
            if (group_rows > 0) out[row_base + lane] = v;
            else out[(size_t)(row_base + lane) * ldo + col0 + c] = v;
        }
    }
}

static inline size_t rff_lds_bytes(int dz) {
    const int dzl = dz > 0 ? dz : 1;
    return ((size_t)dzl * (PW_ROWS + PW_FREQS) + 2 * PW_COLS * PW_FREQS + (PW_SLICES - 1) * PW_COLS * PW_ROWS) * sizeof(double);
}

// Argument errors are found here, before the launch: no output is touched.
static int rff_apply_launch(const double* z, int rows, int ldz, int dz, const double* shift, const double* omega, int ldw, int F, const double* thc,
                            const double* ths, int ldt, int count, int group_rows, double* out, int ldo, hipStream_t stream) {
    if (rows < 0 || F < 0 || count < 0 || group_rows < 0) return GPAR_ARG_ERROR(1);
    if (dz < 0 || dz > GPAR_MAX_DIMS) return GPAR_ARG_ERROR(2);
    if (group_rows > 0 && (long long)group_rows * count != rows) return GPAR_ARG_ERROR(3);
    if (ldz < dz || ldw < dz || ldt < count || (group_rows == 0 && ldo < count)) return GPAR_ARG_ERROR(4);
    if (rows == 0 || count == 0) return 0;
    if (!out || (dz > 0 && (!z || !shift || (F > 0 && !omega))) || (F > 0 && (!thc || !ths))) return GPAR_ARG_ERROR(5);
    const PwShape s = pw_shape(rows, count, group_rows, PW_COLS);
    const size_t lds = rff_lds_bytes(dz);
    if (lds > 48 * 1024) GPAR_HIP_TRY(gpar_set_max_lds(reinterpret_cast<const void*>(&rff_apply_kernel), 160 * 1024));
    hipLaunchKernelGGL(rff_apply_kernel, dim3((unsigned)s.blocks), dim3(256), lds, stream, z, rows, ldz, dz, shift, omega, ldw, F, thc, ths, ldt, count,
                       group_rows, s.tiles, out, ldo);
    GPAR_LAUNCH_CHECK();
    return 0;
}

// ---- gpar_gram_apply_groups -------------------------------------------------------------------------------------------------------------
// out[r] = sum_a k(zs_r, z_a) v[a, g(r)]: the mean pass of posterior_terms_mean_kernel (gram_terms.h) with ONE component holding every
// term - same tiling, same split of the training rows (column tiles bn = split, split + nsplit, ...), same butterfly over the 16 lanes that
// share a row, same ordered sum of the splits - and the vector chosen by the row's group.  v is handed over TRANSPOSED, vt[g * ldv + a]:
// it comes out of the triangular solves that way, and a tile's 64 weights are one contiguous read.  group_rows = 0: the one set of rows
// meets every column, GA_COLS columns per workgroup share a tile's kernel values.
constexpr int GA_COLS = 4;

__global__ __launch_bounds__(256) void gram_apply_groups_kernel(gpar_kspec_t ks, TermGroups tg, const double* __restrict__ zs, int rows, int ldzs,
                                                                const double* __restrict__ z, int n, int ldz, int dz, const double* __restrict__ vt,
                                                                int ldv, int count, int group_rows, int tiles, int nsplit,
                                                                double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(32))) double gsm[];
    const int dzl = dz > 0 ? dz : 1;
    const double* tab = gsm;
    double* Za = gsm + GRAM_TAB_DOUBLES;
    double* Zb = Za + (size_t)dzl * GRAM_LD;
    double* al = Zb + (size_t)dzl * GRAM_LD;   // [GA_COLS][GRAM_LD]: the tile's weights, per column
    double* macc = al + GA_COLS * GRAM_LD;     // [GA_COLS][64]
    const int t = threadIdx.x;
    const int tx = t & 15, ty = t >> 4;
    const int chunk = blockIdx.x / tiles, tile = blockIdx.x - chunk * tiles, split = blockIdx.y;
    const int nrow_all = group_rows > 0 ? group_rows : rows;
    const long long row_base = (group_rows > 0 ? (long long)chunk * group_rows : 0) + (long long)tile * GRAM_T;
    const int nrow = min(GRAM_T, nrow_all - tile * GRAM_T);
    const int col0 = group_rows > 0 ? chunk : chunk * GA_COLS;
    const int ncol = group_rows > 0 ? 1 : min(GA_COLS, count - col0);
    const int nt2 = (n + GRAM_T - 1) / GRAM_T;
    gram_load_tables(gsm, t);
    for (int i = t; i < GA_COLS * GRAM_T; i += 256) macc[i] = 0.0;
    for (int idx = t; idx < GRAM_T * dz; idx += 256) {
        const int r = idx / dz, d = idx - r * dz;
        Za[d * GRAM_LD + r] = r < nrow ? zs[(size_t)(row_base + r) * ldzs + d] : 0.0;
    }
    for (int bn = split; bn < nt2; bn += nsplit) {
        const int cbase = bn * GRAM_T;
        __syncthreads();
        for (int idx = t; idx < GRAM_T * dz; idx += 256) {
            const int r = idx / dz, d = idx - r * dz;
            Zb[d * GRAM_LD + r] = (cbase + r < n) ? z[(size_t)(cbase + r) * ldz + d] : 0.0;
        }
        for (int idx = t; idx < GA_COLS * GRAM_T; idx += 256) {
            const int c = idx / GRAM_T, a = idx - c * GRAM_T;
            al[c * GRAM_LD + a] = (c < ncol && cbase + a < n) ? vt[(size_t)(col0 + c) * ldv + cbase + a] : 0.0;   // (columns past n: weight zero)
        }
        __syncthreads();
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            const int cb = 32 * h + 2 * tx;
            double total[8];
            gram_component8(ks, tg, 0, Za, Zb, tab, ty, cb, total);
#pragma unroll 1
            for (int c = 0; c < ncol; ++c) {
                const double a0 = al[c * GRAM_LD + cb], a1 = al[c * GRAM_LD + cb + 1];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    double p = fma(total[2 * i + 1], a1, total[2 * i] * a0);
#pragma unroll
                    for (int off = 8; off > 0; off >>= 1) p += __shfl_xor(p, off, 16);   // tx = 0 .. 15 of one ty are consecutive lanes
                    if (tx == 0) macc[c * GRAM_T + 4 * ty + i] += p;
                }
            }
        }
    }
    __syncthreads();
    // partial[(split * ncols_out + column) * rows + row]: ncols_out = 1 with groups (the column IS the group), count without
    const int ncols_out = group_rows > 0 ? 1 : count;
    for (int i = t; i < ncol * GRAM_T; i += 256) {
        const int c = i / GRAM_T, r = i - c * GRAM_T;
        const int oc = group_rows > 0 ? 0 : col0 + c;
        if (r < nrow) partial[((size_t)split * ncols_out + oc) * rows + row_base + r] = macc[i];
    }
}

// out[row * ldo + column] = the splits' partial sums, added in order
__global__ __launch_bounds__(256) void gram_apply_reduce_kernel(const double* __restrict__ partial, int nsplit, int ncols, int rows,
                                                                double* __restrict__ out, int ldo) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)ncols * rows) return;
    const int c = (int)(i / rows), r = (int)(i - (long long)c * rows);
    double s = 0.0;
    for (int q = 0; q < nsplit; ++q) s += partial[((size_t)q * ncols + c) * rows + r];
    out[(size_t)r * ldo + c] = s;
}

// Workspace: nsplit * rows * (output columns) partial sums; the recommended size takes the splits of pt_nsplit (gram_terms.h), the call
// takes any workspace that holds ONE split and sizes its splits by what it is given.
static inline long long ga_workspace_doubles(int n, int rows, int ncols_out) {
    if (n < 0 || rows < 0 || ncols_out < 1) return -1;
    const long long w = (long long)pt_nsplit(n, rows) * rows * ncols_out;
    return w > 1 ? w : 1;
}

static int gram_apply_groups_run(const gpar_kspec_t* ks, const TermGroups& tg, const double* zs, int rows, int ldzs, const double* z, int n, int ldz,
                                 int dz, const double* vt, int ldv, int count, int group_rows, double* out, int ldo, double* ws, long long ws_doubles,
                                 hipStream_t stream) {
    const int ncols_out = group_rows > 0 ? 1 : count;
    int nsplit = 0;   // (n = 0: the reduce kernel sums nothing and writes zeros)
    if (n > 0) {
        nsplit = pt_nsplit(n, rows);
        const long long fit = ws_doubles / ((long long)rows * ncols_out);
        if (fit < nsplit) nsplit = (int)fit;
        const PwShape s = pw_shape(rows, count, group_rows, GA_COLS);
        const size_t lds = ((size_t)2 * (dz > 0 ? dz : 1) * GRAM_LD + GRAM_TAB_DOUBLES + GA_COLS * GRAM_LD + GA_COLS * GRAM_T) * sizeof(double);
        if (lds > 48 * 1024) GPAR_HIP_TRY(gpar_set_max_lds(reinterpret_cast<const void*>(&gram_apply_groups_kernel), 160 * 1024));
        hipLaunchKernelGGL(gram_apply_groups_kernel, dim3((unsigned)s.blocks, nsplit), dim3(256), lds, stream, *ks, tg, zs, rows, ldzs, z, n, ldz, dz, vt,
                           ldv, count, group_rows, s.tiles, nsplit, ws);
    }
    const long long total = (long long)ncols_out * rows;
    hipLaunchKernelGGL(gram_apply_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const double*)ws, nsplit, ncols_out, rows,
                       out, ldo);
    GPAR_LAUNCH_CHECK();
    return 0;
}

}  // namespace gpar
