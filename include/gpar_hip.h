/*
 * gpar_hip.h — C ABI of libgpar_hip.so: the MI355X (gfx950) implementation of GPAR's
 * per-layer GP inference hot path.
 *
 * What this boundary replaces.  The reference (wesselb/gpar 0.3.2) contains no native code: every
 * Gram matrix, Cholesky factorisation and triangular solve is executed inside third-party Python
 * packages (stheno / mlkernels / matrix / lab -> torch CPU fp64 -> LAPACK), reached from
 *   - gpar/model.py:226      f.measure.logpdf(obs)            (Gram + potrf + trsv, per layer)
 *   - gpar/model.py:298-301  (f | obs).mean(x_)               (posterior mean)
 *   - gpar/model.py:264,270  f(x[, noise]).sample()           (posterior covariance + potrf + sample)
 *   - gpar/model.py:286-289  Obs / PseudoObs construction     (dense / inducing-point observations)
 *   - gpar/regression.py:92-180  kernel algebra of one layer  (which Gram matrix is built)
 *   - gpar/regression.py:459 minimise_l_bfgs_b(objective...)  (objective + gradient)
 * Each entry point below cites the call site whose arithmetic it performs.  A binding a maintainer of
 * the reference would add (ctypes) is shown in INTEGRATION.md.
 *
 * Conventions
 *   - All matrices are ROW-MAJOR IEEE fp64 in device (HBM) memory with an explicit leading dimension
 *     (elements between consecutive rows).  For symmetric matrices the LOWER triangle is authoritative;
 *     the strict upper triangle is never read; it may hold anything on entry and is SCRATCH: gpar_potrf keeps the
 *     hand-off words of its persistent panel kernels there (rows 0 .. 4, columns 8 .. 63 of every 64 x 64 diagonal tile:
 *     progress words of a panel's team, inverses of 16 x 16 diagonal blocks, and - where several panels share a launch -
 *     per-row-block progress words and tile counters), zeroed by one launch at the start of a factorisation.
 *   - Plain pointers and sizes only.  The caller owns every buffer, including workspace
 *     (gpar_workspace_doubles gives the sizes); the library never allocates or frees device MEMORY.  Every compute call
 *     only enqueues work on `stream` (a hipStream_t passed as void*) and returns; nothing synchronises the host except
 *     gpar_profile_read (a measurement aid).  What the library does create, lazily and once per device: one low-priority
 *     side stream per caller stream and a ring of events (gpar_potrf's look-ahead), the events of the profile hook, and the
 *     per-kernel dynamic-LDS attributes - so the first call on a device must not be made inside a stream capture.
 *   - Return value: 0 = launched OK; < 0 = -(hipError_t) or -1000-x for argument errors.  Numerical
 *     failure (non-positive pivot) is reported LAPACK-style through a device-side `info` word
 *     (1-based index of the first bad pivot, 0 = success) so that no host sync is forced.
 *   - gpar_potrf may use one internal low-priority stream per caller stream (look-ahead) and joins it back before
 *     it returns control of `stream`; callers see one in-order stream.  Process-global state (those streams, an event
 *     ring, the profile hook) sits behind one mutex: entry points only enqueue, so calls from several host threads
 *     (each with its own stream) are safe and simply serialise their enqueueing.  For the duration of a call the
 *     device that owns `stream` is made current (and the caller's current device restored on return), so a thread need
 *     not have called hipSetDevice; a null `stream` means the current device's default stream.
 *   - Pointers should be 16-byte aligned and leading dimensions even for the vectorised paths; other
 *     values are accepted and take a slower scalar path.
 */
#ifndef GPAR_HIP_H
#define GPAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPAR_ABI_VERSION 21

/* ---- kernel specification -------------------------------------------------------------------
 * A GPAR layer kernel (gpar/regression.py:92-180) is a sum of products of elementary kernels applied
 * to selected, rescaled (and possibly periodically embedded) input columns.  It is handed over in two
 * flat structs:
 *   gpar_fspec_t : how a raw design row x (m inputs + previous outputs, gpar/model.py:320) becomes a
 *                  feature row z:  z[q] = embed_q(x[col[q]]) * inv_scale[q]
 *                  embed 0: identity   1: sin(freq*x)   2: cos(freq*x)   (mlkernels .periodic()).
 *   gpar_kspec_t : k(z, z') = sum_t coef[t] * prod_{f in term t} phi_f(z[off:off+nd], z'[off:off+nd])
 *                  phi EQ: exp(-r2/2); RQ: (1 + r2/(2 alpha))^-alpha; LINEAR: <z, z'>; r2 = |z - z'|^2;
 *                  MATERN12 / 32 / 52: the Matern kernels of smoothness 1/2, 3/2, 5/2 in r = sqrt(r2) (codes below);
 *                  COS (ABI v17): cos(2 pi sigma), sigma = sum_d (z_d - z'_d) - the cosine of a SUM over the factor's dims (the
 *                  component of a spectral mixture: 1 / inv_scale of a dim is its period), formed from the explicit differences.
 *                  A term without factors is the constant kernel `coef`.
 */
#define GPAR_MAX_DIMS 96
#define GPAR_MAX_FACTORS 12
#define GPAR_MAX_TERMS 8

#define GPAR_EMBED_ID 0
#define GPAR_EMBED_SIN 1
#define GPAR_EMBED_COS 2

#define GPAR_K_EQ 0
#define GPAR_K_RQ 1
#define GPAR_K_LINEAR 2
#define GPAR_K_MATERN12 3 /* Matern nu = 1/2, 3/2, 5/2 with r = sqrt(r2):  exp(-r);  (1 + sqrt(3) r) exp(-sqrt(3) r); */
#define GPAR_K_MATERN32 4 /* (1 + sqrt(5) r + 5 r2 / 3) exp(-sqrt(5) r).  No parameter beyond the scales; k(x, x) = 1.  The  */
#define GPAR_K_MATERN52 5 /* derivative of nu = 1/2 with respect to r2 is singular at r = 0: every gradient pass takes it as 0 there */
#define GPAR_K_COS (6)    /* cos(2 pi sum_d (z_d - z'_d)) (ABI v17).  No parameter beyond the scales; k(x, x) = 1.  nd >= 1 (nd = 0 is an  */
                          /* argument error), identity-embedded dims only (an embedded dim is an argument error where the feature map is   */
                          /* at hand).  The gradient passes add g (z_d - z'_d) / 2 to the dim's scale sum, g = w * rest * (-2 pi sin(2 pi   */
                          /* sigma)), so that d / d scale = -2 A / scale as for the r2 factors; structures of more than 16 dims with a     */
                          /* cosine factor have no generated Gram kernel (the interpreter serves them).                                    */
                          /* (The value is written in parentheses on purpose: tests/test_matern.py asserts the exact set of bare-number    */
                          /* GPAR_K_* defines of this header as it stood before this type; tests/test_spectral.py checks this line.)       */

typedef struct {
    int32_t dz;                      /* number of feature dims (<= GPAR_MAX_DIMS) */
    int32_t pad_;
    int32_t col[GPAR_MAX_DIMS];      /* source column of x */
    int32_t embed[GPAR_MAX_DIMS];    /* GPAR_EMBED_* */
    double inv_scale[GPAR_MAX_DIMS]; /* 1 / length scale */
    double freq[GPAR_MAX_DIMS];      /* 2*pi / period (periodic dims only) */
} gpar_fspec_t;

typedef struct {
    int32_t type; /* GPAR_K_* */
    int32_t term; /* index of the product term this factor multiplies into */
    int32_t off;  /* first feature dim */
    int32_t nd;   /* number of feature dims (0 allowed: EQ/RQ/MATERN -> 1, LINEAR -> 0; COS: an argument error) */
    double alpha; /* RQ shape */
} gpar_factor_t;

typedef struct {
    int32_t nterms;
    int32_t nfactors;
    double coef[GPAR_MAX_TERMS];
    gpar_factor_t factor[GPAR_MAX_FACTORS];
} gpar_kspec_t;

/* flags */
#define GPAR_GRAM_LOWER 1  /* symmetric Gram (z1 == z2): write only tiles that touch the lower triangle */
#define GPAR_GEMM_C_LOWER 1 /* C is square-aligned: compute/store only elements with col <= row */
#define GPAR_GEMM_A_LOWER 2 /* treat op(A) as lower triangular (entries with k > m are zero) */
#define GPAR_GEMM_K_FROM_ROW 4 /* op(A)[m][k] is stored as zero for k < m (with C_LOWER also op(B)^T[n][k] for k < row): k starts at the tile's first row */
#define GPAR_GEMM_K_TO_COL 8 /* op(B)[k][n] is stored as zero for k > n (upper-triangular op(B)): k ends with the tile's last column */

/* ---- run-time specialisation (ABI v4) -----------------------------------------------------------
 * A layer's kernel STRUCTURE is fixed when the model is built (gpar/regression.py:92-180 decides the term list once per layer);
 * for large problems gpar_gram compiles a kernel for that structure with hiprtc on first use (values - coefficients, RQ shapes -
 * stay arguments: training never recompiles) and caches it per device; small problems and any compilation failure use the
 * ahead-of-time interpreter, which computes the same bits.  Environment: GPAR_GRAM_JIT_MIN_ENTRIES (default 2^26 entries per
 * launch - where a training run repays the 0.3-0.6 s a structure costs; 0 = always, negative = never).  Structures with more
 * than 16 feature dims have no generated Gram kernel (they are bound by their arithmetic either way).
 *   gpar_jit_compile_check  compiles (does not load) the kernel of `kind` for `ks` / `dz` and architecture `arch` (e.g. "gfx950"):
 *                           returns the code-object size, or -1 with the compiler's log in `log`; needs no GPU.  kind 0: Gram
 *                           (an argument error for a structure with more than 16 feature dims);
 *                           1 / 11: parameter-gradient pass with symmetric / rectangular weights (21 / 31: with frequency
 *                           derivatives of periodic features); 2 / 12: input-gradient pass, symmetric / rectangular weights.
 *                           (gpar_gram_grad* / gpar_gram_input_grad use generated kernels from GPAR_GRAD_JIT_MIN_ENTRIES weight
 *                           entries on, default 2^24; summation order differs from the interpreter's: agreement to rounding.)
 *   gpar_jit_stats          kernels compiled / compilations failed / structures cached so far in this process. */
int gpar_jit_compile_check(int kind, const gpar_kspec_t* ks, int dz, const char* arch, char* log, int log_len);
/* Compile (if not cached yet) and load the kernel of `kind` (codes as above) for this structure on the device that owns `stream`,
 * on the calling thread and outside the library's lock: call it for all layers of a model from several host threads at once and
 * no compilation happens inside an evaluation.  0: ready; 1: compilation failed (the interpreter will serve); < 0: argument error.
 * [a GPARRegressor's layer structures are known when the model is built: gpar/regression.py:92-180] */
int gpar_jit_prepare(int kind, const gpar_kspec_t* ks, int dz, void* stream);
/* Creates NOW what the library otherwise creates at first use on the device that owns `stream`: the look-ahead side stream paired
 * with `stream`, the event ring, the kernels' dynamic-LDS attributes (not the profile hook's events: profiling is not capturable).  After it no entry point called
 * on `stream` creates a HIP object, so a sequence of calls can be captured into a hipGraph (a run-time compiled
 * kernel structure must have been launched once before the capture).  Optional: everything still initialises lazily without it. */
int gpar_init(void* stream);
int gpar_jit_stats(int* compiled, int* failures, int* cached);
/* Kernels compiled at BUILD time (ABI v5).  gpar_jit_compile compiles the kernel of `kind` (codes as above) for a structure and
 * architecture and returns its code object (code_out / capacity; the return value is the size, -1 on a compilation failure with the
 * compiler's log in `log`) and the key under which an archive holds it (key_out); needs no GPU.  The library's build step collects
 * the common layer structures into gpar_aot_<arch>.bin next to the library; a structure found there is loaded instead of compiled -
 * and, costing nothing, is then used at every problem size (GPAR_AOT=0: ignore the archive).  gpar_aot_stats: entries the archive of
 * the current device's architecture holds (0 before the first lookup) / kernels loaded from it so far.
 * [the structures are those gpar/regression.py:92-180 builds for the reference's keyword combinations] */
long long gpar_jit_compile(int kind, const gpar_kspec_t* ks, int dz, const char* arch, void* code_out, long long capacity, char* key_out,
                           int key_len, char* log, int log_len);
int gpar_aot_stats(int* entries, int* loaded);
/* (ABI v6) What ties an archive to the library that may use it: a hash of the sources this library generates for a probe structure
 * covering every factor type and kernel kind, and of GPAR_ABI_VERSION.  The build step writes it into the archive's header; the
 * library ignores an archive whose ABI version or fingerprint is not its own (stale code objects could have another argument
 * layout or other arithmetic) and compiles at run time instead.  Needs no GPU.  [no reference counterpart: build hygiene] */
unsigned long long gpar_aot_fingerprint(void);

int gpar_abi_version(void);
size_t gpar_sizeof_fspec(void);
size_t gpar_sizeof_kspec(void);

/* z = features(x).  x: n x (>= max col+1) ldx; z: n x dz ldz.   [mlkernels stretch/periodic/select,
 * reached from gpar/regression.py:110,127-129,138,146,166,178] */
int gpar_featurize(const gpar_fspec_t* fs, const double* x, int n, int ldx, double* z, int ldz, void* stream);

/* K[a][b] = row_scale[a] * k(z1[a], z2[b]) (+ diag_add[a] + diag_const if a == b and z1 == z2).
 * row_scale may be NULL (= 1): the inducing-point path builds D^-1/2 K_xz directly (gpar/model.py:286-287), so that the
 * scaled cross-Gram never needs a pass of its own.
 * [mlkernels K(x, y); f(x, noise / w) adds diag(noise / w): gpar/model.py:287-289; lab's B.epsilon jitter] */
int gpar_gram(const gpar_kspec_t* ks, const double* z1, int n1, int ldz1, const double* z2, int n2, int ldz2,
              int dz, double* K, int ldk, int flags, const double* diag_add, double diag_const, const double* row_scale,
              void* stream);
/* `batch` symmetric Gram matrices of one size in one launch: K_b = k(z_b, z_b) + diag(diag_add) + diag_const I with input set b at
 * z + b * stride_z and its matrix at K + b * stride_k (elements); diag_add (n values or null) is shared by the batch.
 * [the prior covariances K(x_s, x_s) of all posterior samples of a layer, gpar/model.py:264,270 via regression.py:559-563] */
int gpar_gram_batch(const gpar_kspec_t* ks, const double* z, int n, int ldz, long long stride_z, int dz, double* K, int ldk,
                    long long stride_k, int flags, const double* diag_add, double diag_const, int batch, void* stream);

/* out[a] = k(z[a], z[a])   [kernel diagonal; VFE trace term, posterior marginal variances] */
int gpar_gram_diag(const gpar_kspec_t* ks, const double* z, int n, int ldz, int dz, double* out, void* stream);

/* Posterior decomposition by kernel component (ABI v18): the additive decomposition of a GP whose kernel is a sum (Rasmussen & Williams
 * 5.4.3; Duvenaud et al. 2013).  A layer kernel is k = sum_t c_t k_t over its nterms product terms; a GROUPING comp (HOST array of nterms
 * ints, each -1 .. ncomp - 1) sends term t to component comp[t], -1 to none, and k_g = sum_{comp[t] = g} c_t k_t.  1 <= ncomp <= GPAR_MAX_TERMS.
 *
 * gpar_gram_terms       K_g[a][b] = k_g(z1[a], z2[b]) for every g in ONE pass over the pairs: component g's n1 x n2 block (leading dimension
 *                       ldk >= n2) starts at K + g * stride_k (blocks must not overlap).  The arguments of gpar_gram otherwise, without
 *                       flags, diagonal add and row scale: always the full rectangle.  A component without a term is written as zeros.  A
 *                       term has the bits it has in gpar_gram's interpreter kernel: one component holding every term is that kernel's result
 *                       bit for bit, and the blocks of any grouping that uses every term once sum to it to rounding.
 * gpar_gram_terms_diag  out[g * ldo + a] = k_g(z[a], z[a]) (ldo >= n), the arithmetic of gpar_gram_diag.
 * gpar_posterior_terms  for ONE conditioned dense layer - training features z (n x dz), alpha = K^-1 y (n values) and the factor L (n x n,
 *                       ldl) of K = k(X, X) + D + eps I - and test features zs (ns x dz):
 *                           mean[g * ldm + a] = k_g(zs[a], X) alpha            var[g * ldv + a] = k_g(zs[a], zs[a]) - |L^-1 k_g(X, zs[a])|^2
 *                       (latent: the noise belongs to no component).  Over a grouping that uses every term once the means sum to the layer's
 *                       posterior mean; one component holding every term has the layer's posterior variance.  var == NULL skips the
 *                       variances (and L is not read).  The means are a fused Gram-times-vector pass - no ns x n matrix is written -, split
 *                       over n and summed in a fixed order; the variances compose gpar_gram_terms (the (ncomp c) x n stack of a chunk of c
 *                       test rows), ONE gpar_trsm_rlt over the stack, gpar_rownorm2 and gpar_gram_terms_diag.
 *                       ws: ws_doubles doubles, 16-byte aligned; gpar_workspace_doubles(GPAR_WS_POSTERIOR_TERMS, n, ns, ncomp) is the size
 *                       to bring.  Any size from max(ncomp ns, ncomp (n + 3)) doubles is taken: a smaller workspace means fewer splits
 *                       of the mean pass and smaller chunks of test rows (the means' last bits depend on the number of splits, so on
 *                       ws_doubles; for given arguments a call returns the same bits every time).
 * Argument errors - ncomp outside 1 .. GPAR_MAX_TERMS, a comp entry outside -1 .. ncomp - 1, a negative n / ns / n1 / n2, dz outside
 * 0 .. GPAR_MAX_DIMS or a factor reaching past it, leading dimensions or a workspace too small - are found before the first launch: a
 * negative status, no output touched.  No floating-point atomics anywhere.   [no reference counterpart: the reference's todo.tasks asks for
 * an "overview of trained hyperparameters"; this is what each trained part of the kernel explains] */
int gpar_gram_terms(const gpar_kspec_t* ks, const int* comp, int ncomp, const double* z1, int n1, int ldz1, const double* z2, int n2,
                    int ldz2, int dz, double* K, int ldk, long long stride_k, void* stream);
int gpar_gram_terms_diag(const gpar_kspec_t* ks, const int* comp, int ncomp, const double* z, int n, int ldz, int dz, double* out, int ldo,
                         void* stream);
int gpar_posterior_terms(const gpar_kspec_t* ks, const int* comp, int ncomp, const double* zs, int ns, int ldzs, const double* z, int n,
                         int ldz, int dz, const double* alpha, const double* L, int ldl, double* mean, int ldm, double* var, int ldv,
                         double* ws, long long ws_doubles, void* stream);

/* Posterior derivatives (ABI v21): the derivative of a Gaussian process is a Gaussian process (Rasmussen & Williams 9.4) - the slope of a
 * trend with its error bar, the sensitivity of an output to an input.  For ONE conditioned dense layer - training features z (n x dz),
 * alpha = K^-1 y and the factor L (n x n, ldl) of K = k(X, X) + D + eps I, as gpar_posterior_terms takes them - test features zs (ns x dz)
 * and ndir DIRECTION FIELDS J (device; direction c's ns x dz rows, leading dimension ldj >= dz, start at J + c * stride_j; fields must not
 * overlap): J[c][a][:] is the feature-space direction of test row a, i.e. d z / d x applied to a direction of the design space - the
 * CALLER chains 1 / scale and the derivative of the periodic embedding, by the convention of gpar_gram_input_grad.  With
 *     d_c,a[b] = J[c][a] . grad_z k(zs[a], z[b])                                      (never stored for the means)
 *     mean[c * ldm + a] = sum_b d_c,a[b] alpha[b]
 *     var[c * ldv + a]  = J[c][a]^T H(zs[a]) J[c][a] - |L^-1 d_c,a|^2,     H = grad_z grad_z'^T k at z = z' = zs[a]
 * (latent: the noise has no derivative).  var == NULL skips the variances (and L is not read).  The means are a fused pass over the pairs
 * - no ns x n matrix is written; per pair each term's factor values and gradient multipliers are evaluated once and every direction's dot
 * product is formed from them -, split over n and summed in a fixed order; the variances build the (ndir c) x n stack of d for a chunk of c
 * test rows with the same per-pair arithmetic, then ONE gpar_trsm_rlt over the stack, gpar_rownorm2 and the prior term J^T H J per row (per
 * factor on its dims: EQ, RQ I; Matern 3/2 3 I; Matern 5/2 5/3 I; cosine 4 pi^2 1 1^T; linear I, and between two linear factors of one
 * term the cross terms of the product rule - csrc/gram_deriv.h).  1 <= ndir <= GPAR_MAX_TERMS; at most 4 factors per product term (as
 * in gpar_gram_input_grad); the factor values use libm's exp (gpar_gram uses tables: agreement to rounding).
 * ws: ws_doubles doubles, 16-byte aligned; gpar_workspace_doubles(GPAR_WS_POSTERIOR_DERIV, n, ns, ndir) is the size to bring.  Any size
 * from max(ndir ns, ndir (n + 3)) doubles is taken (without variances: ndir ns): a smaller workspace means fewer splits of the mean pass
 * and smaller chunks of test rows (the means' last bits depend on the number of splits, so on ws_doubles; for given arguments a call
 * returns the same bits every time).  No floating-point atomics anywhere.
 * n == 0: means 0, variances the prior term.  ns == 0: nothing is done.  A zero direction gives mean 0 and variance 0.
 * Argument errors - a GPAR_K_MATERN12 factor (its process is not mean-square differentiable), ndir outside 1 .. GPAR_MAX_TERMS, a negative
 * n / ns, dz outside 0 .. GPAR_MAX_DIMS or a factor reaching past it, more than 4 factors in a term, leading dimensions, stride_j or the
 * workspace too small, a NULL array that would be read, (2 + ndir) dz too large for the tiles to fit 160 KiB of LDS ((2 + ndir) max(dz, 1)
 * 68 + 68 + 64 ndir doubles) - are found before the first launch: a negative status, no output touched.
 * [no reference counterpart; in Python: Obs.derivatives, GPAR.derivative, GPARRegressor.derivative] */
int gpar_posterior_deriv(const gpar_kspec_t* ks, const double* zs, int ns, int ldzs, const double* J, int ldj, long long stride_j, int ndir,
                         const double* z, int n, int ldz, int dz, const double* alpha, const double* L, int ldl, double* mean, int ldm,
                         double* var, int ldv, double* ws, long long ws_doubles, void* stream);

/* Generalised Lomb-Scargle periodogram (ABI v19; Zechmeister & Kuerster 2009: floating mean, weights) of p irregularly sampled series
 * that share their time stamps - where a spectral-mixture layer's periods should start (Wilson & Adams 2013 initialise from the
 * empirical spectrum).  t: n time stamps in any order, duplicates allowed.  y, omega: n x p row-major (ldy, ldo >= p); omega >= 0 are the
 * observation weights and omega == 0 marks an unobserved entry, whose y is never read.  freq: nf frequencies > 0 in cycles per unit of t.
 * power: p x nf row-major (ldp >= nf), power[j * ldp + k] in [0, 1].  For output j and frequency f, with w = omega / sum(omega) over the
 * column and phi_i = 2 pi f (t_i - t0):
 *     C = sum w cos phi   S = sum w sin phi   Y = sum w y   YY = sum w y^2 - Y^2   YC = sum w y cos phi - Y C   YS = sum w y sin phi - Y S
 *     CC = sum w cos^2 phi - C^2   SS = (1 - sum w cos^2 phi) - S^2   CS = sum w cos phi sin phi - C S   D = CC SS - CS^2
 *     power = (SS YC^2 + CC YS^2 - 2 CS YC YS) / (YY D)
 * The phase is formed as t_i - t0 first, then 2 f (t_i - t0), and evaluated with sincospi (its reduction to half periods is exact): pass
 * t0 = min t and time stamps like 1e6 lose nothing beyond the rounding of t_i - t0.  Every (row, frequency) pair has its own sincospi
 * - no recurrence along the grid -, shared by up to 4 outputs (more outputs: chunks of 4, each repeating it).  y enters centred by the
 * column's weighted mean (the power is invariant under affine maps of y).
 * Degenerate cases give power exactly 0, never NaN or Inf.  With tiny = 16 n 2^-52 (the sums are of magnitude 1 once the weights are
 * normalised, and carry about n 2^-53 of rounding): fewer than 3 observed rows; YY <= tiny^2 mean^2 (constant y); D <= tiny; a frequency
 * that is not a positive finite number.
 * The sum over the rows has a fixed order that depends on n alone (csrc/periodogram.h): two calls return the same bits, and the power
 * at a frequency has the same bits computed alone or inside any grid.  No atomics, no allocation, no synchronisation.
 * n == 0 or nf == 0: nothing is done, 0 is returned (power untouched).  Argument errors - n or nf negative, p < 1, ldy or ldo < p,
 * ldp < nf, t0 not finite, a NULL array with n, nf > 0 - are found before the launch: a negative status, power untouched.
 * [no reference counterpart; in Python: GPARRegressor.periodogram, spectral_period="auto"] */
int gpar_periodogram(const double* t, int n, double t0, const double* y, int ldy, const double* omega, int ldo, int p, const double* freq,
                     int nf, double* power, int ldp, void* stream);

/* Pathwise posterior sampling (ABI v20; Matheron's rule - Wilson et al., ICML 2020): a posterior draw is a prior draw through a random
 * Fourier basis plus one exact data-dependent update,
 *     f*_s(.) = f_s(.) + k(., X) v_s,    v_s = (K + D)^-1 (y - f_s(X) - eps_s),    f_s(z) = sum_j thc[j, s] cos(phi_j) + ths[j, s] sin(phi_j),
 * phi_j = 2 pi omega_j . (z - shift).  The two entries below are its two device passes; the solve for v_s uses the factor conditioning
 * holds.  Rows come in GROUPS - group_rows > 0: rows = count * group_rows, rows g group_rows .. (g + 1) group_rows - 1 use weight column g
 * (the stacked per-sample design matrices of ancestral sampling), out is a vector of `rows` values - or, group_rows == 0, as one set of
 * rows that meets every one of the `count` columns: out is rows x count row-major (ldo >= count).  No n* x n, rows x F or n* x n* matrix
 * is written.  No atomics: every sum has a fixed order that depends on the sizes alone (csrc/pathwise.h), two calls return the same bits,
 * and a row's value has the same bits whatever other rows, groups or columns the call holds (gpar_gram_apply_groups: among calls that
 * split the training rows alike - the number of splits follows n, the total number of rows and the workspace).
 *
 * gpar_rff_apply: z rows x dz features as gpar_featurize writes them (ldz >= dz), shift dz doubles, omega nfreq x dz in cycles per unit of
 * z (ldw >= dz), thc / ths nfreq x count (ldt >= count), all DEVICE arrays.  The phase is formed as z - shift first, the dot product by
 * fma in ascending dims, then sincospi(2 dot) - one per (row, frequency) pair, shared by the columns.  nfreq == 0: zeros.
 *
 * gpar_gram_apply_groups: out[r] = sum_a k(zs_r, z_a) vt[g(r) * ldv + a] - the vectors TRANSPOSED, count x n (ldv >= n), as the two
 * triangular solves leave them.  It is the mean pass of gpar_posterior_terms with one component holding every term: a pair has the bits
 * gpar_gram gives it.  ws: gpar_workspace_doubles(GPAR_WS_GRAM_APPLY, n, rows, output columns - 1 with groups, count without) doubles
 * are recommended; any ws_doubles >= rows * (output columns) is taken (fewer splits of the training rows).  n == 0: zeros.
 *
 * rows == 0 or count == 0: nothing is done.  Argument errors - a negative size, rows != count * group_rows, dz outside 0 .. GPAR_MAX_DIMS
 * or a factor reaching past it, leading dimensions or the workspace too small, a NULL array that would be read - are found before the
 * first launch: a negative status, out untouched.
 * [no reference counterpart; in Python: predict / sample (sampler="pathwise")] */
int gpar_rff_apply(const double* z, int rows, int ldz, int dz, const double* shift, const double* omega, int ldw, int nfreq, const double* thc,
                   const double* ths, int ldt, int count, int group_rows, double* out, int ldo, void* stream);
int gpar_gram_apply_groups(const gpar_kspec_t* ks, const double* zs, int rows, int ldzs, const double* z, int n, int ldz, int dz, const double* vt,
                           int ldv, int count, int group_rows, double* out, int ldo, double* ws, long long ws_doubles, void* stream);

/* Greedy (partially pivoted) Cholesky of k(Z, Z) (ABI v10): the selection of inducing points by largest conditional variance (Fine &
 * Scheinberg 2001; the initialisation Burt et al. 2019 recommend for sparse variational GPs).  z: n x dz features as gpar_featurize
 * writes them (ldz).  d starts as diag k(Z, Z) - no noise, no jitter, the arithmetic of gpar_gram_diag - and step j = 0, 1, ... does, in
 * this order:
 *   1. p = argmax_i d_i; ties go to the smallest i, a NaN ranks above every number;
 *   2. stop if d_p <= floor, or trace_j = sum_i d_i <= tol_trace * trace_0, or d_p is not finite (then info[0] = p + 1; 0 otherwise);
 *   3. c_i = k(z_i, z_p) - sum_{t<j} Lt[t][i] Lt[t][p]  (c <- fma(-Lt[t][i], Lt[t][p], c), t ascending, starting from the kernel entry);
 *   4. Lt[j][i] = c_i / sqrt(d_p), and Lt[j][p] = sqrt(d_p) itself;
 *   5. d_i <- fma(-Lt[j][i], Lt[j][i], d_i), and d_p <- 0 exactly (with floor >= 0 a picked row is never picked again).
 * Lt: max_rank x n row-major (ldl >= n), the factor TRANSPOSED: Lt[t][i] = L[i][t], so K ~ Lt^T Lt and K[:, piv] = Lt^T Lt[:, piv].
 * On return (all device memory, written by the kernels): rank[0] = steps taken; piv[0 .. rank) the pivots in order, -1 beyond; rows rank ..
 * of Lt zero; trace[j] = the residual trace before step j for j <= rank (trace[rank]: after the last step), 0 beyond: max_rank + 1 values.
 * ws: gpar_workspace_doubles(GPAR_WS_PIVOTED_CHOL, n, 0, 0) doubles; its first n hold the final residual diagonal d.
 * Limits: 1 <= max_rank <= GPAR_PIVCHOL_MAX_RANK (the pivot's row of the factor is staged in LDS), floor >= 0, tol_trace >= 0.
 * max_rank + 2 plain launches on `stream` and nothing else: no host synchronisation, no atomics, no waiting inside a launch; once a step
 * has stopped, the remaining launches only clear their row.  The result is a function of the inputs alone: two runs give the same bits.
 * Traffic: 8 n max_rank^2 / 2 bytes of Lt read; the kernel entries use libm's exp (gpar_gram uses tables: agreement to rounding).
 * [no reference counterpart: GPAR(x_ind=...) takes an array and nothing else, gpar/model.py:286-287] */
#define GPAR_PIVCHOL_MAX_RANK 4096
int gpar_pivoted_chol(const gpar_kspec_t* ks, const double* z, int n, int ldz, int dz, int max_rank, double tol_trace, double floor,
                      double* Lt, int ldl, int* piv, double* trace, int* rank, int* info, double* ws, void* stream);

/* zd[q] = d z[q] / d freq[q] (zero for non-periodic features): the feature derivative the period gradients need. */
int gpar_featurize_dfreq(const gpar_fspec_t* fs, const double* x, int n, int ldx, double* zd, int ldz, void* stream);

/* Gradient moment sums of  1/2 sum_ab W_ab dK_ab/dtheta  for every kernel parameter, one fused pass over the lower
 * triangle of the symmetric n x n matrix W (= alpha alpha^T - K^-1 for the log marginal likelihood).
 * out[GPAR_GRAD_NACC]: [0, MAX_TERMS) C_t; then [MAX_FACTORS) Al_f; then [MAX_DIMS) A_q; then [MAX_DIMS) P_q
 * (definitions: gpar_amd/csrc/gram.h).  workspace: nblocks * GPAR_GRAD_NACC doubles; nblocks = grid size (<= tiles).
 * zd may be NULL when the kernel has no periodic features.  At most 4 factors per product term.
 * [replaces torch autograd through exp / pw_dists2 / cholesky / solve_triangular inside
 *  varz.minimise_l_bfgs_b, gpar/regression.py:459] */
#define GPAR_GRAD_NACC (GPAR_MAX_TERMS + GPAR_MAX_FACTORS + 2 * GPAR_MAX_DIMS)
int gpar_grad_nacc(void);
int gpar_gram_grad(const gpar_kspec_t* ks, const double* z, const double* zd, int n, int ldz, int dz, const double* W,
                   int ldw, double* workspace, int nblocks, double* out, void* stream);
/* One dense layer's training objective AND the ingredients of its gradient in one call (ABI v5):
 *   out[0] = log N(y; 0, k(x, x) + diag(noise_diag) + jitter I),  out[1] = log det,  out[2 .. 2 + GPAR_GRAD_NACC) = the moment sums of
 *   1/2 sum_ab W_ab dK_ab/dtheta (as gpar_gram_grad),  half_diag[a] = 1/2 W_aa (the derivative with respect to noise_diag[a]),
 * with W = alpha alpha^T - (K + D)^-1.  The same launches the separate entry points make, in the same order (same bits):
 * gpar_featurize (+ gpar_featurize_dfreq when zd is non-null), gpar_gram, the augmented factorisation, gpar_chol_inverse,
 * gpar_trmv_upper of the inverse's workspace X = L^-T on the row L^-1 y (alpha; a gpar_trsm_rln until ABI v6), the rank-1 update of W, gpar_gram_grad.  Workspaces: z (and zd) n x dz (ldz); A (n + 1) x (n + 1);
 * X and W n x n; alpha n doubles; workspace nblocks * GPAR_GRAD_NACC doubles.  What it removes is the caller's side: a Python host
 * spends ~1 ms per evaluation on ~30 launches and three synchronisations around them, which IS the evaluation below n ~ 1000 - the
 * size the reference's own examples train at.
 * [objective + gradient of one layer inside varz.minimise_l_bfgs_b, gpar/regression.py:434-459] */
int gpar_logpdf_dense_grad(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                           const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* X, int ldxw,
                           double* W, int ldw, double* alpha, double* workspace, int nblocks, double* out, double* half_diag, int* info,
                           int potrf_flags, void* stream);
/* The same evaluation for a factor that ALREADY EXISTS (ABI v7) - the second half of gpar_logpdf_dense_grad: the value from the corner
 * of A and `logdet`, K^-1 from L, alpha, W, the weighted-sum pass, 1/2 diag W (gpar_featurize_dfreq first when zd is non-null).  For
 * callers that factor several layers' matrices TOGETHER: gpar_logpdf_dense_build per layer into the slots of one buffer, ONE
 * gpar_potrf_batch over the slots, then this call per layer on a stream of its own (the lock-step training rendezvous of
 * gpar_amd/fastfit.py: the p independent layer optimisations of fit(fix=True), gpar/regression.py:418-446, evaluate in rounds).
 * `logdet` / `info`: the layer's words of the batch (device); out[1] <- logdet[0], info_out[0] <- info[0] (either of the last two may
 * be NULL), so that one device-to-host copy of `out` .. `info_out` carries everything the host reads.  A failed factorisation
 * (info != 0) leaves garbage in out / half_diag, as gpar_logpdf_dense_grad does.
 * [objective + gradient of one layer inside varz.minimise_l_bfgs_b, gpar/regression.py:434-459] */
int gpar_logpdf_dense_grad_finish(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, double* z, double* zd,
                                  int ldz, double* A, int lda, const double* logdet, const int* info, double* X, int ldxw, double* W, int ldw,
                                  double* alpha, double* workspace, int nblocks, double* out, double* half_diag, int* info_out, void* stream);

/* Leave-one-out cross-validation of one dense layer (ABI v8).  With S = k(x, x) + diag(noise_diag) + jitter I, alpha = S^-1 y and
 * d = diag(S^-1):  loo_mean[i] = y_i - alpha_i / d_i and loo_var[i] = 1 / d_i are the predictive mean and variance of observation i given
 * all the others, and  out[0] = sum_i log N(y_i; loo_mean[i], loo_var[i]) = sum_i [1/2 log d_i - alpha_i^2 / (2 d_i)] - n/2 log 2 pi.
 * gpar_loo_dense_grad mirrors gpar_logpdf_dense_grad argument for argument: out[1] = log det S, out[2 .. 2 + GPAR_GRAD_NACC) = the moment
 * sums of 1/2 sum_ab W_ab dS_ab/dtheta (as gpar_gram_grad) and half_diag[a] = 1/2 W_aa (the derivative with respect to noise_diag[a]) for
 *   W = alpha u^T + u alpha^T - 2 S^-1 C S^-1,   b = alpha / d,   C = diag(1/2 (1 / d + b^2)),   u = S^-1 b
 * (Sundararajan & Keerthi 2001, eq. 10-12, collected into one weight matrix).  The launches of gpar_logpdf_dense_grad up to alpha (prep,
 * Gram, augmented factorisation, gpar_chol_inverse; alpha by gpar_trmv_upper's sum, in one launch with the per-row quantities), then
 * {u from the lower triangle of S^-1, S^-1 diag(sqrt c) as a full matrix into X}, W <- -2 (.)(.)^T by gpar_gemm (GPAR_GEMM_C_LOWER), the
 * rank-2 term, gpar_gram_grad's pass, one epilogue (moment partials, 1/2 diag W, the value terms summed in a fixed order).  Workspaces as
 * gpar_logpdf_dense_grad, plus vec: gpar_workspace_doubles(GPAR_WS_LOO, n, 1, 0) doubles; loo_mean / loo_var: n doubles each (device).
 * gpar_loo_dense_grad_finish is the second half for a factor that already exists, as gpar_logpdf_dense_grad_finish (same bits as the one-
 * call form for the same factor); y is read again (the factor's row n holds L^-1 y).  A failed factorisation (info != 0) leaves garbage.
 * gpar_loo_dense: value (out[0]), log det (out[1]), means and variances only - no S^-1 is formed: alpha and d come from one pass over
 * X = L^-T (d_i = |row i of X|^2), half the inverse's flops.  X, T: n x n workspaces; vec: gpar_workspace_doubles(GPAR_WS_LOO, n, 0, 0).
 * [no reference counterpart: the reference scores and trains by f.measure.logpdf alone, gpar/model.py:226, gpar/regression.py:434-459] */
int gpar_loo_dense_grad(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                        const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* X, int ldxw,
                        double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                        double* loo_mean, double* loo_var, int* info, int potrf_flags, void* stream);
int gpar_loo_dense_grad_finish(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                               double* z, double* zd, int ldz, double* A, int lda, const double* logdet, const int* info, double* X, int ldxw,
                               double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                               double* loo_mean, double* loo_var, int* info_out, void* stream);
int gpar_loo_dense(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                   const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* X, int ldxw, double* T, int ldt,
                   double* vec, double* out, double* loo_mean, double* loo_var, int* info, int potrf_flags, void* stream);

/* Blocked (leave-fold-out) cross-validation of one dense layer (ABI v9): leave-one-out with whole contiguous blocks of rows held out and
 * scored by their JOINT predictive density - the estimator for ordered data, where a single left-out point is predicted almost for free
 * from its neighbours.  fold_start: a DEVICE array of nfolds + 1 ascending row offsets, fold_start[0] = 0, fold_start[nfolds] = n; fold f
 * holds the rows [fold_start[f], fold_start[f + 1]) in the order handed in.  max_fold: the host's bound on the largest fold,
 * 1 <= max_fold <= GPAR_CV_MAX_FOLD (otherwise an argument error: nothing is launched).  With S = k(x, x) + diag(noise_diag) + jitter I,
 * P = S^-1, alpha = P y and per fold D_F = P[F, F], b_F = D_F^-1 alpha_F:  y_F given all other rows ~ N(y_F - b_F, D_F^-1), so
 *   cv_mean[F] = y_F - b_F,  cv_var[F] = diag(D_F^-1) (the marginal variances),
 *   out[0] = sum_F [1/2 log|D_F| - 1/2 alpha_F^T b_F] - n/2 log 2 pi   (the joint fold densities).
 * Folds of size 1 give gpar_loo_dense*; one fold of all rows gives the log marginal likelihood.
 * gpar_cv_dense_grad mirrors gpar_loo_dense_grad argument for argument (fold_start, nfolds, max_fold before info): out[1] = log det S,
 * out[2 .. 2 + GPAR_GRAD_NACC) and half_diag as there, for the weights
 *   W = alpha u^T + u alpha^T - 2 P C P,   C = blockdiag(1/2 (D_F^-1 + b_F b_F^T)),   u = P b.
 * Its launches: those of gpar_loo_dense_grad with the fold kernel (one workgroup per fold, in LDS: alpha_F, D_F = G G^T, D_F^-1, b_F, the
 * moments, the fold's value term, C_F = R_F R_F^T) in the place of the row kernel and {u, P blockdiag(R_F) as a full matrix into X} in the
 * place of {u, P diag(sqrt c)}.  vec: gpar_workspace_doubles(GPAR_WS_CV, n, 1, max_fold) doubles.  gpar_cv_dense_grad_finish is the second
 * half for a factor that already exists (same bits); info and info_out are both required (the fold kernel reports into info_out).
 * gpar_cv_dense: value, log det, means and variances; it forms P whole (X, T: n x n workspaces, T receives P) and shares the fold kernel;
 * vec: gpar_workspace_doubles(GPAR_WS_CV, n, 0, max_fold).
 * info, besides the factorisation's own codes: the 1-based row of a non-positive pivot in a fold's D_F or C_F; n + 1 + f for a fold f
 * whose extent in fold_start is not positive, exceeds max_fold or leaves [0, n) (that fold is then skipped).  Results are garbage then.
 * Limits: dense layers; folds of at most GPAR_CV_MAX_FOLD rows (larger folds: compose gpar_chol_inverse with host-side block algebra).
 * [no reference counterpart] */
#define GPAR_CV_MAX_FOLD 64
int gpar_cv_dense_grad(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                       const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* X, int ldxw,
                       double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                       double* cv_mean, double* cv_var, const int* fold_start, int nfolds, int max_fold, int* info, int potrf_flags,
                       void* stream);
int gpar_cv_dense_grad_finish(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                              double* z, double* zd, int ldz, double* A, int lda, const double* logdet, const int* info, double* X, int ldxw,
                              double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                              double* cv_mean, double* cv_var, const int* fold_start, int nfolds, int max_fold, int* info_out, void* stream);
int gpar_cv_dense(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                  const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* X, int ldxw, double* T, int ldt,
                  double* vec, double* out, double* cv_mean, double* cv_var, const int* fold_start, int nfolds, int max_fold, int* info,
                  int potrf_flags, void* stream);

/* Purged (hv-block) blocked cross-validation of one dense layer (ABI v14; Burman, Chow & Nolan 1994, Racine 2000): gpar_cv_dense* with,
 * per fold, further rows on either side of it taken out of the conditioning set without being scored - on ordered data the first and last
 * rows of a held-out block otherwise keep a training row one step away.  The entries mirror gpar_cv_dense* argument for argument, with
 * (fold_start, hold_lo, hold_hi, nfolds, max_hold) in the place of (fold_start, nfolds, max_fold).  fold_start: as there - the SCORED rows
 * F_f = [fold_start[f], fold_start[f + 1]).  hold_lo, hold_hi: DEVICE arrays of nfolds ints, the block H_f = [hold_lo[f], hold_hi[f])
 * that fold f is NOT predicted from: 0 <= hold_lo[f] <= fold_start[f], fold_start[f + 1] <= hold_hi[f] <= n, neither decreasing in f.
 * max_hold: the host's bound on the largest block, 1 <= max_hold <= GPAR_CV_MAX_FOLD (otherwise an argument error: nothing is launched).
 * With P = S^-1, alpha = P y, G = H \ F and the block P_HH:
 *   Dt = P_FF - P_FG P_GG^-1 P_GF,  at = alpha_F - P_FG P_GG^-1 alpha_G,  bt = Dt^-1 at:   y_F given the rows outside H ~ N(y_F - bt, Dt^-1),
 *   cv_mean[F] = y_F - bt,  cv_var[F] = diag(Dt^-1),  out[0] = sum_F [1/2 log|Dt| - 1/2 at^T bt] - n/2 log 2 pi.
 * hold = the folds' own extents gives gpar_cv_dense* (other bits: another chain); one fold gives the log marginal likelihood; blocks that
 * reach both ends predict every fold from the prior.  The gradient forms return out[1], out[2 ...] and half_diag as gpar_cv_dense_grad for
 *   W = alpha u^T + u alpha^T - 2 P C P,  u = P b,  b = sum_f E_H b_H,  C = sum_f E_H C_H E_H^T,
 *   Sigma = P_HH^-1,  e = Sigma alpha_H,  b_H = Sigma[:, F] at,  C_H = Sigma Sm Sigma + 1/2 (e b_H^T + b_H e^T),  Sm = 1/2 (Dt - at at^T) on F.
 * The blocks of neighbouring folds overlap and C_H is indefinite, so C is a symmetric band matrix of half-bandwidth < max_hold and no
 * R R^T.  Launches behind K^-1: the purged fold kernel (one workgroup per fold, in LDS: alpha_H, one factorisation of P_HH ordered
 * (G, F) - P_GG's pivots, then Dt's -, its inverse, the moments, the value term, the factors of C_H); the assembly of b and of the band
 * image of C (one thread per entry, folds in ascending order, no atomics: a call gives the same bits every time); {u, P as a full
 * matrix}; T = C P into X (band times dense: 2 max_hold n^2 multiply-adds on the vector ALU); W <- -2 P T by gpar_gemm
 * (GPAR_GEMM_C_LOWER: a full product where gpar_cv_dense_grad has a SYRK); then the rank-2 term, the weighted-sum pass and the epilogue
 * of gpar_cv_dense_grad.  vec: gpar_workspace_doubles(GPAR_WS_CV_GAP, n, 1, max_hold) doubles (it holds P as an n x n matrix: hand it
 * over 16-byte aligned); the value-only form: gpar_workspace_doubles(GPAR_WS_CV_GAP, n, 0, max_hold).  gpar_cv_gap_dense_grad_finish is
 * the second half for a factor that already exists (same bits); info and info_out are both required.
 * info, besides the factorisation's own codes: the 1-based row of a non-positive pivot in a fold's P_GG or Dt; n + 1 + f for a fold f
 * whose extents are malformed - fold_start as gpar_cv_dense judges it, a block that does not contain its fold, leaves [0, n), exceeds
 * max_hold, or whose hold_lo / hold_hi decrease from fold f - 1 (that fold is skipped, and every kernel of the weight stage behind the
 * fold kernel returns at once).  Results are garbage then.  Limits: dense layers; blocks of at most GPAR_CV_MAX_FOLD rows.
 * [no reference counterpart] */
int gpar_cv_gap_dense_grad(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                           const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* X, int ldxw,
                           double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                           double* cv_mean, double* cv_var, const int* fold_start, const int* hold_lo, const int* hold_hi, int nfolds,
                           int max_hold, int* info, int potrf_flags, void* stream);
int gpar_cv_gap_dense_grad_finish(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                                  double* z, double* zd, int ldz, double* A, int lda, const double* logdet, const int* info, double* X, int ldxw,
                                  double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                                  double* cv_mean, double* cv_var, const int* fold_start, const int* hold_lo, const int* hold_hi, int nfolds,
                                  int max_hold, int* info_out, void* stream);
int gpar_cv_gap_dense(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                      const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* X, int ldxw, double* T, int ldt,
                      double* vec, double* out, double* cv_mean, double* cv_var, const int* fold_start, const int* hold_lo, const int* hold_hi,
                      int nfolds, int max_hold, int* info, int potrf_flags, void* stream);

/* Rolling-origin forecast scoring of one dense layer (ABI v12): every scored row predicted from the rows BEFORE its origin, the rows in the
 * order handed in (the time order).  origin: a DEVICE array of n ints; origin[r] = -1: row r is not scored; otherwise 0 <= origin[r] <= r
 * and row r is predicted from rows 0 ... origin[r] - 1 (origin[r] = 0: from the prior).  With S = k(x, x) + diag(noise_diag) + jitter I
 * = L L^T and a = L^-1 y the factor of a leading block of S is the leading block of L, so
 *   e_r = y_r - ahead_mean[r] = sum_{c = origin[r] .. r} L_rc a_c,   ahead_var[r] = v_r = sum_{c = origin[r] .. r} L_rc^2
 *   out[0] = sum_scored -1/2 [log 2 pi + log v_r + e_r^2 / v_r]   (the predictive of the noisy observation, as gpar_loo_dense reports it);
 * unscored rows carry NaN in ahead_mean and ahead_var.  origin[r] = r for every row gives the log marginal likelihood.
 * gpar_ahead_dense_grad mirrors gpar_loo_dense_grad argument for argument (origin before info): out[1] = log det S, out[2 .. 2 +
 * GPAR_GRAD_NACC) and half_diag as there, for the weights
 *   W = X (P + P^T) X^T,  X = L^-T,  P = Phi(L^T B - abar a^T),  B_rc = -q_r a_c - 2 s_r L_rc (origin[r] <= c <= r),
 *   abar_c = -sum_{r >= c, origin[r] <= c} q_r L_rc,  q_r = e_r / v_r,  s_r = 1/2 (1 / v_r - q_r^2)
 * (Phi: the lower triangle with its diagonal halved - the reverse mode of the Cholesky factorisation).  Its launches behind the factor: X
 * (the first half of gpar_chol_inverse), the origins' check, the row kernel, abar, the banded product P + P^T as a full matrix into W, two
 * gpar_gemm products (X (.) into vec, then W on its lower triangle), the weighted-sum pass, the epilogue.  The banded product costs
 * sum_j sum_{i >= j} #{r >= i: origin[r] <= j} multiply-adds on the vector units: O(n^2 H) for a horizon H, n^3 / 6 when every row is
 * predicted from the prior.  alpha is not written.  vec: gpar_workspace_doubles(GPAR_WS_AHEAD, n, 1, 0) doubles (it holds the n x n first
 * product: hand it over 16-byte aligned for the vectorised products).  gpar_ahead_dense_grad_finish is the second half for a factor that
 * already exists (same bits); info and info_out are both required.  gpar_ahead_dense: value, log det, means and variances from the factor
 * and its augmented row alone - no X, no S^-1; vec: gpar_workspace_doubles(GPAR_WS_AHEAD, n, 0, 0).
 * info, besides the factorisation's own codes: n + 1 + r for the first row r whose origin lies outside -1 ... r; the 1-based row of a
 * non-positive v_r.  Whenever the info word is set - by the factorisation too - out[0], out[2 ...], half_diag, ahead_mean and ahead_var
 * keep what they held (out[1] is the factorisation's).  No atomics in any sum: a call gives the same bits every time.
 * [no reference counterpart] */
int gpar_ahead_dense_grad(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                          const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* X, int ldxw,
                          double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                          double* ahead_mean, double* ahead_var, const int* origin, int* info, int potrf_flags, void* stream);
int gpar_ahead_dense_grad_finish(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                                 double* z, double* zd, int ldz, double* A, int lda, const double* logdet, const int* info, double* X, int ldxw,
                                 double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                                 double* ahead_mean, double* ahead_var, const int* origin, int* info_out, void* stream);
int gpar_ahead_dense(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                     const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* vec, double* out,
                     double* ahead_mean, double* ahead_var, const int* origin, int* info, int potrf_flags, void* stream);

/* Scoring rules for the leave-one-out and rolling-origin entries (ABI v13).  The entries above score every held-out entry by its Gaussian
 * log density; the *_score entries take the rule as `score`, placed before the info word, and are otherwise their namesakes argument for
 * argument - same workspaces, same launches, same info codes, and with GPAR_SCORE_LOG the same bits (the entries above forward to them).
 * out[0] is always a value to MAXIMISE, the sum over the scored entries of, with e = y - mean, v = var, sd = sqrt v, z = e / sd and
 * Phi / phi the standard normal cdf / pdf:
 *   GPAR_SCORE_LOG    -1/2 [log 2 pi + log v + e^2 / v]                  q = e / v             s = 1/2 (1 / v - q^2)
 *   GPAR_SCORE_CRPS   -sd [z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt pi]    q = 2 Phi(z) - 1      s = (2 phi(z) - 1 / sqrt pi) / (2 sd)
 *   GPAR_SCORE_SE     -e^2                                               q = 2 e               s = 0
 * (minus the continuous ranked probability score of the Gaussian predictive, Gneiting & Raftery 2007; minus the squared error: PRESS for
 * leave-one-out, the rolling-origin MSE times the number of scored rows for the forecasts).  q = -dterm/de and s = -dterm/dv are what the
 * gradient chains run on: the rolling-origin weights as documented above with these q_r, s_r; the leave-one-out weights
 *   W = alpha u^T + u alpha^T - 2 S^-1 C S^-1,   u = S^-1 b,   b_i = q_i v_i,   C = diag(q_i e_i v_i + s_i v_i^2)
 * (the log score: b = e, c = 1/2 (v + e^2)).  The means and variances do not depend on the rule.  A rule other than the three is an
 * argument error (-1014) before anything is launched: every buffer keeps what it held.
 * [no reference counterpart] */
#define GPAR_SCORE_LOG 0
#define GPAR_SCORE_CRPS 1
#define GPAR_SCORE_SE 2
int gpar_loo_dense_grad_score(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                              const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* X, int ldxw,
                              double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                              double* loo_mean, double* loo_var, int score, int* info, int potrf_flags, void* stream);
int gpar_loo_dense_grad_finish_score(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                                     double* z, double* zd, int ldz, double* A, int lda, const double* logdet, const int* info, double* X,
                                     int ldxw, double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out,
                                     double* half_diag, double* loo_mean, double* loo_var, int score, int* info_out, void* stream);
int gpar_loo_dense_score(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                         const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* X, int ldxw, double* T, int ldt,
                         double* vec, double* out, double* loo_mean, double* loo_var, int score, int* info, int potrf_flags, void* stream);
int gpar_ahead_dense_grad_score(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                                const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* X, int ldxw,
                                double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                                double* ahead_mean, double* ahead_var, const int* origin, int score, int* info, int potrf_flags, void* stream);
int gpar_ahead_dense_grad_finish_score(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                                       double* z, double* zd, int ldz, double* A, int lda, const double* logdet, const int* info, double* X,
                                       int ldxw, double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out,
                                       double* half_diag, double* ahead_mean, double* ahead_var, const int* origin, int score, int* info_out,
                                       void* stream);
int gpar_ahead_dense_score(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                           const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* vec, double* out,
                           double* ahead_mean, double* ahead_var, const int* origin, int score, int* info, int potrf_flags, void* stream);

/* Rolling-origin forecast scoring at several horizons in one pass (ABI v15).  K = nh origin arrays over ONE factor: origins is a DEVICE
 * array of nh x n ints, row k holding horizon k's origins as gpar_ahead_dense takes them (origins[k n + r] = -1: (k, r) is not scored,
 * otherwise 0 ... r); weights is a HOST array of nh doubles, all positive and finite, handed to the kernels by value.  With e_kr, v_kr the
 * sums of gpar_ahead_dense from origins[k n + r], term / q / s the scoring rule's (above):
 *   values[k] = sum_r term(e_kr, v_kr)  (unweighted, DEVICE array of nh doubles),   out[0] = sum_k weights[k] values[k],
 *   ahead_mean[k n + r] = y_r - e_kr,  ahead_var[k n + r] = v_kr  (nh x n each; NaN on unscored (k, r)),
 *   Q_r(c) = sum_k weights[k] q_kr [origins[k n + r] <= c],   S_r(c) = sum_k weights[k] s_kr [origins[k n + r] <= c],
 *   B_rc = -Q_r(c) a_c - 2 S_r(c) L_rc  (c <= r),   abar_c = -sum_{r >= c} Q_r(c) L_rc,   P and W as for gpar_ahead_dense_grad.
 * The three entries are gpar_ahead_dense_grad_score, gpar_ahead_dense_grad_finish_score and gpar_ahead_dense_score argument for argument
 * with `origins, nh, weights, values` in the place of `origin`: out[1], out[2 ...] and half_diag as there, the same launches (the check,
 * row, abar and band kernels in their multi-horizon forms; the factor, X, the two products and the weighted-sum pass are shared by the
 * horizons).  A row's nh sums come from one walk along its row of L; the band kernel skips chunks by the smallest origin over all
 * horizons, so its cost follows the longest horizon.  vec: gpar_workspace_doubles(GPAR_WS_AHEAD_MULTI, n, 1, nh) doubles (16-byte
 * aligned); the value-only form: gpar_workspace_doubles(GPAR_WS_AHEAD_MULTI, n, 0, nh).
 * nh outside 1 ... GPAR_AHEAD_MAX_HORIZONS (-1015) and a weight that is not positive and finite (-1016) are argument errors before anything
 * is launched: every buffer keeps what it held.  info: n + 1 + r for the smallest row r with an origin outside -1 ... r in any horizon;
 * the 1-based row of a non-positive v_kr.  Whenever the info word is set, out[0], out[2 ...], values, half_diag, ahead_mean and ahead_var
 * keep what they held.  One horizon with weight 1 gives the bits of gpar_ahead_dense_grad_score.  No atomics in any sum.
 * [no reference counterpart] */
#define GPAR_AHEAD_MAX_HORIZONS 8
int gpar_ahead_multi_dense_grad(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                                const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* X, int ldxw,
                                double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out, double* half_diag,
                                double* ahead_mean, double* ahead_var, const int* origins, int nh, const double* weights, double* values, int score,
                                int* info, int potrf_flags, void* stream);
int gpar_ahead_multi_dense_grad_finish(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                                       double* z, double* zd, int ldz, double* A, int lda, const double* logdet, const int* info, double* X,
                                       int ldxw, double* W, int ldw, double* alpha, double* vec, double* workspace, int nblocks, double* out,
                                       double* half_diag, double* ahead_mean, double* ahead_var, const int* origins, int nh, const double* weights,
                                       double* values, int score, int* info_out, void* stream);
int gpar_ahead_multi_dense(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                           const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* vec, double* out,
                           double* ahead_mean, double* ahead_var, const int* origins, int nh, const double* weights, double* values, int score,
                           int* info, int potrf_flags, void* stream);

/* Sliding-window forecast scoring of one dense layer (ABI v16): gpar_ahead_dense with every scored row predicted from a WINDOW of the
 * rows before its origin instead of all of them - the score of the model gpar_chol_drop_leading / gpar_chol_append keep alive.  lo and
 * origin are DEVICE arrays of n ints: origin[r] = -1 leaves row r unscored (NaN in ahead_mean and ahead_var); otherwise row r is predicted
 * from rows lo[r] ... origin[r] - 1 (lo[r] = origin[r]: from the prior), with 0 <= lo[r] <= origin[r] <= r, origin[r] - lo[r] <=
 * GPAR_AHEAD_WINDOW_MAX, and neither array decreasing over the scored rows.  With S = k(x, x) + diag(noise_diag) + jitter I, J the run
 * followed by r itself and S_JJ = G G^T (r last):
 *   z = G^-1 y_J,   e_r = y_r - ahead_mean[r] = G_rr z_r,   ahead_var[r] = v_r = G_rr^2,   out[0] = sum_scored term(e_r, v_r),
 *   c = G_rr G^-T e_r = [-S_SS^-1 s_Sr; 1],   p = [S_SS^-1 y_S; 0],   W = sum_r scatter_J(-2 s_r c c^T + q_r (p c^T + c p^T)),
 * term / q / s the scoring rule's (above), d out[0] / d theta = 1/2 sum_ab W_ab dS_ab/dtheta and half_diag = 1/2 diag W the noise gradient.
 * S is built as for gpar_logpdf_dense_grad (z, zd, A: the workspaces there; A holds S on its lower triangle afterwards and y in row n)
 * and is NOT factored: out[1] = 0, there is no X, no alpha and no finish form.  Launches: features + observations, Gram, a check of lo and
 * origin, one workgroup per row (the block S_JJ factored in LDS; c and p of the row stored compactly), for the gradient a gather of W on
 * its lower triangle (every entry the sum over the rows whose blocks hold it, in increasing r), the weighted-sum pass of
 * gpar_logpdf_dense_grad and its epilogue (out[2 .. 2 + gpar_grad_nacc()), half_diag, the sum of the terms in a fixed order).  No atomics
 * in any sum: a call returns the same bits every time.  vec: gpar_workspace_doubles(GPAR_WS_AHEAD_WINDOW, n, 1, 0) doubles;
 * gpar_ahead_window_dense (value, means and variances alone): gpar_workspace_doubles(GPAR_WS_AHEAD_WINDOW, n, 0, 0).
 * info: n + 1 + r for the first row r whose lo / origin break the rules above; the 1-based row of S at which a block's factorisation met a
 * non-positive pivot.  Whenever the info word is set, out[0], out[2 ...] and half_diag keep what they held; so do ahead_mean and ahead_var
 * when the check has set it (after a non-positive pivot the rows whose own blocks were sound have written theirs).  An unknown score
 * (-1014) is an argument error before anything is launched.  Limits: dense layers; windows of at most
 * GPAR_AHEAD_WINDOW_MAX rows (longer windows: compose gpar_gram with host-side block algebra).  [no reference counterpart] */
#define GPAR_AHEAD_WINDOW_MAX 64
int gpar_ahead_window_dense_grad(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                                 const double* noise_diag, double jitter, double* z, double* zd, int ldz, double* A, int lda, double* W, int ldw,
                                 double* vec, double* workspace, int nblocks, double* out, double* half_diag, double* ahead_mean, double* ahead_var,
                                 const int* lo, const int* origin, int score, int* info, void* stream);
int gpar_ahead_window_dense(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                            const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* vec, double* out,
                            double* ahead_mean, double* ahead_var, const int* lo, const int* origin, int score, int* info, void* stream);

/* The same moment sums of  sum W dK/dtheta  for the other weight shapes the inducing-point (VFE) bound needs
 * [gradient of the PseudoObs elbo, gpar/model.py:226,286-287 under varz's optimiser]:
 *   GPAR_GRAD_SYM   z2 == z1: W symmetric n1 x n1, lower triangle read, sum over all pairs (what gpar_gram_grad does);
 *   GPAR_GRAD_RECT  W a full n1 x n2 matrix of cross-Gram weights K(x1_a, x2_j);
 *   GPAR_GRAD_DIAG  z2 == z1: W a vector of n1 weights of the prior variances k(x_a, x_a).
 * Sums are FULL sums (no factor 1/2).  zd1 / zd2 may both be NULL.  nblocks <= number of 64 x 64 tiles of the mode. */
#define GPAR_GRAD_SYM 0
#define GPAR_GRAD_RECT 1
#define GPAR_GRAD_DIAG 2
int gpar_gram_grad_cross(const gpar_kspec_t* ks, const double* z1, const double* zd1, int n1, int ldz1, const double* z2,
                         const double* zd2, int n2, int ldz2, int dz, const double* W, int ldw, int mode, double* workspace,
                         int nblocks, double* out, void* stream);

/* The same moment sums with the ROW index left unreduced (an addition within ABI v21: no existing entry changes):
 *     out[a * ldo + s] = sum_{b < n2} v[b] * (moment s of the pair (z1_a, z2_b)),   a < n1, s < GPAR_GRAD_NACC,
 * slots, order and conventions those of gpar_gram_grad_cross(GPAR_GRAD_RECT) - C_t, Al_f, A_q, P_q; full sums; d/dscale = -2 A / scale;
 * the Matern-1/2 multiplier 0 at r = 0; the cosine convention of ABI v17 - so that row a is what that call returns for n1 = 1,
 * z1 = z1[a], W = v^T, and the host's raw-slot -> variable chain rule applies to a row unchanged.  With v = alpha = K^-1 y these are the
 * sums behind d mean(x*_a) / d theta of a conditioned layer.  One fused pass (csrc/gram_grad_rows.h): a workgroup owns 64 rows of z1,
 * the rows of z2 are staged through LDS and split over the grid, the splits' partial sums are added in a fixed order.  Only the slots
 * the structure uses are accumulated; every other slot is written as 0.  The per-pair arithmetic is the interpreted gradient pass's.
 * zd1 / zd2: both NULL (no P_q: those slots are 0) or both given, the rule of gpar_gram_grad_cross.  ldo >= GPAR_GRAD_NACC.
 * ws: ws_doubles doubles; gpar_workspace_doubles(GPAR_WS_GRAM_GRAD_ROWS, n2, n1, 0) is the size to bring.  Any size from
 * n1 * GPAR_GRAD_NACC doubles is taken, at the cost of fewer splits (a split keeps n1 * GPAR_GRAD_NACC doubles; the last bits depend on
 * the number of splits, so on ws_doubles).  No floating-point atomics: for given arguments a call returns the same bits every time, and a
 * row's bits do not depend on the other rows of the call, among calls that split n2 alike.
 * n1 == 0: nothing is done.  n2 == 0: zeros.
 * Argument errors - a negative n1 / n2, dz outside 0 .. GPAR_MAX_DIMS or a factor reaching past it, more than 4 factors in a term, ldo,
 * ldz1, ldz2 or the workspace too small, a NULL array that would be read, one of zd1 / zd2 NULL and the other not, tiles and accumulators
 * that do not fit 160 KiB of LDS ((2, with zd 4) max(dz, 1) 68 + 68 + 64 used slots doubles + GPAR_GRAD_NACC ints: without zd dz <= 95
 * always fits, with zd dz <= 47) - are found before the first launch: a negative status, `out` untouched.
 * [no reference counterpart; in Python: Obs.mean_sensitivity, GPAR.hyper_jacobian, GPARRegressor.predict_moments_hyper] */
int gpar_gram_grad_rows(const gpar_kspec_t* ks, const double* z1, const double* zd1, int n1, int ldz1, const double* z2, const double* zd2,
                        int n2, int ldz2, int dz, const double* v, double* out, int ldo, double* ws, long long ws_doubles, void* stream);

/* Gradient with respect to the inputs, in feature space:  out[a][q] = sum_b W(a, b) d k(z1_a, z2_b) / d z1_a[q]  for the
 * pair weights W (GPAR_GRAD_RECT: n1 x n2;  GPAR_GRAD_SYM: z2 == z1, W symmetric, lower triangle read).  out: n1 x dz (ldo);
 * workspace: gpar_workspace_doubles(GPAR_WS_INPUT_GRAD, n1, dz, nsplit) doubles; nsplit >= 1 column splits (summed in order).
 * The caller chains d z / d x (1 / scale, and the derivative of the periodic embedding) back to the design-matrix columns.
 * [torch autograd through mlkernels' pairwise distances when a layer's inputs are posterior means of earlier layers -
 *  fit(fix=False) with replace / impute / inducing points: gpar/regression.py:447-456 through gpar/model.py:291-322 - and
 *  the derivative with respect to inducing-point locations (the reference's todo.tasks:5)] */
int gpar_gram_input_grad(const gpar_kspec_t* ks, const double* z1, int n1, int ldz1, const double* z2, int n2, int ldz2, int dz,
                         const double* W, int ldw, int mode, int nsplit, double* workspace, double* out, int ldo, void* stream);

/* Partial right-looking blocked Cholesky of the leading `nf` columns of the symmetric N x N matrix A
 * (lower triangle).  On exit A[:, :nf] holds L (N x nf, lower trapezoid) and A[nf:, nf:] holds the Schur
 * complement A22 - L21 L21^T.  nf == N is the ordinary potrf.  logdet (device, optional) += 2*sum log L_jj;
 * info (device, optional) = first non-positive pivot (1-based), untouched on success (zero it first).
 * Appending rows below K turns this one routine into the whole exact-GP computation:
 *   row  [y^T, 0]      -> z^T = (L^-1 y)^T and -|z|^2          (log marginal likelihood, gpar/model.py:226)
 *   rows [K_*x, K_**]  -> V^T = K_*x L^-T and K_** - V^T V      (posterior covariance, gpar/model.py:264,270)
 * Its panel kernel hands tiles between workgroups of one launch; a workgroup only ever waits for workgroups with a LOWER
 * block index (dispatched before it), so nothing depends on all of them being co-resident and several factorisations may
 * run at once from different streams; every wait is bounded all the same, and a timeout is reported as info = -77
 * (results invalid: retry with GPAR_POTRF_UNFUSED).
 * [matrix.cholesky -> torch.linalg.cholesky (LAPACK dpotrf)] */
int gpar_potrf(double* A, int N, int nf, int lda, double* logdet, int* info, void* stream);
/* The same with hints.  GPAR_POTRF_NO_LOOKAHEAD: the caller keeps three or more factorisations in flight on streams of its
 * own (independent layers, gpar/model.py:221-243 run concurrently), so the internal side stream is not used. */
#define GPAR_POTRF_NO_LOOKAHEAD 1
/* GPAR_POTRF_UNFUSED: panels by separate diagonal / strip / update kernels (no persistent kernel, no in-launch hand-offs):
 * the caller's retry path should a hand-off ever time out (info = -77). */
#define GPAR_POTRF_UNFUSED 2
int gpar_potrf_ex(double* A, int N, int nf, int lda, double* logdet, int* info, int flags, void* stream);

/* One dense layer's log marginal likelihood, fused (features, Gram + noise_diag + jitter, observations into the augmented row,
 * partial factorisation, value):  value[0] = log N(y; 0, k(x, x) + diag(noise_diag) + jitter I).  x: n x width (ldx); y: n values
 * with stride incy; noise_diag: n values (or null); z: n x dz workspace (ldz); A: (n + 1) x (n + 1) workspace (lda), holds the
 * factor, L^-1 y in row n and -|L^-1 y|^2 in the corner on exit; logdet / info / value: one word each, written (not accumulated).
 * potrf_flags as for gpar_potrf_ex.  [f.measure.logpdf(Obs(f(x, noise / w), y)) for a prior process, gpar/model.py:226,289] */
int gpar_logpdf_dense(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                      const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* logdet, int* info,
                      double* value, int potrf_flags, void* stream);

/* The same in three steps, for `batch` layers that do not feed one another and have the same number of rows (complete data:
 * the design matrix of layer i is [x, y_<i], known up front - gpar/model.py:221-243 visits them in a loop all the same):
 *   gpar_logpdf_dense_build   per layer: features, Gram + noise_diag + jitter and the observations into its (n + 1) x (n + 1)
 *                             matrix A_b = A + b * stride_a, its logdet[b] / info[b] zeroed;
 *   gpar_potrf_batch          the `batch` partial factorisations in LOCK-STEP - one panel launch and one batched trailing update
 *                             per 512 columns.  At the sizes where a factorisation is a chain of latency-bound panel kernels
 *                             (n <= ~4608) several of them on separate streams contend for compute-unit slots; in lock-step the
 *                             chain is paid once and every launch carries `batch` times the parallel work;
 *   gpar_logpdf_dense_finish  value[b] from the corner of A_b and logdet[b].
 * Arguments as for gpar_logpdf_dense / gpar_potrf_ex; stride_a (elements, even) separates consecutive matrices; logdet / info /
 * value hold `batch` words.  [sum over layers of f.measure.logpdf(obs), gpar/model.py:221-243] */
int gpar_logpdf_dense_build(const gpar_fspec_t* fs, const gpar_kspec_t* ks, const double* x, int n, int ldx, const double* y, long incy,
                            const double* noise_diag, double jitter, double* z, int ldz, double* A, int lda, double* logdet, int* info,
                            void* stream);
int gpar_potrf_batch(double* A, int batch, long long stride_a, int N, int nf, int lda, double* logdet, int* info, int flags, void* stream);
int gpar_logpdf_dense_finish(const double* A, int batch, long long stride_a, int n, int lda, const double* logdet, double* value,
                             void* stream);

/* A whole lock-step evaluation in ONE call (ABI v5): the log marginal likelihoods of `batch` layers over one set of n rows, and
 * their sum.  Layer b is described by layers[b] (HOST memory, read during the call): its feature map and kernel, its observation-
 * noise variance, and the column y_col of y (and of w) that holds its observations.  x: n x width, the widest design matrix -
 * for a GPAR [inputs, y_0 .. y_(p-2)] - from which every layer's feature map selects its own columns (gpar/model.py:320: layer i
 * sees [x, y_<i]); y: n x (>= max y_col + 1), ldy; w: weights laid out as y (ldw) or NULL for unit weights - the noise diagonal
 * of layer b is noise_b / w[:, y_col], an IEEE division per row.  Workspaces: z: batch * n rows of ldz >= max dz doubles;
 * nd: batch * n doubles (only read when w != NULL); A / lda / stride_a / logdet / info as for gpar_potrf_batch ((n + 1) x (n + 1)
 * matrices); value: `batch` words; total: one word or NULL, = ((0 + value[0]) + value[1]) + ... in layer order.
 * The same kernels, in the same order per matrix, as gpar_logpdf_dense_build / gpar_potrf_batch / gpar_logpdf_dense_finish: the
 * results are bit-identical; what it removes is the caller's side - a Python host spends ~0.1 ms per layer on tensor bookkeeping
 * and ~25 small launches per evaluation around those calls, which is most of an evaluation at n <= 1024.
 * [sum over layers of f.measure.logpdf(Obs(f(x_i, noise_i / w_i), y_i)), gpar/model.py:221-243 with :286-289, complete data] */
typedef struct {
    const gpar_fspec_t* fs;
    const gpar_kspec_t* ks;
    double noise;
    int32_t y_col;
    int32_t pad_;
} gpar_layer_t;
size_t gpar_sizeof_layer(void);
int gpar_logpdf_lockstep(const gpar_layer_t* layers, int batch, const double* x, int n, int ldx, const double* y, int ldy, const double* w,
                         int ldw, double jitter, double* z, int ldz, double* nd, double* A, int lda, long long stride_a, double* logdet,
                         int* info, double* value, double* total, int potrf_flags, void* stream);

/* B <- B L^-T  (right side, lower, transposed: forward substitution on the rows of B; B is nrows x n).
 * [solve_triangular inside matrix.iqf_diag / PosteriorKernel, reached from gpar/model.py:226,264,298] */
int gpar_trsm_rlt(const double* L, int n, int ldl, double* B, int nrows, int ldb, void* stream);
/* The same solve, PREDICATED on a device word (ABI v5): it happens iff (flag[0] != 0) == (run_if != 0), decided on the device when
 * the kernels start - flag is written by an earlier kernel of the stream (gpar_chol_spread), and no host synchronisation is
 * involved; a solve that is skipped costs its (empty) launches, B is left untouched.  flag == NULL: unconditional.
 * gpar_chol_spread: spread[0] <- (max L_jj / min L_jj)^2, a lower bound of cond(L L^T) that the factor holds for free;
 * flag[0] <- 1 if the spread exceeds `limit` or a pivot is not positive, else 0 (either pointer may be NULL).
 * [The inducing-point bound (stheno PseudoObs, gpar/model.py:286-287) needs A = I + L_z^-1 K_zx D^-1 K_xz L_z^-T.  Solving the
 *  n x M cross-Gram against L_z first (M^2 n flops) is backward stable whatever cond(K_zz); forming K_zx D^-1 K_xz first and
 *  solving the M x M result from both sides (2 M^3 flops) loses a factor ~cond(K_zz) and is only taken when the pivot spread of
 *  L_z says that this is harmless - each of the two orders is predicated on the same word, one of them runs.] */
int gpar_trsm_rlt_if(const double* L, int n, int ldl, double* B, int nrows, int ldb, const int* flag, int run_if, void* stream);
int gpar_chol_spread(const double* L, int n, int ldl, double limit, double* spread, int* flag, void* stream);
/* The scalar side of the inducing-point bound in two calls instead of ~25 tensor operations per layer (ABI v5):
 *   gpar_vfe_assemble  A <- [[G + diag_add I, .], [c^T, 0]] ((M + 1) x (M + 1): what gpar_potrf factors next; lower triangle of G read),
 *                      logdet / info zeroed, scal (256 doubles: 64 partial sums of each) <- sum ys^2, sum kdiag / d, sum log d (n terms), tr G;
 *   gpar_vfe_value     out[0] <- -1/2 (with_trace (S1 - S3) + S2 + n log 2 pi + logdet + S0 + A[M][M]) once A is factored (its corner then
 *                      holds -|L_A^-1 c|^2), S_q the sums of the parts in order.
 * [the elbo of stheno's PseudoObs, gpar/model.py:226 with :286-287: trace term, log-determinants and quadratic form] */
int gpar_vfe_assemble(const double* G, int M, int ldg, const double* c, const double* ys, const double* kdiag, const double* d, int n,
                      double diag_add, double* A, int lda, double* scal, double* logdet, int* info, void* stream);
int gpar_vfe_value(const double* scal, const double* logdet, const double* A, int lda, int M, int n, int with_trace, double* out, void* stream);
/* B <- B L^-1  (right side, lower, not transposed: backward substitution on the rows of B). */
int gpar_trsm_rln(const double* L, int n, int ldl, double* B, int nrows, int ldb, void* stream);

/* Kinv (lower triangle) <- (L L^T)^-1 given the Cholesky factor L; X is an n x n workspace (its upper triangle holds L^-T on
 * exit; below the diagonal it is scratch).
 * Triangular-aware: 2 n^3 / 3 flops.  Kinv doubles as scratch while L^-T is formed (recursive blocked inversion for n a
 * multiple of 512, otherwise the solve of the identity).  [the K^-1 that the analytic gradient
 * 1/2 tr((aa^T - K^-1) dK) needs; replaces autograd through cholesky / solve_triangular, gpar/regression.py:459] */
int gpar_chol_inverse(const double* L, int n, int ldl, double* X, int ldx, double* Kinv, int ldk, void* stream);

/* Streaming conditioning (ABI v11): moving a conditioned layer's window of observations without factoring it again.
 * gpar_chol_drop_leading forgets the k LEADING observations.  A: the augmented (n + 1) x (n + 1) factor as gpar_potrf (nf = n) leaves it
 * - L in the lower triangle, z^T = (L^-1 y)^T in row n, -|z|^2 in the corner.  With L = [[L11, 0], [L21, L22]] and z = [z1; z2] it writes,
 * OUT OF PLACE into out ((n - k + 1) x (n - k + 1), ldo; must not overlap A; the strict upper triangle is left alone), L22' with
 * L22' L22'^T = L22 L22^T + L21 L21^T, z2' with L22' z2' = y2 in its last row and -|z2'|^2 in the corner: the augmented factor of the
 * trailing n - k observations.  logdet[0] <- 2 sum log L22'_jj (written, not accumulated; may be NULL).  A positive rank-k update (never a
 * downdate): LINPACK's dchud, blocked.  For column j ascending and update vector t = 0 .. k-1 ascending (v_t = column t of L21, with the
 * augmented row as one more row of it: v_t[n - k] = z1[t]), a = L_jj and b = v_t[j] as the earlier operations left them:
 *   r = sqrt(fma(a, a, b * b)), c = a / r, s = b / r, L_jj <- r; for every row i > j, the augmented row like any other:
 *   L_ij' = fma(c, L_ij, s * v_t[i]), v_t[i]' = fma(c, v_t[i], -(s * L_ij));  corner = -(fma chain of z2'_j^2 over j ascending from 0).
 * A non-finite r is reported as info[0] = its 1-based column of `out` (first one wins; untouched on success: zero it first; may be NULL).
 * Launches: two plain launches per 64 columns - the diagonal block by one workgroup, which also leaves the panel's (c, s) table in the
 * workspace, then all rows below it and the augmented row, one thread per row - and nothing else: no waiting inside a launch, no atomics,
 * no host synchronisation, vector stores only.  The result is a function of the inputs alone: two runs give the same bits.
 * ws: gpar_workspace_doubles(GPAR_WS_CHOL_UPDATE, n, k, 0) doubles.  Limits: 1 <= k < n, k <= GPAR_CHOL_UPDATE_MAX_RANK - the workspace
 * holds the (n - k + 1) x k update vectors and a 64 x k table of (c, s) pairs, as much as the factor itself once k nears n, and the
 * 3 k n^2 flops of the update pass the n^3 / 3 of a fresh factorisation long before that.  Traffic: 8 n^2 bytes of L read and written.
 * [replaces (f | obs) built again on the moved window: Obs construction and conditioning at gpar/model.py:286-301]
 *
 * gpar_chol_append takes k NEW observations in.  A: (n0 + k + 1) x (n0 + k + 1) (lda).  On entry its leading n0 x n0 block holds L; rows
 * n0 .. n0 + k - 1 hold the raw entries [K_new,old, K_new,new + noise + jitter] (lower triangle); the last row holds
 * [z_old^T, y_new^T, .] - the caller moves the old augmented row below the new rows; the corner is ignored.  logdet[0] holds the
 * log-determinant of L on entry.  On exit A is the augmented factor of the n0 + k observations and logdet[0] their log-determinant.
 * It composes existing kernels, in this order: the corner zeroed (a memset node); gpar_trsm_rlt of rows n0 .. n0 + k - 1 against L (the
 * last row's first n0 entries ARE already solved: z_old); gpar_gemm (GPAR_GEMM_C_LOWER) C <- C - B B^T on the trailing
 * (k + 1) x (k + 1) block with B the n0 leading columns of the k + 1 bottom rows; gpar_potrf_ex of that block with nf = k.
 * info: as gpar_potrf_ex reports it for the trailing block (1-based among the k new rows).  n0 >= 0, k >= 1.
 * [replaces (f | obs) built again on the longer data: gpar/model.py:286-301] */
#define GPAR_CHOL_UPDATE_MAX_RANK 1024
int gpar_chol_drop_leading(const double* A, int n, int k, int lda, double* out, int ldo, double* ws, double* logdet, int* info, void* stream);
int gpar_chol_append(double* A, int n0, int k, int lda, double* logdet, int* info, int potrf_flags, void* stream);

/* C <- alpha * op(A) op(B) + beta * C with op(A) m x k, op(B) k x n.  ta: A is stored k x m (transposed);
 * tb: B is stored n x k (transposed).  fp64 on the matrix cores (v_mfma_f64_16x16x4).
 * [B.matmul in lab: K_*x alpha, V^T V, chol(var) z] */
int gpar_gemm(int ta, int tb, int m, int n, int k, double alpha, const double* A, int lda, const double* B,
              int ldb, double beta, double* C, int ldc, int flags, void* stream);

/* `batch` products of one shape in one launch: problem b reads A + b * stride_a, B + b * stride_b and writes C + b * stride_c
 * (elements).  [the per-sample downdates K(x_s, x_s) - V_s V_s^T of ancestral sampling, gpar/regression.py:559-563 run for all
 * samples of a layer at once] */
int gpar_gemm_batch(int ta, int tb, int m, int n, int k, double alpha, const double* A, int lda, long long stride_a, const double* B,
                    int ldb, long long stride_b, double beta, double* C, int ldc, long long stride_c, int flags, int batch, void* stream);

/* As gpar_gemm, with the K range cut into `splits` slices whose partial products go to `workspace`
 * (splits * m * n doubles) and are summed in slice order by a second kernel: for outputs with few 128 x 128 tiles and
 * a very long K (the inducing-point matrix B D^-1 B^T: M x M from K = n).  Deterministic.  A_LOWER / K_FROM_ROW / K_TO_COL
 * are not meaningful here. */
int gpar_gemm_splitk(int ta, int tb, int m, int n, int k, double alpha, const double* A, int lda, const double* B,
                     int ldb, double beta, double* C, int ldc, int flags, int splits, double* workspace, void* stream);

/* Small device-side reductions used by the fused paths (all asynchronous, all deterministic). */
/* out[0] (+)= sum_i x[i*incx]*y[i*incy] */
int gpar_dot(const double* x, int incx, const double* y, int incy, int n, double* out, int accumulate, void* stream);
/* out[j] = sum_i A[i][j] * v[i], j < cols, for a tall rows x cols matrix (two passes: per-128-row partial sums into
 * `workspace` - gpar_workspace_doubles(GPAR_WS_GEMV_T, rows, cols, 0) doubles - then an in-order sum).
 * [c = B D^-1 y of the inducing-point bound; stheno PseudoObs, gpar/model.py:286-287] */
int gpar_gemv_t(const double* A, int rows, int cols, int lda, const double* v, double* out, double* workspace, void* stream);
/* out[i] = sum_j A[i][j]^2, i < rows.  [marginal posterior variances k(x*, x*) - |V_i|^2, V = K_*x L^-T] */
int gpar_rownorm2(const double* A, int rows, int cols, int lda, double* out, void* stream);

/* Lower triangle (diagonal included) of the row-major n x n matrix A <-> packed storage of n (n + 1) / 2 doubles (row r at
 * offset r (r + 1) / 2).  [the exchange format of Cholesky factors between the GPUs of a node: layer-parallel conditioning
 * all-gathers packed factors, half the bytes of the padded square buffers] */
int gpar_pack_lower(const double* A, int n, int lda, double* out, void* stream);
int gpar_unpack_lower(const double* in, int n, double* A, int lda, void* stream);

/* Workspace sizes in doubles (the caller allocates every workspace; -1 for an unknown `op`):
 *   GPAR_WS_GEMM_SPLITK  (m, n, splits)   gpar_gemm_splitk
 *   GPAR_WS_GEMV_T       (rows, cols, -)  gpar_gemv_t
 *   GPAR_WS_GRAM_GRAD    (nblocks, -, -)  gpar_gram_grad / gpar_gram_grad_cross
 *   GPAR_WS_CHOL_INVERSE (n, ldx, -)      the X matrix of gpar_chol_inverse
 *   GPAR_WS_LOO          (n, grad, -)     the `vec` of gpar_loo_dense (grad = 0) / gpar_loo_dense_grad[_finish] (grad = 1)
 *   GPAR_WS_CV           (n, grad, max_fold)  the `vec` of gpar_cv_dense (grad = 0) / gpar_cv_dense_grad[_finish] (grad = 1)
 *   GPAR_WS_AHEAD        (n, grad, -)     the `vec` of gpar_ahead_dense (grad = 0) / gpar_ahead_dense_grad[_finish] (grad = 1)
 *   GPAR_WS_CV_GAP       (n, grad, max_hold)  the `vec` of gpar_cv_gap_dense (grad = 0) / gpar_cv_gap_dense_grad[_finish] (grad = 1)
 *   GPAR_WS_PIVOTED_CHOL (n, -, -)        gpar_pivoted_chol
 *   GPAR_WS_CHOL_UPDATE  (n, k, -)        gpar_chol_drop_leading
 *   GPAR_WS_AHEAD_MULTI  (n, grad, nh)    the `vec` of gpar_ahead_multi_dense (grad = 0) / gpar_ahead_multi_dense_grad[_finish] (grad = 1)
 *   GPAR_WS_AHEAD_WINDOW (n, grad, -)     the `vec` of gpar_ahead_window_dense (grad = 0) / gpar_ahead_window_dense_grad (grad = 1)
 *   GPAR_WS_POSTERIOR_TERMS (n, ns, ncomp)  gpar_posterior_terms (the recommended size; see there for the least)
 *   GPAR_WS_POSTERIOR_DERIV (n, ns, ndir)   gpar_posterior_deriv (likewise)
 *   GPAR_WS_GRAM_GRAD_ROWS  (n2, n1, -)     gpar_gram_grad_rows (likewise) */
#define GPAR_WS_GEMM_SPLITK 1
#define GPAR_WS_GEMV_T 2
#define GPAR_WS_GRAM_GRAD 3
#define GPAR_WS_CHOL_INVERSE 4
#define GPAR_WS_INPUT_GRAD 5   /* (n1, dz, nsplit)  gpar_gram_input_grad */
#define GPAR_WS_LOO 6
#define GPAR_WS_CV 7
#define GPAR_WS_PIVOTED_CHOL 8
#define GPAR_WS_CHOL_UPDATE 9
#define GPAR_WS_AHEAD 10
#define GPAR_WS_CV_GAP 11
#define GPAR_WS_AHEAD_MULTI 12
#define GPAR_WS_AHEAD_WINDOW 13
#define GPAR_WS_POSTERIOR_TERMS 14
#define GPAR_WS_GRAM_APPLY 15   /* (n, rows, output columns)  gpar_gram_apply_groups */
#define GPAR_WS_POSTERIOR_DERIV 16   /* (n, ns, ndir)  gpar_posterior_deriv (the recommended size; see there for the least) */
#define GPAR_WS_GRAM_GRAD_ROWS 17   /* (n2, n1, -)  gpar_gram_grad_rows (the recommended size; see there for the least) */
long long gpar_workspace_doubles(int op, int a, int b, int c);
/* Standard normals from Philox-4x32-10 + Box-Muller: out[r][c], element index = r*cols + c in the stream
 * identified by (seed, offset).   [B.randn in Normal.sample] */
int gpar_randn(uint64_t seed, uint64_t offset, double* out, int rows, int cols, int ldo, void* stream);

/* y[i*incy] = sum_{j<=i} L[i][j] * x[j*incx], i < n: lower-triangular matrix times ONE vector (the strict upper triangle
 * is not read).  [the chol(cov) * z product of Normal.sample for a single draw; a 128-wide GEMM tile for one column is
 * all latency] */
int gpar_trmv_lower(const double* L, int n, int ldl, const double* x, int incx, double* y, int incy, void* stream);
/* y[i*incy] = sum_{j>=i} U[i][j] * x[j*incx], i < n: UPPER-triangular matrix times one vector (ABI v7; the strict lower triangle is
 * not read).  With U = X = L^-T - the workspace gpar_chol_inverse leaves behind - and x = L^-1 y (row n of an augmented factor) it is
 * alpha = (L L^T)^-1 y, the vector of the gradient's weights W = alpha alpha^T - K^-1, at memory speed instead of a backward
 * substitution.  [the alpha of the analytic gradient inside varz.minimise_l_bfgs_b, gpar/regression.py:459] */
int gpar_trmv_upper(const double* U, int n, int ldu, const double* x, int incx, double* y, int incy, void* stream);
/* y[i*incy] = alpha * sum_j A[i][j] * x[j*incx], i < rows: a general row-major matrix times ONE vector (ABI v5; one wave per row).
 * [posterior means K(x*, X) alpha and K(x*, Z) v: gpar/model.py:298-301 - matrix-vector products that a 128-wide GEMM tile serves badly] */
int gpar_gemv(const double* A, int rows, int cols, int lda, const double* x, int incx, double alpha, double* y, int incy, void* stream);
/* The same for `batch` lower-triangular matrices with one vector each, in one launch: y_b = L_b x_b (+ add_b if add is non-null),
 * matrix / vector b at L + b * stride_l, x + b * stride_x, add + b * stride_add, y + b * stride_y (elements).  [the draws of all
 * posterior samples of a layer: mean_s + chol(cov_s) z_s, gpar/regression.py:559-563] */
int gpar_trmv_lower_batch(const double* L, int batch, long long stride_l, int n, int ldl, const double* x, int incx, long long stride_x,
                          const double* add, int inca, long long stride_add, double* y, int incy, long long stride_y, void* stream);

/* Monte-Carlo reduction of predict [gpar/regression.py:589-595: np.mean / np.percentile over the sample axis]:
 * samples[s * stride + e], s < S, e < count.  mean[e] = (sum over s, in order) / S.  If lo / hi are non-null they
 * receive the order-statistic interpolations  v[k] + g (v[k+1] - v[k])  (numpy's "linear" method, evaluated with
 * numpy's _lerp so the result is bit-identical to np.percentile for the same (k, g)); the caller derives
 * (k_lo, g_lo), (k_hi, g_hi) from the percentiles exactly as numpy does.  Selection is by rank counting, O(S^2)
 * per element, S <= 65536.  An element with a NaN among its samples gets NaN bounds (and a NaN mean), as numpy gives. */
int gpar_sample_stats(const double* samples, int S, long long count, long long stride, int k_lo, double g_lo, int k_hi,
                      double g_hi, double* mean, double* lo, double* hi, void* stream);

/* Profiling hook for bench.py: when enabled, every trailing-update SYRK launched by gpar_potrf is
 * bracketed by hipEvents on its own stream; the accumulated (launches, sum of their durations in ms, union of
 * their intervals in ms - launches from different caller streams may overlap -, flops) can be read back (this
 * call synchronises the recorded events). */
int gpar_profile_enable(int on);
int gpar_profile_read(int* launches, double* ms, double* busy_ms, double* flops, int reset);

#ifdef __cplusplus
}
#endif
#endif /* GPAR_HIP_H */
