// Arithmetic shared VERBATIM by the ahead-of-time Gram kernels (gram.h includes this file as code) and the per-specification
// kernels generated at run time (gram_jit.h includes it as a string literal that is prepended to the generated source): one
// text, so the two paths round identically.  Written inside a macro argument: no preprocessor directives, _Pragma("unroll")
// instead of #pragma unroll.
GPAR_DEVICE_CODE(

typedef double g_d2 __attribute__((ext_vector_type(2)));
typedef double g_d4 __attribute__((ext_vector_type(4)));

constexpr int GRAM_T = 64;
constexpr int GRAM_LD = 68;

// Squared distances / inner products of a 4 x 2 micro-tile over ND feature dims starting at d0, fully unrolled: all 3 ND
// LDS reads are issued before the first fused multiply-add (a rolled loop over a run-time dim count waits out the LDS
// latency and pays the loop overhead once per dim: the kernel ran at 46 % of the vector-ALU issue rate).
template <int ND, bool LINEAR>
__device__ __forceinline__ void gram_accum(const double* __restrict__ Za, const double* __restrict__ Zb, int d0, int ty, int cb,
                                           double (&s)[8]) {
    g_d4 za[ND];
    g_d2 zb[ND];
    _Pragma("unroll")
    for (int q = 0; q < ND; ++q) {
        za[q] = *reinterpret_cast<const g_d4*>(&Za[(d0 + q) * GRAM_LD + 4 * ty]);
        zb[q] = *reinterpret_cast<const g_d2*>(&Zb[(d0 + q) * GRAM_LD + cb]);
    }
    _Pragma("unroll")
    for (int q = 0; q < ND; ++q) {
        _Pragma("unroll")
        for (int i = 0; i < 4; ++i) {
            if (LINEAR) {
                s[2 * i] = fma(za[q][i], zb[q][0], s[2 * i]);
                s[2 * i + 1] = fma(za[q][i], zb[q][1], s[2 * i + 1]);
            } else {
                const double d0_ = za[q][i] - zb[q][0];
                const double d1_ = za[q][i] - zb[q][1];
                s[2 * i] = fma(d0_, d0_, s[2 * i]);
                s[2 * i + 1] = fma(d1_, d1_, s[2 * i + 1]);
            }
        }
    }
}

// The same over a run-time range of dims [off, off + nd), four at a time (eight at a time needed 220 registers).
template <bool LINEAR>
__device__ __forceinline__ void gram_accum_dims(const double* __restrict__ Za, const double* __restrict__ Zb, int off, int nd, int ty,
                                                int cb, double (&s)[8]) {
    int d = off;
    for (; d + 4 <= off + nd; d += 4) gram_accum<4, LINEAR>(Za, Zb, d, ty, cb, s);
    switch (off + nd - d) {
        case 3: gram_accum<3, LINEAR>(Za, Zb, d, ty, cb, s); break;
        case 2: gram_accum<2, LINEAR>(Za, Zb, d, ty, cb, s); break;
        case 1: gram_accum<1, LINEAR>(Za, Zb, d, ty, cb, s); break;
        default: break;
    }
}

// ... and over a COMPILE-TIME range (generated kernels): the same groups of four in the same order, so the sums round alike.
template <int OFF, int ND, bool LINEAR>
__device__ __forceinline__ void gram_accum_static(const double* __restrict__ Za, const double* __restrict__ Zb, int ty, int cb,
                                                  double (&s)[8]) {
    if constexpr (ND >= 4) {
        gram_accum<4, LINEAR>(Za, Zb, OFF, ty, cb, s);
        // (left alone, the LDS reads of every later group are hoisted to the front and the multiply-adds sunk behind them: 512
        // registers and spills at 42 dims.  The empty statements pin the partial sums and fence the reads; they emit nothing.)
        _Pragma("unroll")
        for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(s[e]) : : "memory");
        gram_accum_static<OFF + 4, ND - 4, LINEAR>(Za, Zb, ty, cb, s);
    } else if constexpr (ND > 0) {
        gram_accum<ND, LINEAR>(Za, Zb, OFF, ty, cb, s);
    }
}

// Tables of the two elementary functions below, staged into LDS by every workgroup (gram_load_tables; tools/gen_gram_tables.py): 2^(j/64), j < 64, then
// for the 128 intervals of the mantissa range [0.5, 1) the pairs { v_j = 1 / c_j rounded, log(2 / v_j) },
// c_j = (1 + (j + 1/2) / 128) / 2: with M = 2 m in [1, 2), r = m v_j - 1 and log M = log(2 / v_j) + log1p(r) - small table values near M = 1.  (Generated with 200-bit arithmetic; hexadecimal literals are exact.)
constexpr int GRAM_EXP_TAB = 64;
constexpr int GRAM_TAB_DOUBLES = GRAM_EXP_TAB + 256;
__device__ const double GRAM_TAB[GRAM_TAB_DOUBLES] = {
        0x1.0000000000000p+0, 0x1.02c9a3e778061p+0, 0x1.059b0d3158574p+0, 0x1.0874518759bc8p+0,
        0x1.0b5586cf9890fp+0, 0x1.0e3ec32d3d1a2p+0, 0x1.11301d0125b51p+0, 0x1.1429aaea92de0p+0,
        0x1.172b83c7d517bp+0, 0x1.1a35beb6fcb75p+0, 0x1.1d4873168b9aap+0, 0x1.2063b88628cd6p+0,
        0x1.2387a6e756238p+0, 0x1.26b4565e27cddp+0, 0x1.29e9df51fdee1p+0, 0x1.2d285a6e4030bp+0,
        0x1.306fe0a31b715p+0, 0x1.33c08b26416ffp+0, 0x1.371a7373aa9cbp+0, 0x1.3a7db34e59ff7p+0,
        0x1.3dea64c123422p+0, 0x1.4160a21f72e2ap+0, 0x1.44e086061892dp+0, 0x1.486a2b5c13cd0p+0,
        0x1.4bfdad5362a27p+0, 0x1.4f9b2769d2ca7p+0, 0x1.5342b569d4f82p+0, 0x1.56f4736b527dap+0,
        0x1.5ab07dd485429p+0, 0x1.5e76f15ad2148p+0, 0x1.6247eb03a5585p+0, 0x1.6623882552225p+0,
        0x1.6a09e667f3bcdp+0, 0x1.6dfb23c651a2fp+0, 0x1.71f75e8ec5f74p+0, 0x1.75feb564267c9p+0,
        0x1.7a11473eb0187p+0, 0x1.7e2f336cf4e62p+0, 0x1.82589994cce13p+0, 0x1.868d99b4492edp+0,
        0x1.8ace5422aa0dbp+0, 0x1.8f1ae99157736p+0, 0x1.93737b0cdc5e5p+0, 0x1.97d829fde4e50p+0,
        0x1.9c49182a3f090p+0, 0x1.a0c667b5de565p+0, 0x1.a5503b23e255dp+0, 0x1.a9e6b5579fdbfp+0,
        0x1.ae89f995ad3adp+0, 0x1.b33a2b84f15fbp+0, 0x1.b7f76f2fb5e47p+0, 0x1.bcc1e904bc1d2p+0,
        0x1.c199bdd85529cp+0, 0x1.c67f12e57d14bp+0, 0x1.cb720dcef9069p+0, 0x1.d072d4a07897cp+0,
        0x1.d5818dcfba487p+0, 0x1.da9e603db3285p+0, 0x1.dfc97337b9b5fp+0, 0x1.e502ee78b3ff6p+0,
        0x1.ea4afa2a490dap+0, 0x1.efa1bee615a27p+0, 0x1.f50765b6e4540p+0, 0x1.fa7c1819e90d8p+0,
        0x1.fe01fe01fe020p+0, 0x1.ff00aa2b10ba0p-9, 0x1.fa11caa01fa12p+0, 0x1.7dc475f810a69p-7,
        0x1.f6310aca0dbb5p+0, 0x1.3cea44346a584p-6, 0x1.f25f644230ab5p+0, 0x1.b9fc027af919ap-6,
        0x1.ee9c7f8458e02p+0, 0x1.1b0d98923d97fp-5, 0x1.eae807aba01ebp+0, 0x1.58a5bafc8e4d3p-5,
        0x1.e741aa59750e4p+0, 0x1.95c830ec8e3f2p-5, 0x1.e3a9179dc1a73p+0, 0x1.d276b8adb0b56p-5,
        0x1.e01e01e01e01ep+0, 0x1.075983598e471p-4, 0x1.dca01dca01dcap+0, 0x1.253f62f0a1417p-4,
        0x1.d92f2231e7f8ap+0, 0x1.42edcbea646eep-4, 0x1.d5cac807572b2p+0, 0x1.60658a93750c4p-4,
        0x1.d272ca3fc5b1ap+0, 0x1.7da766d7b12d0p-4, 0x1.cf26e5c44bfc6p+0, 0x1.9ab42462033aep-4,
        0x1.cbe6d9601cbe7p+0, 0x1.b78c82bb0eda0p-4, 0x1.c8b265afb8a42p+0, 0x1.d4313d66cb35dp-4,
        0x1.c5894d10d4986p+0, 0x1.f0a30c01162a4p-4, 0x1.c26b5392ea01cp+0, 0x1.0671512ca596fp-3,
        0x1.bf583ee868d8bp+0, 0x1.14785846742acp-3, 0x1.bc4fd65883e7bp+0, 0x1.2266f190a5acdp-3,
        0x1.b951e2b18ff23p+0, 0x1.303d718e47fd5p-3, 0x1.b65e2e3beee05p+0, 0x1.3dfc2b0ecc62ap-3,
        0x1.b37484ad806cep+0, 0x1.4ba36f39a55e5p-3, 0x1.b094b31d922a4p+0, 0x1.59338d9982085p-3,
        0x1.adbe87f94905ep+0, 0x1.66acd4272ad51p-3, 0x1.aaf1d2f87ebfdp+0, 0x1.740f8f54037a3p-3,
        0x1.a82e65130e159p+0, 0x1.815c0a14357e9p-3, 0x1.a574107688a4ap+0, 0x1.8e928de886d41p-3,
        0x1.a2c2a87c51ca0p+0, 0x1.9bb362e7dfb85p-3, 0x1.a01a01a01a01ap+0, 0x1.a8becfc882f19p-3,
        0x1.9d79f176b682dp+0, 0x1.b5b519e8fb5a6p-3, 0x1.9ae24ea5510dap+0, 0x1.c2968558c18c2p-3,
        0x1.9852f0d8ec0ffp+0, 0x1.cf6354e09c5ddp-3, 0x1.95cbb0be377aep+0, 0x1.dc1bca0abec7bp-3,
        0x1.934c67f9b2ce6p+0, 0x1.e8c0252aa5a60p-3, 0x1.90d4f120190d5p+0, 0x1.f550a564b7b37p-3,
        0x1.8e6527af1373fp+0, 0x1.00e6c45ad501dp-2, 0x1.8bfce8062ff3ap+0, 0x1.071b85fcd590dp-2,
        0x1.899c0f601899cp+0, 0x1.0d46b579ab74bp-2, 0x1.87427bcc092b9p+0, 0x1.136870293a8b0p-2,
        0x1.84f00c2780614p+0, 0x1.1980d2dd4236fp-2, 0x1.82a4a0182a4a0p+0, 0x1.1f8ff9e48a2f3p-2,
        0x1.8060180601806p+0, 0x1.2596010df763ap-2, 0x1.7e225515a4f1dp+0, 0x1.2b9303ab89d25p-2,
        0x1.7beb3922e017cp+0, 0x1.31871c9544185p-2, 0x1.79baa6bb6398bp+0, 0x1.3772662bfd85cp-2,
        0x1.77908119ac60dp+0, 0x1.3d54fa5c1f710p-2, 0x1.756cac201756dp+0, 0x1.432ef2a04e813p-2,
        0x1.734f0c541fe8dp+0, 0x1.49006804009d0p-2, 0x1.713786d9c7c09p+0, 0x1.4ec9732600269p-2,
        0x1.6f26016f26017p+0, 0x1.548a2c3add263p-2, 0x1.6d1a62681c861p+0, 0x1.5a42ab0f4cfe2p-2,
        0x1.6b1490aa31a3dp+0, 0x1.5ff3070a793d4p-2, 0x1.691473a88d0c0p+0, 0x1.659b57303e1f2p-2,
        0x1.6719f3601671ap+0, 0x1.6b3bb2235943dp-2, 0x1.6524f853b4aa3p+0, 0x1.70d42e2789236p-2,
        0x1.63356b88ac0dep+0, 0x1.7664e1239dbcfp-2, 0x1.614b36831ae94p+0, 0x1.7bede0a37afbfp-2,
        0x1.5f66434292dfcp+0, 0x1.816f41da0d495p-2, 0x1.5d867c3ece2a5p+0, 0x1.86e919a330ba1p-2,
        0x1.5babcc647fa91p+0, 0x1.8c5b7c858b48bp-2, 0x1.59d61f123ccaap+0, 0x1.91c67eb45a83ep-2,
        0x1.5805601580560p+0, 0x1.972a341135159p-2, 0x1.56397ba7c52e2p+0, 0x1.9c86b02dc0862p-2,
        0x1.54725e6bb82fep+0, 0x1.a1dc064d5b995p-2, 0x1.52aff56a8054bp+0, 0x1.a72a4966bd9e9p-2,
        0x1.50f22e111c4c5p+0, 0x1.ac718c258b0e5p-2, 0x1.4f38f62dd4c9bp+0, 0x1.b1b1e0ebdfc5ap-2,
        0x1.4d843bedc2c4cp+0, 0x1.b6eb59d3cf35cp-2, 0x1.4bd3edda68fe1p+0, 0x1.bc1e08b0dad0ap-2,
        0x1.4a27fad76014ap+0, 0x1.c149ff115f027p-2, 0x1.4880522014880p+0, 0x1.c66f4e3ff6ff9p-2,
        0x1.46dce34596066p+0, 0x1.cb8e0744d7acap-2, 0x1.453d9e2c776cap+0, 0x1.d0a63ae721e64p-2,
        0x1.43a2730abee4dp+0, 0x1.d5b7f9ae2c684p-2, 0x1.420b5265e5951p+0, 0x1.dac353e2c5955p-2,
        0x1.40782d10e6566p+0, 0x1.dfc859906d5b5p-2, 0x1.3ee8f42a5af07p+0, 0x1.e4c71a8687704p-2,
        0x1.3d5d991aa75c6p+0, 0x1.e9bfa659861f5p-2, 0x1.3bd60d9232955p+0, 0x1.eeb20c640ddf3p-2,
        0x1.3a524387ac822p+0, 0x1.f39e5bc811e5dp-2, 0x1.38d22d366088ep+0, 0x1.f884a36fe9ec1p-2,
        0x1.3755bd1c945eep+0, 0x1.fd64f20f61571p-2, 0x1.35dce5f9f2af8p+0, 0x1.011fab125ff8ap-1,
        0x1.34679ace01346p+0, 0x1.0389eefce633cp-1, 0x1.32f5ced6a1dfap+0, 0x1.05f14bd26459cp-1,
        0x1.3187758e9ebb6p+0, 0x1.0855c884b450ep-1, 0x1.301c82ac40260p+0, 0x1.0ab76bece14d2p-1,
        0x1.2eb4ea1fed14bp+0, 0x1.0d163ccb9d6b8p-1, 0x1.2d50a012d50a0p+0, 0x1.0f7241c9b497dp-1,
        0x1.2bef98e5a3711p+0, 0x1.11cb81787ccf8p-1, 0x1.2a91c92f3c105p+0, 0x1.1422025243d45p-1,
        0x1.293725bb804a5p+0, 0x1.1675cababa60ep-1, 0x1.27dfa38a1ce4dp+0, 0x1.18c6e0ff5cf07p-1,
        0x1.268b37cd60127p+0, 0x1.1b154b57da29ep-1, 0x1.2539d7e9177b2p+0, 0x1.1d610fe677003p-1,
        0x1.23eb79717605bp+0, 0x1.1faa34b87094cp-1, 0x1.22a0122a0122ap+0, 0x1.21f0bfc65beecp-1,
        0x1.21579804855e6p+0, 0x1.2434b6f483934p-1, 0x1.2012012012012p+0, 0x1.26762013430e0p-1,
        0x1.1ecf43c7fb84cp+0, 0x1.28b500df60783p-1, 0x1.1d8f5672e4abdp+0, 0x1.2af15f02640acp-1,
        0x1.1c522fc1ce059p+0, 0x1.2d2b4012edc9dp-1, 0x1.1b17c67f2bae3p+0, 0x1.2f62a99509546p-1,
        0x1.19e0119e0119ep+0, 0x1.3197a0fa7fe6ap-1, 0x1.18ab083902bdbp+0, 0x1.33ca2ba328994p-1,
        0x1.1778a191bd684p+0, 0x1.35fa4edd36ea0p-1, 0x1.1648d50fc3201p+0, 0x1.38280fe58797fp-1,
        0x1.151b9a3fdd5c9p+0, 0x1.3a5373e7ebdf9p-1, 0x1.13f0e8d344724p+0, 0x1.3c7c7fff73206p-1,
        0x1.12c8b89edc0acp+0, 0x1.3ea33936b2f5bp-1, 0x1.11a3019a74826p+0, 0x1.40c7a4880dceap-1,
        0x1.107fbbe011080p+0, 0x1.42e9c6ddf80bfp-1, 0x1.0f5edfab325a2p+0, 0x1.4509a5133bb0ap-1,
        0x1.0e40655826011p+0, 0x1.472743f33aaadp-1, 0x1.0d24456359e3ap+0, 0x1.4942a83a2fc07p-1,
        0x1.0c0a7868b4171p+0, 0x1.4b5bd6956e273p-1, 0x1.0af2f722eecb5p+0, 0x1.4d72d3a39fd01p-1,
        0x1.09ddba6af8360p+0, 0x1.4f87a3f5026e9p-1, 0x1.08cabb37565e2p+0, 0x1.519a4c0ba3446p-1,
        0x1.07b9f29b8eae2p+0, 0x1.53aad05b99b7cp-1, 0x1.06ab59c7912fbp+0, 0x1.55b9354b40bcep-1,
        0x1.059eea0727586p+0, 0x1.57c57f336f191p-1, 0x1.04949cc1664c5p+0, 0x1.59cfb25fae87fp-1,
        0x1.038c6b78247fcp+0, 0x1.5bd7d30e71c73p-1, 0x1.02864fc7729e9p+0, 0x1.5ddde57149923p-1,
        0x1.0182436517a37p+0, 0x1.5fe1edad18919p-1, 0x1.0080402010080p+0, 0x1.61e3efda46467p-1};

__device__ __forceinline__ void gram_load_tables(double* __restrict__ tab, int t) {
    for (int i = t; i < GRAM_TAB_DOUBLES; i += 256) tab[i] = GRAM_TAB[i];
}

// exp(-E / 2) for eight independent arguments E >= 0 (E = squared scaled distance of EQ factors + 2 alpha log1p(.) of RQ factors),
// the eight chains interleaved.  With x = -E / 2 = (64 e + j) ln2 / 64 + r, |r| <= ln2 / 128:  exp(x) = 2^e * 2^(j/64) * exp(r).
//   k = rint(-E * 32 / ln2) = 64 e + j;   r2 = E + k * ln2 / 32 = -2 r  (one fused multiply-add: the constant is ln2 / 32 rounded, so
//       r2 carries an error of |k| * 1.7e-18 - RELATIVE error of the result |k| * 8.7e-19, i.e. ABSOLUTE error at most 3e-17
//       (at |k| = 92): entries near 1 are as exact as before, entries near 1e-9 lose three digits they never had a use for);
//   exp(r) = sum_j (-r2 / 2)^j / j!, degree 5 (remainder r^6 / 720 <= 3.5e-17 relative), the -1/2 folded into the coefficients;
//   2^(j/64) from the LDS table (64 entries on 64 banks of 4 bytes: two entries per bank pair, at worst a two-way conflict);
//   2^e by v_ldexp_f64, which also flushes to zero / denormals below -708.
// 15 vector instructions per value, index arithmetic included (round 3's first version: 32-entry table, degree 6, two-step
// reduction, the -1/2 applied by the caller: 17; round 2: ln2 / 2 reduction and a degree-13 polynomial, 23).
__device__ __forceinline__ void gram_exph8(double (&x)[8], const double* __restrict__ tab) {
    _Pragma("clang fp contract(off)")   // every fused multiply-add below is written out: the two compilations must not differ
    constexpr double NR32L2 = -0x1.71547652b82fep+5;   // -32 / ln2
    constexpr double L32 = 0x1.62e42fefa39efp-6;        // ln2 / 32
    double k[8];
    double r[8];
    double p[8];
    double tj[8];
    int ki[8];
    _Pragma("unroll")
    for (int i = 0; i < 8; ++i) k[i] = __builtin_rint(x[i] * NR32L2);
    _Pragma("unroll")
    for (int i = 0; i < 8; ++i) { ki[i] = (int)k[i]; tj[i] = tab[ki[i] & (GRAM_EXP_TAB - 1)]; }
    _Pragma("unroll")
    for (int i = 0; i < 8; ++i) r[i] = fma(k[i], L32, x[i]);
    _Pragma("unroll")
    for (int i = 0; i < 8; ++i) p[i] = fma(-1.0 / 3840.0, r[i], 1.0 / 384.0);
    _Pragma("unroll")
    for (int i = 0; i < 8; ++i) p[i] = fma(p[i], r[i], -1.0 / 48.0);
    _Pragma("unroll")
    for (int i = 0; i < 8; ++i) p[i] = fma(p[i], r[i], 0.125);
    _Pragma("unroll")
    for (int i = 0; i < 8; ++i) p[i] = fma(p[i], r[i], -0.5);
    _Pragma("unroll")
    for (int i = 0; i < 8; ++i) p[i] = fma(p[i], r[i], 1.0);
    _Pragma("unroll")
    for (int i = 0; i < 8; ++i) x[i] = __builtin_amdgcn_ldexp(p[i] * tj[i], ki[i] >> 6);
}

// exp(x), x <= 0: the gradient passes' form (they keep the exponent itself).
__device__ __forceinline__ void gram_exp8(double (&x)[8], const double* __restrict__ tab) {
    _Pragma("unroll")
    for (int i = 0; i < 8; ++i) x[i] *= -2.0;
    gram_exph8(x, tab);
}

// RQ factor: expo -= alpha log1p(u), u = s / 2 alpha >= 0   [(1 + s / 2 alpha)^-alpha = exp(-alpha log1p(s / 2 alpha))]
//   w = fl(1 + u), c = u - (w - 1) (the exact rounding error),  w = m 2^e,  j = top 7 mantissa bits of m,  r = m v_j - 1, |r| < 2^-8:
//   log1p(u) = (e - 1) ln2 + log(2 / v_j) + log1p(r) + c / w,      log1p(r) = r + r^2 (-1/2 + r (1/3 + r (-1/4 + r (1/5 - r/6))))
// with v_j, log(2 / v_j) from the LDS table and c / w ~ c v_j 2^-e (a correction of at most 1e-16: 1 % accuracy is plenty).
// Relative error at most 8.1 * 2^-53 = 9.0e-16 for u >= 2^-7 and absolute error at most 17 * 2^-62 = 3.7e-18 below (the table value
// and log1p(r) cancel there; the degree-6 truncation r^7 / 7 = 1.9e-18 at the interval ends is half of it) - a rounding analysis, written
// out in tests/test_gram_math.py, whose sweep of an operation-by-operation emulation measures 1.9 * 2^-53 and 2.6e-18; below u ~ 1e-17 the
// result is 1.7e-18 whatever u is, so only the absolute bound holds there.  That is what the exponent -alpha log1p(u) needs (alpha L times
// the relative bound stays inside 1e-13 at exponents of 100); u == 0 gives exactly 0, so that the diagonal of an RQ Gram matrix is exactly
// its coefficient.  ~20 vector instructions per value where the library's
// log1p (double-double arithmetic, every special case) takes ~130 - it was 60 % of the C5 kernel's instructions.
__device__ __forceinline__ double gram_log1p_pos(double u, const double* __restrict__ tab) {
    _Pragma("clang fp contract(off)")   // (1 + s h would otherwise be fused in one compilation and not in the other)
    constexpr double LN2HI = 0x1.62e42fefa2000p-1;
    constexpr double LN2LO = 0x1.9ef35793c7673p-41;
    const double w = 1.0 + u;
    const double c = u - (w - 1.0);
    const double m = __builtin_amdgcn_frexp_mant(w);
    const int e = __builtin_amdgcn_frexp_exp(w);
    const int j = (int)((__builtin_bit_cast(unsigned long long, m) >> 45) & 127ull);
    const g_d2 te = *reinterpret_cast<const g_d2*>(tab + GRAM_EXP_TAB + 2 * j);
    const double r = fma(m, te[0], -1.0);
    double q = fma(-1.0 / 6.0, r, 0.2);
    q = fma(q, r, -0.25);
    q = fma(q, r, 1.0 / 3.0);
    q = fma(q, r, -0.5);
    const double poly = fma(r * r, q, r);
    const double ed = (double)(e - 1);
    const double small = fma(ed, LN2LO, __builtin_amdgcn_ldexp(c * te[0], -e));
    const double lg = fma(ed, LN2HI, te[1]) + (poly + small);
    return u == 0.0 ? 0.0 : lg;
}

// RQ factor in the exponent's doubled form (gram_exph8 evaluates exp(-E / 2)):  E += 2 alpha log1p(s / 2 alpha).
__device__ __forceinline__ void gram_rqh8(const double (&s)[8], double alpha, double (&expo)[8], const double* __restrict__ tab) {
    _Pragma("clang fp contract(off)")
    const double h2a = 0.5 / alpha, a2 = 2.0 * alpha;
    _Pragma("unroll")
    for (int i = 0; i < 8; ++i) {
        expo[i] = fma(a2, gram_log1p_pos(s[i] * h2a, tab), expo[i]);
        // two chains in flight at a time (interleaving all eight costs ~25 live registers each: spills beside 42 feature dims)
        if (i & 1) __builtin_amdgcn_sched_barrier(0);
    }
}

// Matern factor of smoothness NU2 / 2 (NU2 = 1, 3, 5) in the same split: with r = sqrt(s), c = sqrt(NU2),
//   k = poly(r) exp(-c r),   poly = 1 | 1 + c r | 1 + c r + c^2 s / 3:
// the exponent joins the term's DOUBLED exponent sum (E += 2 c r; gram_exph8 evaluates exp(-E / 2)), the polynomial joins the
// product of the linear factors.  The square root is the correctly rounded one (the bare v_sqrt_f64 is good to ~2^-23 only).
// s == 0 gives r = 0, E += 0 and poly = 1 exactly: the diagonal of a Matern Gram matrix is exactly its coefficient.
constexpr double GRAM_SQRT3 = 0x1.bb67ae8584caap+0;
constexpr double GRAM_SQRT5 = 0x1.1e3779b97f4a8p+1;
constexpr double GRAM_5_3 = 0x1.aaaaaaaaaaaabp+0;
template <int NU2>
__device__ __forceinline__ void gram_maternh8(const double (&s)[8], double (&expo)[8], double (&lin)[8]) {
    _Pragma("clang fp contract(off)")
    constexpr double C = NU2 == 1 ? 1.0 : (NU2 == 3 ? GRAM_SQRT3 : GRAM_SQRT5);
    _Pragma("unroll")
    for (int i = 0; i < 8; ++i) {
        const double cr = C * __builtin_sqrt(s[i]);
        expo[i] = fma(2.0, cr, expo[i]);
        if (NU2 == 3) lin[i] *= 1.0 + cr;
        if (NU2 == 5) lin[i] *= fma(GRAM_5_3, s[i], 1.0 + cr);
    }
}

// ... and for the gradient passes of the generated kernels: value phi = k(s) and derivative dk = dk / ds of eight entries,
//   nu = 1/2: -exp(-r) / (2 r), taken as 0 where r = 0 (it only ever multiplies (z_a - z_b)^2 or (z_a - z_b), which vanish there:
//             the divisor is replaced, never a 0 / 0 or an infinity formed);   nu = 3/2: -(3/2) exp(-c r);
//   nu = 5/2: -(5/6)(1 + c r) exp(-c r).
template <int NU2>
__device__ __forceinline__ void gram_matern_grad8(const double (&s)[8], double (&phi)[8], double (&dk)[8], const double* __restrict__ tab) {
    constexpr double C = NU2 == 1 ? 1.0 : (NU2 == 3 ? GRAM_SQRT3 : GRAM_SQRT5);
    double cr[8];
    _Pragma("unroll")
    for (int i = 0; i < 8; ++i) { cr[i] = C * __builtin_sqrt(s[i]); phi[i] = 2.0 * cr[i]; }
    gram_exph8(phi, tab);   // exp(-c r)
    _Pragma("unroll")
    for (int i = 0; i < 8; ++i) {
        if (NU2 == 1) {
            dk[i] = cr[i] == 0.0 ? 0.0 : -0.5 * phi[i] / (cr[i] == 0.0 ? 1.0 : cr[i]);
        } else if (NU2 == 3) {
            dk[i] = -1.5 * phi[i];
            phi[i] *= 1.0 + cr[i];
        } else {
            dk[i] = (-0.5 * GRAM_5_3) * (1.0 + cr[i]) * phi[i];
            phi[i] *= fma(GRAM_5_3, s[i], 1.0 + cr[i]);
        }
    }
}

// Cosine factor: phi = cos(2 pi sigma), sigma = sum_d (za_d - zb_d) over the factor's dims - the cosine of a SUM over the dims, the
// spectral-mixture component (a length scale of the dim is its period).  sigma is summed from the explicit differences, in dim order:
// per-row angles A = sum_d za_d with cos A cos A' + sin A sin A' would round the phase at the size of the rows' angles (time stamps of
// 1e5 over periods near 1: four digits left), the differences of nearby rows are exact.  sigma(b, a) = -sigma(a, b) exactly, so a
// Gram matrix of one point set is symmetric in bits; sigma = 0 gives exactly 1.  Plain additions only: nothing a compilation could fuse.
template <int ND>
__device__ __forceinline__ void gram_accum_diff(const double* __restrict__ Za, const double* __restrict__ Zb, int d0, int ty, int cb,
                                                double (&s)[8]) {
    g_d4 za[ND];
    g_d2 zb[ND];
    _Pragma("unroll")
    for (int q = 0; q < ND; ++q) {
        za[q] = *reinterpret_cast<const g_d4*>(&Za[(d0 + q) * GRAM_LD + 4 * ty]);
        zb[q] = *reinterpret_cast<const g_d2*>(&Zb[(d0 + q) * GRAM_LD + cb]);
    }
    _Pragma("unroll")
    for (int q = 0; q < ND; ++q) {
        _Pragma("unroll")
        for (int i = 0; i < 4; ++i) {
            s[2 * i] += za[q][i] - zb[q][0];
            s[2 * i + 1] += za[q][i] - zb[q][1];
        }
    }
}

// ... over a run-time range of dims (the interpreter) and over a compile-time range (generated kernels): the same order, the same sums.
__device__ __forceinline__ void gram_accum_diff_dims(const double* __restrict__ Za, const double* __restrict__ Zb, int off, int nd, int ty,
                                                     int cb, double (&s)[8]) {
    int d = off;
    for (; d + 4 <= off + nd; d += 4) gram_accum_diff<4>(Za, Zb, d, ty, cb, s);
    switch (off + nd - d) {
        case 3: gram_accum_diff<3>(Za, Zb, d, ty, cb, s); break;
        case 2: gram_accum_diff<2>(Za, Zb, d, ty, cb, s); break;
        case 1: gram_accum_diff<1>(Za, Zb, d, ty, cb, s); break;
        default: break;
    }
}

template <int OFF, int ND>
__device__ __forceinline__ void gram_accum_diff_static(const double* __restrict__ Za, const double* __restrict__ Zb, int ty, int cb,
                                                       double (&s)[8]) {
    if constexpr (ND >= 4) {
        gram_accum_diff<4>(Za, Zb, OFF, ty, cb, s);
        _Pragma("unroll")
        for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(s[e]) : : "memory");   // (as in gram_accum_static)
        gram_accum_diff_static<OFF + 4, ND - 4>(Za, Zb, ty, cb, s);
    } else if constexpr (ND > 0) {
        gram_accum_diff<ND>(Za, Zb, OFF, ty, cb, s);
    }
}

// The factor's value multiplies into the product of the term's linear factors: lin *= cospi(2 sigma) - the argument is reduced in units
// of half periods, exactly (2 sigma is exact), where cos(2 pi sigma) would first round 2 pi sigma.  fp64 cospi is a software sequence
// (fraction, two short polynomials, a select): two chains in flight at a time, as gram_rqh8 keeps it.
__device__ __forceinline__ void gram_cosh8(const double (&s)[8], double (&lin)[8]) {
    _Pragma("unroll")
    for (int i = 0; i < 8; ++i) {
        lin[i] *= cospi(2.0 * s[i]);
        if (i & 1) __builtin_amdgcn_sched_barrier(0);
    }
}

// ... and for the gradient passes: value phi = cos(2 pi sigma) and derivative dk = d phi / d sigma = -2 pi sin(2 pi sigma) of eight
// entries from one range reduction each.  sigma = 0 (every pair of the DIAG mode) gives phi = 1 and dk = 0 exactly.
constexpr double GRAM_2PI = 0x1.921fb54442d18p+2;
__device__ __forceinline__ void gram_cos_grad8(const double (&s)[8], double (&phi)[8], double (&dk)[8]) {
    _Pragma("unroll")
    for (int i = 0; i < 8; ++i) {
        double sn, cs;
        sincospi(2.0 * s[i], &sn, &cs);
        phi[i] = cs;
        dk[i] = -GRAM_2PI * sn;
        if (i & 1) __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- gradient passes (generated kernels only; grad_jit.h) ---------------------------------------------------------------------
// Per-dim moment sums of one factor over a 4 x 2 micro-tile, dims [OFF, OFF + ND) at compile time:
//   EQ / RQ:  accA[d] += g (za - zb)^2,   accP[d] += g (za - zb)(zda - zdb)   (HAS_ZD: frequency derivatives of periodic features)
//   linear:   accA[d] += g za zb
// with g[2 i + j] the weight of entry (row i, column j).  The accumulators are indexed by constants: they live in registers
// across all tiles of a workgroup and are reduced once, at the end of the kernel.
template <int OFF, int ND, bool LINEAR, bool HAS_ZD, int NA>
__device__ __forceinline__ void grad_dims_static(const double* __restrict__ Za, const double* __restrict__ Zb, const double* __restrict__ Zda,
                                                 const double* __restrict__ Zdb, int ty, int cb, const double (&g)[8], double (&accA)[NA],
                                                 double (&accP)[NA]) {
    if constexpr (ND > 0) {
        const g_d4 za = *reinterpret_cast<const g_d4*>(&Za[OFF * GRAM_LD + 4 * ty]);
        const g_d2 zb = *reinterpret_cast<const g_d2*>(&Zb[OFF * GRAM_LD + cb]);
        double a = accA[OFF];
        if constexpr (LINEAR) {
            _Pragma("unroll")
            for (int i = 0; i < 4; ++i) {
                a = fma(g[2 * i], za[i] * zb[0], a);
                a = fma(g[2 * i + 1], za[i] * zb[1], a);
            }
        } else if constexpr (HAS_ZD) {
            const g_d4 zda = *reinterpret_cast<const g_d4*>(&Zda[OFF * GRAM_LD + 4 * ty]);
            const g_d2 zdb = *reinterpret_cast<const g_d2*>(&Zdb[OFF * GRAM_LD + cb]);
            double pp = accP[OFF];
            _Pragma("unroll")
            for (int i = 0; i < 4; ++i) {
                const double d0 = za[i] - zb[0];
                const double d1 = za[i] - zb[1];
                a = fma(g[2 * i], d0 * d0, a);
                a = fma(g[2 * i + 1], d1 * d1, a);
                pp = fma(g[2 * i], d0 * (zda[i] - zdb[0]), pp);
                pp = fma(g[2 * i + 1], d1 * (zda[i] - zdb[1]), pp);
            }
            accP[OFF] = pp;
        } else {
            _Pragma("unroll")
            for (int i = 0; i < 4; ++i) {
                const double d0 = za[i] - zb[0];
                const double d1 = za[i] - zb[1];
                a = fma(g[2 * i], d0 * d0, a);
                a = fma(g[2 * i + 1], d1 * d1, a);
            }
        }
        accA[OFF] = a;
        grad_dims_static<OFF + 1, ND - 1, LINEAR, HAS_ZD, NA>(Za, Zb, Zda, Zdb, ty, cb, g, accA, accP);
    }
}

// Per-row input-gradient sums of one factor: accX[i][d] += sum_j g[2 i + j] * (za_i - zb_j)  (EQ / RQ)  or  g * zb_j  (linear).
template <int OFF, int ND, bool LINEAR, int NA>
__device__ __forceinline__ void grad_rows_static(const double* __restrict__ Za, const double* __restrict__ Zb, int ty, int cb,
                                                 const double (&g)[8], double (&accX)[4][NA]) {
    if constexpr (ND > 0) {
        const g_d4 za = *reinterpret_cast<const g_d4*>(&Za[OFF * GRAM_LD + 4 * ty]);
        const g_d2 zb = *reinterpret_cast<const g_d2*>(&Zb[OFF * GRAM_LD + cb]);
        _Pragma("unroll")
        for (int i = 0; i < 4; ++i) {
            double a = accX[i][OFF];
            a = fma(g[2 * i], LINEAR ? zb[0] : za[i] - zb[0], a);
            a = fma(g[2 * i + 1], LINEAR ? zb[1] : za[i] - zb[1], a);
            accX[i][OFF] = a;
        }
        grad_rows_static<OFF + 1, ND - 1, LINEAR, NA>(Za, Zb, ty, cb, g, accX);
    }
}

// The two sums of a COSINE factor, g = w * rest * d phi / d sigma:   accA[d] += g (za - zb) / 2   - half the first difference, so that the
// host's rule for the squared-distance factors, d / d scale = -2 A / scale, is the cosine's too (d sigma / d scale_d = -(za - zb) / scale_d) -
// and   accX[i][d] += sum_j g   (d sigma / d za_d = 1 for every dim of the factor).
template <int OFF, int ND, int NA>
__device__ __forceinline__ void grad_dims_cos_static(const double* __restrict__ Za, const double* __restrict__ Zb, int ty, int cb,
                                                     const double (&g)[8], double (&accA)[NA]) {
    if constexpr (ND > 0) {
        const g_d4 za = *reinterpret_cast<const g_d4*>(&Za[OFF * GRAM_LD + 4 * ty]);
        const g_d2 zb = *reinterpret_cast<const g_d2*>(&Zb[OFF * GRAM_LD + cb]);
        double a = accA[OFF];
        _Pragma("unroll")
        for (int i = 0; i < 4; ++i) {
            a = fma(g[2 * i], 0.5 * (za[i] - zb[0]), a);
            a = fma(g[2 * i + 1], 0.5 * (za[i] - zb[1]), a);
        }
        accA[OFF] = a;
        grad_dims_cos_static<OFF + 1, ND - 1, NA>(Za, Zb, ty, cb, g, accA);
    }
}

template <int OFF, int ND, int NA>
__device__ __forceinline__ void grad_rows_cos_static(const double (&g)[8], double (&accX)[4][NA]) {
    if constexpr (ND > 0) {
        _Pragma("unroll")
        for (int i = 0; i < 4; ++i) accX[i][OFF] += g[2 * i] + g[2 * i + 1];
        grad_rows_cos_static<OFF + 1, ND - 1, NA>(g, accX);
    }
}

)
