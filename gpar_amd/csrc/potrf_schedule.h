// The schedule of a blocked Cholesky factorisation (potrf_exec, potrf.h) as data: the policy - every switch and size rule, resolved
// once per call -, and the step that starts at a given column as a pure function of the policy and the shape.  Host-only, nothing
// from HIP: tools/potrf_schedule.cpp prints the steps of a shape without a GPU, tests/test_potrf_schedule.py checks them.
//
// The schedule - panel widths, which steps are grouped, which are fused into one launch, the tile form of every update - is a
// function of the SHAPE (N, nf, lda, alignment) AND OF `batch`, and of nothing else: the same bits with and without look-ahead,
// alone or beside other work, on any stream.  potrf_step does not see the look-ahead setting; that is what guarantees it.  A matrix
// factored inside a lock-step batch takes another summation order than the same matrix alone (pair_rows, fuse2_rows and the
// half-tile rule of the updates all look at the batch): equal to rounding, not to the bit
// (tests/test_full_size_gpu.py::test_batch_geometry_changes_the_summation_order_not_the_factor).
#pragma once
#include <stdlib.h>

#include "../../include/gpar_hip.h"

namespace gpar {

constexpr int POTRF_NBI = 64;          // inner block (diag / strip width)
constexpr int POTRF_SMALL_ROWS = 16;   // an update of at most this many rows is the one-wave kernel (potrf_small_update_kernel)
constexpr int POTRF_TILE_ROWS = 128;   // rows of a tile of the matrix-core update (GEMM_BM)

static int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

struct PotrfShape {
    int N, nf, lda;   // rows, columns to factor, leading dimension
    int batch;        // matrices factored in lock-step
    bool aligned;     // A is 16-byte aligned
    bool even_stride; // the stride between the matrices of a batch is even (0 for a lone matrix)
};

// ---- blocking policy: the only place of the factorisation driver that reads the environment ----------
struct PotrfPolicy {
    int nbo;        // top-level panel width: K of the trailing SYRK
    int nbm;        // mid-level width inside a panel
    int lookahead;  // overlap panel k+1 with the trailing update of panel k on a second stream
    int split;      // factor the diagonal block first, then solve the rows below (see potrf_panel_split)
    int fused;      // factor each top-level panel with the persistent fused kernel (panel.h)
    int pair_rows;  // panels with at least this many rows left are factored in groups (one rank-group*nbo trailing update)
    int group;      // panels per group
    int lockstep_min;     // a batch factors in lock-step (and the hand-off flags are zeroed up front) from this many columns on
    bool prezero;         // hand-off flags of all panels zeroed once, ahead of the first panel (panel.h)
    bool lockstep;        // a batch takes ONE potrf_exec; otherwise it is factored matrix by matrix
    int panel_pairs;      // GPAR_PANEL_PAIRS
    int fuse2_rows;       // a step with at most this many rows left takes two or more panels in one launch (already divided by `batch`)
    bool fuse2_on;
    int fuse_max;         // panels per fused launch, at most
    int small_update;     // updates of at most POTRF_SMALL_ROWS rows by the one-wave kernel
    int la_small_tiles;   // a slice of at most this many 64 x 64 tiles takes the small tile kernel (panel2.h) ...
    int la_small_tiles2;  // ... and this many behind a fused pair of panels (K >= 1024)
    bool tail_split;      // the augmented rows leave the matrix-core updates (potrf_tail_split)
};

static PotrfPolicy potrf_policy(const PotrfShape& sh, int flags) {
    const int N = sh.N, batch = sh.batch;
    const bool pair_rows_set = getenv("GPAR_POTRF_PAIR_ROWS") != nullptr, lookahead_set = getenv("GPAR_POTRF_LOOKAHEAD") != nullptr;
    PotrfPolicy p;
    // wider top-level panels amortise the read-modify-write of the trailing matrix over more flops (measured SYRK
    // rate at n = 16384: K = 128 31, K = 256 42, K = 512 53 TFLOP/s); the panel itself is factored recursively
    // with the fused panel kernel (panel.h) the panel is cheap, so the widest panel it supports wins at every size
    // (measured n = 1024 .. 16384, profiles/r01_potrf_nbo_sweep.txt); the unfused fallback prefers narrower ones
    const int nbo_unfused = N >= 12288 ? 512 : (N >= 6144 ? 256 : (N >= 1536 ? 128 : 64));
    p.fused = env_int("GPAR_POTRF_FUSED", 1);
    p.nbo = p.fused ? 512 : nbo_unfused;
    p.nbm = p.nbo >= 512 ? 128 : 64;
    // Look-ahead: the fused panel kernel of panel k+1 (70.8 KB LDS: fits on a CU beside one SYRK workgroup) runs on
    // the caller's stream under the trailing update of panel k on a low-priority side stream.  Pays once the
    // trailing updates are long enough to hide it (measured with half-tile workgroups for the small launches: n = 5120
    // 3.12 -> 2.97 ms, 6144 4.06 -> 3.81, 8192 6.75 -> 5.98; a wash at 4096, a loss at 3072).  The unfused fallback keeps
    // it off (its small kernels starve behind the SYRK).
    // (round 4, with the small look-ahead update kernel and two panels per launch: n = 3072 1.152 -> 1.097 ms, 4096 1.767 -> 1.631, 4600
    // 2.248 -> 1.96, a wash at 2048: profiles/r04_exp_potrf_fuse2.txt)
    p.lookahead = (p.fused && N >= 2560) ? 1 : 0;
    p.nbo = env_int("GPAR_POTRF_NBO", p.nbo);
    p.nbm = env_int("GPAR_POTRF_NBM", p.nbm);
    p.lookahead = env_int("GPAR_POTRF_LOOKAHEAD", p.lookahead);
    p.split = env_int("GPAR_POTRF_SPLIT", 0);
    // n = 8192 measured slower grouped (5.38 vs 5.19 ms alone).  From N = 12288 on panels stay grouped until 6144 rows are left:
    // with two factorisations in flight (the pipelined C3 evaluation) the longer serial stretch hides under the other stream's
    // updates, 197.9 -> 194.9 ms per evaluation; alone it costs 0.5 % at n = 16384 (tools/exp_pair_rows.sh).  The rule depends
    // on the size only, so that a factorisation returns the same bits whatever runs beside it.
    p.pair_rows = env_int("GPAR_POTRF_PAIR_ROWS", N >= 12288 ? 6144 : 9216);
    p.group = env_int("GPAR_POTRF_GROUP", 3);
    if (p.nbo < 64) p.nbo = 64;
    if (p.nbm < 64) p.nbm = 64;
    // a LONE large factorisation stops grouping earlier (from 7680 rows on the steps are single panels with look-ahead, the last 7680 rows
    // then one fused launch of fifteen panels): n = 16384 25.10 -> 24.97 ms, n = 12288 11.84 -> 11.79; a lock-step batch keeps 6144 (C3:
    // 180.2 against 180.7 ms with 7680; profiles/r05_exp_fuse_rows.txt)
    if (batch == 1 && N >= 12288 && !pair_rows_set) p.pair_rows = 7680;
    // a wide lock-step batch of large matrices groups its panels down to 2560 rows: its rank-1536 updates are `batch` times a lone
    // matrix's and hide the longer serial stretch, and spare the launch-wide read and write of the trailing matrices two times in three
    // (C5, 16 x 8193: 55.5 -> 53.7 ms; 12 x 8192 40.8 -> 39.5, 12 x 10240 73.7 -> 72.5; batches of 2-8 and matrices below 8192 rows:
    // equal or slower, C3 - 8 x 16385 - equal: profiles/r05_exp_batch_pair.txt)
    if (batch >= 12 && N >= 8192 && !pair_rows_set) p.pair_rows = 2560;
    // the caller runs several factorisations at once (three or more layer streams): each one's look-ahead side stream would
    // add a queue to an already over-subscribed chip (C5, three streams at n = 8192: 78 -> 72 ms per evaluation without)
    if ((flags & GPAR_POTRF_NO_LOOKAHEAD) && !lookahead_set) p.lookahead = 0;
    if (flags & GPAR_POTRF_UNFUSED) {   // the caller's retry after a hand-off timeout: separate leaf kernels, nothing spins
        p.fused = 0;
        p.lookahead = 0;
        p.nbo = nbo_unfused;
        p.nbm = p.nbo >= 512 ? 128 : 64;
    }
    // lock-step batch: its updates are `batch` times longer than one matrix's - long enough to hide a panel kernel behind at any N
    if (batch > 1 && p.fused && !lookahead_set) p.lookahead = env_int("GPAR_POTRF_BATCH_LOOKAHEAD", 1);
    const bool even = (sh.lda % 2 == 0) && sh.even_stride && sh.aligned;
    p.lockstep_min = env_int("GPAR_POTRF_LOCKSTEP_MIN", 1);
    p.prezero = p.fused && env_int("GPAR_POTRF_PREZERO", 1) && sh.nf >= p.lockstep_min;
    // Anything the fused path cannot take (alignment, unfused retry) is factored matrix by matrix.
    p.lockstep = batch > 1 && p.fused && p.nbo % 64 == 0 && even && sh.nf >= p.lockstep_min;
    // (The last columns through ONE panel kernel of up to 16 column blocks - GPAR_POTRF_TAIL, round 3 - measured slower: n = 1024 0.43
    // against 0.33 ms, C4 18.1 -> 19.7 ms; retired in round 6.)
    // Two or more panels in ONE launch (potrf_group_kernel, panel2.h; at most GPAR_POTRF_FUSE_MAX) once the rows that are left make a step latency-bound: at most
    // GPAR_POTRF_FUSE2_ROWS rows from the step's first column on (a lock-step batch: GPAR_POTRF_FUSE2_BATCH_ROWS over the batch - it
    // fills the chip sooner).  Measured (tools/exp_potrf_fuse2.py, profiles/r04_exp_potrf_fuse2.txt): lone n = 1024 / 2048 / 3072 /
    // 4096 0.333 -> 0.310 / 0.753 -> 0.651 / 1.246 -> 1.146 / 1.869 -> 1.765 ms with every step fused; where a trailing update runs
    // beside the panels on the side stream (look-ahead, N >= 2560) the waiting tile workgroups cost it compute-unit slots, and only the
    // last ~2500 rows gain (n = 8192 5.04 -> 4.92 ms, 5.30 fused from 5120 rows on; n = 4096 1.640 -> 1.579, 3072 1.130 -> 1.079, 2560
    // 0.924 -> 0.866; n = 4600 1.94 / 1.95 / 2.00 / 2.18 ms fused never / from 2560 / 4200 / 5120 rows; n = 16384 inside the noise); a lock-step batch of
    // four gains 1 % on its last pair of panels and loses when more are fused (4 x 4096: 2.74 -> 2.71 / 2.84 ms).  Geometry only, like
    // every other rule here: the same bits with and without look-ahead.
    // Round 5 (the next team's rows updated tile by tile, progressive hand-off): a factorisation of up to 5200 rows is ONE launch (n = 4096
    // 1.56 -> 1.26 ms); a larger one fuses its last eight panels (profiles/r05_exp_fuse_rows.txt: n = 8192 4.77 / 4.72 / 4.60 / 4.71 / 4.66 / 4.79 ms
    // fused from 5200 / 4700 / 4200 / 3600 / 3100 / 2560 rows; n = 5632 .. 16384 all flat within 2 % between 3600 and 4700).
    // With the launch's tiles taking published column blocks without polling and fetching the next one under the current product
    // (grp_la_tile: a tile's share of the earlier panels 6 -> ~3.5 us per column block) a lock-step batch gains from fusing too: four matrices
    // of 4096 rows in ONE launch 3.55 -> 2.81 ms against 3.05 with their last 1536 rows fused (rows x batch <= 16500: C2, 4 x 3072 1.82 ->
    // 1.62 ms, 8 x 2048 1.55 -> 1.36; C3 and C5 - the last 2048 / 1024 rows - unchanged; profiles/r05_exp_batch_fuse.txt).
    p.fuse2_rows = batch == 1 ? env_int("GPAR_POTRF_FUSE2_ROWS", N <= 5200 ? 5200 : (N >= 12288 ? 8300 : 4200))
                              : env_int("GPAR_POTRF_FUSE2_BATCH_ROWS", 16500) / batch;
    p.panel_pairs = env_int("GPAR_PANEL_PAIRS", 1);
    p.fuse2_on = p.fused && p.prezero && p.nbo == 512 && p.panel_pairs && even && p.fuse2_rows > 0;
    // (more than two panels per launch add little - between panels inside a launch the next team waits ~45 us for the last column
    // blocks of its own rows, which the bulk row blocks of the panel before finish behind the chain - : n = 1536 0.497 -> 0.452 ms with
    // three, n = 2048 0.647 -> 0.637 with four, nothing beyond; 4 measured equal or better than 2 / 3 / 8 at every size)
    // (from N = 12288 on the last sixteen panels: with the faster update tiles n = 12288 12.0-12.1 -> 11.9 ms, n = 16384 25.4-25.5 -> 25.1-25.2;
    // n = 8192 4.66-4.70 / 4.59 / 4.74-4.77 ms fused from 4200 / 6200 / 8300 rows: profiles/r05_exp_fuse_rows.txt)
    p.fuse_max = env_int("GPAR_POTRF_FUSE_MAX", N >= 12288 ? 16 : 10);
    p.small_update = env_int("GPAR_POTRF_SMALL_UPDATE", 1);
    p.la_small_tiles = env_int("GPAR_POTRF_LA_SMALL_TILES", 512);
    p.la_small_tiles2 = env_int("GPAR_POTRF_LA_SMALL_TILES2", 2048);
    // Tail split: a matrix with a short unfactored tail - 0 < N - nf <= POTRF_SMALL_ROWS, the augmented row(s) [y^T, 0] of the log
    // marginal likelihood; not the posterior's n* appended rows - gave every matrix-core update below a last tile row for those few
    // rows: (T + 1)(T + 2) / 2 tiles where T (T + 1) / 2 cover the factor, and the surplus ones end the launch.  An update whose first
    // row is `r0` stops at row nf, and the tail rows receive the same rank-K update from potrf_tail_update, whenever leaving them out
    // removes a tile row (potrf_tail_split).  Geometry only.
    // Lock-step batches only: there the surplus tiles are `batch` times as many and the panel chain hides under the batched update.  In a
    // LONE factorisation the companion in front of every panel lengthens the serial chain by what the tile row saved or more (measured,
    // parent / split: n = 16384 25.05 / 25.06 ms, n = 8192 4.63 / 4.68; batches of 2 / 4 / 16 at n = 8192 8.4 / 8.4, 13.8 / 13.6, 48.4 / 47.4 ms,
    // 3 x 6656 6.58 / 6.45, 2 x 16384 47.5 / 47.2, C3 - 8 x 16384 - 182.3 / 179.9: profiles/r08_tail_split_bench.txt).
    p.tail_split = batch > 1 && N - sh.nf > 0 && N - sh.nf <= POTRF_SMALL_ROWS;
    return p;
}

// ---- one step ----------
enum PotrfPanelForm {
    POTRF_PANEL_GROUPED,      // G panel launches back to back, each after an update of its columns by the group's earlier panels
    POTRF_PANEL_FUSED_GROUP,  // G panels in one launch (potrf_group_fused)
    POTRF_PANEL_FUSED,        // one fused panel launch
    POTRF_PANEL_LEAF_BATCH,   // leaf kernels, one launch each for the whole batch
    POTRF_PANEL_LEAF,         // leaf kernels, matrix by matrix (`leaf_split`: diagonal block first, then the rows below)
};
enum PotrfUpdateForm {
    POTRF_UPDATE_NONE,        // no rows below the step
    POTRF_UPDATE_ONE,         // one launch over everything that is left
    POTRF_UPDATE_SLICE_REST,  // the next step's columns [kend, next_end), then everything from next_end on
};
struct PotrfStep {
    int k0, kend;             // the step factors columns [k0, kend)
    PotrfPanelForm panel;
    int G;                    // panels of a grouped step or fused launch (else 1)
    bool leaf_split;
    PotrfUpdateForm update;
    int next_end;             // end of the first update launch: the next step's columns (N: it is the only one)
    bool slice_small;         // [kend, next_end) by the small tile kernel (panel2.h), else the matrix-core update
    bool slice_tail;          // the slice stops at row nf; potrf_tail_update follows it
    bool rest_tail;           // the rest stops at row nf; potrf_tail_update follows the NEXT step's panel launches
};

// Early in the factorisation `group` panels are factored back to back (each after a narrow update of its own columns by the
// ones before) and the rest of the matrix then receives ONE rank-group*nbo update: the trailing update reads and writes every
// remaining element once per group instead of once per 512 columns, and a K = 1024 SYRK runs ~8 % faster than two K = 512 ones.
// The price is a longer serial stretch per step, so the grouping stops once the trailing update is too short to hide it (`pair_rows`).
static inline bool potrf_groupable(const PotrfPolicy& p, const PotrfShape& sh, int k) {
    return p.group > 1 && k > 0 && p.fused && p.nbo % 64 == 0 && k + p.group * p.nbo <= sh.nf && (sh.N - k) >= p.pair_rows && (k % 2 == 0) &&
           (sh.lda % 2 == 0) && sh.aligned;
}

// panels the step at column k takes in one launch (0: the step is not fused)
static inline int potrf_fuse_panels(const PotrfPolicy& p, const PotrfShape& sh, int k) {
    if (!p.fuse2_on || potrf_groupable(p, sh, k) || k % 64 != 0 || sh.N - k > p.fuse2_rows) return 0;
    int G = (sh.nf - k) / p.nbo;
    if (G > p.fuse_max) G = p.fuse_max;
    return G >= 2 ? G : 0;
}

// end of the columns a step at column k claims (before the ragged-tail cut of potrf_step)
static inline int potrf_span_end(const PotrfPolicy& p, const PotrfShape& sh, int k) {
    if (potrf_groupable(p, sh, k)) return k + p.group * p.nbo;
    const int G = potrf_fuse_panels(p, sh, k);
    if (G > 0) return k + G * p.nbo;
    return k + p.nbo >= sh.nf ? sh.nf : k + p.nbo;
}

// Does a matrix-core update whose first row is `r0` leave the augmented rows to potrf_tail_update?  Whenever that removes a tile
// row.  (Where it removes none - nf - r0 not within N - nf of a multiple of 128 from below - the update keeps all rows: the split
// would add a launch and save nothing.)
static inline bool potrf_tail_split(const PotrfPolicy& p, const PotrfShape& sh, int r0) {
    const int T = POTRF_TILE_ROWS;
    return p.tail_split && r0 < sh.nf && (sh.N - r0 + T - 1) / T > (sh.nf - r0 + T - 1) / T;
}

// Does the update of the NEXT step's columns [kend, la_end) take the one-tile-per-workgroup kernel (panel2.h) instead of the GEMM?
// While it has at most GPAR_POTRF_LA_SMALL_TILES 64 x 64 tiles over the whole batch: then its duration is one tile's, and the
// small kernel's tile is several times shorter.
static inline bool potrf_slice_small(const PotrfPolicy& p, const PotrfShape& sh, int k0, int kend, int la_end) {
    const int cols = la_end - kend, K = kend - k0;
    if (cols <= 0 || cols % 64 != 0 || K <= 0 || K % 64 != 0 || (sh.lda & 1) || !sh.aligned || !sh.even_stride || (k0 & 1) || sh.N - kend <= POTRF_SMALL_ROWS)
        return false;
    const int nc = cols / 64, tr = (sh.N - kend + 63) / 64;
    if (tr < nc) return false;
    const long long tiles = ((long long)nc * (nc + 1) / 2 + (long long)(tr - nc) * nc) * sh.batch;
    // behind a fused pair of panels (K >= 1024, potrf_group_kernel) a tile is 16 chunks and the alternative a K = 1024 GEMM tile of
    // ~200 us: several rounds of small tiles still win
    return tiles <= (K >= 1024 ? p.la_small_tiles2 : p.la_small_tiles);
}

// The step that starts at column k0 < nf.
static inline PotrfStep potrf_step(const PotrfPolicy& p, const PotrfShape& sh, int k0) {
    const int N = sh.N, nf = sh.nf;
    PotrfStep s{};
    s.k0 = k0;
    s.kend = potrf_span_end(p, sh, k0);
    // a ragged tail (nf not a multiple of 64) becomes its own narrow panel so the wide part stays fusable
    if (p.fused && (s.kend - k0) > 64 && (s.kend - k0) % 64 != 0) s.kend = k0 + (s.kend - k0) / 64 * 64;
    const int w = s.kend - k0;
    s.G = 1;
    if (potrf_groupable(p, sh, k0)) {
        s.panel = POTRF_PANEL_GROUPED;
        s.G = p.group;
    } else if (potrf_fuse_panels(p, sh, k0) > 0) {
        s.panel = POTRF_PANEL_FUSED_GROUP;
        s.G = potrf_fuse_panels(p, sh, k0);
    } else if (p.fused && w % 64 == 0 && w <= 1024 && N - k0 >= 64 && (k0 % 2 == 0) && (sh.lda % 2 == 0) && sh.aligned) {
        s.panel = POTRF_PANEL_FUSED;
    } else if (sh.batch > 1 && w <= POTRF_NBI && !p.split) {   // a narrow (ragged last) panel of a lock-step batch
        s.panel = POTRF_PANEL_LEAF_BATCH;
    } else {
        s.panel = POTRF_PANEL_LEAF;
        s.leaf_split = p.split != 0;
    }
    // The update.  While a further step follows, two launches: the columns it factors (one panel, or all of a group), then everything
    // to their right - the look-ahead schedule's two launches whether or not look-ahead is on: the update kernel picks its tile shape
    // by the size of the launch, and a tile that preloads C rounds differently from one that adds it at the end, so ONE launch over
    // everything would not return the same bits.  Behind the last step (the augmented rows, the posterior's appended rows), or when
    // the next step's columns are all that is left, one launch.
    s.next_end = s.kend < nf ? potrf_span_end(p, sh, s.kend) : N;
    s.update = s.kend >= N ? POTRF_UPDATE_NONE : (s.next_end < N ? POTRF_UPDATE_SLICE_REST : POTRF_UPDATE_ONE);
    if (s.update != POTRF_UPDATE_NONE) {
        s.slice_small = s.kend < nf && potrf_slice_small(p, sh, k0, s.kend, s.next_end);
        s.slice_tail = !s.slice_small && potrf_tail_split(p, sh, s.kend);
        s.rest_tail = s.update == POTRF_UPDATE_SLICE_REST && potrf_tail_split(p, sh, s.next_end);
    }
    return s;
}

}   // namespace gpar
