// Prints the schedule of a Cholesky factorisation (gpar_amd/csrc/potrf_schedule.h) - what a kernel trace of potrf_run would show,
// without a GPU.  Host-only:
//     c++ -std=c++17 -O1 tools/potrf_schedule.cpp -o potrf_schedule
//     potrf_schedule N nf lda batch flags      (flags: 1 GPAR_POTRF_NO_LOOKAHEAD, 2 GPAR_POTRF_UNFUSED)
//     potrf_schedule < shapes                  (one "N nf lda batch flags" per line)
// The matrix is taken as 16-byte aligned with an even batch stride; the GPAR_POTRF_* switches apply as they do in the library.
// One "policy" line (the only one that names the look-ahead setting), then one line per step:
//     step [k0,kend) <panel form> G=<panels> update <none | one | slice+rest> [kend,next_end) <gemm | small>[+tail] rest [next_end,N)[+tail]
#include <stdio.h>

#include "../gpar_amd/csrc/potrf_schedule.h"

using namespace gpar;

static void print_schedule(int N, int nf, int lda, int batch, int flags) {
    PotrfShape sh{N, nf, lda, batch, true, true};
    PotrfPolicy p = potrf_policy(sh, flags);
    printf("shape N=%d nf=%d lda=%d batch=%d flags=%d\n", N, nf, lda, batch, flags);
    if (batch > 1 && !p.lockstep) {   // (potrf_run_batch)
        printf("not lock-step: matrix by matrix\n");
        sh.batch = 1;
        p = potrf_policy(sh, flags);
    }
    printf("policy lookahead=%d fused=%d nbo=%d nbm=%d split=%d pair_rows=%d group=%d prezero=%d lockstep=%d fuse2_on=%d fuse2_rows=%d fuse_max=%d tail_split=%d\n",
           p.lookahead, p.fused, p.nbo, p.nbm, p.split, p.pair_rows, p.group, (int)p.prezero, (int)p.lockstep, (int)p.fuse2_on, p.fuse2_rows,
           p.fuse_max, (int)p.tail_split);
    static const char* const panel[] = {"grouped", "fused-group", "fused", "leaf-batch", "leaf"};
    static const char* const update[] = {"none", "one", "slice+rest"};
    for (int k0 = 0; k0 < nf;) {
        const PotrfStep s = potrf_step(p, sh, k0);
        printf("step [%d,%d) %s%s G=%d update %s", s.k0, s.kend, panel[s.panel], s.leaf_split ? "-split" : "", s.G, update[s.update]);
        if (s.update != POTRF_UPDATE_NONE) printf(" [%d,%d) %s%s", s.kend, s.next_end, s.slice_small ? "small" : "gemm", s.slice_tail ? "+tail" : "");
        if (s.update == POTRF_UPDATE_SLICE_REST) printf(" rest [%d,%d)%s", s.next_end, N, s.rest_tail ? "+tail" : "");
        printf("\n");
        k0 = s.kend;
    }
}

int main(int argc, char** argv) {
    int v[5];
    if (argc == 6) {
        for (int i = 0; i < 5; ++i) v[i] = atoi(argv[i + 1]);
        print_schedule(v[0], v[1], v[2], v[3], v[4]);
        return 0;
    }
    if (argc != 1) {
        fprintf(stderr, "usage: %s N nf lda batch flags   (or shapes on standard input, one per line)\n", argv[0]);
        return 2;
    }
    while (scanf("%d %d %d %d %d", &v[0], &v[1], &v[2], &v[3], &v[4]) == 5) print_schedule(v[0], v[1], v[2], v[3], v[4]);
    return 0;
}
