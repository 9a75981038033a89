// Launcher of lp_batch.hip: B small dense linear programs
//
//     minimize c_b'x   subject to   G_b x + s = h_b,  s >= 0,  A_b x = b_b
//
// by the self-dual embedding of conelp on the orthant (coneprog.py:662-1436 with the Newton systems of misc.kkt_chol2,
// misc.py:1395-1563, its F['singular'] repair included), one workgroup per member from the starting point to its status or
// its infeasibility certificate, the whole batch in one launch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace kvx {
// The limits of a member, the workgroup, the rows of G staged per step of the assembly of S, and the numbers of `stats`.
enum { LPB_MAX_N = 64, LPB_MAX_ML = 512, LPB_THREADS = 256, LPB_TILE = 32, LPB_NSTAT = 10 };
// What a member ends with (the `exit` of kvxopt_amd.lpbatch).
enum { LPB_OPTIMAL = 0, LPB_MAXITERS = 1, LPB_SINGULAR = 2, LPB_RANK = 3, LPB_PRIMAL_INFEASIBLE = 4, LPB_DUAL_INFEASIBLE = 5 };

struct LpBatchArgs {
    int64_t B;
    int n, ml, p;
    // device pointers; matrices dense and column-major per member (G ml x n; A p x n); s*: distance between two members in
    // doubles, 0: one for all
    const double *c, *G, *h, *A, *b;
    int64_t sc, sG, sh, sA, sb;
    int maxiters;
    double abstol, reltol, feastol;
    // results: x (n x B), y (p x B), s, z (ml x B), stats (LPB_NSTAT x B: gap, relative gap, primal and dual objective, primal
    // and dual infeasibility, primal and dual slack, residual as primal and as dual infeasibility certificate; NaN where the
    // reference returns None), iterations and exit (B each)
    double *x, *y, *s, *z, *stats;
    int64_t *iters, *exitc;
};

// LDS of one workgroup in bytes: S, the region X and K share with the staged rows of G, and every vector of a member.
size_t lp_batch_lds_bytes(int n, int ml, int p);
hipError_t launch_lp_batch(hipStream_t st, const LpBatchArgs &a);
}  // namespace kvx
