// Launcher of qp_batch.hip: B small dense quadratic programs
//
//     minimize (1/2) x'P_b x + q_b'x   subject to   G_b x <= h_b,  A_b x = b_b
//
// by the interior-point method of coneqp on the orthant (coneprog.py:2044-2547 with the Newton systems of misc.kkt_chol2,
// misc.py:1489-1563), one workgroup per member from the starting point to its status, the whole batch in one launch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace kvx {
// The limits of a member, the workgroup, the rows of G staged per step of the assembly of S, and the numbers of `stats`.
enum { QPB_MAX_N = 64, QPB_MAX_ML = 512, QPB_THREADS = 256, QPB_TILE = 32, QPB_NSTAT = 8 };
// What a member ends with (the `exit` of kvxopt_amd.qpbatch).
enum { QPB_OPTIMAL = 0, QPB_MAXITERS = 1, QPB_SINGULAR = 2, QPB_RANK = 3 };

struct QpBatchArgs {
    int64_t B;
    int n, ml, p;
    // device pointers; matrices dense and column-major per member (P n x n, its lower triangle read; G ml x n; A p x n);
    // s*: distance between two members in doubles, 0: one for all
    const double *P, *q, *G, *h, *A, *b;
    int64_t sP, sq, sG, sh, sA, sb;
    int maxiters;
    double abstol, reltol, feastol;
    int correction;
    // results: x (n x B), y (p x B), s, z (ml x B), stats (QPB_NSTAT x B: gap, relative gap or NaN, primal and dual objective,
    // primal and dual infeasibility, primal and dual slack), iterations and exit (B each)
    double *x, *y, *s, *z, *stats;
    int64_t *iters, *exitc;
};

// LDS of one workgroup in bytes: S, the region X and K share with the staged rows of G, and every vector of a member.
size_t qp_batch_lds_bytes(int n, int ml, int p);
hipError_t launch_qp_batch(hipStream_t st, const QpBatchArgs &a);
}  // namespace kvx
