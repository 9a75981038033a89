// Launcher of gp_batch.hip: B small dense geometric programs
//
//     minimize log sum exp(F0_b x + g0_b)   subject to   log sum exp(Fi_b x + gi_b) <= 0 (i = 1..mnl),  G_b x <= h_b,  A_b x = b_b
//
// by cvxprog.cpl on cp's epigraph form (cvxprog.py:556-1356, 1746-1964, the evaluator of cvxprog.py:2094-2153) with the Newton
// systems of misc.kkt_chol2 (misc.py:1489-1563) at refinement 0, one workgroup per member from x = 0 to its status, the whole
// batch in one launch.
#pragma once
#include "batch_host.hpp"

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace kvx {
// The limits of a member (n variables, N = mnl + 1 + ml orthant rows, l terms), the workgroup, the rows staged per step of the
// assembly of S, the numbers of `stats`, and the halvings of the step after which a line search is given up.
enum { GPB_MAX_N = 63, GPB_MAX_ROWS = 192, GPB_MAX_L = 768, GPB_THREADS = 256, GPB_TILE = 32, GPB_NSTAT = 8, GPB_MAX_HALVINGS = 64 };
// What a member ends with (the `exit` of kvxopt_amd.gpbatch).
enum { GPB_OPTIMAL = 0, GPB_MAXITERS = 1, GPB_SINGULAR = 2, GPB_RANK = 3, GPB_LINESEARCH = 4 };

// BatchArgs with g (l per member) as its c, G ml x n, A p x n and s, z (mnl + 1 + ml) x B with the objective row first.  stats
// (GPB_NSTAT x B): gap, relative gap or NaN, primal and dual objective, primal and dual infeasibility, primal and dual slack.
struct GpBatchArgs : BatchArgs {
    int m, l;                                 // m = mnl + 1 blocks, l = sum K terms
    unsigned short K[GPB_MAX_ROWS];           // the terms of block i; they travel with the arguments
    const double *F;                          // l x n per member, column-major
    int64_t sF;
    double *scratch;                          // gp_batch_scratch_doubles per member: the padded A and the saved line-search state
};

// LDS of one workgroup in bytes, and the doubles of HBM scratch one member needs
size_t gp_batch_lds_bytes(int n, int m, int l, int ml, int p);
int64_t gp_batch_scratch_doubles(int n, int m, int ml, int p);
hipError_t launch_gp_batch(hipStream_t st, const GpBatchArgs &a);

namespace gphost {
// The limits of a member, as the solver's and the derivative's entries refuse them before anything else; on success the blocks
// are placed in `a`.
inline int place_blocks(const char *who, GpBatchArgs &a, int64_t mnl, const int64_t *K)
{
    using batchhost::refuse;
    if (a.B < 1 || a.B > 2147483647) return refuse(who, "1 <= B <= 2147483647 is required");
    if (a.n < 1 || a.n > GPB_MAX_N) return refuse(who, "1 <= n <= 63 is required");
    if (mnl < 0 || mnl + 1 > GPB_MAX_ROWS) return refuse(who, "0 <= mnl and N = mnl + 1 + ml <= 192 are required");
    if (!K) return refuse(who, "the block sizes K are NULL");
    int64_t l = 0;
    for (int64_t i = 0; i <= mnl; i++) {
        if (K[i] < 1) return refuse(who, "every block size K[i] is a positive integer");
        if (K[i] > GPB_MAX_L) return refuse(who, "l = sum(K) <= 768 is required");
        l += K[i];
    }
    if (l > GPB_MAX_L) return refuse(who, "l = sum(K) <= 768 is required");
    if (a.ml < 0) return refuse(who, "ml >= 0 is required");
    if (mnl + 1 + a.ml > GPB_MAX_ROWS) return refuse(who, "0 <= mnl and N = mnl + 1 + ml <= 192 are required");
    if (a.p < 0 || a.p > a.n) return refuse(who, "0 <= p <= n is required");
    a.m = (int)mnl + 1;
    a.l = (int)l;
    for (int i = 0; i < GPB_MAX_ROWS; i++) a.K[i] = i < a.m ? (unsigned short)K[i] : 0;
    return KVX_OK;
}
}  // namespace gphost
}  // namespace kvx
