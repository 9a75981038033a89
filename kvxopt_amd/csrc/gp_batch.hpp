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
}  // namespace kvx
