// Launcher of qp_batch.hip: B small dense quadratic programs
//
//     minimize (1/2) x'P_b x + q_b'x   subject to   G_b x <= h_b,  A_b x = b_b
//
// by the interior-point method of coneqp on the orthant (coneprog.py:2044-2547 with the Newton systems of misc.kkt_chol2,
// misc.py:1489-1563), one workgroup per member from the starting point to its status, the whole batch in one launch.
#pragma once
#include "batch_host.hpp"

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace kvx {
// The limits of a member, the workgroup, the rows of G staged per step of the assembly of S, and the numbers of `stats`.
enum { QPB_MAX_N = 64, QPB_MAX_ML = 512, QPB_THREADS = 256, QPB_TILE = 32, QPB_NSTAT = 8 };
// What a member ends with (the `exit` of kvxopt_amd.qpbatch).
enum { QPB_OPTIMAL = 0, QPB_MAXITERS = 1, QPB_SINGULAR = 2, QPB_RANK = 3 };

// BatchArgs with q as its c, G ml x n and s, z ml x B.  stats (QPB_NSTAT x B): gap, relative gap or NaN, primal and dual
// objective, primal and dual infeasibility, primal and dual slack.
struct QpBatchArgs : BatchArgs {
    const double *P;                          // n x n per member, column-major, its lower triangle read
    int64_t sP;
    int correction;
};

// LDS of one workgroup in bytes: S, the region X and K share with the staged rows of G, and every vector of a member.
size_t qp_batch_lds_bytes(int n, int ml, int p);
hipError_t launch_qp_batch(hipStream_t st, const QpBatchArgs &a);
}  // namespace kvx
