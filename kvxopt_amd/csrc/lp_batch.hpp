// Launcher of lp_batch.hip: B small dense linear programs
//
//     minimize c_b'x   subject to   G_b x + s = h_b,  s >= 0,  A_b x = b_b
//
// by the self-dual embedding of conelp on the orthant (coneprog.py:662-1436 with the Newton systems of misc.kkt_chol2,
// misc.py:1395-1563, its F['singular'] repair included), one workgroup per member from the starting point to its status or
// its infeasibility certificate, the whole batch in one launch.
#pragma once
#include "batch_host.hpp"

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace kvx {
// The limits of a member, the workgroup, the rows of G staged per step of the assembly of S, and the numbers of `stats`.
enum { LPB_MAX_N = 64, LPB_MAX_ML = 512, LPB_THREADS = 256, LPB_TILE = 32, LPB_NSTAT = 10 };
// What a member ends with (the `exit` of kvxopt_amd.lpbatch): the CONELP_ codes of batch_conelp.hpp.

// BatchArgs with G ml x n and s, z ml x B.  stats (LPB_NSTAT x B): gap, relative gap, primal and dual objective, primal and dual
// infeasibility, primal and dual slack, residual as primal and as dual infeasibility certificate; NaN where the reference
// returns None.
struct LpBatchArgs : BatchArgs {};

// LDS of one workgroup in bytes: S, the region X and K share with the staged rows of G, and every vector of a member.
size_t lp_batch_lds_bytes(int n, int ml, int p);
hipError_t launch_lp_batch(hipStream_t st, const LpBatchArgs &a);
}  // namespace kvx
