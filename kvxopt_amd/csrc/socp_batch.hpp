// Launcher of socp_batch.hip: B small dense second-order-cone programs
//
//     minimize c_b'x   subject to   G_b x + s = h_b,  s in K = R^ml_+ x Q^{q_0} x ... x Q^{q_{nq-1}},  A_b x = b_b
//
// by the self-dual embedding of conelp (coneprog.py:662-1436 with the Newton systems of misc.kkt_chol2, misc.py:1395-1563, its
// F['singular'] repair included, on Gs = W^-T G with the Nesterov-Todd scaling of the 'q' blocks), one workgroup per member from
// the starting point to its status or its infeasibility certificate, the whole batch in one launch.  The cone is the same for
// every member.
#pragma once
#include "batch_host.hpp"

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace kvx {
// The limits of a member (N = ml + sum q_k rows), the workgroup, the rows of W^-T G staged per step of the assembly of S, the
// order up to which one thread adds a cone's column of (J v)'G by itself, and the numbers of `stats`.
enum { SOCPB_MAX_N = 64, SOCPB_MAX_ROWS = 512, SOCPB_MAX_NQ = 128, SOCPB_THREADS = 256, SOCPB_TILE = 32, SOCPB_SERIAL = 16,
       SOCPB_NSTAT = 10 };
// What a member ends with (the `exit` of kvxopt_amd.socpbatch): the CONELP_ codes of batch_conelp.hpp.

// BatchArgs with G N x n and s, z N x B.  stats (SOCPB_NSTAT x B) as in lp_batch.hpp; the slacks are -max_step over the whole
// cone.
struct SocpBatchArgs : BatchArgs {
    int nq, N;
    unsigned short q[SOCPB_MAX_NQ];           // the cone orders travel with the kernel's arguments: no device copy of them
};

// LDS of one workgroup in bytes: at most 150 KiB on the box of the limits above.
size_t socp_batch_lds_bytes(int n, int N, int nq, int p);
hipError_t launch_socp_batch(hipStream_t st, const SocpBatchArgs &a);
}  // namespace kvx
