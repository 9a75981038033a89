// Launcher of sdp_batch.hip: B small dense semidefinite programs
//
//     minimize c_b'x   subject to   G_b x + s = h_b,  s in K = R^ml_+ x S^{m_0}_+ x ... x S^{m_{ns-1}}_+,  A_b x = b_b
//
// by the self-dual embedding of conelp (coneprog.py:662-1436 with the Newton systems of misc.kkt_chol2, misc.py:1395-1563, its
// F['singular'] repair included, on Gs = W^-T G with the Nesterov-Todd scaling of the 's' blocks), one workgroup per member from
// the starting point to its status or its infeasibility certificate, the whole batch in one launch.  The cone is the same for
// every member.  An 's' block is its m_k x m_k matrix in column-major order; only its lower triangle is read in G and h.
#pragma once
#include "batch_host.hpp"

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace kvx {
// The limits of a member (N = ml + sum m_k^2 rows), the workgroup, the rows of W^-T G staged per step of the assembly of S, the
// cap on the sweeps of one Jacobi iteration, and the numbers of `stats`.
enum { SDPB_MAX_N = 64, SDPB_MAX_ROWS = 384, SDPB_MAX_NS = 32, SDPB_MAX_M = 16, SDPB_THREADS = 256, SDPB_TILE = 32, SDPB_SWEEPS = 60,
       SDPB_NSTAT = 10 };
// What a member ends with (the `exit` of kvxopt_amd.sdpbatch): the CONELP_ codes of batch_conelp.hpp.

// BatchArgs with G N x n and s, z N x B, 's' blocks as full symmetric matrices.  stats (SDPB_NSTAT x B) as in lp_batch.hpp; the
// slacks are -max_step over the whole cone.
struct SdpBatchArgs : BatchArgs {
    int ns, N, Nd, Np;                        // Nd = ml + sum m_k (lmbda), Np = ml + sum m_k (m_k + 1) / 2 (packed rows)
    unsigned char m[SDPB_MAX_NS];             // the block orders travel with the kernel's arguments: no device copy of them
};

// LDS of one workgroup in bytes: at most 150 KiB on the box of the limits above.
size_t sdp_batch_lds_bytes(int n, int ml, int ns, const unsigned char *m, int p);
hipError_t launch_sdp_batch(hipStream_t st, const SdpBatchArgs &a);
}  // namespace kvx
