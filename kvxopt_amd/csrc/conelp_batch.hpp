// Launcher of conelp_batch.hip: B small dense cone programs
//
//     minimize c_b'x   subject to   G_b x + s = h_b,  s in K = R^ml_+ x Q^{q_0} x ... x S^{m_0}_+ x ...,  A_b x = b_b
//
// by the self-dual embedding of conelp (coneprog.py:662-1436 with the Newton systems of misc.kkt_chol2, misc.py:1395-1563, its
// F['singular'] repair included, on Gs = W^-T G with the Nesterov-Todd scaling of the 'q' and the 's' blocks), one workgroup per
// member from the starting point to its status or its infeasibility certificate, the whole batch in one launch.  The cone is the
// same for every member and has all three kinds at once: the 'l' rows, then the 'q' cones, then every 's' block as its
// m_k x m_k matrix in column-major order, of which only the lower triangle is read in G and h.
#pragma once
#include "batch_host.hpp"

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace kvx {
// The limits of a member (N = ml + sum q_k + sum m_k^2 rows), the workgroup, the rows of W^-T G staged per step of the assembly
// of S, the order up to which one thread adds a cone's column of (J v)'G by itself, the cap on the sweeps of one Jacobi
// iteration, and the numbers of `stats`.
enum { CONEB_MAX_N = 64, CONEB_MAX_ROWS = 384, CONEB_MAX_NQ = 128, CONEB_MAX_NS = 32, CONEB_MAX_M = 16, CONEB_THREADS = 256,
       CONEB_TILE = 32, CONEB_SERIAL = 16, CONEB_SWEEPS = 60, CONEB_NSTAT = 10 };
// What a member ends with (the `exit` of kvxopt_amd.conelpbatch): the CONELP_ codes of batch_conelp.hpp.

// BatchArgs with G N x n and s, z N x B, 's' blocks as full symmetric matrices.  stats (CONEB_NSTAT x B) as in lp_batch.hpp; the
// slacks are -max_step over the whole cone.
struct ConelpBatchArgs : BatchArgs {
    int nq, ns, Ms, N, Nd, Np;                // Ms = ml + sum q_k (the first 's' row), Nd = Ms + sum m_k (lmbda),
                                              // Np = Ms + sum m_k (m_k + 1) / 2 (packed rows)
    unsigned short q[CONEB_MAX_NQ];           // the cone and block orders travel with the kernel's arguments: no device copy
    unsigned char m[CONEB_MAX_NS];
};

// LDS of one workgroup in bytes: at most 160 KiB on the box of the limits above (DESIGN 17 has the formula and the corners).
size_t conelp_batch_lds_bytes(int n, int ml, int nq, const unsigned short *q, int ns, const unsigned char *m, int p);
hipError_t launch_conelp_batch(hipStream_t st, const ConelpBatchArgs &a);
}  // namespace kvx
