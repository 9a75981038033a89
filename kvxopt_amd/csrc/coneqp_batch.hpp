// Launcher of coneqp_batch.hip: B small dense cone QPs
//
//     minimize (1/2) x'P_b x + q_b'x   subject to   G_b x + s = h_b,  s in K = R^ml_+ x Q^{q_0} x ... x S^{m_0}_+ x ...,  A_b x = b_b
//
// by the interior-point method of coneqp (coneprog.py:2044-2547 with the Newton systems of misc.kkt_chol, H = P, on Gs = W^-T G
// with the Nesterov-Todd scaling of the 'q' and the 's' blocks), one workgroup per member from the starting point to its status,
// the whole batch in one launch.  The cone, its limits and its rows are those of conelp_batch.hpp.
#pragma once
#include "conelp_batch.hpp"

namespace kvx {
enum { CONEQPB_NSTAT = 8 };                   // the numbers of `stats`, as in qp_batch.hpp
// What a member ends with (the `exit` of kvxopt_amd.coneqpbatch): the CONEQP_ codes of batch_coneqp.hpp, those of qp_batch.hpp.

// ConelpBatchArgs with q as its c.  stats (CONEQPB_NSTAT x B) as in qp_batch.hpp; the slacks are -max_step over the whole cone.
struct ConeqpBatchArgs : ConelpBatchArgs {
    const double *P;                          // n x n per member, column-major, its lower triangle read
    int64_t sP;
    int correction;
};

// LDS of one workgroup in bytes: below conelp_batch_lds_bytes at every shape (DESIGN 18 has the formula and the corners).
size_t coneqp_batch_lds_bytes(int n, int ml, int nq, const unsigned short *q, int ns, const unsigned char *m, int p);
hipError_t launch_coneqp_batch(hipStream_t st, const ConeqpBatchArgs &a);
}  // namespace kvx
