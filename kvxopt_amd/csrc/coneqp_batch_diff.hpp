// Launcher of coneqp_batch_diff.hip: derivatives of B solved small dense cone QPs (coneqp_batch.hpp) with respect to their data.
// Differentiating the KKT conditions of member b gives a linear system with the matrix
//
//     [ P  A'  G'   ]
//     [ A  0   0    ]        W the Nesterov-Todd scaling of (s, z),
//     [ G  0  -W'W  ]
//
// the Newton matrix k_coneqp_batch factors at every iteration.  On the 'q' and 's' rows W'W linearises the complementarity
// condition exactly only on the central path (lmbda o lmbda = mu e), and the point k_coneqp_batch returns is not on it.  So
// k_coneqp_batch_diff first takes at most `centering` centring steps from the returned x, y, s, z -- a Newton step of coneqp with
// sigma = 1, no Mehrotra term and mu = s'z / degree of the incoming point, the step length min(1, 0.99 / t), the scaling updated
// as the solver updates it -- until |lmbda o lmbda - mu e|_2 <= centol mu, and then solves the system once at the centred point
// with `refinement` steps of iterative refinement on the full system (qp_batch_diff.hpp has the scheme), for the right-hand
// side of a vector-Jacobian product (reverse mode) or of a Jacobian-vector product (forward mode).  One workgroup per member,
// one launch; launch_batch_outer_sum (qp_batch_diff.hpp) adds the gradient of a matrix all members share.
#pragma once
#include "coneqp_batch.hpp"
#include "qp_batch_diff.hpp"

namespace kvx {
enum { CQD_MAX_CENTERING = 16 };
// What a member ends with (the `exit` of kvxopt_amd.coneqpbatchdiff): done; skipped, since its exitcode of coneqp_batch is not 0;
// the scaling or a pivot failed, or a value is not finite; not centred within `centering` steps.  1, 2 and 3 leave zeros.
enum { CQD_DONE = 0, CQD_SKIPPED = 1, CQD_FAILED = 2, CQD_NOT_CENTRED = 3 };

// ConeqpBatchArgs with, as inputs, the solution x (n x B), y (p x B), s, z (N x B, 's' blocks full symmetric matrices) of
// coneqp_batch; c, h, b enter the centring steps; the tolerances, maxiters, stats, iters and correction do not enter; exitc is
// the exit of the derivative.
struct ConeqpDiffArgs : ConeqpBatchArgs {
    const int64_t *solexit;                   // exitcode of coneqp_batch, B
    int mode, refinement, centering;          // mode: QPD_VJP or QPD_JVP
    double centol;
    double *centrality;                       // B: the final |lmbda o lmbda - mu e|_2 / mu; NaN for a member with exit 1 or 2
    int64_t *steps;                           // B: the centring steps taken
    // The centred point, written where the pointer is not null (the sums of the shared matrices read it): n x B, p x B, N x B
    double *xc, *yc, *zc;
    // QPD_VJP: the cotangent gx (n x B).  Results ux (n x B), uy (p x B), uz (N x B) and, where the pointer is not null and the
    // matrix has a member stride, the member's gradient gP = (ux x' + x ux') / 2 (n x n), gG = uz x' + z ux' (N x n),
    // gA = uy x' + y ux' (p x n) at the centred x, y, z, column-major, one member after the other.  In the 's' rows z and uz are
    // full symmetric blocks, so rows (i, j) and (j, i) of gG evaluate one expression.
    const double *gx;
    double *gP, *gG, *gA;
    // QPD_JVP: the perturbations, each with its member stride (0: one for all); a null pointer is a zero perturbation.  Of dP and
    // of every 's' block of dG and dh the lower triangle is read.  Results ux = dx, uy = dy, uz = dz and us = ds = -W'W dz (N x B).
    const double *dP, *dq, *dG, *dh, *dA, *db;
    int64_t sdP, sdq, sdG, sdh, sdA, sdb;
    double *ux, *uy, *uz, *us;
};

// LDS of one workgroup in bytes: that of k_coneqp_batch and one more n-vector and p-vector (DESIGN 21 has the corners).
size_t coneqp_batch_diff_lds_bytes(int n, int ml, int nq, const unsigned short *q, int ns, const unsigned char *m, int p);
hipError_t launch_coneqp_batch_diff(hipStream_t st, const ConeqpDiffArgs &a);
}  // namespace kvx
