// Launchers of qp_batch_diff.hip: derivatives of B solved small dense QPs (qp_batch.hpp) at their returned x, y, s, z.
// Differentiating the KKT conditions of member b gives a linear system with the matrix
//
//     [ P  A'  G'   ]
//     [ A  0   0    ]        W'W = diag(s / z),
//     [ G  0  -W'W  ]
//
// the one k_qp_batch factors at every iteration: S = P + G' diag(z / s) G = L L', X = L^-1 A', K = X'X.  k_qp_batch_diff solves
// it once per member, one workgroup each, with `refinement` steps of iterative refinement on the full system (the shape of f4,
// coneprog.py:2288-2316), for the right-hand side of a vector-Jacobian product (reverse mode) or of a Jacobian-vector product
// (forward mode); k_batch_outer_sum adds the outer products of the members into the gradient of a matrix all members share.
// The mathematics is that of Amos & Kolter, "OptNet" (2017), section 3.
#pragma once
#include "batch_device.hpp"
#include "batch_host.hpp"
#include "qp_batch.hpp"

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace kvx {
enum { QPD_VJP = 0, QPD_JVP = 1, QPD_MAX_REFINEMENT = 3 };
// What a member ends with (the `exit` of kvxopt_amd.qpbatchdiff): done; skipped, since its exitcode of qp_batch is not 0; a
// failed pivot or an s_k, z_k that is not positive and finite.  1 and 2 leave zeros.
enum { QPD_DONE = 0, QPD_SKIPPED = 1, QPD_FAILED = 2 };

// BatchArgs with G ml x n and, as inputs, the solution x (n x B), y (p x B), s, z (ml x B) of qp_batch; c, h, b, the tolerances
// and stats do not enter; exitc is the exit of the derivative.
struct QpDiffArgs : BatchArgs {
    const double *P;                          // n x n per member, column-major, its lower triangle read
    int64_t sP;
    const int64_t *solexit;                   // exitcode of qp_batch, B
    int mode, refinement;
    // QPD_VJP: the cotangent gx (n x B).  Results ux (n x B), uy (p x B), uz (ml x B) and, where the pointer is not null and the
    // matrix has a member stride, the member's gradient gP = (ux x' + x ux') / 2 (n x n), gG = uz x' + z ux' (ml x n),
    // gA = uy x' + y ux' (p x n), column-major, one member after the other.
    const double *gx;
    double *gP, *gG, *gA;
    // QPD_JVP: the perturbations, each with its member stride (0: one for all); a null pointer is a zero perturbation.  dP is
    // symmetric and its lower triangle is read.  Results ux = dx, uy = dy, uz = dz and us = ds (ml x B).
    const double *dP, *dq, *dG, *dh, *dA, *db;
    int64_t sdP, sdq, sdG, sdh, sdA, sdb;
    double *ux, *uy, *uz, *us;
};

namespace qpdiff {
// LDS of one workgroup of k_qp_batch_diff in doubles from the base; every part starts on 16 bytes.  S, X, K and the staged rows
// as in qp_batch.hip; three n-vectors, three p-vectors, five ml-vectors against the nine of k_qp_batch, so every admissible
// shape fits where the forward kernel fits.
struct Layout {
    int ldn, ldp;
    int S, XK, X, K, bx, ux, rx, by, uy, ry, di, w, bz, uz, rz, red, total;
};

using batchdev::even;

__host__ __device__ inline Layout layout(int n, int ml, int p)
{
    Layout L;
    L.ldn = n | 1;
    L.ldp = p | 1;
    int o = 0;
    L.S = o; o += even(n * L.ldn);
    const int xsz = even(p * L.ldn), ksz = even(p * L.ldp), tsz = even(QPB_TILE * L.ldn);
    L.XK = L.X = o; L.K = o + xsz; o += (xsz + ksz > tsz ? xsz + ksz : tsz);
    const int nv = even(n), pv = even(p), mv = even(ml);
    L.bx = o; o += nv; L.ux = o; o += nv; L.rx = o; o += nv;
    L.by = o; o += pv; L.uy = o; o += pv; L.ry = o; o += pv;
    L.di = o; o += mv; L.w = o; o += mv; L.bz = o; o += mv; L.uz = o; o += mv; L.rz = o; o += mv;
    L.red = o; o += batchdev::NW * batchdev::NRED;
    L.total = o;
    return L;
}
}  // namespace qpdiff

inline size_t qp_batch_diff_lds_bytes(int n, int ml, int p) { return (size_t)qpdiff::layout(n, ml, p).total * sizeof(double); }
hipError_t launch_qp_batch_diff(hipStream_t st, const QpDiffArgs &a);

// C (rows x n, column-major) = scale * sum over the members b with gexit[b] == 0, in an order fixed at compile time, of
// u1_b v1_b' + u2_b v2_b'; u1, u2 are rows x B and v1, v2 n x B.  sym (rows = n, u1 = v2, v1 = u2): C is symmetric to the last bit.
// ldu: the distance between two members in u1 and u2 where they are `rows` rows of longer columns; 0: rows.
hipError_t launch_batch_outer_sum(hipStream_t st, int64_t B, int rows, int n, const double *u1, const double *v1, const double *u2,
                                  const double *v2, double scale, bool sym, const int64_t *gexit, double *C, int ldu = 0);
}  // namespace kvx
