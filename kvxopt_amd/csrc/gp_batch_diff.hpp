// Launcher of gp_batch_diff.hip: derivatives of B solved small dense geometric programs (gp_batch.hpp) at their returned
// x, y, s, z.  With zeta_0 = 1 and zeta_i = znl_i, y_i = softmax(F_i x + g_i) and Df_i = y_i'F_i per block, differentiating the
// optimality conditions of member b in x (the epigraph row is gone: its dual tends to 1) gives a linear system with the matrix
//
//     [ H  A'  J'   ]        H = sum_{i >= 0} zeta_i F_i'(diag y_i - y_i y_i')F_i,
//     [ A  0   0    ]        J = [Df_1 .. Df_mnl; G],
//     [ J  0  -W'W  ]        W'W = diag(s / z) over the mnl + ml rows of J,
//
// whose reduced matrix S = H + J' diag(z / s) J is the Schur complement on t of the S k_gp_batch factors at every iteration.
// k_gp_batch_diff assembles it from the same staged rows (gp_batch_device.hpp), solves once per member, one workgroup each, with
// `refinement` steps of iterative refinement on the full system, for the right-hand side of a vector-Jacobian product (reverse
// mode) or of a Jacobian-vector product (forward mode); k_batch_outer_sum (qp_batch_diff.hpp) adds the outer products of the
// members into the gradient of a matrix all members share.  The mathematics is that of Amos & Kolter, "OptNet" (2017),
// section 3, with the data entering through the softmax weights.
#pragma once
#include "batch_device.hpp"
#include "gp_batch.hpp"
#include "qp_batch_diff.hpp"

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace kvx {
enum { GPD_VJP = 0, GPD_JVP = 1, GPD_MAX_REFINEMENT = 3 };
// What a member ends with (the `exit` of kvxopt_amd.gpbatchdiff): done; skipped, since its exitcode of gp_batch is not 0; a
// failed pivot or an s_k, z_k (k >= 1) that is not positive and finite.  1 and 2 leave zeros.
enum { GPD_DONE = 0, GPD_SKIPPED = 1, GPD_FAILED = 2 };

// GpBatchArgs with, as inputs, the solution x (n x B), y (p x B), s, z (N x B, N = m + ml, as k_gp_batch writes them: row 0,
// the objective row of the epigraph form, is not read); h, b, the tolerances, stats and scratch do not enter; exitc is the exit
// of the derivative.  uz and us have N rows as well, and row 0 is written as 0.
struct GpDiffArgs : GpBatchArgs {
    const int64_t *solexit;                   // exitcode of gp_batch, B
    int mode, refinement;
    // GPD_VJP: the cotangent gx (n x B).  Results ux (n x B), uy (p x B), uz (N x B), gg (l x B) = dl/dg with
    // gg_k = y_k (zeta_i e_k + uz_i), e_k = (F_k - Df_i) ux; where the pointer is not null and the matrix has a member stride,
    // the member's gradient gF = a ux' + gg x' (l x n), a_k = zeta_i y_k, gG = uzl x' + zl ux' (ml x n), gA = uy x' + y ux'
    // (p x n), column-major, one member after the other.  ga (l x B, may be null): a, for the sum of a shared F.
    const double *gx;
    double *gg, *ga, *gF, *gG, *gA;
    // GPD_JVP: the perturbations, each with its member stride (0: one for all); a null pointer is a zero perturbation.
    // Results ux = dx, uy = dy, uz = dz and us = ds (N x B).
    const double *dF, *dg, *dG, *dh, *dA, *db;
    int64_t sdF, sdg, sdG, sdh, sdA, sdb;
    double *ux, *uy, *uz, *us;
};

namespace gpdiff {
// LDS of one workgroup of k_gp_batch_diff in doubles from the base; every part starts on 16 bytes.  S of order n, the X / K /
// tile region of gp_batch.hip at that order, four n-vectors, three p-vectors, six N-vectors (k_gp_batch: fourteen) and the m
// weights zeta, three l-vectors and the two integer maps of the blocks.
struct Layout {
    int N, ldn, ldp;
    int S, XK, X, K, Gs, x, bx, ux, rx, by, uy, ry, di, sz, bz, uz, rz, ws, zeta, yv, w, tv, off, blk, red, total;
};

using batchdev::even;

__host__ __device__ inline Layout layout(int n, int m, int l, int ml, int p)
{
    Layout L;
    L.N = m + ml;
    L.ldn = n | 1;
    L.ldp = p | 1;
    int o = 0;
    L.S = o; o += even(n * L.ldn);
    const int xsz = even(p * L.ldn), ksz = even(p * L.ldp), tsz = even(GPB_TILE * L.ldn);
    L.XK = L.X = o; L.K = o + xsz; L.Gs = o + tsz; o += (xsz + ksz > 2 * tsz ? xsz + ksz : 2 * tsz);
    const int nv = even(n), pv = even(p), mv = even(L.N), bv = even(m), lv = even(l);
    L.x = o; o += nv; L.bx = o; o += nv; L.ux = o; o += nv; L.rx = o; o += nv;
    L.by = o; o += pv; L.uy = o; o += pv; L.ry = o; o += pv;
    L.di = o; o += mv; L.sz = o; o += mv; L.bz = o; o += mv; L.uz = o; o += mv; L.rz = o; o += mv; L.ws = o; o += mv;
    L.zeta = o; o += bv;
    L.yv = o; o += lv; L.w = o; o += lv; L.tv = o; o += lv;
    L.off = o; o += even(m + 1) / 2;          // ints: the first term of every block and l
    L.blk = o; o += even(l) / 2;              // ints: the block of every term
    o = even(o);
    L.red = o; o += batchdev::NW * batchdev::NRED;
    L.total = o;
    return L;
}
}  // namespace gpdiff

inline size_t gp_batch_diff_lds_bytes(int n, int m, int l, int ml, int p)
{
    return (size_t)gpdiff::layout(n, m, l, ml, p).total * sizeof(double);
}
hipError_t launch_gp_batch_diff(hipStream_t st, const GpDiffArgs &a);
}  // namespace kvx
