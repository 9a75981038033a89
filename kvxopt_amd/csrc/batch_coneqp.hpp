// coneqp_member: one workgroup carries one member of a batch of small dense cone QPs
//
//     minimize (1/2) x'P x + q'x   subject to   G x + s = h,  s in K,  A x = b
//
// from its starting point to its status.  It is the device restatement of _ipm.coneqp_start / _ipm.coneqp_loop with refinement 0:
// coneprog.py:2044-2105 (start with W = I, the two pushes), 2167-2234 (residuals, stopping test), 2243-2316 (scaling, f4_no_ir),
// 2357-2456 (the two directions, the Mehrotra correction), 2459-2547 (step and scaling update), with the Newton solve of
// misc.kkt_chol on S = P + Gs'Gs, K = X'X (batch_kkt.hpp; no A'A repair, as in k_qp_batch and cone.coneqp).  It is the loop of
// k_qp_batch (qp_batch.hip) with every orthant expression replaced by a call of the policy `Cone` of batch_conelp.hpp: there is no
// embedding, one KKT solve per direction and no constant system.  k_qp_batch keeps its own loop: its members' bytes are pinned.
//
// Beyond the operations conelp_member uses (for_rows, load_h, start, max_step, push, first_scaling, lam_sq, kkt_before, kkt_after,
// gemv_t, update) the policy is asked for
//
//   degree()                 the degree of the cone, ml + nq + sum m_k, for mu = gap / degree
//   assemble_qp()            the lower triangle of S = P + Gs'Gs, started from the lower triangle of P
//   rhs_qp(ws, smu)          ds := lmbda o\ (-lmbda o lmbda + smu e [- ws3 if ws]), dz := -rz - W'ds; no barrier at the end
//   combine_qp(save, dot, mx) ds -= dz, dot := ds'dz, ws3 := ds o dz if save, both scaled by lmbda; mx as in max_step
//
// and C.M has P beside the data of a ConelpMem, with q as its c.  x1, y1, z1 of the member are not touched.
//
// The scalars gap, mu, sigma, step are computed by every thread from the same reduced values, so every branch around a barrier is
// workgroup-uniform.  Sums have the fixed order of batch_device.hpp.  Every loop is bounded by maxiters or by the member's
// dimensions.  A NaN or Inf never passes a pivot test and makes every comparison of the stopping test false, so such a member
// ends with exit 3, 2 or 1.
#pragma once
#include "batch_conelp.hpp"

namespace kvx {
namespace batchdev {

// What a member ends with: the `exit` of kvxopt_amd.qpbatch and coneqpbatch.
enum { CONEQP_OPTIMAL = 0, CONEQP_MAXITERS = 1, CONEQP_SINGULAR = 2, CONEQP_RANK = 3 };
constexpr int CONEQP_NSTAT = 8;

// The KKT factorisation in the current scaling (misc.py:1436-1487 with H = P): S = P + Gs'Gs and its factor in place, for p > 0
// X, K and its factor.  false on a failed pivot.  Barriers before (the caller's) and after.
template <class Cone>
__device__ __forceinline__ bool coneqp_factor(const Cone &C)
{
    C.assemble_qp();
    return chol_lds(C.M.S, C.M.ldn, C.M.n) && kkt_equalities(C.M);
}

// The member blockIdx.x of the batch `a`, whose cone is C and whose data and LDS vectors are bound in C.M.  correction: with
// the Mehrotra term.  Barrier before: the caller's, after it has set up the cone.
template <class Cone>
__device__ __forceinline__ void coneqp_member(const Cone &C, const BatchArgs &a, bool correction)
{
    const auto &M = C.M;
    const int tid = threadIdx.x, n = M.n, N = M.N, p = M.p;
    const int64_t bm = blockIdx.x;
    double *xo = a.x + bm * n, *yo = p ? a.y + bm * p : nullptr, *so = a.s + bm * N, *zo = a.z + bm * N, *st = a.stats + bm * CONEQP_NSTAT;

    int code = CONEQP_RANK, iters = 0;                     // solvers.coneqp: ValueError("Rank(A) < p or Rank([P; A; G]) < n")
    double gap = NAN, relgap = NAN, pcost = NAN, dcost = NAN, pres = NAN, dres = NAN;
    double resx0 = 1.0, resy0 = 1.0, resz0 = 1.0;

    // ---- starting point (coneprog.py:2044-2105): W = I, [P A' G'; A 0 0; G 0 -I][x; y; z] = [-q; b; h], s = -z, both pushed
    //      into the cone along e
    if (tid < n) M.x[tid] = -M.c[tid];
    if (tid < p) M.y[tid] = M.b[tid];
    C.start();
    C.load_h(M.z);
    __syncthreads();
    bool run = coneqp_factor(C);
    if (run) {
        conelp_kkt_solve(C, false, M.x, M.y, M.z);
        double mx[2] = {-INFINITY, -INFINITY}, nr[2] = {0.0, 0.0}, r0[3] = {0.0, 0.0, 0.0};
        if (tid < n) r0[0] = M.c[tid] * M.c[tid];
        if (tid < p) r0[1] = M.b[tid] * M.b[tid];
        for (int k = tid; k < N; k += NT) M.s[k] = -M.z[k];
        __syncthreads();
        C.for_rows([&](auto row) {
            const int k = row.k;
            const double sk = M.s[k], zk = M.z[k], hk = M.h[k];
            nr[0] += row.w(sk * sk); nr[1] += row.w(zk * zk);
            r0[2] += row.w(hk * hk);
        });
        blk_reduce<2, false>(nr, M.red);
        blk_reduce<3, false>(r0, M.red);
        C.max_step(M.s, 1.0, M.z, 1.0, mx);
        resx0 = fmax(1.0, sqrt(r0[0])); resy0 = fmax(1.0, sqrt(r0[1])); resz0 = fmax(1.0, sqrt(r0[2]));
        const bool ps = mx[0] >= -1e-8 * fmax(sqrt(nr[0]), 1.0), pz = mx[1] >= -1e-8 * fmax(sqrt(nr[1]), 1.0);
        C.push(ps, pz, mx);
        __syncthreads();
        double g[1] = {0.0};
        C.for_rows([&](auto row) { g[0] += row.w(M.s[row.k] * M.z[row.k]); });
        blk_reduce<1, false>(g, M.red);                    // its barriers also publish x, y, s, z
        gap = g[0];
        code = CONEQP_MAXITERS;
    }

    for (; run; iters++) {
        // ---- residuals and objectives (coneprog.py:2167-2203): rx = P x + q + A'y + G'z, ry = A x - b, rz = s + G x - h
        double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};               // x'(Px + q), x'q, |rx|^2, |ry|^2, |rz|^2, y'ry, z'rz
        if (tid < n) {
            double t = 0.0;
            for (int j = 0; j < n; j++) t += (j <= tid ? M.P[tid + j * n] : M.P[j + tid * n]) * M.x[j];
            t += M.c[tid];
            M.rx[tid] = t;
            v[0] = M.x[tid] * t;
            v[1] = M.x[tid] * M.c[tid];
        }
        if (tid < p) {
            const double t = row_dot(M.A, p, n, tid, M.x) - M.b[tid];
            M.ry[tid] = t;
            v[3] = t * t;
            v[5] = M.y[tid] * t;
        }
        C.for_rows([&](auto row) {
            const int k = row.k;
            const double t = (M.s[k] - M.h[k]) + row_dot(M.G, N, n, k, M.x);
            row.put(M.rz, t);
            v[4] += row.w(t * t);
            v[6] += row.w(M.z[k] * t);
        });
        __syncthreads();
        if (p > 0) gemv_t_add(M.A, p, n, M.y, nullptr, 1.0, M.rx);
        __syncthreads();
        C.gemv_t(M.z, 1.0, M.rx);
        __syncthreads();
        if (tid < n) v[2] = M.rx[tid] * M.rx[tid];
        blk_reduce<7, false>(v, M.red);
        const double f0 = 0.5 * (v[0] + v[1]);
        pcost = f0;
        dcost = f0 + v[5] + v[6] - gap;
        relgap = pcost < 0.0 ? gap / -pcost : (dcost > 0.0 ? gap / dcost : NAN);
        pres = fmax(sqrt(v[3]) / resy0, sqrt(v[4]) / resz0);
        dres = sqrt(v[2]) / resx0;
        if (iters == a.maxiters) { code = CONEQP_MAXITERS; break; }
        if (pres <= a.feastol && dres <= a.feastol && (gap <= a.abstol || relgap <= a.reltol)) { code = CONEQP_OPTIMAL; break; }

        // ---- scaling of the first iteration (misc.compute_scaling, coneprog.py:2230-2231), the factorisation
        if (iters == 0) {
            if (!C.first_scaling()) { code = CONEQP_RANK; break; }   // lapack.potrf's ArithmeticError in misc.compute_scaling
        }
        __syncthreads();
        if (!coneqp_factor(C)) { code = iters == 0 ? CONEQP_RANK : CONEQP_SINGULAR; break; }

        // ---- the affine-scaling and the combined direction (coneprog.py:2357-2456) through f4_no_ir (:2288-2316)
        const double mu = gap / C.degree();
        double sigma = 0.0, step = 0.0;
        for (int i = 0; i < 2; i++) {
            C.rhs_qp(correction && i == 1, sigma * mu);
            if (tid < n) M.dx[tid] = -M.rx[tid];
            if (tid < p) M.dy[tid] = -M.ry[tid];
            __syncthreads();
            conelp_kkt_solve(C, false, M.dx, M.dy, M.dz);
            double dsdz = 0.0, mx[2] = {-INFINITY, -INFINITY};
            C.combine_qp(correction && i == 0, dsdz, mx);
            const double t = fmax(0.0, fmax(mx[0], mx[1]));
            step = t == 0.0 ? 1.0 : (i == 0 ? fmin(1.0, 1.0 / t) : fmin(1.0, 0.99 / t));
            if (i == 0) {
                const double u = fmin(1.0, fmax(0.0, 1.0 - step + dsdz / gap * (step * step)));
                sigma = u * u * u;
            }
        }

        // ---- the step, the scaling update (misc.update_scaling), s and z of the next iteration (coneprog.py:2459-2547)
        if (tid < n) M.x[tid] += step * M.dx[tid];
        if (tid < p) M.y[tid] += step * M.dy[tid];
        C.update(step);
        __syncthreads();
        gap = C.lam_sq();                                  // its barriers also publish x, y, s, z
    }

    // ---- the member's result (coneprog.py:2213-2234, 2261-2275); after a first factorisation that failed: zeros.  The slacks
    //      are -max_step of s and z over the whole cone.
    const bool rank = code == CONEQP_RANK;
    double mx[2] = {-INFINITY, -INFINITY};
    __syncthreads();
    for (int k = tid; k < N; k += NT) { so[k] = rank ? 0.0 : M.s[k]; zo[k] = rank ? 0.0 : M.z[k]; }
    if (tid < n) xo[tid] = rank ? 0.0 : M.x[tid];
    if (tid < p) yo[tid] = rank ? 0.0 : M.y[tid];
    if (!rank) C.max_step(M.s, 1.0, M.z, 1.0, mx);
    if (tid == 0) {
        const double out[CONEQP_NSTAT] = {gap, relgap, pcost, dcost, pres, dres, -mx[0], -mx[1]};
#pragma unroll
        for (int k = 0; k < CONEQP_NSTAT; k++) st[k] = rank ? NAN : out[k];
        a.iters[bm] = rank ? 0 : iters;
        a.exitc[bm] = code;
    }
}

}  // namespace batchdev
}  // namespace kvx
