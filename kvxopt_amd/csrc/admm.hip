// Kernels of the ADMM iteration behind kvxopt.osqp (admm_api.cpp; the reference only binds an external library, src/C/osqp.c).
// On the scaled problem, with S = P + sigma I + A' diag(rho) A factored once (kvx_chol), iteration k is
//
//     k_admm_rhs     xt = sigma x - q + A'(rho o z - y)                                    one 16-lane group per column of A
//     (solve)        xt = S^-1 xt                                                          kvx_chol_solve_async_dev
//     k_admm_update  zt = A xt, v = alpha zt + (1 - alpha) z, z+ = clip(v + y / rho, l, u), y+ = y + rho o (v - z+),
//                    dy = y+ - y; x+ = alpha xt + (1 - alpha) x, dx = x+ - x               rows of A, then the n-long part
//
// and k_admm_residuals + k_admm_reduce2 give the 24 numbers a termination check reads.  Rows with fewer than ADMM_ROW_WAVE entries
// are summed by 16 lanes, the others by a wavefront; every lane of a launch runs every shuffle (a group without a row works on
// an empty range).  Every sum runs in a fixed order -- strided partial sums, then a fixed butterfly -- and every output is
// written once: no floating-point atomics, the same bits on every call.  The row groups, the reductions and the 24 numbers are
// those of admm_device.hpp, shared with the batch and the polish.
#include "admm_device.hpp"

namespace kvx {
namespace {

__global__ __launch_bounds__(256) void k_admm_rhs(AdmmDev a)
{
    const int sub = threadIdx.x & 15;
    const int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const bool live = j < a.n;
    const int64_t e0 = live ? a.Ap[j] : 0, e1 = live ? a.Ap[j + 1] : 0;
    double acc = 0.0;
    for (int64_t e = e0 + sub; e < e1; e += 16) {
        const int64_t i = a.Ai[e];
        acc += a.Ax[e] * (a.rho[i] * a.z[i] - a.y[i]);
    }
    acc = group_sum<16>(acc);
    if (live && sub == 0) a.xt[j] = (a.sigma * a.x[j] - a.q[j]) + acc;
}

// workgroups [0, nbs + nbl): the rows of A (row_group); the rest: 256 entries of x each
__global__ __launch_bounds__(256) void k_admm_update(AdmmDev a, unsigned nbs, unsigned nbl)
{
    if (blockIdx.x < nbs + nbl) {
        const RowGroup g = row_group(a, nbs, blockIdx.x, threadIdx.x);
        const double zt = row_dot(a, g, a.xt);
        if (g.lead()) update_row(a.alpha, a.rho[g.row], a.l[g.row], a.u[g.row], zt, a.z + g.row, a.y + g.row, a.dy + g.row);
    } else {
        const int64_t j = (int64_t)(blockIdx.x - nbs - nbl) * 256 + threadIdx.x;
        if (j < a.n) update_x(a.alpha, a.xt[j], a.x + j, a.dx + j);
    }
}

// workgroups [0, nbs + nbl): the rows of A (row_group); the rest: 16 columns each
__global__ __launch_bounds__(256) void k_admm_residuals(AdmmDev a, unsigned nbs, unsigned nbl, double *__restrict__ part)
{
    __shared__ double sh[4 * 14];
    const int64_t nb = gridDim.x;
    if (blockIdx.x < nbs + nbl) {
        double v[10];
        reduce_identity<10, ROW_LSUM>(v);
        const RowGroup g = row_group(a, nbs, blockIdx.x, threadIdx.x);
        const double ax = row_dot(a, g, a.x);
        const double adx = row_dot(a, g, a.dx);
        if (g.lead()) {
            const int64_t i = g.row;
            residual_row(a.z[i], a.l[i], a.u[i], a.dy[i], a.E[i], a.Einv[i], a.cinv, ax, adx, v);
        }
        block_reduce<10, ROW_LSUM>(v, sh, RK, part, nb, blockIdx.x);
    } else {
        double v[14];
        reduce_identity<14, COL_LSUM>(v);
        const int sub = threadIdx.x & 15;
        const int64_t j = (int64_t)(blockIdx.x - nbs - nbl) * 16 + (threadIdx.x >> 4);
        const bool live = j < a.n;
        const int64_t e0 = live ? a.Ap[j] : 0, e1 = live ? a.Ap[j + 1] : 0;
        double aty = 0.0, atd = 0.0;
        for (int64_t e = e0 + sub; e < e1; e += 16) {
            const int64_t i = a.Ai[e];
            const double ax = a.Ax[e];
            aty += ax * a.y[i];
            atd += ax * cut_dy(a.dy[i], a.l[i], a.u[i]);
        }
        aty = group_sum<16>(aty);
        atd = group_sum<16>(atd);
        const int64_t f0 = live ? a.Fp[j] : 0, f1 = live ? a.Fp[j + 1] : 0;
        const double px = group_dot<16>(f0, f1, sub, a.Fi, a.Fx, a.x);
        const double pdx = group_dot<16>(f0, f1, sub, a.Fi, a.Fx, a.dx);
        if (live && sub == 0) residual_col(a.q[j], a.x[j], a.dx[j], a.D[j], a.Dinv[j], a.cinv, px, pdx, aty, atd, v);
        block_reduce<14, COL_LSUM>(v, sh, CK, part, nb, blockIdx.x);
    }
}

// second stage: one wavefront per entry k of the result, over the workgroups that hold it
__global__ __launch_bounds__(64) void k_admm_reduce2(const double *__restrict__ part, int64_t nbr, int64_t nb, double *__restrict__ res)
{
    const int k = blockIdx.x;
    int64_t b0, b1;
    residual_range(k, nbr, nb, &b0, &b1);
    const double acc = wave_reduce2(part + (int64_t)k * nb, b0, b1, (SUMMASK >> k) & 1u);
    if (threadIdx.x == 0) res[k] = acc;
}

}  // namespace

void launch_admm_rhs(hipStream_t st, const AdmmDev &a)
{
    if (a.n > 0) hipLaunchKernelGGL(k_admm_rhs, dim3(AdmmGrid(a).nbc), dim3(256), 0, st, a);
}

void launch_admm_update(hipStream_t st, const AdmmDev &a)
{
    const AdmmGrid g(a);
    if (g.rows() + g.nbx > 0) hipLaunchKernelGGL(k_admm_update, dim3(g.rows() + g.nbx), dim3(256), 0, st, a, g.nbs, g.nbl);
}

int64_t admm_residual_blocks(const AdmmDev &a)
{
    const AdmmGrid g(a);
    return (int64_t)g.rows() + g.nbc;
}

void launch_admm_residuals(hipStream_t st, const AdmmDev &a, double *part, double *res)
{
    const AdmmGrid g(a);
    const unsigned nb = g.rows() + g.nbc;
    if (nb > 0) hipLaunchKernelGGL(k_admm_residuals, dim3(nb), dim3(256), 0, st, a, g.nbs, g.nbl, part);
    hipLaunchKernelGGL(k_admm_reduce2, dim3(ADMM_NRES), dim3(64), 0, st, part, (int64_t)g.rows(), (int64_t)nb, res);
}
}  // namespace kvx
