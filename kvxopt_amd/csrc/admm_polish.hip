// Kernels of a kept kvx_admm problem beyond the iteration of admm.hip (admm_api.cpp: kvx_admm_update, kvx_admm_warm_start,
// kvx_admm_polish).  The polish works in the scaled problem on S_pol = P + delta I + A' diag(w) A (w = 1 / delta on the active
// rows, 0 elsewhere; b: the bound an active row sits at).  From xh = yh = 0, 1 + refine_iter times
//
//     k_polish_rows     e2 = b - A xh on active rows, 0 elsewhere; w o e2                  rows of A
//     k_polish_cols     e1 = -q - (P xh + A' yh),  rhs = e1 + A'(w o e2)                   one 16-lane group per column
//     (solve)           rhs = S_pol^-1 rhs                                                 kvx_chol_solve_async_dev
//     k_polish_correct  yh += w o (A rhs - e2);  xh += rhs                                 rows of A, then the n-long part
//
// The first pass is OSQP's first solve (e1 = -q and e2 = b exactly, and 0 + d = d), the others its iterative refinement against the
// unregularised system.  k_polish_finish clips z and forms the residuals.  The mapping is that of admm.hip, from admm_device.hpp:
// rows with fewer than ADMM_ROW_WAVE entries are summed by 16 lanes, the others by a wavefront, columns by 16 lanes; every lane
// of a launch runs every shuffle; strided partial sums, then a fixed butterfly; every output is written once and nothing uses
// floating-point atomics, so two runs give the same bytes.  The per-workgroup results meet in k_polish_reduce2: the second
// stage of k_admm_reduce2, over the first c.nb[k] slots of entry k.
#include "admm_polish.hpp"
#include "admm_device.hpp"

#include <algorithm>

namespace kvx {
namespace {

// entries of the result (include/kvxhip.h: out[1 + k]); bit k of P_SUMMASK: entry k is a sum, otherwise a maximum
enum { R_NLOW = 0, R_NUPP = 1, R_PRI = 2, R_DUA = 3, R_PRI_U = 4, R_DUA_U = 5, R_XPX = 6, R_QX = 7, R_E1 = 8, R_E2 = 9 };
constexpr unsigned P_SUMMASK = (1u << R_NLOW) | (1u << R_NUPP) | (1u << R_XPX) | (1u << R_QX);
// the entries each kernel gives to block_reduce
__device__ constexpr int KEY_ACTIVE[2] = {R_NLOW, R_NUPP}, KEY_ROWS[1] = {R_E2}, KEY_COLS[1] = {R_E1}, KEY_PRI[2] = {R_PRI, R_PRI_U},
                         KEY_DUA[4] = {R_DUA, R_DUA_U, R_XPX, R_QX};

struct PolishCounts { int64_t nb[POLISH_NRES]; };

// ---- the active set: lower z - l < -y, upper u - z < y (z is clipped, so at most one holds) ----------------------------------
__global__ __launch_bounds__(256) void k_polish_active(PolishDev p, double *__restrict__ part, int64_t stride)
{
    __shared__ double sh[4 * 2];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v[2] = {0.0, 0.0};
    if (i < p.a.m) {
        const double z = p.a.z[i], y = p.a.y[i], l = p.a.l[i], u = p.a.u[i];
        const bool lo = z - l < -y, up = !lo && u - z < y;
        p.act[i] = lo ? -1 : (up ? 1 : 0);
        p.w[i] = (lo || up) ? 1.0 / p.delta : 0.0;
        p.b[i] = lo ? l : (up ? u : 0.0);
        v[0] = lo ? 1.0 : 0.0;
        v[1] = up ? 1.0 : 0.0;
    }
    block_reduce<2, 3u>(v, sh, KEY_ACTIVE, part, stride, blockIdx.x);
}

__global__ __launch_bounds__(256) void k_polish_rows(PolishDev p, unsigned nbs, double *__restrict__ part, int64_t stride)
{
    __shared__ double sh[4];
    const RowGroup g = row_group(p.a, nbs, blockIdx.x, threadIdx.x);
    const double ax = row_dot(p.a, g, p.xh);
    double v[1] = {NEG_MAX};
    if (g.lead()) {
        const int64_t i = g.row;
        const double e2 = p.act[i] != 0 ? p.b[i] - ax : 0.0;
        p.e2[i] = e2;
        p.we2[i] = p.w[i] * e2;
        v[0] = fabs(e2);
    }
    block_reduce<1, 0u>(v, sh, KEY_ROWS, part, stride, blockIdx.x);
}

__global__ __launch_bounds__(256) void k_polish_cols(PolishDev p, double *__restrict__ part, int64_t stride)
{
    __shared__ double sh[4];
    const AdmmDev &a = p.a;
    const int sub = threadIdx.x & 15;
    const int64_t j = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = j < a.n;
    const int64_t e0 = live ? a.Ap[j] : 0, e1 = live ? a.Ap[j + 1] : 0;
    double aty = 0.0, awe = 0.0;
    for (int64_t e = e0 + sub; e < e1; e += 16) {
        const int64_t i = a.Ai[e];
        const double ax = a.Ax[e];
        aty += ax * p.yh[i];
        awe += ax * p.we2[i];
    }
    aty = group_sum<16>(aty);
    awe = group_sum<16>(awe);
    const double px = group_dot<16>(live ? a.Fp[j] : 0, live ? a.Fp[j + 1] : 0, sub, a.Fi, a.Fx, p.xh);
    double v[1] = {NEG_MAX};
    if (live && sub == 0) {
        const double r1 = -a.q[j] - (px + aty);
        p.rhs[j] = r1 + awe;
        v[0] = fabs(r1);
    }
    block_reduce<1, 0u>(v, sh, KEY_COLS, part, stride, blockIdx.x);
}

// workgroups [0, nbs + nbl): rows; the rest: 256 entries of x each (rhs holds the correction of x)
__global__ __launch_bounds__(256) void k_polish_correct(PolishDev p, unsigned nbs, unsigned nbl)
{
    if (blockIdx.x < nbs + nbl) {
        const RowGroup g = row_group(p.a, nbs, blockIdx.x, threadIdx.x);
        const double adx = row_dot(p.a, g, p.rhs);
        if (g.lead()) p.yh[g.row] += p.w[g.row] * (adx - p.e2[g.row]);
    } else {
        const int64_t j = (int64_t)(blockIdx.x - nbs - nbl) * 256 + threadIdx.x;
        if (j < p.a.n) p.xh[j] += p.rhs[j];
    }
}

// workgroups [0, nbs + nbl): rows (zh, the primal residual); the rest: 16 columns each (the dual residual, the objective terms)
__global__ __launch_bounds__(256) void k_polish_finish(PolishDev p, unsigned nbs, unsigned nbl, double *__restrict__ part, int64_t stride)
{
    __shared__ double sh[4 * 4];
    const AdmmDev &a = p.a;
    if (blockIdx.x < nbs + nbl) {
        const RowGroup g = row_group(a, nbs, blockIdx.x, threadIdx.x);
        const double ax = row_dot(a, g, p.xh);
        double v[2] = {NEG_MAX, NEG_MAX};
        if (g.lead()) {
            const int64_t i = g.row;
            const double z = fmin(fmax(ax, a.l[i]), a.u[i]);
            p.zh[i] = z;
            v[0] = fabs(ax - z);
            v[1] = fabs(a.Einv[i] * (ax - z));
        }
        block_reduce<2, 0u>(v, sh, KEY_PRI, part, stride, blockIdx.x);
    } else {
        const int sub = threadIdx.x & 15;
        const int64_t blk = (int64_t)blockIdx.x - nbs - nbl;
        const int64_t j = blk * 16 + (threadIdx.x >> 4);
        const bool live = j < a.n;
        const int64_t e0 = live ? a.Ap[j] : 0, e1 = live ? a.Ap[j + 1] : 0;
        double aty = 0.0;
        for (int64_t e = e0 + sub; e < e1; e += 16) aty += a.Ax[e] * p.yh[a.Ai[e]];
        aty = group_sum<16>(aty);
        const double px = group_dot<16>(live ? a.Fp[j] : 0, live ? a.Fp[j + 1] : 0, sub, a.Fi, a.Fx, p.xh);
        double v[4] = {NEG_MAX, NEG_MAX, 0.0, 0.0};
        if (live && sub == 0) {
            const double q = a.q[j], x = p.xh[j];
            const double rd = px + q + aty;
            v[0] = fabs(rd);
            v[1] = fabs(rd * a.Dinv[j] * a.cinv);
            v[2] = x * px;
            v[3] = q * x;
        }
        block_reduce<4, (1u << 2) | (1u << 3)>(v, sh, KEY_DUA, part, stride, blk);
    }
}

// second stage: one wavefront per entry k of the result, over the c.nb[k] workgroups that wrote it, in ascending order
__global__ __launch_bounds__(64) void k_polish_reduce2(const double *__restrict__ part, int64_t stride, PolishCounts c, double *__restrict__ res)
{
    const int k = blockIdx.x;
    const double acc = wave_reduce2(part + (int64_t)k * stride, 0, c.nb[k], (P_SUMMASK >> k) & 1u);
    if (threadIdx.x == 0) res[k] = acc;
}

// ---- update and warm start: element-wise ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_admm_scale_q(AdmmDev a, double c, const double *__restrict__ raw, double *__restrict__ q)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < a.n) q[j] = (c * a.D[j]) * raw[j];
}

__global__ __launch_bounds__(256) void k_admm_scale_bound(AdmmDev a, bool upper, const double *__restrict__ raw, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.m) out[i] = scaled_bound(raw[i], a.E + i, upper);
}

__global__ __launch_bounds__(256) void k_admm_warm_x(AdmmDev a, const double *__restrict__ raw)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < a.n) a.x[j] = a.Dinv[j] * raw[j];
}

__global__ __launch_bounds__(256) void k_admm_warm_z(AdmmDev a, unsigned nbs)
{
    const RowGroup g = row_group(a, nbs, blockIdx.x, threadIdx.x);
    const double ax = row_dot(a, g, a.x);
    if (g.lead()) a.z[g.row] = ax;
}

__global__ __launch_bounds__(256) void k_admm_warm_y(AdmmDev a, double c, const double *__restrict__ raw)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.m) a.y[i] = (c * a.Einv[i]) * raw[i];
}

}  // namespace

int64_t polish_part_stride(const AdmmDev &a)
{
    const AdmmGrid g(a);
    return std::max<int64_t>(1, std::max<int64_t>(std::max<int64_t>(g.nbm, g.rows()), g.nbc));
}

void launch_polish_active(hipStream_t st, const PolishDev &p, double *part)
{
    hipLaunchKernelGGL(k_polish_active, dim3(AdmmGrid(p.a).nbm), dim3(256), 0, st, p, part, polish_part_stride(p.a));
}

void launch_polish_residual(hipStream_t st, const PolishDev &p, double *part)
{
    const AdmmGrid g(p.a);
    const int64_t stride = polish_part_stride(p.a);
    hipLaunchKernelGGL(k_polish_rows, dim3(g.rows()), dim3(256), 0, st, p, g.nbs, part, stride);
    hipLaunchKernelGGL(k_polish_cols, dim3(g.nbc), dim3(256), 0, st, p, part, stride);
}

void launch_polish_correct(hipStream_t st, const PolishDev &p)
{
    const AdmmGrid g(p.a);
    hipLaunchKernelGGL(k_polish_correct, dim3(g.rows() + g.nbx), dim3(256), 0, st, p, g.nbs, g.nbl);
}

void launch_polish_finish(hipStream_t st, const PolishDev &p, double *part, double *res)
{
    const AdmmGrid g(p.a);
    const int64_t stride = polish_part_stride(p.a);
    hipLaunchKernelGGL(k_polish_finish, dim3(g.rows() + g.nbc), dim3(256), 0, st, p, g.nbs, g.nbl, part, stride);
    PolishCounts c;
    c.nb[R_NLOW] = c.nb[R_NUPP] = g.nbm;
    c.nb[R_PRI] = c.nb[R_PRI_U] = c.nb[R_E2] = g.rows();
    c.nb[R_DUA] = c.nb[R_DUA_U] = c.nb[R_XPX] = c.nb[R_QX] = c.nb[R_E1] = g.nbc;
    hipLaunchKernelGGL(k_polish_reduce2, dim3(POLISH_NRES), dim3(64), 0, st, part, stride, c, res);
}

void launch_admm_scale_q(hipStream_t st, const AdmmDev &a, double c, const double *raw, double *q)
{
    hipLaunchKernelGGL(k_admm_scale_q, dim3(AdmmGrid(a).nbx), dim3(256), 0, st, a, c, raw, q);
}

void launch_admm_scale_bound(hipStream_t st, const AdmmDev &a, bool upper, const double *raw, double *out)
{
    hipLaunchKernelGGL(k_admm_scale_bound, dim3(AdmmGrid(a).nbm), dim3(256), 0, st, a, upper, raw, out);
}

void launch_admm_warm_x(hipStream_t st, const AdmmDev &a, const double *raw)
{
    const AdmmGrid g(a);
    hipLaunchKernelGGL(k_admm_warm_x, dim3(g.nbx), dim3(256), 0, st, a, raw);
    hipLaunchKernelGGL(k_admm_warm_z, dim3(g.rows()), dim3(256), 0, st, a, g.nbs);
}

void launch_admm_warm_y(hipStream_t st, const AdmmDev &a, double c, const double *raw)
{
    hipLaunchKernelGGL(k_admm_warm_y, dim3(AdmmGrid(a).nbm), dim3(256), 0, st, a, c, raw);
}
}  // namespace kvx
