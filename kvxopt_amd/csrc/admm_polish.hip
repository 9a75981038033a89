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
// unregularised system.  k_polish_finish clips z and forms the residuals.  The mapping is that of admm.hip: rows with fewer
// than ADMM_ROW_WAVE entries are summed by 16 lanes, the others by a wavefront, columns by 16 lanes; every lane of a launch runs
// every shuffle; strided partial sums, then a fixed butterfly; every output is written once and nothing uses floating-point
// atomics, so two runs give the same bytes.  The per-workgroup results meet in k_polish_reduce2, the second stage of
// k_admm_reduce2 with the ranges given per entry (admm.hip keeps its own inside an unnamed namespace).
#include "admm_polish.hpp"

#include <algorithm>

namespace kvx {
namespace {

constexpr double POLISH_INF = 1e26, POLISH_INFTY = 1e30;
constexpr double NEG_MAX = -1.7976931348623157e308;
// entries of the result (include/kvxhip.h: out[1 + k]); bit k of P_SUMMASK: entry k is a sum, otherwise a maximum
enum { R_NLOW = 0, R_NUPP = 1, R_PRI = 2, R_DUA = 3, R_PRI_U = 4, R_DUA_U = 5, R_XPX = 6, R_QX = 7, R_E1 = 8, R_E2 = 9 };
constexpr unsigned P_SUMMASK = (1u << R_NLOW) | (1u << R_NUPP) | (1u << R_XPX) | (1u << R_QX);

struct PolishCounts { int64_t nb[POLISH_NRES]; };

static inline unsigned blocks_of(int64_t threads) { return (unsigned)((threads + 255) / 256); }

template <int G>
__device__ inline double group_sum(double v)
{
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
    return v;
}

template <int G>
__device__ inline double group_dot(int64_t e0, int64_t e1, int sub, const int64_t *__restrict__ Mi, const double *__restrict__ Mx,
                                   const double *__restrict__ w)
{
    double acc = 0.0;
    for (int64_t e = e0 + sub; e < e1; e += G) acc += Mx[e] * w[Mi[e]];
    return group_sum<G>(acc);
}

// (A w)_i for the row this group of the launch owns: workgroups [0, nbs) hold 16 short rows each, [nbs, nbs + nbl) 4 long rows.
// Every lane runs the shuffles; *row < 0 for a group without a row, and only lane 0 of a group (*lead) writes.
__device__ inline double row_dot(const AdmmDev &a, unsigned nbs, const double *__restrict__ w, int64_t *row, bool *lead)
{
    if (blockIdx.x < nbs) {
        const int64_t t = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
        const bool live = t < a.ns;
        const int64_t i = live ? a.rs[t] : 0;
        *row = live ? i : -1;
        *lead = (threadIdx.x & 15) == 0;
        return group_dot<16>(live ? a.Tp[i] : 0, live ? a.Tp[i + 1] : 0, threadIdx.x & 15, a.Ti, a.Tx, w);
    }
    const int64_t t = (int64_t)(blockIdx.x - nbs) * 4 + (threadIdx.x >> 6);
    const bool live = t < a.nl;
    const int64_t i = live ? a.rl[t] : 0;
    *row = live ? i : -1;
    *lead = (threadIdx.x & 63) == 0;
    return group_dot<64>(live ? a.Tp[i] : 0, live ? a.Tp[i + 1] : 0, threadIdx.x & 63, a.Ti, a.Tx, w);
}

// v[k] of every thread -> one value per workgroup in a fixed order (butterfly inside a wavefront, the four wavefronts in order);
// part[key[k] * stride + slot] receives it.  LSUM: bit k set = local entry k is a sum.
template <int K, unsigned LSUM>
__device__ inline void block_reduce(double (&v)[K], double *sh, const int (&key)[K], double *__restrict__ part, int64_t stride, int64_t slot)
{
#pragma unroll
    for (int k = 0; k < K; k++) {
        double t = v[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double w = __shfl_xor(t, o);
            t = ((LSUM >> k) & 1u) ? t + w : fmax(t, w);
        }
        if ((threadIdx.x & 63) == 0) sh[(threadIdx.x >> 6) * K + k] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) {
            const bool sum = (LSUM >> k) & 1u;
            double r = sh[k];
            for (int w = 1; w < 4; w++) r = sum ? r + sh[w * K + k] : fmax(r, sh[w * K + k]);
            part[(int64_t)key[k] * stride + slot] = r;
        }
    }
}

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
    const int key[2] = {R_NLOW, R_NUPP};
    block_reduce<2, 3u>(v, sh, key, part, stride, blockIdx.x);
}

__global__ __launch_bounds__(256) void k_polish_rows(PolishDev p, unsigned nbs, double *__restrict__ part, int64_t stride)
{
    __shared__ double sh[4];
    int64_t i;
    bool lead;
    const double ax = row_dot(p.a, nbs, p.xh, &i, &lead);
    double v[1] = {NEG_MAX};
    if (i >= 0 && lead) {
        const double e2 = p.act[i] != 0 ? p.b[i] - ax : 0.0;
        p.e2[i] = e2;
        p.we2[i] = p.w[i] * e2;
        v[0] = fabs(e2);
    }
    const int key[1] = {R_E2};
    block_reduce<1, 0u>(v, sh, key, part, stride, blockIdx.x);
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
    const int key[1] = {R_E1};
    block_reduce<1, 0u>(v, sh, key, part, stride, blockIdx.x);
}

// workgroups [0, nbs + nbl): rows; the rest: 256 entries of x each (rhs holds the correction of x)
__global__ __launch_bounds__(256) void k_polish_correct(PolishDev p, unsigned nbs, unsigned nbl)
{
    if (blockIdx.x < nbs + nbl) {
        int64_t i;
        bool lead;
        const double adx = row_dot(p.a, nbs, p.rhs, &i, &lead);
        if (i >= 0 && lead) p.yh[i] += p.w[i] * (adx - p.e2[i]);
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
        int64_t i;
        bool lead;
        const double ax = row_dot(a, nbs, p.xh, &i, &lead);
        double v[2] = {NEG_MAX, NEG_MAX};
        if (i >= 0 && lead) {
            const double z = fmin(fmax(ax, a.l[i]), a.u[i]);
            p.zh[i] = z;
            v[0] = fabs(ax - z);
            v[1] = fabs(a.Einv[i] * (ax - z));
        }
        const int key[2] = {R_PRI, R_PRI_U};
        block_reduce<2, 0u>(v, sh, key, part, stride, blockIdx.x);
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
        const int key[4] = {R_DUA, R_DUA_U, R_XPX, R_QX};
        block_reduce<4, (1u << 2) | (1u << 3)>(v, sh, key, part, stride, blk);
    }
}

// second stage: one wavefront per entry k of the result, over the c.nb[k] workgroups that wrote it, in ascending order
__global__ __launch_bounds__(64) void k_polish_reduce2(const double *__restrict__ part, int64_t stride, PolishCounts c, double *__restrict__ res)
{
    const int k = blockIdx.x;
    const bool sum = (P_SUMMASK >> k) & 1u;
    const double *p = part + (int64_t)k * stride;
    const int64_t nb = c.nb[k];
    double acc = sum ? 0.0 : NEG_MAX;
    for (int64_t b = threadIdx.x; b < nb; b += 64) acc = sum ? acc + p[b] : fmax(acc, p[b]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(acc, o);
        acc = sum ? acc + w : fmax(acc, w);
    }
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
    if (i < a.m) {
        const double v = raw[i];
        const bool inf = upper ? v >= POLISH_INF : v <= -POLISH_INF;
        out[i] = inf ? (upper ? POLISH_INFTY : -POLISH_INFTY) : a.E[i] * v;
    }
}

__global__ __launch_bounds__(256) void k_admm_warm_x(AdmmDev a, const double *__restrict__ raw)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < a.n) a.x[j] = a.Dinv[j] * raw[j];
}

__global__ __launch_bounds__(256) void k_admm_warm_z(AdmmDev a, unsigned nbs)
{
    int64_t i;
    bool lead;
    const double ax = row_dot(a, nbs, a.x, &i, &lead);
    if (i >= 0 && lead) a.z[i] = ax;
}

__global__ __launch_bounds__(256) void k_admm_warm_y(AdmmDev a, double c, const double *__restrict__ raw)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.m) a.y[i] = (c * a.Einv[i]) * raw[i];
}

inline unsigned row_blocks_short(const AdmmDev &a) { return blocks_of(a.ns * 16); }
inline unsigned row_blocks_long(const AdmmDev &a) { return blocks_of(a.nl * 64); }

}  // namespace

int64_t polish_part_stride(const AdmmDev &a)
{
    const int64_t rows = (int64_t)row_blocks_short(a) + row_blocks_long(a);
    return std::max<int64_t>(1, std::max<int64_t>(std::max<int64_t>(blocks_of(a.m), rows), blocks_of(a.n * 16)));
}

void launch_polish_active(hipStream_t st, const PolishDev &p, double *part)
{
    hipLaunchKernelGGL(k_polish_active, dim3(blocks_of(p.a.m)), dim3(256), 0, st, p, part, polish_part_stride(p.a));
}

void launch_polish_residual(hipStream_t st, const PolishDev &p, double *part)
{
    const unsigned nbs = row_blocks_short(p.a), nbl = row_blocks_long(p.a);
    const int64_t stride = polish_part_stride(p.a);
    hipLaunchKernelGGL(k_polish_rows, dim3(nbs + nbl), dim3(256), 0, st, p, nbs, part, stride);
    hipLaunchKernelGGL(k_polish_cols, dim3(blocks_of(p.a.n * 16)), dim3(256), 0, st, p, part, stride);
}

void launch_polish_correct(hipStream_t st, const PolishDev &p)
{
    const unsigned nbs = row_blocks_short(p.a), nbl = row_blocks_long(p.a);
    hipLaunchKernelGGL(k_polish_correct, dim3(nbs + nbl + blocks_of(p.a.n)), dim3(256), 0, st, p, nbs, nbl);
}

void launch_polish_finish(hipStream_t st, const PolishDev &p, double *part, double *res)
{
    const unsigned nbs = row_blocks_short(p.a), nbl = row_blocks_long(p.a), nbc = blocks_of(p.a.n * 16);
    const int64_t stride = polish_part_stride(p.a);
    hipLaunchKernelGGL(k_polish_finish, dim3(nbs + nbl + nbc), dim3(256), 0, st, p, nbs, nbl, part, stride);
    PolishCounts c;
    const int64_t nbr = (int64_t)nbs + nbl;
    c.nb[R_NLOW] = c.nb[R_NUPP] = blocks_of(p.a.m);
    c.nb[R_PRI] = c.nb[R_PRI_U] = c.nb[R_E2] = nbr;
    c.nb[R_DUA] = c.nb[R_DUA_U] = c.nb[R_XPX] = c.nb[R_QX] = c.nb[R_E1] = nbc;
    hipLaunchKernelGGL(k_polish_reduce2, dim3(POLISH_NRES), dim3(64), 0, st, part, stride, c, res);
}

void launch_admm_scale_q(hipStream_t st, const AdmmDev &a, double c, const double *raw, double *q)
{
    hipLaunchKernelGGL(k_admm_scale_q, dim3(blocks_of(a.n)), dim3(256), 0, st, a, c, raw, q);
}

void launch_admm_scale_bound(hipStream_t st, const AdmmDev &a, bool upper, const double *raw, double *out)
{
    hipLaunchKernelGGL(k_admm_scale_bound, dim3(blocks_of(a.m)), dim3(256), 0, st, a, upper, raw, out);
}

void launch_admm_warm_x(hipStream_t st, const AdmmDev &a, const double *raw)
{
    const unsigned nbs = row_blocks_short(a), nbl = row_blocks_long(a);
    hipLaunchKernelGGL(k_admm_warm_x, dim3(blocks_of(a.n)), dim3(256), 0, st, a, raw);
    hipLaunchKernelGGL(k_admm_warm_z, dim3(nbs + nbl), dim3(256), 0, st, a, nbs);
}

void launch_admm_warm_y(hipStream_t st, const AdmmDev &a, double c, const double *raw)
{
    hipLaunchKernelGGL(k_admm_warm_y, dim3(blocks_of(a.m)), dim3(256), 0, st, a, c, raw);
}
}  // namespace kvx
