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
// written once: no floating-point atomics, the same bits on every call.
#include "admm.hpp"

namespace kvx {
namespace {

constexpr double ADMM_INF = 1e26;               // |bound| >= INFTY * 1e-4 is infinite (INFTY = 1e30)
constexpr double NEG_MAX = -1.7976931348623157e308;

static inline unsigned blocks_of(int64_t threads) { return (unsigned)((threads + 255) / 256); }

template <int G>
__device__ inline double group_sum(double v)
{
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
    return v;
}

// sum_e Mx[e] * w[Mi[e]] over e in [e0, e1) by the G lanes of a group: lane `sub` takes e0 + sub, e0 + sub + G, ...
template <int G>
__device__ inline double group_dot(int64_t e0, int64_t e1, int sub, const int64_t *__restrict__ Mi, const double *__restrict__ Mx,
                                   const double *__restrict__ w)
{
    double acc = 0.0;
    for (int64_t e = e0 + sub; e < e1; e += G) acc += Mx[e] * w[Mi[e]];
    return group_sum<G>(acc);
}

// the part of dy that does not push against an infinite bound (the polar of the recession cone of [l, u])
__device__ inline double cut_dy(double dy, double l, double u)
{
    const bool ui = u >= ADMM_INF, li = l <= -ADMM_INF;
    if (ui && li) return 0.0;
    if (ui) return fmin(dy, 0.0);
    if (li) return fmax(dy, 0.0);
    return dy;
}

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

__device__ inline void update_row(const AdmmDev &a, int64_t i, double zt)
{
    const double z = a.z[i], y = a.y[i], rho = a.rho[i];
    const double v = a.alpha * zt + (1.0 - a.alpha) * z;
    const double zn = fmin(fmax(v + y / rho, a.l[i]), a.u[i]);
    const double yn = y + rho * (v - zn);
    a.z[i] = zn;
    a.y[i] = yn;
    a.dy[i] = yn - y;
}

// workgroups [0, nbs): short rows, 16 of them each; [nbs, nbs + nbl): long rows, 4 each; the rest: 256 entries of x each
__global__ __launch_bounds__(256) void k_admm_update(AdmmDev a, unsigned nbs, unsigned nbl)
{
    if (blockIdx.x < nbs) {
        const int sub = threadIdx.x & 15;
        const int64_t t = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
        const bool live = t < a.ns;
        const int64_t i = live ? a.rs[t] : 0;
        const double zt = group_dot<16>(live ? a.Tp[i] : 0, live ? a.Tp[i + 1] : 0, sub, a.Ti, a.Tx, a.xt);
        if (live && sub == 0) update_row(a, i, zt);
    } else if (blockIdx.x < nbs + nbl) {
        const int sub = threadIdx.x & 63;
        const int64_t t = (int64_t)(blockIdx.x - nbs) * 4 + (threadIdx.x >> 6);
        const bool live = t < a.nl;
        const int64_t i = live ? a.rl[t] : 0;
        const double zt = group_dot<64>(live ? a.Tp[i] : 0, live ? a.Tp[i + 1] : 0, sub, a.Ti, a.Tx, a.xt);
        if (live && sub == 0) update_row(a, i, zt);
    } else {
        const int64_t j = (int64_t)(blockIdx.x - nbs - nbl) * 256 + threadIdx.x;
        if (j < a.n) {
            const double x = a.x[j];
            const double xn = a.alpha * a.xt[j] + (1.0 - a.alpha) * x;
            a.x[j] = xn;
            a.dx[j] = xn - x;
        }
    }
}

// ---- residuals ---------------------------------------------------------------------------------------------------------
// Entries of the result (include/kvxhip.h).  Those of RK come from the rows of A, those of CK from the columns; bit k of
// SUMMASK: entry k is a sum, otherwise a maximum.
__device__ const int RK[10] = {0, 1, 2, 7, 8, 9, 14, 15, 20, 21};
__device__ const int CK[14] = {3, 4, 5, 6, 10, 11, 12, 13, 16, 17, 18, 19, 22, 23};
constexpr unsigned SUMMASK = (1u << 15) | (1u << 18) | (1u << 22) | (1u << 23);
constexpr unsigned ROWMASK = (1u << 0) | (1u << 1) | (1u << 2) | (1u << 7) | (1u << 8) | (1u << 9) | (1u << 14) | (1u << 15) | (1u << 20) |
                             (1u << 21);

// v[k] of every thread -> one value per workgroup, in a fixed order: butterfly inside a wavefront, the four wavefronts in order.
// LSUM: bit k set = local entry k is a sum.  part[key[k] * nb + blockIdx.x] receives the result.
template <int K, unsigned LSUM>
__device__ inline void block_reduce(double (&v)[K], double *sh, const int *key, double *__restrict__ part, int64_t nb)
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
    if (threadIdx.x < K) {
        const int k = threadIdx.x;
        const bool sum = (LSUM >> k) & 1u;
        double r = sh[k];
        for (int w = 1; w < 4; w++) r = sum ? r + sh[w * K + k] : fmax(r, sh[w * K + k]);
        part[(int64_t)key[k] * nb + blockIdx.x] = r;
    }
}

__device__ inline void residual_row(const AdmmDev &a, int64_t i, double ax, double adx, double (&v)[10])
{
    const double z = a.z[i], l = a.l[i], u = a.u[i], ei = a.Einv[i];
    v[0] = fabs(ax - z);
    v[1] = fabs(ax);
    v[2] = fabs(z);
    v[3] = fabs(ei * (ax - z));
    v[4] = fabs(ei * ax);
    v[5] = fabs(ei * z);
    const double d = cut_dy(a.dy[i], l, u);
    v[6] = fabs(a.E[i] * d * a.cinv);
    v[7] = ((u < ADMM_INF ? u * fmax(d, 0.0) : 0.0) + (l > -ADMM_INF ? l * fmin(d, 0.0) : 0.0)) * a.cinv;
    if (u < ADMM_INF) v[8] = ei * adx;
    if (l > -ADMM_INF) v[9] = -(ei * adx);
}

// workgroups [0, nbs): short rows; [nbs, nbs + nbl): long rows; the rest: 16 columns each
__global__ __launch_bounds__(256) void k_admm_residuals(AdmmDev a, unsigned nbs, unsigned nbl, double *__restrict__ part)
{
    __shared__ double sh[4 * 14];
    const int64_t nb = gridDim.x;
    if (blockIdx.x < nbs + nbl) {
        double v[10] = {NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, 0.0, NEG_MAX, NEG_MAX};
        if (blockIdx.x < nbs) {
            const int sub = threadIdx.x & 15;
            const int64_t t = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
            const bool live = t < a.ns;
            const int64_t i = live ? a.rs[t] : 0;
            const int64_t e0 = live ? a.Tp[i] : 0, e1 = live ? a.Tp[i + 1] : 0;
            const double ax = group_dot<16>(e0, e1, sub, a.Ti, a.Tx, a.x);
            const double adx = group_dot<16>(e0, e1, sub, a.Ti, a.Tx, a.dx);
            if (live && sub == 0) residual_row(a, i, ax, adx, v);
        } else {
            const int sub = threadIdx.x & 63;
            const int64_t t = (int64_t)(blockIdx.x - nbs) * 4 + (threadIdx.x >> 6);
            const bool live = t < a.nl;
            const int64_t i = live ? a.rl[t] : 0;
            const int64_t e0 = live ? a.Tp[i] : 0, e1 = live ? a.Tp[i + 1] : 0;
            const double ax = group_dot<64>(e0, e1, sub, a.Ti, a.Tx, a.x);
            const double adx = group_dot<64>(e0, e1, sub, a.Ti, a.Tx, a.dx);
            if (live && sub == 0) residual_row(a, i, ax, adx, v);
        }
        block_reduce<10, (1u << 7)>(v, sh, RK, part, nb);
    } else {
        double v[14] = {NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, 0.0, NEG_MAX, 0.0, 0.0};
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
        if (live && sub == 0) {
            const double q = a.q[j], x = a.x[j], dx = a.dx[j], s = a.Dinv[j];
            const double rd = px + q + aty;
            v[0] = fabs(rd);
            v[1] = fabs(px);
            v[2] = fabs(aty);
            v[3] = fabs(q);
            v[4] = fabs(rd * s * a.cinv);
            v[5] = fabs(px * s * a.cinv);
            v[6] = fabs(aty * s * a.cinv);
            v[7] = fabs(q * s * a.cinv);
            v[8] = fabs(atd * s * a.cinv);
            v[9] = fabs(a.D[j] * dx);
            v[10] = q * dx * a.cinv;
            v[11] = fabs(pdx * s * a.cinv);
            v[12] = x * px;
            v[13] = q * x;
        }
        block_reduce<14, (1u << 10) | (1u << 12) | (1u << 13)>(v, sh, CK, part, nb);
    }
}

// second stage: one wavefront per entry k of the result, over the workgroups that hold it (rows: [0, nbr), columns: [nbr, nb))
__global__ __launch_bounds__(64) void k_admm_reduce2(const double *__restrict__ part, int64_t nbr, int64_t nb, double *__restrict__ res)
{
    const int k = blockIdx.x;
    const bool sum = (SUMMASK >> k) & 1u, row = (ROWMASK >> k) & 1u;
    const int64_t b0 = row ? 0 : nbr, b1 = row ? nbr : nb;
    const double *p = part + (int64_t)k * nb;
    double acc = sum ? 0.0 : NEG_MAX;
    for (int64_t b = b0 + threadIdx.x; b < b1; b += 64) acc = sum ? acc + p[b] : fmax(acc, p[b]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(acc, o);
        acc = sum ? acc + w : fmax(acc, w);
    }
    if (threadIdx.x == 0) res[k] = acc;
}

}  // namespace

void launch_admm_rhs(hipStream_t st, const AdmmDev &a)
{
    if (a.n > 0) hipLaunchKernelGGL(k_admm_rhs, dim3(blocks_of(a.n * 16)), dim3(256), 0, st, a);
}

void launch_admm_update(hipStream_t st, const AdmmDev &a)
{
    const unsigned nbs = blocks_of(a.ns * 16), nbl = blocks_of(a.nl * 64), nbx = blocks_of(a.n);
    if (nbs + nbl + nbx > 0) hipLaunchKernelGGL(k_admm_update, dim3(nbs + nbl + nbx), dim3(256), 0, st, a, nbs, nbl);
}

int64_t admm_residual_blocks(const AdmmDev &a)
{
    return (int64_t)blocks_of(a.ns * 16) + blocks_of(a.nl * 64) + blocks_of(a.n * 16);
}

void launch_admm_residuals(hipStream_t st, const AdmmDev &a, double *part, double *res)
{
    const unsigned nbs = blocks_of(a.ns * 16), nbl = blocks_of(a.nl * 64), nbc = blocks_of(a.n * 16);
    const unsigned nb = nbs + nbl + nbc;
    if (nb > 0) hipLaunchKernelGGL(k_admm_residuals, dim3(nb), dim3(256), 0, st, a, nbs, nbl, part);
    hipLaunchKernelGGL(k_admm_reduce2, dim3(ADMM_NRES), dim3(64), 0, st, part, (int64_t)(nbs + nbl), (int64_t)nb, res);
}
}  // namespace kvx
