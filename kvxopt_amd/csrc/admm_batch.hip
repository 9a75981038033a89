// The ADMM iteration of admm.hip for a batch: B data sets (q_b, l_b, u_b) on one scaled A and P, one rho vector and one kept
// factor of S = P + sigma I + A' diag(rho) A (kvx_admm_batch_*, admm_api.cpp).  State and data are column-major, member b in
// column b (ld = n or m): the layout kvx_chol_solve_async_dev takes for nrhs = B, so an iteration is
//
//     k_admm_batch_rhs     xt_b = sigma x_b - q_b + A'(rho o z_b - y_b)                       (zero for a frozen member)
//     (solve)              xt = S^-1 xt, B right-hand sides at once
//     k_admm_batch_update  z_b, y_b, dy_b from A xt_b; x_b, dx_b                                  (running members only)
//
// and k_admm_batch_residuals + k_admm_batch_reduce2 give 24 numbers per running member.  The work is cut as in admm.hip -- a
// 16-lane group per column or short row of A, a wavefront per row of ADMM_ROW_WAVE entries and more -- and a group carries a
// strip of members (workgroup index y): it reads the (index, value) stream of its row or column once and keeps one partial sum
// per member.  Per member the sums run in the order of admm.hip: strided partial sums, then the fixed butterfly; every output
// is written once, no floating-point atomics.  run[b] == 0 freezes member b: the flag is uniform over a workgroup, every lane of
// a launch still runs every shuffle (a frozen member contributes empty sums), and nothing of the member is written.
#include "admm_batch.hpp"

namespace kvx {
namespace {

constexpr double ADMM_INF = 1e26;               // |bound| >= INFTY * 1e-4 is infinite (INFTY = 1e30)
constexpr double ADMM_INFTY = 1e30;
constexpr double NEG_MAX = -1.7976931348623157e308;

static inline unsigned blocks_of(int64_t threads) { return (unsigned)((threads + 255) / 256); }
static inline unsigned strips_of(int64_t B, int strip) { return (unsigned)((B + strip - 1) / strip); }

template <int G>
__device__ inline double group_sum(double v)
{
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
    return v;
}

// bit s set: member b0 + s exists and runs
template <int NB>
__device__ inline unsigned strip_mask(const AdmmBatchDev &b, int64_t b0)
{
    unsigned act = 0;
#pragma unroll
    for (int s = 0; s < NB; s++)
        if (b0 + s < b.B && b.run[b0 + s] != 0) act |= 1u << s;
    return act;
}

// out[s] = sum_e Mx[e] * w[Mi[e] + (b0 + s) ld] over e in [e0, e1), lane `sub` of G taking e0 + sub, e0 + sub + G, ...
template <int G, int NB>
__device__ inline void strip_dot(int64_t e0, int64_t e1, int sub, const int64_t *__restrict__ Mi, const double *__restrict__ Mx,
                                 const double *__restrict__ w, int64_t ld, int64_t b0, unsigned act, double (&out)[NB])
{
    double acc[NB];
#pragma unroll
    for (int s = 0; s < NB; s++) acc[s] = 0.0;
    for (int64_t e = e0 + sub; e < e1; e += G) {
        const int64_t i = Mi[e];
        const double v = Mx[e];
#pragma unroll
        for (int s = 0; s < NB; s++)
            if ((act >> s) & 1u) acc[s] += v * w[i + (b0 + s) * ld];
    }
#pragma unroll
    for (int s = 0; s < NB; s++) out[s] = group_sum<G>(acc[s]);
}

__device__ inline double cut_dy(double dy, double l, double u)
{
    const bool ui = u >= ADMM_INF, li = l <= -ADMM_INF;
    if (ui && li) return 0.0;
    if (ui) return fmin(dy, 0.0);
    if (li) return fmax(dy, 0.0);
    return dy;
}

// ---- data -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_admm_batch_scale_q(AdmmBatchDev b, double c, const double *__restrict__ raw)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, bm = blockIdx.y;
    if (j < b.a.n) b.q[j + bm * b.a.n] = raw ? (c * b.a.D[j]) * raw[j + bm * b.a.n] : b.a.q[j];
}

__global__ __launch_bounds__(256) void k_admm_batch_scale_bound(AdmmBatchDev b, bool upper, const double *__restrict__ raw)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, bm = blockIdx.y;
    if (i >= b.a.m) return;
    double *out = upper ? b.u : b.l;
    if (!raw) {
        out[i + bm * b.a.m] = upper ? b.a.u[i] : b.a.l[i];
        return;
    }
    const double v = raw[i + bm * b.a.m];
    const bool inf = upper ? v >= ADMM_INF : v <= -ADMM_INF;
    out[i + bm * b.a.m] = inf ? (upper ? ADMM_INFTY : -ADMM_INFTY) : b.a.E[i] * v;
}

// ---- the iteration ----------------------------------------------------------------------------------------------------------
// workgroup (x, y): 16 columns of A, the members of strip y
__global__ __launch_bounds__(256) void k_admm_batch_rhs(AdmmBatchDev b)
{
    const AdmmDev &a = b.a;
    const int sub = threadIdx.x & 15;
    const int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int64_t b0 = (int64_t)blockIdx.y * ADMM_STRIP;
    const unsigned act = strip_mask<ADMM_STRIP>(b, b0);
    const bool live = j < a.n;
    const int64_t e0 = live ? a.Ap[j] : 0, e1 = live ? a.Ap[j + 1] : 0;
    double acc[ADMM_STRIP];
#pragma unroll
    for (int s = 0; s < ADMM_STRIP; s++) acc[s] = 0.0;
    for (int64_t e = e0 + sub; e < e1; e += 16) {
        const int64_t i = a.Ai[e];
        const double ax = a.Ax[e], rho = a.rho[i];
#pragma unroll
        for (int s = 0; s < ADMM_STRIP; s++)
            if ((act >> s) & 1u) {
                const int64_t t = i + (b0 + s) * a.m;
                acc[s] += ax * (rho * b.z[t] - b.y[t]);
            }
    }
#pragma unroll
    for (int s = 0; s < ADMM_STRIP; s++) {
        const double sum = group_sum<16>(acc[s]);
        if (live && sub == 0 && b0 + s < b.B) {
            const int64_t t = j + (b0 + s) * a.n;
            b.xt[t] = ((act >> s) & 1u) ? (a.sigma * b.x[t] - b.q[t]) + sum : 0.0;     // a frozen member is solved for zero
        }
    }
}

__device__ inline void update_row(const AdmmBatchDev &b, int64_t i, int64_t t, double zt)
{
    const double z = b.z[t], y = b.y[t], rho = b.a.rho[i];
    const double v = b.a.alpha * zt + (1.0 - b.a.alpha) * z;
    const double zn = fmin(fmax(v + y / rho, b.l[t]), b.u[t]);
    const double yn = y + rho * (v - zn);
    b.z[t] = zn;
    b.y[t] = yn;
    b.dy[t] = yn - y;
}

// workgroups x in [0, nbs): short rows, 16 of them each; [nbs, nbs + nbl): long rows, 4 each; the rest: 256 entries of x each
__global__ __launch_bounds__(256) void k_admm_batch_update(AdmmBatchDev b, unsigned nbs, unsigned nbl)
{
    const AdmmDev &a = b.a;
    const int64_t b0 = (int64_t)blockIdx.y * ADMM_STRIP;
    const unsigned act = strip_mask<ADMM_STRIP>(b, b0);
    if (blockIdx.x < nbs + nbl) {
        const bool shortrow = blockIdx.x < nbs;
        const int sub = shortrow ? (threadIdx.x & 15) : (threadIdx.x & 63);
        const int64_t t = shortrow ? (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4) : (int64_t)(blockIdx.x - nbs) * 4 + (threadIdx.x >> 6);
        const bool live = t < (shortrow ? a.ns : a.nl);
        const int64_t i = live ? (shortrow ? a.rs[t] : a.rl[t]) : 0;
        const int64_t e0 = live ? a.Tp[i] : 0, e1 = live ? a.Tp[i + 1] : 0;
        double zt[ADMM_STRIP];
        if (shortrow) strip_dot<16, ADMM_STRIP>(e0, e1, sub, a.Ti, a.Tx, b.xt, a.n, b0, act, zt);
        else strip_dot<64, ADMM_STRIP>(e0, e1, sub, a.Ti, a.Tx, b.xt, a.n, b0, act, zt);
        if (live && sub == 0) {
#pragma unroll
            for (int s = 0; s < ADMM_STRIP; s++)
                if ((act >> s) & 1u) update_row(b, i, i + (b0 + s) * a.m, zt[s]);
        }
    } else {
        const int64_t j = (int64_t)(blockIdx.x - nbs - nbl) * 256 + threadIdx.x;
        if (j < a.n) {
#pragma unroll
            for (int s = 0; s < ADMM_STRIP; s++)
                if ((act >> s) & 1u) {
                    const int64_t t = j + (b0 + s) * a.n;
                    const double x = b.x[t];
                    const double xn = a.alpha * b.xt[t] + (1.0 - a.alpha) * x;
                    b.x[t] = xn;
                    b.dx[t] = xn - x;
                }
        }
    }
}

// ---- residuals: the entries of admm.hip (include/kvxhip.h, kvx_admm_iterate), 24 per member -----------------------------------
__device__ const int RK[10] = {0, 1, 2, 7, 8, 9, 14, 15, 20, 21};
__device__ const int CK[14] = {3, 4, 5, 6, 10, 11, 12, 13, 16, 17, 18, 19, 22, 23};
constexpr unsigned SUMMASK = (1u << 15) | (1u << 18) | (1u << 22) | (1u << 23);
constexpr unsigned ROWMASK = (1u << 0) | (1u << 1) | (1u << 2) | (1u << 7) | (1u << 8) | (1u << 9) | (1u << 14) | (1u << 15) | (1u << 20) |
                             (1u << 21);

// v[k] of every thread -> one value per workgroup: butterfly inside a wavefront, the four wavefronts in order.
// part[key[k] * nb + blockIdx.x] receives the result (part: the member's 24 x nb block).  Ends with a barrier: sh is free again.
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
    __syncthreads();
}

__device__ inline void residual_row(const AdmmBatchDev &b, int64_t i, int64_t t, double ax, double adx, double (&v)[10])
{
    const AdmmDev &a = b.a;
    const double z = b.z[t], l = b.l[t], u = b.u[t], ei = a.Einv[i];
    v[0] = fabs(ax - z);
    v[1] = fabs(ax);
    v[2] = fabs(z);
    v[3] = fabs(ei * (ax - z));
    v[4] = fabs(ei * ax);
    v[5] = fabs(ei * z);
    const double d = cut_dy(b.dy[t], l, u);
    v[6] = fabs(a.E[i] * d * a.cinv);
    v[7] = ((u < ADMM_INF ? u * fmax(d, 0.0) : 0.0) + (l > -ADMM_INF ? l * fmin(d, 0.0) : 0.0)) * a.cinv;
    if (u < ADMM_INF) v[8] = ei * adx;
    if (l > -ADMM_INF) v[9] = -(ei * adx);
}

// workgroups x in [0, nbs): short rows; [nbs, nbs + nbl): long rows; the rest: 16 columns each; y: the strip of members
__global__ __launch_bounds__(256) void k_admm_batch_residuals(AdmmBatchDev b, unsigned nbs, unsigned nbl, double *__restrict__ part)
{
    __shared__ double sh[4 * 14];
    const AdmmDev &a = b.a;
    const int64_t nb = gridDim.x;
    const int64_t b0 = (int64_t)blockIdx.y * ADMM_RSTRIP;
    const unsigned act = strip_mask<ADMM_RSTRIP>(b, b0);
    if (blockIdx.x < nbs + nbl) {
        const bool shortrow = blockIdx.x < nbs;
        const int sub = shortrow ? (threadIdx.x & 15) : (threadIdx.x & 63);
        const int64_t t = shortrow ? (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4) : (int64_t)(blockIdx.x - nbs) * 4 + (threadIdx.x >> 6);
        const bool live = t < (shortrow ? a.ns : a.nl);
        const int64_t i = live ? (shortrow ? a.rs[t] : a.rl[t]) : 0;
        const int64_t e0 = live ? a.Tp[i] : 0, e1 = live ? a.Tp[i + 1] : 0;
        double ax[ADMM_RSTRIP], adx[ADMM_RSTRIP];
        if (shortrow) {
            strip_dot<16, ADMM_RSTRIP>(e0, e1, sub, a.Ti, a.Tx, b.x, a.n, b0, act, ax);
            strip_dot<16, ADMM_RSTRIP>(e0, e1, sub, a.Ti, a.Tx, b.dx, a.n, b0, act, adx);
        } else {
            strip_dot<64, ADMM_RSTRIP>(e0, e1, sub, a.Ti, a.Tx, b.x, a.n, b0, act, ax);
            strip_dot<64, ADMM_RSTRIP>(e0, e1, sub, a.Ti, a.Tx, b.dx, a.n, b0, act, adx);
        }
#pragma unroll
        for (int s = 0; s < ADMM_RSTRIP; s++) {
            if (!((act >> s) & 1u)) continue;                           // uniform over the workgroup
            double v[10] = {NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, 0.0, NEG_MAX, NEG_MAX};
            if (live && sub == 0) residual_row(b, i, i + (b0 + s) * a.m, ax[s], adx[s], v);
            block_reduce<10, (1u << 7)>(v, sh, RK, part + (b0 + s) * ADMM_NRES * nb, nb);
        }
    } else {
        const int sub = threadIdx.x & 15;
        const int64_t j = (int64_t)(blockIdx.x - nbs - nbl) * 16 + (threadIdx.x >> 4);
        const bool live = j < a.n;
        const int64_t e0 = live ? a.Ap[j] : 0, e1 = live ? a.Ap[j + 1] : 0;
        double aty[ADMM_RSTRIP], atd[ADMM_RSTRIP], px[ADMM_RSTRIP], pdx[ADMM_RSTRIP];
#pragma unroll
        for (int s = 0; s < ADMM_RSTRIP; s++) aty[s] = atd[s] = 0.0;
        for (int64_t e = e0 + sub; e < e1; e += 16) {
            const int64_t i = a.Ai[e];
            const double w = a.Ax[e];
#pragma unroll
            for (int s = 0; s < ADMM_RSTRIP; s++)
                if ((act >> s) & 1u) {
                    const int64_t t = i + (b0 + s) * a.m;
                    aty[s] += w * b.y[t];
                    atd[s] += w * cut_dy(b.dy[t], b.l[t], b.u[t]);
                }
        }
#pragma unroll
        for (int s = 0; s < ADMM_RSTRIP; s++) {
            aty[s] = group_sum<16>(aty[s]);
            atd[s] = group_sum<16>(atd[s]);
        }
        const int64_t f0 = live ? a.Fp[j] : 0, f1 = live ? a.Fp[j + 1] : 0;
        strip_dot<16, ADMM_RSTRIP>(f0, f1, sub, a.Fi, a.Fx, b.x, a.n, b0, act, px);
        strip_dot<16, ADMM_RSTRIP>(f0, f1, sub, a.Fi, a.Fx, b.dx, a.n, b0, act, pdx);
#pragma unroll
        for (int s = 0; s < ADMM_RSTRIP; s++) {
            if (!((act >> s) & 1u)) continue;                           // uniform over the workgroup
            double v[14] = {NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, NEG_MAX, 0.0, NEG_MAX, 0.0, 0.0};
            if (live && sub == 0) {
                const int64_t t = j + (b0 + s) * a.n;
                const double q = b.q[t], x = b.x[t], dx = b.dx[t], sc = a.Dinv[j];
                const double rd = px[s] + q + aty[s];
                v[0] = fabs(rd);
                v[1] = fabs(px[s]);
                v[2] = fabs(aty[s]);
                v[3] = fabs(q);
                v[4] = fabs(rd * sc * a.cinv);
                v[5] = fabs(px[s] * sc * a.cinv);
                v[6] = fabs(aty[s] * sc * a.cinv);
                v[7] = fabs(q * sc * a.cinv);
                v[8] = fabs(atd[s] * sc * a.cinv);
                v[9] = fabs(a.D[j] * dx);
                v[10] = q * dx * a.cinv;
                v[11] = fabs(pdx[s] * sc * a.cinv);
                v[12] = x * px[s];
                v[13] = q * x;
            }
            block_reduce<14, (1u << 10) | (1u << 12) | (1u << 13)>(v, sh, CK, part + (b0 + s) * ADMM_NRES * nb, nb);
        }
    }
}

// second stage: workgroup (k, b), one wavefront: entry k of member b over the workgroups that hold it (rows: [0, nbr), columns:
// [nbr, nb)).  The numbers of a frozen member stay what its last check left.
__global__ __launch_bounds__(64) void k_admm_batch_reduce2(AdmmBatchDev b, const double *__restrict__ part, int64_t nbr, int64_t nb,
                                                          double *__restrict__ res)
{
    const int k = blockIdx.x;
    const int64_t bm = blockIdx.y;
    const bool on = b.run[bm] != 0;
    const bool sum = (SUMMASK >> k) & 1u, row = (ROWMASK >> k) & 1u;
    const int64_t b0 = row ? 0 : nbr, b1 = on ? (row ? nbr : nb) : b0;
    const double *p = part + (bm * ADMM_NRES + k) * nb;
    double acc = sum ? 0.0 : NEG_MAX;
    for (int64_t w = b0 + threadIdx.x; w < b1; w += 64) acc = sum ? acc + p[w] : fmax(acc, p[w]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(acc, o);
        acc = sum ? acc + w : fmax(acc, w);
    }
    if (on && threadIdx.x == 0) res[bm * ADMM_NRES + k] = acc;
}

}  // namespace

void launch_admm_batch_scale_q(hipStream_t st, const AdmmBatchDev &b, double c, const double *raw)
{
    if (b.a.n > 0 && b.B > 0) hipLaunchKernelGGL(k_admm_batch_scale_q, dim3(blocks_of(b.a.n), (unsigned)b.B), dim3(256), 0, st, b, c, raw);
}

void launch_admm_batch_scale_bound(hipStream_t st, const AdmmBatchDev &b, bool upper, const double *raw)
{
    if (b.a.m > 0 && b.B > 0) hipLaunchKernelGGL(k_admm_batch_scale_bound, dim3(blocks_of(b.a.m), (unsigned)b.B), dim3(256), 0, st, b, upper, raw);
}

void launch_admm_batch_rhs(hipStream_t st, const AdmmBatchDev &b)
{
    if (b.a.n > 0 && b.B > 0)
        hipLaunchKernelGGL(k_admm_batch_rhs, dim3(blocks_of(b.a.n * 16), strips_of(b.B, ADMM_STRIP)), dim3(256), 0, st, b);
}

void launch_admm_batch_update(hipStream_t st, const AdmmBatchDev &b)
{
    const unsigned nbs = blocks_of(b.a.ns * 16), nbl = blocks_of(b.a.nl * 64), nbx = blocks_of(b.a.n);
    if (nbs + nbl + nbx > 0 && b.B > 0)
        hipLaunchKernelGGL(k_admm_batch_update, dim3(nbs + nbl + nbx, strips_of(b.B, ADMM_STRIP)), dim3(256), 0, st, b, nbs, nbl);
}

int64_t admm_batch_residual_blocks(const AdmmBatchDev &b)
{
    return (int64_t)blocks_of(b.a.ns * 16) + blocks_of(b.a.nl * 64) + blocks_of(b.a.n * 16);
}

void launch_admm_batch_residuals(hipStream_t st, const AdmmBatchDev &b, double *part, double *res)
{
    const unsigned nbs = blocks_of(b.a.ns * 16), nbl = blocks_of(b.a.nl * 64), nbc = blocks_of(b.a.n * 16);
    const unsigned nb = nbs + nbl + nbc;
    if (b.B <= 0) return;
    if (nb > 0) hipLaunchKernelGGL(k_admm_batch_residuals, dim3(nb, strips_of(b.B, ADMM_RSTRIP)), dim3(256), 0, st, b, nbs, nbl, part);
    hipLaunchKernelGGL(k_admm_batch_reduce2, dim3(ADMM_NRES, (unsigned)b.B), dim3(64), 0, st, b, part, (int64_t)(nbs + nbl), (int64_t)nb, res);
}
}  // namespace kvx
