// What the kernels of admm.hip, admm_batch.hip and admm_polish.hip share: the constants, the cut of A's rows into 16-lane and
// wavefront groups, the two-stage reduction and the definition of the 24 numbers a termination check reads.  Every sum runs in
// a fixed order -- strided partial sums, then a fixed butterfly; the four wavefronts of a workgroup in order; the workgroups
// strided by 64, then the butterfly again -- so a value does not depend on which kernel asked for it.
#pragma once
#include "admm.hpp"

namespace kvx {

constexpr double ADMM_INF = 1e26;               // |bound| >= INFTY * 1e-4 is infinite
constexpr double ADMM_INFTY = 1e30;
constexpr double NEG_MAX = -1.7976931348623157e308;

static inline unsigned blocks_of(int64_t threads) { return (unsigned)((threads + 255) / 256); }

// Workgroups of 256 threads a launch over the problem needs: nbs for the short rows (16 each), nbl for the long rows (4 each),
// nbc for the columns by 16-lane groups (16 each), nbx / nbm for the entries of an n- / m-vector (256 each).
struct AdmmGrid {
    unsigned nbs, nbl, nbc, nbx, nbm;
    explicit AdmmGrid(const AdmmDev &a)
        : nbs(blocks_of(a.ns * 16)), nbl(blocks_of(a.nl * 64)), nbc(blocks_of(a.n * 16)), nbx(blocks_of(a.n)), nbm(blocks_of(a.m)) {}
    unsigned rows() const { return nbs + nbl; }
};

// l or u of the scaled problem from the raw bound v and the row scaling *E (read for a finite bound only)
__device__ inline double scaled_bound(double v, const double *E, bool upper)
{
    const bool inf = upper ? v >= ADMM_INF : v <= -ADMM_INF;
    return inf ? (upper ? ADMM_INFTY : -ADMM_INFTY) : *E * v;
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

// ---- rows of A ----------------------------------------------------------------------------------------------------------
// The group of lanes a thread belongs to in a launch over the rows: workgroups [0, nbs) hold 16 short rows each, one per 16
// lanes; [nbs, nbs + nbl) hold 4 long rows each, one per wavefront.  A group without a row (row = -1) has the empty range
// [0, 0): every lane of a launch still runs every shuffle.  `wide` is uniform over a workgroup.
struct RowGroup {
    int64_t row, e0, e1;                        // the row, its entries [e0, e1) of Ti / Tx
    int sub;                                    // the lane inside the group
    bool wide;                                  // a wavefront, not 16 lanes
    __device__ bool lead() const { return row >= 0 && sub == 0; }        // the one lane that owns the row's results
};

__device__ inline RowGroup row_group(const AdmmDev &a, unsigned nbs, unsigned block, unsigned thread)
{
    RowGroup g;
    g.wide = block >= nbs;
    g.sub = thread & (g.wide ? 63 : 15);
    const int64_t t = g.wide ? (int64_t)(block - nbs) * 4 + (thread >> 6) : (int64_t)block * 16 + (thread >> 4);
    const bool live = t < (g.wide ? a.nl : a.ns);
    const int64_t i = live ? (g.wide ? a.rl : a.rs)[t] : 0;
    g.row = live ? i : -1;
    g.e0 = live ? a.Tp[i] : 0;
    g.e1 = live ? a.Tp[i + 1] : 0;
    return g;
}

// (A w)_row, on every lane of the group
__device__ inline double row_dot(const AdmmDev &a, const RowGroup &g, const double *__restrict__ w)
{
    return g.wide ? group_dot<64>(g.e0, g.e1, g.sub, a.Ti, a.Tx, w) : group_dot<16>(g.e0, g.e1, g.sub, a.Ti, a.Tx, w);
}

// ---- the two stages of a reduction --------------------------------------------------------------------------------------
// LSUM: bit k set = local entry k is a sum, otherwise a maximum.  What a thread without a value contributes:
template <int K, unsigned LSUM>
__device__ inline void reduce_identity(double (&v)[K])
{
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = ((LSUM >> k) & 1u) ? 0.0 : NEG_MAX;
}

// v[k] of every thread -> one value per workgroup, in a fixed order: butterfly inside a wavefront, the four wavefronts in order.
// part[key[k] * stride + slot] receives entry k.  A caller that uses sh again issues a barrier first.
template <int K, unsigned LSUM>
__device__ inline void block_reduce(double (&v)[K], double *sh, const int *key, double *__restrict__ part, int64_t stride, int64_t slot)
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
        part[(int64_t)key[k] * stride + slot] = r;
    }
}

// second stage, one wavefront: the per-workgroup values p[b0 .. b1) into one, strided by 64, then the butterfly
__device__ inline double wave_reduce2(const double *__restrict__ p, int64_t b0, int64_t b1, bool sum)
{
    double acc = sum ? 0.0 : NEG_MAX;
    for (int64_t b = b0 + threadIdx.x; b < b1; b += 64) acc = sum ? acc + p[b] : fmax(acc, p[b]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(acc, o);
        acc = sum ? acc + w : fmax(acc, w);
    }
    return acc;
}

// ---- the 24 numbers (include/kvxhip.h, kvx_admm_iterate) --------------------------------------------------------------------
// Those of RK come from the rows of A (residual_row), those of CK from the columns (residual_col); bit k of SUMMASK: entry k is
// a sum, otherwise a maximum.  The row workgroups of the first stage are [0, nbr), the column workgroups [nbr, nb).
__device__ constexpr int RK[10] = {0, 1, 2, 7, 8, 9, 14, 15, 20, 21};
__device__ constexpr int CK[14] = {3, 4, 5, 6, 10, 11, 12, 13, 16, 17, 18, 19, 22, 23};
constexpr unsigned SUMMASK = (1u << 15) | (1u << 18) | (1u << 22) | (1u << 23);

template <int K>
constexpr unsigned entries_of(const int (&key)[K])                      // bit key[k] for every k
{
    unsigned m = 0;
    for (int k = 0; k < K; k++) m |= 1u << key[k];
    return m;
}
template <int K>
constexpr unsigned local_sums(const int (&key)[K])                      // the LSUM of block_reduce for the entries key[k]
{
    unsigned m = 0;
    for (int k = 0; k < K; k++) m |= ((SUMMASK >> key[k]) & 1u) << k;
    return m;
}
constexpr unsigned ROWMASK = entries_of(RK), ROW_LSUM = local_sums(RK), COL_LSUM = local_sums(CK);
static_assert((ROWMASK ^ entries_of(CK)) == (1u << ADMM_NRES) - 1, "every entry comes from the rows or from the columns");

// the range of first-stage workgroups that hold entry k
__device__ inline void residual_range(int k, int64_t nbr, int64_t nb, int64_t *b0, int64_t *b1)
{
    const bool row = (ROWMASK >> k) & 1u;
    *b0 = row ? 0 : nbr;
    *b1 = row ? nbr : nb;
}

// The two relaxations below are a sum of two products, of which one is fused into the addition.  Which one decides the last
// bit, so it is written out, not left to the compiler's contraction: alpha zt is the fused product of a row, (1 - alpha) x
// that of an entry of x.

// z, y, dy of one row from zt = (A xt)_i
__device__ inline void update_row(double alpha, double rho, double l, double u, double zt, double *z, double *y, double *dy)
{
    const double z0 = *z, y0 = *y;
    const double v = fma(alpha, zt, (1.0 - alpha) * z0);
    const double zn = fmin(fmax(v + y0 / rho, l), u);
    const double yn = fma(rho, v - zn, y0);
    *z = zn;
    *y = yn;
    *dy = yn - y0;
}

// x, dx of one entry from xt
__device__ inline void update_x(double alpha, double xt, double *x, double *dx)
{
    const double x0 = *x;
    const double xn = fma(1.0 - alpha, x0, alpha * xt);
    *x = xn;
    *dx = xn - x0;
}

// the entries RK of one row: ax = (A x)_i, adx = (A dx)_i; e, ei: E_i and its inverse
__device__ inline void residual_row(double z, double l, double u, double dy, double e, double ei, double cinv, double ax, double adx,
                                    double (&v)[10])
{
    v[0] = fabs(ax - z);
    v[1] = fabs(ax);
    v[2] = fabs(z);
    v[3] = fabs(ei * (ax - z));
    v[4] = fabs(ei * ax);
    v[5] = fabs(ei * z);
    const double d = cut_dy(dy, l, u);
    v[6] = fabs(e * d * cinv);
    v[7] = ((u < ADMM_INF ? u * fmax(d, 0.0) : 0.0) + (l > -ADMM_INF ? l * fmin(d, 0.0) : 0.0)) * cinv;
    if (u < ADMM_INF) v[8] = ei * adx;
    if (l > -ADMM_INF) v[9] = -(ei * adx);
}

// the entries CK of one column: px = (P x)_j, pdx = (P dx)_j, aty = (A' y)_j, atd = (A' cut_dy)_j; d, s: D_j and its inverse
__device__ inline void residual_col(double q, double x, double dx, double d, double s, double cinv, double px, double pdx, double aty,
                                    double atd, double (&v)[14])
{
    const double rd = px + q + aty;
    v[0] = fabs(rd);
    v[1] = fabs(px);
    v[2] = fabs(aty);
    v[3] = fabs(q);
    v[4] = fabs(rd * s * cinv);
    v[5] = fabs(px * s * cinv);
    v[6] = fabs(aty * s * cinv);
    v[7] = fabs(q * s * cinv);
    v[8] = fabs(atd * s * cinv);
    v[9] = fabs(d * dx);
    v[10] = q * dx * cinv;
    v[11] = fabs(pdx * s * cinv);
    v[12] = x * px;
    v[13] = q * x;
}
}  // namespace kvx
