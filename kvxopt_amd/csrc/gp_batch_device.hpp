// What k_gp_batch (gp_batch.hip) and k_gp_batch_diff (gp_batch_diff.hip) share: the part of a geometric program that depends
// on the point alone.  The blocks of the terms, the evaluator y = exp(u) / sum exp(u) per block (cvxprog.py:2109-2126), the
// products with J = [Df; G], which is never held, the block gradients Df_i = y_i'F_i and the assembly of
// S = H + J' diag(di^2) J from staged rows through kkt_s_add_rows (batch_kkt.hpp): the centred factors
// sqrt(zeta_i y_k) (F_k - Df_i) of cvxprog.py:2135-2150, the rows di_i Df_i and the rows di_k G_k.
//
// EPI says which system a kernel has.  true, the solver: cp's epigraph form of order n + 1 with t in column n, where row 0, the
// objective f_0 - t, is an orthant row like the others: it has the gradient row di_0 (Df_0, -1) and the weight zeta_0 = z_0.
// false, the derivative: the system in x of order n, where block 0 has the weight the caller puts into zeta_0 (1) and no
// gradient row; row 0 of an N-vector is carried and stays 0.  Every function is inlined into its kernel (batch_kkt.hpp says
// why); with EPI = true the bodies are those k_gp_batch had in its own file, statement for statement.
#pragma once
#include "batch_kkt.hpp"
#include "gp_batch.hpp"

#include <cmath>

namespace kvx {
namespace gpdev {

using namespace batchdev;
static_assert(NT == GPB_THREADS, "the shared helpers are written for the workgroup of k_gp_batch");

struct GpMem : KktMem {                       // KktMem::n is the order of the system: nx + 1 with EPI, nx without
    int nx, m, ml, l;                         // nx: the variables of the program (with EPI the column of t); m = mnl + 1 blocks
    const double *F, *g, *G;
    const int *off, *blk;
    double *Gs;                               // the block gradients beside the staged rows
    double *yv, *w;                           // l-vectors in LDS: the weights y at the point, and work
};

// off[i]: the first term of block i, off[m] = l; blk[k]: the block of term k.  The caller's barrier stands after.
template <class Args>
__device__ __forceinline__ void gp_blocks(const Args &a, int *off, int *blk)
{
    const int tid = threadIdx.x, m = a.m;
    if (tid == 0) {
        int o = 0;
        for (int i = 0; i < m; i++) { off[i] = o; o += a.K[i]; }
        off[m] = o;
    }
    __syncthreads();
    for (int i = tid; i < m; i += NT)
        for (int k = off[i]; k < off[i + 1]; k++) blk[k] = i;
}

// The evaluator at the point xe (cvxprog.py:2109-2126): yv = exp(u) / sum exp(u) per block, u = F x + g, the maximum of a
// block taken before exp, and with EPI f (m values, -t on row 0; t = xe[nx]).  A wavefront per block, lanes along its terms.
// Barriers before (the caller's) and after.
template <bool EPI>
__device__ __forceinline__ void lse_eval(const GpMem &M, const double *xe, double *f, double *yv)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < M.l; k += NT) yv[k] = row_dot(M.F, M.l, M.nx, k, xe) + M.g[k];
    __syncthreads();
    for (int i = w; i < M.m; i += NW) {
        const int a = M.off[i], b = M.off[i + 1];
        double mx = -INFINITY;
        for (int k = a + lane; k < b; k += 64) mx = fmax(mx, yv[k]);
        mx = wave_max(mx);
        double sm = 0.0;
        for (int k = a + lane; k < b; k += 64) {
            const double e = exp(yv[k] - mx);
            yv[k] = e;
            sm += e;
        }
        sm = wave_sum(sm);
        for (int k = a + lane; k < b; k += 64) yv[k] /= sm;
        if (EPI && lane == 0) f[i] = mx + log(sm) - (i == 0 ? xe[M.nx] : 0.0);
    }
    __syncthreads();
}

// out += sign * J'(sc o v) (sc null: ones) for the N-vector v, J = [Df; G] at the point whose weights are yv.  Without EPI the
// caller keeps sc_0 v_0 = 0.  Barriers before (the caller's) and after.
template <bool EPI>
__device__ __forceinline__ void jt_add(const GpMem &M, const double *yv, const double *v, const double *sc, double sign, double *out)
{
    for (int k = threadIdx.x; k < M.l; k += NT) {
        const int i = M.blk[k];
        M.w[k] = yv[k] * (sc ? sc[i] * v[i] : v[i]);
    }
    __syncthreads();
    gemv_t_add(M.F, M.l, M.nx, M.w, nullptr, sign, out);
    if (EPI && threadIdx.x == NT - 1) out[M.nx] -= sign * (sc ? sc[0] * v[0] : v[0]);     // column n holds -1 in row 0 and nothing else
    __syncthreads();
    if (M.ml > 0) gemv_t_add(M.G, M.ml, M.nx, v + M.m, sc ? sc + M.m : nullptr, sign, out);
    __syncthreads();
}

// out := J u for the vector u of the system's order; without EPI row 0 is Df_0 u, which the caller does not use.  Barriers
// before (the caller's) and after.
template <bool EPI>
__device__ __forceinline__ void j_mul(const GpMem &M, const double *yv, const double *u, double *out)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < M.l; k += NT) M.w[k] = yv[k] * row_dot(M.F, M.l, M.nx, k, u);
    for (int k = threadIdx.x; k < M.ml; k += NT) out[M.m + k] = row_dot(M.G, M.ml, M.nx, k, u);
    __syncthreads();
    for (int i = w; i < M.m; i += NW) {
        double acc = 0.0;
        for (int k = M.off[i] + lane; k < M.off[i + 1]; k += 64) acc += M.w[k];
        acc = wave_sum(acc);
        if (lane == 0) out[i] = acc - (EPI && i == 0 ? u[M.nx] : 0.0);
    }
    __syncthreads();
}

// dst[j * ldn + c] := sc_i Df_i[c] (sc null: 1) for the blocks i = i0 + j, j < nb, c < nx: a wavefront per entry, lanes along
// the terms of the block.  With EPI and sc, column n of the row as well: -sc_0 on block 0, else 0.  No barrier.
template <bool EPI>
__device__ __forceinline__ void block_grads(const GpMem &M, int i0, int nb, const double *sc, double *dst)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int t = w; t < nb * M.nx; t += NW) {
        const int j = t / M.nx, c = t - j * M.nx, i = i0 + j;
        double acc = 0.0;
        for (int k = M.off[i] + lane; k < M.off[i + 1]; k += 64) acc += M.yv[k] * M.F[k + (int64_t)c * M.l];
        acc = wave_sum(acc);
        if (lane == 0) dst[j * M.ldn + c] = sc ? sc[i] * acc : acc;
    }
    if (EPI && sc)
        for (int j = threadIdx.x; j < nb; j += NT) dst[j * M.ldn + M.nx] = i0 + j == 0 ? -sc[0] : 0.0;
}

// The lower triangle of S = H + J' diag(di^2) J (misc.py:1436-1458) of the system's order from staged rows: the centred factors
// with the weights zeta (m values), then the gradient rows -- every block with EPI, the blocks from 1 without -- then the rows
// of G; with sing A'A as well (the repair of kkt_factor; A has the system's order in columns).  A one-term block has y = 1 and
// Df_i = F_k, so its factors are exact zeros.  Barriers before (the caller's) and after.
template <bool EPI>
__device__ __forceinline__ void gp_assemble(const GpMem &M, const double *zeta, const double *di, bool sing)
{
    const int ne = M.n, nx = M.nx, l = M.l, ml = M.ml, m = M.m, ldn = M.ldn;
    kkt_s_init(M, sing);
    for (int k0 = 0; k0 < l; k0 += GPB_TILE) {                       // sqrt(zeta_i y_k) (F_k - Df_i)
        const int kt = min((int)GPB_TILE, l - k0), i0 = M.blk[k0], nb = M.blk[k0 + kt - 1] - i0 + 1;
        __syncthreads();                                   // the staged rows of the previous step have been read
        block_grads<EPI>(M, i0, nb, nullptr, M.Gs);
        __syncthreads();
        for (int e = threadIdx.x; e < GPB_TILE * ne; e += NT) {
            const int kk = e & (GPB_TILE - 1), c = e / GPB_TILE;
            if (kk < kt) {
                const int k = k0 + kk, i = M.blk[k];
                M.T[kk * ldn + c] = c < nx ? sqrt(zeta[i] * M.yv[k]) * (M.F[k + (int64_t)c * l] - M.Gs[(i - i0) * ldn + c]) : 0.0;
            }
        }
        __syncthreads();
        kkt_s_add_rows(M, kt);
    }
    for (int i0 = EPI ? 0 : 1; i0 < m; i0 += GPB_TILE) {             // di_i Df_i
        const int it = min((int)GPB_TILE, m - i0);
        __syncthreads();
        block_grads<EPI>(M, i0, it, di, M.T);
        __syncthreads();
        kkt_s_add_rows(M, it);
    }
    for (int k0 = 0; k0 < ml; k0 += GPB_TILE) {                      // di_k G_k
        const int kt = min((int)GPB_TILE, ml - k0);
        __syncthreads();
        for (int e = threadIdx.x; e < GPB_TILE * ne; e += NT) {
            const int kk = e & (GPB_TILE - 1), c = e / GPB_TILE;
            if (kk < kt) M.T[kk * ldn + c] = c < nx ? di[m + k0 + kk] * M.G[k0 + kk + (int64_t)c * ml] : 0.0;
        }
        __syncthreads();
        kkt_s_add_rows(M, kt);
    }
    __syncthreads();
}

}  // namespace gpdev
}  // namespace kvx
