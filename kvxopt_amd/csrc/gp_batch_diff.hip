// k_gp_batch_diff: one workgroup (256 threads, four wavefronts) differentiates one solved member of gp_batch at its returned
// x, y, s, z (gp_batch_diff.hpp).  The weights y = softmax(F x + g) are taken once at x.  The reduced matrix
// S = H + J' diag(z / s) J of order n is assembled from the staged rows k_gp_batch stages (gp_batch_device.hpp, EPI = false:
// block 0 has the weight 1 and no gradient row) and factored through batch_kkt.hpp; neither H nor J = [Df_1 .. Df_mnl; G] is
// held.  Where S alone fails its factorisation and p > 0 the member is factored on S + A'A, the repair of misc.kkt_chol2
// (kkt_factor): at a vertex of a program whose blocks have one term each H is zero, the inactive rows weigh 1e-15 of the active
// ones, and the rank of S in float64 comes from A.  The rows are an orthant, so diag(s / z) linearises complementarity exactly
// at any point.  As in k_qp_batch_diff the right-hand side is kept, the residual of the full 3 x 3 system is formed in float64
// from F, G, A in HBM, and the same factors solve for the correction.  One pass over the terms serves the first and the third
// block row: with t_k = F_k u and c_i = sum_k y_k t_k over block i,
//
//     H u + J' uz = F' w + G' uzl,   w_k = y_k (zeta_i (t_k - c_i) + uz_i),      (J u)_i = c_i,
//
// and at the solution w is the gradient of g (centre()).  An N-vector has row 0 for the objective, as the solver's s and z have
// it; here that row is 0 throughout (di_0 = 0), is not read from s and z and is written as 0.
//
// Reverse mode: K u = (-gx, 0, 0); dl/dg = w, dl/dh = -uzl, dl/db = -uy, and a matrix with a member stride gets its gradient as
// outer products written by the workgroup: dl/dF = a ux' + w x' with a_k = zeta_i y_k.  Forward mode: with v = dF x + dg the
// same pass gives the right-hand side, bx = -(F'(zeta y (v - c)) + dF' a + dG' zl + dA' y), by = db - dA x,
// bz = (-c_i; dh - dG x), and ds = -(s / z) dz.
//
// The rules of gp_batch.hip hold: every sum has a fixed order, no atomics, no communication between workgroups; every loop is
// bounded by n, N, p, l, K_i or `refinement`; every branch around a barrier is taken on values all threads read from the same
// LDS words.  A NaN or Inf in s or z (rows >= 1) ends in exit 2 through their test, one in x, F, g, G or A through the pivot
// test.
#include "gp_batch_diff.hpp"
#include "batch_kkt.hpp"
#include "gp_batch_device.hpp"

#include <cmath>

namespace kvx {
namespace {

using namespace gpdev;

struct Member : GpMem {                       // KktMem::n is nx, the order of the system
    int N;
    double *x, *bx, *ux, *rx, *by, *uy, *ry, *di, *sz, *bz, *uz, *rz, *ws, *zeta, *tv, *red;
};

// With t = M.tv: ws_i := sum_k y_k t_k over block i (every block), then w_k := y_k (zeta_i (t_k - ws_i) + uz_i), uz null or on
// block 0: 0.  A wavefront per block, lanes along its terms.  Barriers before (the caller's) and after.
__device__ __forceinline__ void centre(const Member &M, const double *uz)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int i = w; i < M.m; i += NW) {
        double acc = 0.0;
        for (int k = M.off[i] + lane; k < M.off[i + 1]; k += 64) acc += M.yv[k] * M.tv[k];
        acc = wave_sum(acc);
        if (lane == 0) M.ws[i] = acc;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < M.l; k += NT) {
        const int i = M.blk[k];
        M.w[k] = M.yv[k] * (M.zeta[i] * (M.tv[k] - M.ws[i]) + (uz && i > 0 ? uz[i] : 0.0));
    }
    __syncthreads();
}

// (vx, vy, vz) := K^-1 (vx, vy, vz) by the reduced solve (misc.py:1489-1563) in the scaling di = sqrt(z / s), as kkt_solve of
// gp_batch.hip; kkt_reduced_solve leaves W uz, so di once more.  Row 0 of vz ends as 0.  Barriers before (the caller's) and
// after.
__device__ __forceinline__ void kkt_solve(const Member &M, bool sing, double *vx, double *vy, double *vz)
{
    for (int k = threadIdx.x; k < M.N; k += NT) vz[k] *= M.di[k];
    __syncthreads();
    jt_add<false>(M, M.yv, vz, M.di, 1.0, vx);
    kkt_reduced_solve(M, sing, vx, vy);
    j_mul<false>(M, M.yv, vx, M.ws);
    for (int k = threadIdx.x; k < M.N; k += NT) vz[k] = k == 0 ? 0.0 : M.di[k] * (M.di[k] * M.ws[k] - vz[k]);
    __syncthreads();
}

__global__ void __launch_bounds__(GPB_THREADS) k_gp_batch_diff(GpDiffArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, n = a.n, m = a.m, l = a.l, ml = a.ml, p = a.p;
    const int64_t bm = blockIdx.x;
    const bool jvp = a.mode == GPD_JVP;
    const gpdiff::Layout L = gpdiff::layout(n, m, l, ml, p);
    const int N = L.N;
    int *const off = reinterpret_cast<int *>(lds + L.off), *const blk = reinterpret_cast<int *>(lds + L.blk);
    Member M;
    M.n = n; M.p = p; M.ldn = L.ldn; M.ldp = L.ldp; M.nx = n; M.m = m; M.ml = ml; M.l = l; M.N = N;
    M.F = a.F + bm * a.sF; M.g = a.c + bm * a.sc; M.G = ml ? a.G + bm * a.sG : nullptr; M.A = p ? a.A + bm * a.sA : nullptr;
    M.off = off; M.blk = blk;
    M.S = lds + L.S; M.T = lds + L.XK; M.X = lds + L.X; M.K = lds + L.K; M.Gs = lds + L.Gs;
    M.x = lds + L.x; M.bx = lds + L.bx; M.ux = lds + L.ux; M.rx = lds + L.rx; M.by = lds + L.by; M.uy = lds + L.uy; M.ry = lds + L.ry;
    M.di = lds + L.di; M.sz = lds + L.sz; M.bz = lds + L.bz; M.uz = lds + L.uz; M.rz = lds + L.rz; M.ws = lds + L.ws;
    M.zeta = lds + L.zeta; M.yv = lds + L.yv; M.w = lds + L.w; M.tv = lds + L.tv; M.red = lds + L.red;
    const double *xs = a.x + bm * n, *ys = p ? a.y + bm * p : nullptr, *ss = a.s + bm * N, *zs = a.z + bm * N;
    double *uxo = a.ux + bm * n, *uyo = p ? a.uy + bm * p : nullptr, *uzo = a.uz + bm * N, *uso = jvp ? a.us + bm * N : nullptr;
    double *ggo = !jvp ? a.gg + bm * l : nullptr, *gao = !jvp && a.ga ? a.ga + bm * l : nullptr;
    double *gF = !jvp && a.gF && a.sF ? a.gF + bm * l * n : nullptr, *gG = !jvp && ml && a.gG && a.sG ? a.gG + bm * ml * n : nullptr;
    double *gA = !jvp && p && a.gA && a.sA ? a.gA + bm * p * n : nullptr;

    // ---- the blocks; the scaling di = sqrt(z / s), W'W = s / z, on the rows from 1; is the member one to differentiate?
    gp_blocks(a, off, blk);
    int code = GPD_DONE;
    bool sing = false;                                     // S was repaired by A'A
    {
        double bad[2] = {0.0, tid == 0 && a.solexit[bm] != 0 ? 1.0 : 0.0};
        for (int k = tid; k < N; k += NT) {
            double dk = 0.0, wk = 0.0;
            if (k > 0) {
                const double sk = ss[k], zk = zs[k];
                if (!(sk > 0.0 && sk < INFINITY && zk > 0.0 && zk < INFINITY)) bad[0] = 1.0;
                dk = sqrt(zk / sk);
                wk = sk / zk;
                if (k < m) M.zeta[k] = zk;
            } else {
                M.zeta[0] = 1.0;
            }
            M.di[k] = dk;
            M.sz[k] = wk;
        }
        if (tid < n) M.x[tid] = xs[tid];
        blk_reduce<2, true>(bad, M.red);                   // its barriers also publish the blocks, di, sz, zeta and x
        if (bad[1] != 0.0) code = GPD_SKIPPED;
        else if (bad[0] != 0.0) code = GPD_FAILED;
    }
    if (code == GPD_DONE) {
        lse_eval<false>(M, M.x, nullptr, M.yv);
        if (!kkt_factor(M, sing, true, [&](bool s) { gp_assemble<false>(M, M.zeta, M.di, s); })) code = GPD_FAILED;
    }
    if (code != GPD_DONE) {
        for (int k = tid; k < N; k += NT) { uzo[k] = 0.0; if (jvp) uso[k] = 0.0; }
        if (tid < n) uxo[tid] = 0.0;
        if (tid < p) uyo[tid] = 0.0;
        if (ggo) for (int k = tid; k < l; k += NT) ggo[k] = 0.0;
        if (gao) for (int k = tid; k < l; k += NT) gao[k] = 0.0;
        if (gF) for (int e = tid; e < l * n; e += NT) gF[e] = 0.0;
        if (gG) for (int e = tid; e < ml * n; e += NT) gG[e] = 0.0;
        if (gA) for (int e = tid; e < p * n; e += NT) gA[e] = 0.0;
        if (tid == 0) a.exitc[bm] = code;
        return;
    }

    // ---- the right-hand side, kept in bx, by, bz for the refinement
    if (!jvp) {
        if (tid < n) M.bx[tid] = -a.gx[bm * n + tid];
        if (tid < p) M.by[tid] = 0.0;
        for (int k = tid; k < N; k += NT) M.bz[k] = 0.0;
    } else {
        const double *dF = a.dF ? a.dF + bm * a.sdF : nullptr, *dg = a.dg ? a.dg + bm * a.sdg : nullptr;
        const double *dG = ml && a.dG ? a.dG + bm * a.sdG : nullptr, *dh = ml && a.dh ? a.dh + bm * a.sdh : nullptr;
        const double *dA = p && a.dA ? a.dA + bm * a.sdA : nullptr, *db = p && a.db ? a.db + bm * a.sdb : nullptr;
        if (tid < n) M.bx[tid] = 0.0;
        if (tid < p) {
            M.ry[tid] = ys[tid];                           // y and zl in the residual vectors, which are not live yet
            M.by[tid] = (db ? db[tid] : 0.0) - (dA ? row_dot(dA, p, n, tid, M.x) : 0.0);
        }
        for (int k = tid; k < ml; k += NT) {
            M.rz[m + k] = zs[m + k];
            M.bz[m + k] = (dh ? dh[k] : 0.0) - (dG ? row_dot(dG, ml, n, k, M.x) : 0.0);
        }
        for (int k = tid; k < l; k += NT) M.tv[k] = (dF ? row_dot(dF, l, n, k, M.x) : 0.0) + (dg ? dg[k] : 0.0);      // v
        __syncthreads();
        centre(M, nullptr);
        for (int i = tid; i < m; i += NT) M.bz[i] = i == 0 ? 0.0 : 0.0 - M.ws[i];
        gemv_t_add(M.F, l, n, M.w, nullptr, -1.0, M.bx);
        __syncthreads();
        if (dF) {
            for (int k = tid; k < l; k += NT) M.tv[k] = M.zeta[M.blk[k]] * M.yv[k];
            __syncthreads();
            gemv_t_add(dF, l, n, M.tv, nullptr, -1.0, M.bx);
            __syncthreads();
        }
        if (dG) gemv_t_add(dG, ml, n, M.rz + m, nullptr, -1.0, M.bx);
        __syncthreads();
        if (dA) gemv_t_add(dA, p, n, M.ry, nullptr, -1.0, M.bx);
    }
    __syncthreads();

    // ---- u = K^-1 b, then `refinement` times u += K^-1 (b - K u)
    if (tid < n) M.ux[tid] = M.bx[tid];
    if (tid < p) M.uy[tid] = M.by[tid];
    for (int k = tid; k < N; k += NT) M.uz[k] = M.bz[k];
    __syncthreads();
    kkt_solve(M, sing, M.ux, M.uy, M.uz);
    for (int it = 0; it < a.refinement; it++) {
        for (int k = tid; k < l; k += NT) M.tv[k] = row_dot(M.F, l, n, k, M.ux);
        if (tid < n) M.rx[tid] = M.bx[tid];
        if (tid < p) M.ry[tid] = M.by[tid] - row_dot(M.A, p, n, tid, M.ux);
        for (int k = tid; k < ml; k += NT)
            M.rz[m + k] = M.bz[m + k] - (row_dot(M.G, ml, n, k, M.ux) - M.sz[m + k] * M.uz[m + k]);
        __syncthreads();
        centre(M, M.uz);
        for (int i = tid; i < m; i += NT) M.rz[i] = i == 0 ? 0.0 : M.bz[i] - (M.ws[i] - M.sz[i] * M.uz[i]);
        gemv_t_add(M.F, l, n, M.w, nullptr, -1.0, M.rx);
        __syncthreads();
        if (p > 0) gemv_t_add(M.A, p, n, M.uy, nullptr, -1.0, M.rx);
        __syncthreads();
        if (ml > 0) gemv_t_add(M.G, ml, n, M.uz + m, nullptr, -1.0, M.rx);
        __syncthreads();
        kkt_solve(M, sing, M.rx, M.ry, M.rz);
        if (tid < n) M.ux[tid] += M.rx[tid];
        if (tid < p) M.uy[tid] += M.ry[tid];
        for (int k = tid; k < N; k += NT) M.uz[k] += M.rz[k];
        __syncthreads();
    }

    // ---- the member's result
    if (tid < n) uxo[tid] = M.ux[tid];
    if (tid < p) uyo[tid] = M.uy[tid];
    for (int k = tid; k < N; k += NT) {
        uzo[k] = M.uz[k];
        if (jvp) uso[k] = 0.0 - M.sz[k] * M.uz[k];
    }
    if (!jvp) {
        for (int k = tid; k < l; k += NT) M.tv[k] = row_dot(M.F, l, n, k, M.ux);
        __syncthreads();
        centre(M, M.uz);                                   // w: the gradient of g
        for (int k = tid; k < l; k += NT) {
            ggo[k] = M.w[k];
            if (gao) gao[k] = M.zeta[M.blk[k]] * M.yv[k];
        }
        if (gF)
            for (int e = tid; e < l * n; e += NT) {
                const int c = e / l, k = e - c * l;
                gF[e] = M.zeta[M.blk[k]] * M.yv[k] * M.ux[c] + M.w[k] * M.x[c];
            }
        if (gG)
            for (int e = tid; e < ml * n; e += NT) {
                const int c = e / ml, k = e - c * ml;
                gG[e] = M.uz[m + k] * M.x[c] + zs[m + k] * M.ux[c];
            }
        if (gA)
            for (int e = tid; e < p * n; e += NT) {
                const int c = e / p, r = e - c * p;
                gA[e] = M.uy[r] * M.x[c] + ys[r] * M.ux[c];
            }
    }
    if (tid == 0) a.exitc[bm] = GPD_DONE;
}

}  // namespace

hipError_t launch_gp_batch_diff(hipStream_t st, const GpDiffArgs &a)
{
    // per device, so asked of the current one at every launch
    const hipError_t e = hipFuncSetAttribute((const void *)k_gp_batch_diff, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    k_gp_batch_diff<<<dim3((unsigned)a.B), dim3(GPB_THREADS), gp_batch_diff_lds_bytes(a.n, a.m, a.l, a.ml, a.p), st>>>(a);
    return hipGetLastError();
}

}  // namespace kvx
