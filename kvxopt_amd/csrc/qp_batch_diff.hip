// k_qp_batch_diff: one workgroup (256 threads, four wavefronts) differentiates one solved member of qp_batch at its returned
// x, y, s, z (qp_batch_diff.hpp).  The matrix of the differentiated KKT conditions is the Newton matrix of k_qp_batch in the
// scaling di = sqrt(z / s), so the member is assembled and factored exactly as qp_batch.hip's factor() does it, through
// batch_kkt.hpp: S = P + G' diag(di^2) G, its factor L in place, X = L^-1 A', K = X'X and its factor, all in LDS.  What is new
// against every batch kernel before it is iterative refinement, in the shape of f4 (coneprog.py:2288-2316): the right-hand side
// is kept, the residual of the full 3 x 3 system is formed in float64 from P (lower triangle), G, A in HBM as the forward
// kernel forms its residuals, and the same factors solve for the correction.  Every entry of s / z is far from 1 -- tiny on
// active rows, huge on inactive ones -- and one step takes the reduced solve's error from 1e-4 .. 1e-9 to 1e-7 .. 1e-15
// (DESIGN 20).
//
// Reverse mode: K u = (-gx, 0, 0); the gradients of q, h, b are ux, -uz, -uy, and a matrix with a member stride gets its
// gradient as outer products written by the workgroup.  Forward mode: K d = (-(dP x + dq + dG'z + dA'y), db - dA x, dh - dG x)
// formed here from the perturbations in HBM, and ds = -(s / z) dz.
//
// The rules of qp_batch.hip hold: every sum has a fixed order (a thread's partial sum over its indices ascending, an xor
// butterfly per wavefront, the four wavefront sums added 0..3), no atomics, no communication between workgroups; every loop is
// bounded by n, ml, p or `refinement`; every branch around a barrier is taken on values all threads read from the same LDS
// words.  A NaN or Inf in s or z ends in exit 2 through the test of s and z, one in P, G or A through the pivot test.
//
// k_batch_outer_sum: the gradient of a matrix all members share, the sum over the members of their outer products, eight
// threads per entry in an order fixed at compile time.
#include "qp_batch_diff.hpp"
#include "batch_diff_device.hpp"
#include "batch_kkt.hpp"

#include <cmath>

namespace kvx {
namespace {

using namespace batchdev;
static_assert(NT == QPB_THREADS, "the shared helpers are written for the workgroup of k_qp_batch");

struct Member : KktMem {                      // one member's data in HBM and its vectors and matrices in LDS
    int ml;
    const double *P, *G;
    double *bx, *ux, *rx, *by, *uy, *ry, *di, *w, *bz, *uz, *rz, *red;
};

// qp_batch.hip's factor(): S = P + G' diag(di^2) G, its factor, and for p > 0 X, K and its factor.  false on a failed pivot.
// Barriers before (the caller's) and after.
__device__ __forceinline__ bool factor(const Member &M)
{
    const int tid = threadIdx.x, n = M.n, ml = M.ml, ldn = M.ldn;
    for (int e = tid; e < n * n; e += NT) {
        const int j = e / n, i = e - j * n;
        if (i >= j) M.S[i + j * ldn] = M.P[i + j * n];
    }
    for (int k0 = 0; k0 < ml; k0 += QPB_TILE) {
        const int kt = min((int)QPB_TILE, ml - k0);
        __syncthreads();                                   // the staged rows of the previous step have been read
        orth_stage<QPB_TILE>(M, M.G, ml, M.di, k0, kt);
        __syncthreads();
        kkt_s_add_rows(M, kt);
    }
    __syncthreads();
    return chol_lds(M.S, ldn, n) && kkt_equalities(M);
}

// (vx, vy, vz) := K^-1 (vx, vy, vz) by the reduced solve (misc.py:1489-1563); kkt_reduced_solve leaves W uz, so di once more.
// Barriers before (the caller's) and after.
__device__ __forceinline__ void kkt_solve(const Member &M, double *vx, double *vy, double *vz)
{
    orth_kkt_before(M.G, M.ml, M.n, M.di, vx, vz);
    kkt_reduced_solve(M, false, vx, vy);
    orth_kkt_after(M.G, M.ml, M.n, M.di, vx, vz);
    for (int k = threadIdx.x; k < M.ml; k += NT) vz[k] *= M.di[k];       // each thread scales the entries it wrote itself
    __syncthreads();
}

__global__ void __launch_bounds__(QPB_THREADS) k_qp_batch_diff(QpDiffArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, n = a.n, ml = a.ml, p = a.p;
    const int64_t bm = blockIdx.x;
    const bool jvp = a.mode == QPD_JVP;
    const qpdiff::Layout L = qpdiff::layout(n, ml, p);
    Member M;
    M.n = n; M.ml = ml; M.p = p; M.ldn = L.ldn; M.ldp = L.ldp;
    M.P = a.P + bm * a.sP; M.G = a.G + bm * a.sG; M.A = p ? a.A + bm * a.sA : nullptr;
    M.S = lds + L.S; M.T = lds + L.XK; M.X = lds + L.X; M.K = lds + L.K;
    M.bx = lds + L.bx; M.ux = lds + L.ux; M.rx = lds + L.rx; M.by = lds + L.by; M.uy = lds + L.uy; M.ry = lds + L.ry;
    M.di = lds + L.di; M.w = lds + L.w; M.bz = lds + L.bz; M.uz = lds + L.uz; M.rz = lds + L.rz; M.red = lds + L.red;
    const double *xs = a.x + bm * n, *ys = p ? a.y + bm * p : nullptr, *ss = a.s + bm * ml, *zs = a.z + bm * ml;
    double *uxo = a.ux + bm * n, *uyo = p ? a.uy + bm * p : nullptr, *uzo = a.uz + bm * ml, *uso = jvp ? a.us + bm * ml : nullptr;
    double *gP = !jvp && a.gP && a.sP ? a.gP + bm * n * n : nullptr, *gG = !jvp && a.gG && a.sG ? a.gG + bm * ml * n : nullptr;
    double *gA = !jvp && p && a.gA && a.sA ? a.gA + bm * p * n : nullptr;

    // ---- the scaling di = sqrt(z / s), W'W = s / z; is the member one to differentiate?
    int code = QPD_DONE;
    {
        double bad[2] = {0.0, tid == 0 && a.solexit[bm] != 0 ? 1.0 : 0.0};
        for (int k = tid; k < ml; k += NT) {
            const double sk = ss[k], zk = zs[k];
            if (!(sk > 0.0 && sk < INFINITY && zk > 0.0 && zk < INFINITY)) bad[0] = 1.0;
            M.di[k] = sqrt(zk / sk);
            M.w[k] = sk / zk;
        }
        blk_reduce<2, true>(bad, M.red);                   // its barriers also publish di and w
        if (bad[1] != 0.0) code = QPD_SKIPPED;
        else if (bad[0] != 0.0) code = QPD_FAILED;
    }
    if (code == QPD_DONE && !factor(M)) code = QPD_FAILED;
    if (code != QPD_DONE) {
        for (int k = tid; k < ml; k += NT) { uzo[k] = 0.0; if (jvp) uso[k] = 0.0; }
        if (tid < n) uxo[tid] = 0.0;
        if (tid < p) uyo[tid] = 0.0;
        if (gP) for (int e = tid; e < n * n; e += NT) gP[e] = 0.0;
        if (gG) for (int e = tid; e < ml * n; e += NT) gG[e] = 0.0;
        if (gA) for (int e = tid; e < p * n; e += NT) gA[e] = 0.0;
        if (tid == 0) a.exitc[bm] = code;
        return;
    }

    // ---- the right-hand side, kept in bx, by, bz for the refinement
    if (!jvp) {
        if (tid < n) M.bx[tid] = -a.gx[bm * n + tid];
        if (tid < p) M.by[tid] = 0.0;
        for (int k = tid; k < ml; k += NT) M.bz[k] = 0.0;
    } else {
        const double *dP = a.dP ? a.dP + bm * a.sdP : nullptr, *dq = a.dq ? a.dq + bm * a.sdq : nullptr;
        const double *dG = a.dG ? a.dG + bm * a.sdG : nullptr, *dh = a.dh ? a.dh + bm * a.sdh : nullptr;
        const double *dA = p && a.dA ? a.dA + bm * a.sdA : nullptr, *db = p && a.db ? a.db + bm * a.sdb : nullptr;
        if (tid < n) M.rx[tid] = xs[tid];                  // x, y, z in the residual vectors, which are not live yet
        if (tid < p) M.ry[tid] = ys[tid];
        for (int k = tid; k < ml; k += NT) M.rz[k] = zs[k];
        __syncthreads();
        if (tid < n) M.bx[tid] = -((dP ? sym_row_dot(dP, n, tid, M.rx) : 0.0) + (dq ? dq[tid] : 0.0));
        if (tid < p) M.by[tid] = (db ? db[tid] : 0.0) - (dA ? row_dot(dA, p, n, tid, M.rx) : 0.0);
        for (int k = tid; k < ml; k += NT) M.bz[k] = (dh ? dh[k] : 0.0) - (dG ? row_dot(dG, ml, n, k, M.rx) : 0.0);
        __syncthreads();
        if (dG) gemv_t_add(dG, ml, n, M.rz, nullptr, -1.0, M.bx);
        __syncthreads();
        if (dA) gemv_t_add(dA, p, n, M.ry, nullptr, -1.0, M.bx);
    }
    __syncthreads();

    // ---- u = K^-1 b, then `refinement` times u += K^-1 (b - K u)
    if (tid < n) M.ux[tid] = M.bx[tid];
    if (tid < p) M.uy[tid] = M.by[tid];
    for (int k = tid; k < ml; k += NT) M.uz[k] = M.bz[k];
    __syncthreads();
    kkt_solve(M, M.ux, M.uy, M.uz);
    for (int it = 0; it < a.refinement; it++) {
        if (tid < n) M.rx[tid] = M.bx[tid] - sym_row_dot(M.P, n, tid, M.ux);
        if (tid < p) M.ry[tid] = M.by[tid] - row_dot(M.A, p, n, tid, M.ux);
        for (int k = tid; k < ml; k += NT) M.rz[k] = M.bz[k] - (row_dot(M.G, ml, n, k, M.ux) - M.w[k] * M.uz[k]);
        __syncthreads();
        if (p > 0) gemv_t_add(M.A, p, n, M.uy, nullptr, -1.0, M.rx);
        __syncthreads();
        gemv_t_add(M.G, ml, n, M.uz, nullptr, -1.0, M.rx);
        __syncthreads();
        kkt_solve(M, M.rx, M.ry, M.rz);
        if (tid < n) M.ux[tid] += M.rx[tid];
        if (tid < p) M.uy[tid] += M.ry[tid];
        for (int k = tid; k < ml; k += NT) M.uz[k] += M.rz[k];
        __syncthreads();
    }

    // ---- the member's result
    if (tid < n) uxo[tid] = M.ux[tid];
    if (tid < p) uyo[tid] = M.uy[tid];
    for (int k = tid; k < ml; k += NT) {
        uzo[k] = M.uz[k];
        if (jvp) uso[k] = -(M.w[k] * M.uz[k]);
    }
    // Entries (i, j) and (j, i) of gP evaluate one expression, so gP is symmetric to the last bit.
    if (gP)
        for (int e = tid; e < n * n; e += NT) {
            const int c = e / n, r = e - c * n, i = max(r, c), j = min(r, c);
            gP[e] = 0.5 * (M.ux[i] * xs[j] + xs[i] * M.ux[j]);
        }
    if (gG)
        for (int e = tid; e < ml * n; e += NT) {
            const int c = e / ml, k = e - c * ml;
            gG[e] = M.uz[k] * xs[c] + zs[k] * M.ux[c];
        }
    if (gA)
        for (int e = tid; e < p * n; e += NT) {
            const int c = e / p, r = e - c * p;
            gA[e] = M.uy[r] * xs[c] + ys[r] * M.ux[c];
        }
    if (tid == 0) a.exitc[bm] = QPD_DONE;
}

// A workgroup holds OUTER_TILE entries of C.  Part q of OUTER_SPLIT adds the members q, q + OUTER_SPLIT, ... of an entry in
// that order, the parts are added 0 .. OUTER_SPLIT - 1: an order that depends on these two constants alone, not on B, the
// grid or the entry.  A member that is not done adds +0.  sym (the sum for P, rows = n): entries (r, c) and (c, r) evaluate one
// expression, so the sum is symmetric to the last bit.  ldu: two members of u1, u2 are that far apart (gp_batch_diff: the rows
// of G inside columns of N rows).
enum { OUTER_TILE = 32, OUTER_SPLIT = 8, OUTER_THREADS = OUTER_TILE * OUTER_SPLIT };

__global__ void __launch_bounds__(OUTER_THREADS)
k_batch_outer_sum(int64_t B, int rows, int ldu, int n, const double *__restrict__ u1, const double *__restrict__ v1, const double *__restrict__ u2,
                  const double *__restrict__ v2, double scale, int sym, const int64_t *__restrict__ gexit, double *__restrict__ C)
{
    __shared__ double part[OUTER_SPLIT][OUTER_TILE];
    const int le = threadIdx.x % OUTER_TILE, q = threadIdx.x / OUTER_TILE, e = blockIdx.x * OUTER_TILE + le;
    const bool in = e < rows * n;
    int c = in ? e / rows : 0, r = in ? e - c * rows : 0;
    if (sym && r < c) { const int t = r; r = c; c = t; }
    double acc = 0.0;
#pragma unroll 4
    for (int64_t b = q; b < B; b += OUTER_SPLIT) {
        const double t = u1[r + b * ldu] * v1[c + b * n] + u2[r + b * ldu] * v2[c + b * n];
        acc += gexit[b] == 0 ? t : 0.0;
    }
    part[q][le] = acc;
    __syncthreads();
    if (q == 0 && in) {
        double t = part[0][le];
#pragma unroll
        for (int u = 1; u < OUTER_SPLIT; u++) t += part[u][le];
        C[e] = scale * t;
    }
}

}  // namespace

hipError_t launch_qp_batch_diff(hipStream_t st, const QpDiffArgs &a)
{
    // per device, so asked of the current one at every launch
    const hipError_t e = hipFuncSetAttribute((const void *)k_qp_batch_diff, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    k_qp_batch_diff<<<dim3((unsigned)a.B), dim3(QPB_THREADS), qp_batch_diff_lds_bytes(a.n, a.ml, a.p), st>>>(a);
    return hipGetLastError();
}

hipError_t launch_batch_outer_sum(hipStream_t st, int64_t B, int rows, int n, const double *u1, const double *v1, const double *u2,
                                  const double *v2, double scale, bool sym, const int64_t *gexit, double *C, int ldu)
{
    if (rows * n == 0) return hipSuccess;
    k_batch_outer_sum<<<dim3((unsigned)((rows * n + OUTER_TILE - 1) / OUTER_TILE)), dim3(OUTER_THREADS), 0, st>>>(
        B, rows, ldu ? ldu : rows, n, u1, v1, u2, v2, scale, sym ? 1 : 0, gexit, C);
    return hipGetLastError();
}

}  // namespace kvx
