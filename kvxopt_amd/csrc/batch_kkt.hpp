// The reduced KKT solve of misc.kkt_chol2 (misc.py:1395-1563) as the four one-workgroup-per-member kernels share it
// (k_qp_batch, k_lp_batch, k_socp_batch, k_sdp_batch): the start of S and its S += T'T over staged rows, the factorisation with
// the F['singular'] repair, X = L^-1 A', K = X'X and its factor, and the five substitutions of a solve.  What depends on the cone
// -- the rows of W^-T G a kernel stages, W^-T and W^-1 around the solve -- stays with the kernel and comes in as a callable or
// stands around the call.  Every function here is inlined into its kernel: as real calls, or with the member's struct behind a
// pointer, these bodies cost 228 to 432 bytes of scratch per lane.
#pragma once
#include "batch_device.hpp"

namespace kvx {
namespace batchdev {

struct KktMem {                               // the part of a member the KKT core works on: A in HBM, the rest in LDS
    int n, p, ldn, ldp;
    const double *A;
    double *S, *T, *X, *K;                    // T: the staged rows, in the region X and K take once S is factored
};

// The lower triangle of S := A'A (sing) or 0.  No barrier.
__device__ __forceinline__ void kkt_s_init(const KktMem &M, bool sing)
{
    const int n = M.n, p = M.p;
    for (int e = threadIdx.x; e < tri_count(n); e += NT) {
        int i, j;
        if (!tri_map(e, n, i, j)) continue;
        double acc = 0.0;
        if (sing)
            for (int a = 0; a < p; a++) acc += M.A[a + (int64_t)i * p] * M.A[a + (int64_t)j * p];
        M.S[i + j * M.ldn] = acc;
    }
}

// The lower triangle of S += T'T over the first `rows` staged rows.  The caller's barriers stand before and after.
__device__ __forceinline__ void kkt_s_add_rows(const KktMem &M, int rows)
{
    const int n = M.n, ldn = M.ldn;
    for (int e = threadIdx.x; e < tri_count(n); e += NT) {
        int i, j;
        if (!tri_map(e, n, i, j)) continue;
        double acc = 0.0;
        for (int kk = 0; kk < rows; kk++) acc += M.T[kk * ldn + i] * M.T[kk * ldn + j];
        M.S[i + j * ldn] += acc;
    }
}

// With the factor L of S in place: X = L^-1 A', K = X'X and its factor (misc.py:1460-1487).  true for p = 0; false on a failed
// pivot of K.  The staged rows are dead: X takes their place.  Barriers before (the caller's) and after.
__device__ __forceinline__ bool kkt_equalities(const KktMem &M)
{
    const int tid = threadIdx.x, n = M.n, p = M.p, ldn = M.ldn, ldp = M.ldp;
    if (p == 0) return true;
    const int lane = tid & 63, w = tid >> 6;
    for (int a = w; a < p; a += NW) {
        double v = lane < n ? M.A[a + (int64_t)lane * p] : 0.0;
        v = wave_trsv_n(M.S, ldn, n, v);
        if (lane < n) M.X[lane + a * ldn] = v;
    }
    __syncthreads();
    for (int e = tid; e < tri_count(p); e += NT) {
        int a, c;
        if (!tri_map(e, p, a, c)) continue;
        double acc = 0.0;
        for (int i = 0; i < n; i++) acc += M.X[i + a * ldn] * M.X[i + c * ldn];
        M.K[a + c * ldp] = acc;
    }
    __syncthreads();
    return chol_lds(M.K, ldp, p);
}

// The KKT factorisation (misc.py:1395-1487): assemble(sing) leaves the lower triangle of S [+ A'A] in LDS and ends with a
// barrier.  first: the member's first factorisation, where a failed factor of S with p > 0 sets `sing` and is repeated on
// S + A'A (F['singular'], misc.py:1433-1458); the flag belongs to the member.  false on a failed pivot.  Barriers before (the
// caller's) and after.
template <class Assemble>
__device__ __forceinline__ bool kkt_factor(const KktMem &M, bool &sing, bool first, Assemble assemble)
{
    assemble(sing);
    if (!chol_lds(M.S, M.ldn, M.n)) {
        if (!first || M.p == 0) return false;
        sing = true;
        __syncthreads();                                   // every thread has read the failed pivot
        assemble(true);
        if (!chol_lds(M.S, M.ldn, M.n)) return false;
    }
    return kkt_equalities(M);
}

// The middle of a solve (misc.py:1519-1553) on the LDS vectors vx, vy: [x += A'y of a repaired member,] x := L^-1 x,
// y := X'x - y, y := K^-1 y, x := x - X y, x := L^-T x.  Barriers before (the caller's) and after.
__device__ __forceinline__ void kkt_reduced_solve(const KktMem &M, bool sing, double *vx, double *vy)
{
    const int tid = threadIdx.x, n = M.n, p = M.p, lane = tid & 63, w = tid >> 6;
    if (sing) {                                                                            // x += A' by
        gemv_t_add(M.A, p, n, vy, nullptr, 1.0, vx);
        __syncthreads();
    }
    if (w == 0) {                                                                          // x := L^-1 x
        const double v = wave_trsv_n(M.S, M.ldn, n, lane < n ? vx[lane] : 0.0);
        if (lane < n) vx[lane] = v;
    }
    __syncthreads();
    if (p > 0) {
        if (tid < p) {                                                                     // y := X'x - y
            double acc = 0.0;
            for (int i = 0; i < n; i++) acc += M.X[i + tid * M.ldn] * vx[i];
            vy[tid] = acc - vy[tid];
        }
        __syncthreads();
        if (w == 0) {                                                                      // y := K^-1 y
            double v = wave_trsv_n(M.K, M.ldp, p, lane < p ? vy[lane] : 0.0);
            v = wave_trsv_t(M.K, M.ldp, p, v);
            if (lane < p) vy[lane] = v;
        }
        __syncthreads();
        if (tid < n) {                                                                     // x := x - X y
            double acc = 0.0;
            for (int a = 0; a < p; a++) acc += M.X[tid + a * M.ldn] * vy[a];
            vx[tid] -= acc;
        }
        __syncthreads();
    }
    if (w == 0) {                                                                          // x := L^-T x
        const double v = wave_trsv_t(M.S, M.ldn, n, lane < n ? vx[lane] : 0.0);
        if (lane < n) vx[lane] = v;
    }
    __syncthreads();
}

// ---- the orthant, as all four kernels treat their 'l' rows: ml rows with the scaling d, di = 1 / d and lmbda = lm

// One tile of the assembly: rows k0 .. k0 + kt of diag(di) G into the staged rows.  G has `rows` rows.  No barrier.
template <int TILE>
__device__ __forceinline__ void orth_stage(const KktMem &M, const double *__restrict__ G, int rows, const double *di, int k0, int kt)
{
    for (int e = threadIdx.x; e < TILE * M.n; e += NT) {
        const int kk = e & (TILE - 1), c = e / TILE;
        if (kk < kt) M.T[kk * M.ldn + c] = di[k0 + kk] * G[k0 + kk + (int64_t)c * rows];
    }
}

// misc.compute_scaling on 'l' rows (misc.py:284-287): d = sqrt(s / z), lmbda = sqrt(s z).  No barrier.
__device__ __forceinline__ void orth_first_scaling(int ml, const double *s, const double *z, double *d, double *di, double *lm)
{
    for (int k = threadIdx.x; k < ml; k += NT) {
        const double sk = s[k], zk = z[k], dk = sqrt(sk / zk);
        d[k] = dk; di[k] = 1.0 / dk; lm[k] = sqrt(sk * zk);
    }
}

// misc.update_scaling on 'l' rows (misc.py:444-464) after the step along the scaled ds, dz, and s = d lmbda, z = lmbda / d of
// the next iteration.  The thread's part of the new lmbda'lmbda.  No barrier.
__device__ __forceinline__ double orth_update(int ml, double step, const double *ds, const double *dz, double *d, double *di, double *lm,
                                              double *s, double *z)
{
    double g = 0.0;
    for (int k = threadIdx.x; k < ml; k += NT) {
        const double lk = lm[k], rs = sqrt((1.0 + step * ds[k]) * lk), rz = sqrt((1.0 + step * dz[k]) * lk);
        const double dk = d[k] * rs / rz, dik = 1.0 / dk, ln = rs * rz;
        d[k] = dk; di[k] = dik; lm[k] = ln;
        s[k] = dk * ln; z[k] = dik * ln;
        g += ln * ln;
    }
    return g;
}

// Around kkt_reduced_solve on the orthant alone (k_qp_batch, k_lp_batch): z := W^-T bz and x += G'W^-1 z before it,
// W uz = W^-T (G ux - bz) after it.  Barriers before (the caller's) and after.
__device__ __forceinline__ void orth_kkt_before(const double *__restrict__ G, int ml, int n, const double *di, double *vx, double *vz)
{
    for (int k = threadIdx.x; k < ml; k += NT) vz[k] *= di[k];
    __syncthreads();
    gemv_t_add(G, ml, n, vz, di, 1.0, vx);
    __syncthreads();
}

__device__ __forceinline__ void orth_kkt_after(const double *__restrict__ G, int ml, int n, const double *di, const double *vx, double *vz)
{
    for (int k = threadIdx.x; k < ml; k += NT) vz[k] = di[k] * row_dot(G, ml, n, k, vx) - vz[k];
    __syncthreads();
}

}  // namespace batchdev
}  // namespace kvx
