// Device helpers shared by the four one-workgroup-per-member kernels k_qp_batch, k_lp_batch, k_socp_batch and k_sdp_batch: the
// fixed-order wavefront and workgroup reductions, the triangle map of the assembly of S and K, the products with the
// column-major matrices of a member in HBM, the Cholesky factor of an order <= 64 matrix in LDS and the two wavefront
// substitutions.  batch_kkt.hpp builds the KKT core and the orthant on them, batch_conelp.hpp the conelp loop of the three cone
// kernels.  A workgroup is 256 threads, four wavefronts.  Every sum has a fixed order: a thread's partial sum runs over its
// indices ascending, a wavefront adds by an xor butterfly, the four wavefront sums are added 0..3.  No atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace kvx {
namespace batchdev {

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int NRED = 8;                       // values one block reduction carries at most

__host__ __device__ inline int even(int v) { return (v + 1) & ~1; }

__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ inline double wave_max(double v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// v[0..K) := the workgroup's sums (MAX: maxima) of v[0..K), the same bytes in every thread
template <int K, bool MAX>
__device__ inline void blk_reduce(double (&v)[K], double *red)
{
    static_assert(K <= NRED, "blk_reduce carries at most NRED values");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = MAX ? wave_max(v[k]) : wave_sum(v[k]);
    __syncthreads();                          // the readers of the previous reduction are done with red
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) red[w * NRED + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        double t = red[k];
#pragma unroll
        for (int u = 1; u < NW; u++) t = MAX ? fmax(t, red[u * NRED + k]) : t + red[u * NRED + k];
        v[k] = t;
    }
}

// Entry e < tri_count(m) of the lower triangle of order m as (i, c), i >= c: column c and column m - 1 - c share one row of
// m + 1 entries, so no thread idles on the upper half.  false: e is the unused half of the middle column of an odd m.
__device__ inline int tri_count(int m) { return ((m + 1) >> 1) * (m + 1); }

__device__ inline bool tri_map(int e, int m, int &i, int &c)
{
    const int cc = e / (m + 1), r = e - cc * (m + 1);
    if (r < m - cc) { c = cc; i = cc + r; return true; }
    c = m - 1 - cc;
    i = c + (r - (m - cc));
    return c != cc;
}

// sum over columns c of M(k, c) v[c]: row k of the column-major rows x cols matrix M in HBM times the LDS vector v
__device__ inline double row_dot(const double *__restrict__ M, int rows, int cols, int k, const double *v)
{
    double acc = 0.0;
    for (int c = 0; c < cols; c++) acc += M[k + (int64_t)c * rows] * v[c];
    return acc;
}

// v[c] += sign * sum over rows k of M(k, c) u1[k] u2[k] (u2 null: ones): a wavefront per column, lanes along the rows.
// The caller's barriers stand before and after.
__device__ inline void gemv_t_add(const double *__restrict__ M, int rows, int cols, const double *u1, const double *u2, double sign, double *v)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c = w; c < cols; c += NW) {
        double acc = 0.0;
        for (int k = lane; k < rows; k += 64) acc += M[k + (int64_t)c * rows] * (u2 ? u1[k] * u2[k] : u1[k]);
        acc = wave_sum(acc);
        if (lane == 0) v[c] += sign * acc;
    }
}

// In-place Cholesky factor (lower, column by column) of the order-m matrix F in LDS, m <= 64.  false, for every thread, on a
// pivot that is <= 0 or not finite.  Ends with a barrier.
__device__ inline bool chol_lds(double *F, int ld, int m)
{
    const int i = threadIdx.x & 63, c0 = threadIdx.x >> 6;
    for (int j = 0; j < m; j++) {
        const double piv = F[j + j * ld];
        if (!(piv > 0.0 && piv < INFINITY)) return false;
        const double l = sqrt(piv);
        if (c0 == 0 && i > j && i < m) F[i + j * ld] /= l;
        __syncthreads();
        if (threadIdx.x == 0) F[j + j * ld] = l;          // nobody reads the old pivot after the barrier above
        if (i < m) {
            const double lij = F[i + j * ld];
            for (int c = j + 1 + c0; c <= i; c += NW) F[i + c * ld] -= lij * F[c + j * ld];
        }
        __syncthreads();
    }
    return true;
}

// x := L^-1 x and x := L^-T x for one wavefront: lane i holds x[i], lanes >= m hold anything
__device__ inline double wave_trsv_n(const double *L, int ld, int m, double x)
{
    const int lane = threadIdx.x & 63;
    for (int j = 0; j < m; j++) {
        const double xj = __shfl(x, j) / L[j + j * ld];
        if (lane == j) x = xj;
        else if (lane > j && lane < m) x -= L[lane + j * ld] * xj;
    }
    return x;
}

__device__ inline double wave_trsv_t(const double *L, int ld, int m, double x)
{
    const int lane = threadIdx.x & 63;
    for (int j = m - 1; j >= 0; j--) {
        const double xj = __shfl(x, j) / L[j + j * ld];
        if (lane == j) x = xj;
        else if (lane < j) x -= L[j + lane * ld] * xj;
    }
    return x;
}

}  // namespace batchdev
}  // namespace kvx
