// Kernels of the geometric-program evaluator (gp_api.cpp): for the blocks F_i, g_i of a gp
//
//     f_i(x) = log sum_k exp(F_i x + g_i)_k,   Df_i = y_i' F_i,   H = sum_i z_i F_i' (diag(y_i) - y_i y_i') F_i,
//
// y_i = exp(F_i x + g_i) / sum -- what the reference's Fgp closure computes block by block with dense BLAS
// (cvxprog.py:2102-2153).  The Hessian is formed as the reference forms it, from the centred and scaled factors
// Fsc_i = diag(y_i)^1/2 (F_i - 1 Df_i) (cvxprog.py:2135-2150): they are written densely over the columns a block touches and
// their Gram matrices come from the FP64 MFMA tiles of kkt_cone.hip (launch_cone_gram).
// Every output is written once, every sum runs in a fixed order (strided partial sums, then a fixed butterfly): no
// floating-point atomics, the same bits on every call.
#include "gp.hpp"

namespace kvx {
namespace {

static inline unsigned grid_of(int64_t n, int bs = 256)
{
    int64_t b = (n + bs - 1) / bs;
    if (b > 4096) b = 4096;
    if (b < 1) b = 1;
    return (unsigned)b;
}

#define GP_LOOP(i, n) \
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

__device__ inline double row_value(int64_t r, const int64_t *__restrict__ rp, const int64_t *__restrict__ ci, const int64_t *__restrict__ src,
                                   const double *__restrict__ Fx, const double *__restrict__ g, const double *__restrict__ x)
{
    double a = g[r];                                            // y = g, then += F(:, j) x_j by ascending j (gemv, cvxprog.py:2110-2111)
    for (int64_t e = rp[r]; e < rp[r + 1]; e++) a = __builtin_fma(Fx[src[e]], x[ci[e]], a);
    return a;
}

// G lanes (16 or 64, a power of two inside one wavefront) per block.  Every lane of the launch runs every shuffle: a group
// without a block (`live` false) works on no rows.
template <int G>
__global__ __launch_bounds__(256) void k_gp_lse_group(int64_t nb, const int64_t *__restrict__ list, const int64_t *__restrict__ boff,
                                                      const int64_t *__restrict__ rp, const int64_t *__restrict__ ci,
                                                      const int64_t *__restrict__ src, const double *__restrict__ Fx,
                                                      const double *__restrict__ g, const double *__restrict__ x, double *__restrict__ y,
                                                      double *__restrict__ f)
{
    const int lane = threadIdx.x % G;
    const int64_t ngroups = (int64_t)gridDim.x * (256 / G);
    for (int64_t t0 = (int64_t)blockIdx.x * (256 / G); t0 < nb; t0 += ngroups) {     // t0: the same for the whole workgroup
        const int64_t t = t0 + threadIdx.x / G;
        const bool live = t < nb;
        const int64_t b = live ? list[t] : 0;
        const int64_t r0 = live ? boff[b] : 0, r1 = live ? boff[b + 1] : 0;
        double m = -__builtin_inf();
        for (int64_t r = r0 + lane; r < r1; r += G) {
            const double v = row_value(r, rp, ci, src, Fx, g, x);
            y[r] = v;
            m = fmax(m, v);
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, G));
        double s = 0.0;
        for (int64_t r = r0 + lane; r < r1; r += G) {
            const double e = exp(y[r] - m);
            y[r] = e;
            s += e;
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, G);
        const double si = 1.0 / s;
        for (int64_t r = r0 + lane; r < r1; r += G) y[r] *= si;
        if (live && lane == 0) f[b] = m + log(s);
    }
}

// one 256-thread workgroup per block: strided partial results, then a fixed tree in LDS
__global__ __launch_bounds__(256) void k_gp_lse_wg(int64_t nb, const int64_t *__restrict__ list, const int64_t *__restrict__ boff,
                                                   const int64_t *__restrict__ rp, const int64_t *__restrict__ ci,
                                                   const int64_t *__restrict__ src, const double *__restrict__ Fx,
                                                   const double *__restrict__ g, const double *__restrict__ x, double *__restrict__ y,
                                                   double *__restrict__ f)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    for (int64_t t = blockIdx.x; t < nb; t += gridDim.x) {
        const int64_t b = list[t];
        const int64_t r0 = boff[b], r1 = boff[b + 1];
        double m = -__builtin_inf();
        for (int64_t r = r0 + tid; r < r1; r += 256) {
            const double v = row_value(r, rp, ci, src, Fx, g, x);
            y[r] = v;
            m = fmax(m, v);
        }
        red[tid] = m;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
            __syncthreads();
        }
        m = red[0];
        __syncthreads();
        double s = 0.0;
        for (int64_t r = r0 + tid; r < r1; r += 256) {
            const double e = exp(y[r] - m);
            y[r] = e;
            s += e;
        }
        red[tid] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        s = red[0];
        __syncthreads();
        const double si = 1.0 / s;
        for (int64_t r = r0 + tid; r < r1; r += 256) y[r] *= si;
        if (tid == 0) f[b] = m + log(s);
    }
}

__global__ void k_gp_grad_thread(int64_t ne, const int64_t *__restrict__ list, const int64_t *__restrict__ seg, const int64_t *__restrict__ pos,
                                 const int64_t *__restrict__ row, const double *__restrict__ Fx, const double *__restrict__ y,
                                 double *__restrict__ Dfx)
{
    GP_LOOP(t, ne) {
        const int64_t e = list[t];
        double a = 0.0;
        for (int64_t p = seg[e]; p < seg[e + 1]; p++) a = __builtin_fma(Fx[pos[p]], y[row[p]], a);
        Dfx[e] = a;
    }
}

__global__ __launch_bounds__(256) void k_gp_grad_wave(int64_t ne, const int64_t *__restrict__ list, const int64_t *__restrict__ seg,
                                                      const int64_t *__restrict__ pos, const int64_t *__restrict__ row,
                                                      const double *__restrict__ Fx, const double *__restrict__ y, double *__restrict__ Dfx)
{
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t t0 = (int64_t)blockIdx.x * 4; t0 < ne; t0 += nwaves) {
        const int64_t t = t0 + (threadIdx.x >> 6);
        const bool live = t < ne;
        const int64_t e = live ? list[t] : 0;
        const int64_t p0 = live ? seg[e] : 0, p1 = live ? seg[e + 1] : 0;
        double a = 0.0;
        for (int64_t p = p0 + lane; p < p1; p += 64) a = __builtin_fma(Fx[pos[p]], y[row[p]], a);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (live && lane == 0) Dfx[e] = a;
    }
}

__global__ void k_gp_fsc_fill(int64_t dtot, int64_t nblk, const int64_t *__restrict__ foff, const int64_t *__restrict__ boff,
                              const int64_t *__restrict__ coff, const int64_t *__restrict__ dpos, const double *__restrict__ Dfx,
                              const double *__restrict__ y, double *__restrict__ D)
{
    GP_LOOP(e, dtot) {
        int64_t lo = 0, hi = nblk;                              // the block b with foff[b] <= e < foff[b + 1]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (foff[mid] <= e) lo = mid; else hi = mid;
        }
        const int64_t K = boff[lo + 1] - boff[lo], u = e - foff[lo];
        const int64_t r = u % K, a = u / K;
        D[e] = (0.0 - Dfx[dpos[coff[lo] + a]]) * sqrt(y[boff[lo] + r]);
    }
}

__global__ void k_gp_fsc_nz(int64_t nnz, const int64_t *__restrict__ pos, const int64_t *__restrict__ row, const int64_t *__restrict__ dd,
                            const int64_t *__restrict__ dfe, const double *__restrict__ Fx, const double *__restrict__ Dfx,
                            const double *__restrict__ y, double *__restrict__ D)
{
    GP_LOOP(p, nnz) D[dd[p]] = (Fx[pos[p]] - Dfx[dfe[p]]) * sqrt(y[row[p]]);
}

__global__ void k_gp_hgather(int64_t hnz, const int64_t *__restrict__ hptr, const int32_t *__restrict__ hblk, const int64_t *__restrict__ hidx,
                             const double *__restrict__ z, const double *__restrict__ C, double *__restrict__ Hx)
{
    GP_LOOP(e, hnz) {
        double a = 0.0;
        for (int64_t u = hptr[e]; u < hptr[e + 1]; u++) a = __builtin_fma(z[hblk[u]], C[hidx[u]], a);
        Hx[e] = a;
    }
}

}  // namespace

void launch_gp_lse(hipStream_t st, int cls, int64_t nb, const int64_t *list, const int64_t *boff, const int64_t *rp, const int64_t *ci,
                   const int64_t *src, const double *Fx, const double *g, const double *x, double *y, double *f)
{
    if (nb <= 0) return;
    if (cls == 0)
        hipLaunchKernelGGL(k_gp_lse_group<16>, dim3(grid_of(nb, 16)), dim3(256), 0, st, nb, list, boff, rp, ci, src, Fx, g, x, y, f);
    else if (cls == 1)
        hipLaunchKernelGGL(k_gp_lse_group<64>, dim3(grid_of(nb, 4)), dim3(256), 0, st, nb, list, boff, rp, ci, src, Fx, g, x, y, f);
    else
        hipLaunchKernelGGL(k_gp_lse_wg, dim3(grid_of(nb, 1)), dim3(256), 0, st, nb, list, boff, rp, ci, src, Fx, g, x, y, f);
}

void launch_gp_grad(hipStream_t st, int wave, int64_t ne, const int64_t *list, const int64_t *seg, const int64_t *pos, const int64_t *row,
                    const double *Fx, const double *y, double *Dfx)
{
    if (ne <= 0) return;
    if (wave)
        hipLaunchKernelGGL(k_gp_grad_wave, dim3(grid_of(ne, 4)), dim3(256), 0, st, ne, list, seg, pos, row, Fx, y, Dfx);
    else
        hipLaunchKernelGGL(k_gp_grad_thread, dim3(grid_of(ne)), dim3(256), 0, st, ne, list, seg, pos, row, Fx, y, Dfx);
}

void launch_gp_fsc_fill(hipStream_t st, int64_t dtot, int64_t nblk, const int64_t *foff, const int64_t *boff, const int64_t *coff,
                        const int64_t *dpos, const double *Dfx, const double *y, double *D)
{ if (dtot > 0) hipLaunchKernelGGL(k_gp_fsc_fill, dim3(grid_of(dtot)), dim3(256), 0, st, dtot, nblk, foff, boff, coff, dpos, Dfx, y, D); }

void launch_gp_fsc_nz(hipStream_t st, int64_t nnz, const int64_t *pos, const int64_t *row, const int64_t *dd, const int64_t *dfe,
                      const double *Fx, const double *Dfx, const double *y, double *D)
{ if (nnz > 0) hipLaunchKernelGGL(k_gp_fsc_nz, dim3(grid_of(nnz)), dim3(256), 0, st, nnz, pos, row, dd, dfe, Fx, Dfx, y, D); }

void launch_gp_hgather(hipStream_t st, int64_t hnz, const int64_t *hptr, const int32_t *hblk, const int64_t *hidx, const double *z,
                       const double *C, double *Hx)
{ if (hnz > 0) hipLaunchKernelGGL(k_gp_hgather, dim3(grid_of(hnz)), dim3(256), 0, st, hnz, hptr, hblk, hidx, z, C, Hx); }

}  // namespace kvx
