// Iterative refinement of the sparse LU solves (kvx_lu_solve_refine; what UMFPACK's solve does with UMFPACK_IRSTEP = 2,
// umfpack.c:630-640): residual, componentwise backward error and the accept / reject step, all on the device -- the host reads
// nothing between the steps.  Three kernels for gfx950 (wave64), no floating-point atomics: two runs give the same bytes.
//
//   k_lu_resid   r = b - op(A) (x [+ d]) and the ratio |r_i| / (|op(A)| |x [+ d]| + |b|)_i, one pass over the rows of op(A)
//   k_lu_berr    omega = max_i ratio_i per column: a fixed tree
//   k_lu_accept  per column: keep x + d when its omega is smaller than the current one, else keep x and stop that column
#include "lu_device.hpp"

#include <algorithm>

// The error-free sums below are exact only as written: a product must be rounded before it is added (no contraction of
// hi + v * x into one fma, which the compiler's default for device code would do).
#pragma clang fp contract(off)

namespace kvx {

namespace {

// The residual is a difference of nearly equal numbers: summed in plain double its rounding error is as large as the residual of
// a backward-stable solution itself, and omega would be noise.  The products and their sum are therefore carried as unevaluated
// pairs hi + lo (error-free product by fma, error-free sum): the rounded result is that of a sum in about twice the precision.
__device__ __forceinline__ void dd_add(double &hi, double &lo, double p, double q)              // (hi, lo) += (p, q)
{
    const double s = hi + p, bb = s - hi;
    const double e = ((hi - (s - bb)) + (p - bb)) + (lo + q);
    hi = s + e;
    lo = e - (hi - s);
}

// One 16-lane group per row (the mapping of k_gp_lse_group<16>, gp.hip): the lanes stride over the row, a fixed xor butterfly adds
// the partial sums.  Rows longer than 16 entries need nothing beyond the stride.  rp / ci: the row-wise view of op(A); src: index of
// every entry in the caller's value order (nullptr: the entries are in that order already -- the CCS is the row-wise view of A').
// d == nullptr: the residual of x; else that of x + d (the candidate of a refinement step, not stored anywhere yet).
__global__ __launch_bounds__(256) void k_lu_resid(int64_t n, int nrhs, const int64_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                  const int32_t *__restrict__ src, const double *__restrict__ Ax,
                                                  const double *__restrict__ B, int64_t ldb, const double *__restrict__ X, int64_t ldx,
                                                  const double *__restrict__ D, int64_t ldd, double *__restrict__ R, int64_t ldr,
                                                  double *__restrict__ ratio)
{
    constexpr int G = 16;
    const int lane = threadIdx.x % G;
    const int64_t ngroups = (int64_t)gridDim.x * (256 / G);
    for (int j = blockIdx.y; j < nrhs; j += gridDim.y) {
        const double *x = X + (int64_t)j * ldx, *d = D ? D + (int64_t)j * ldd : nullptr, *b = B + (int64_t)j * ldb;
        for (int64_t i0 = (int64_t)blockIdx.x * (256 / G); i0 < n; i0 += ngroups) {      // i0: the same for the whole workgroup
            const int64_t i = i0 + threadIdx.x / G;
            const bool live = i < n;
            const int64_t e0 = live ? rp[i] : 0, e1 = live ? rp[i + 1] : 0;
            double s = 0.0, sl = 0.0, a = 0.0;                                           // op(A) x as s + sl, |op(A)| |x|
            for (int64_t e = e0 + lane; e < e1; e += G) {
                const int32_t c = ci[e];
                const double v = Ax[src ? (int64_t)src[e] : e];
                const double xc = d ? x[c] + d[c] : x[c];
                const double p = v * xc;
                dd_add(s, sl, p, fma(v, xc, -p));
                a += fabs(p);
            }
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) {
                const double ph = __shfl_xor(s, o, G), pl = __shfl_xor(sl, o, G);
                dd_add(s, sl, ph, pl);
                a += __shfl_xor(a, o, G);
            }
            if (live && lane == 0) {
                double r = b[i], rl = 0.0;
                dd_add(r, rl, -s, -sl);
                const double den = a + fabs(b[i]), ar = fabs(r);
                R[i + (int64_t)j * ldr] = r;
                const double q = den > 0.0 ? ar / den : (ar > 0.0 ? __builtin_inf() : 0.0);              // 0 / 0 counts as 0
                ratio[i + (int64_t)j * n] = q == q ? q : __builtin_inf();                                // (a NaN must not win by being ignored)
            }
        }
    }
}

// Workgroup (p, j) takes the maximum of in[j * ld + p * chunk .. + chunk) (clipped to len): strided partial maxima, then a fixed
// tree in LDS.  Launched once over the ratios (one chunk per workgroup) and, when that took several workgroups per column, once
// more over their partial results.  out2 / act (may be nullptr): a second copy of the result / the column's "still improving" flag.
__global__ __launch_bounds__(256) void k_lu_berr(int64_t len, int64_t chunk, const double *__restrict__ in, int64_t ld,
                                                 double *__restrict__ out, int64_t out_ld, int64_t out_stride, double *__restrict__ out2,
                                                 int64_t out2_stride, int32_t *__restrict__ act)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int64_t p = blockIdx.x, j = blockIdx.y;
    const int64_t b0 = p * chunk, b1 = b0 + chunk < len ? b0 + chunk : len;
    const double *v = in + j * ld;
    double m = 0.0;
    for (int64_t i = b0 + tid; i < b1; i += 256) m = fmax(m, v[i]);
    red[tid] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
        __syncthreads();
    }
    if (tid == 0) {
        out[j * out_ld + p * out_stride] = red[0];
        if (out2) out2[j * out2_stride] = red[0];
        if (act) act[j] = 1;
    }
}

// Per column j: the candidate x + d is kept only if its backward error om_cand[j] is SMALLER than the current om_in[j] and the column
// has not stopped before; otherwise x stays and the column stops changing.  The state goes from (om_in, act_in) to (om_out,
// act_out) -- other arrays, so that no thread reads what another has already replaced.  d == nullptr: nothing to select, x is
// copied to `out` (which may be X itself: every thread reads an entry before it writes it).  om_final (may be nullptr): where
// the caller reads the backward error of what `out` now holds.
__global__ __launch_bounds__(256) void k_lu_accept(int64_t n, const double *X, int64_t ldx, const double *__restrict__ D,
                                                   int64_t ldd, double *out, int64_t ldo, const double *__restrict__ om_in,
                                                   const int32_t *__restrict__ act_in, const double *__restrict__ om_cand,
                                                   double *__restrict__ om_out, int32_t *__restrict__ act_out, double *__restrict__ om_final,
                                                   int64_t final_stride)
{
    const int64_t j = blockIdx.y;
    const bool take = D && act_in[j] && om_cand[j] < om_in[j];
    const double *x = X + j * ldx, *d = D ? D + j * ldd : nullptr;
    double *o = out + j * ldo;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) o[i] = take ? x[i] + d[i] : x[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double om = take ? om_cand[j] : om_in[j];
        if (om_out) om_out[j] = om;
        if (act_out) act_out[j] = take ? 1 : 0;
        if (om_final) om_final[j * final_stride] = om;
    }
}

}  // namespace

int64_t lu_berr_parts(int64_t n) { return n <= LU_BERR_CHUNK ? 1 : (n + LU_BERR_CHUNK - 1) / LU_BERR_CHUNK; }

void launch_lu_resid(int64_t n, int nrhs, const int64_t *rp, const int32_t *ci, const int32_t *src, const double *Ax, const double *B,
                     int64_t ldb, const double *X, int64_t ldx, const double *D, int64_t ldd, double *R, int64_t ldr, double *ratio,
                     hipStream_t st)
{
    if (n <= 0 || nrhs <= 0) return;
    const int64_t gx = std::min<int64_t>((n + 15) / 16, (int64_t)1 << 20);
    hipLaunchKernelGGL(k_lu_resid, dim3((unsigned)gx, (unsigned)std::min(nrhs, 65535)), dim3(256), 0, st, n, nrhs, rp, ci, src, Ax, B, ldb, X,
                       ldx, D, ldd, R, ldr, ratio);
}

// omega[j * om_stride] = max_i ratio[i + j * n] (part: lu_berr_parts(n) doubles per column); the same value to om2[j * om2_stride]
// and act[j] = 1 where those are given.
void launch_lu_berr(int64_t n, int nrhs, const double *ratio, double *part, double *om, int64_t om_stride, double *om2, int64_t om2_stride,
                    int32_t *act, hipStream_t st)
{
    if (n <= 0 || nrhs <= 0) return;
    const int64_t np = lu_berr_parts(n);
    if (np == 1) {
        hipLaunchKernelGGL(k_lu_berr, dim3(1, (unsigned)nrhs), dim3(256), 0, st, n, n, ratio, n, om, om_stride, (int64_t)0, om2, om2_stride, act);
        return;
    }
    hipLaunchKernelGGL(k_lu_berr, dim3((unsigned)np, (unsigned)nrhs), dim3(256), 0, st, n, (int64_t)LU_BERR_CHUNK, ratio, n, part, np, (int64_t)1,
                       (double *)nullptr, (int64_t)0, (int32_t *)nullptr);
    hipLaunchKernelGGL(k_lu_berr, dim3(1, (unsigned)nrhs), dim3(256), 0, st, np, np, (const double *)part, np, om, om_stride, (int64_t)0, om2,
                       om2_stride, act);
}

void launch_lu_accept(int64_t n, int nrhs, const double *X, int64_t ldx, const double *D, int64_t ldd, double *out, int64_t ldo,
                      const double *om_in, const int32_t *act_in, const double *om_cand, double *om_out, int32_t *act_out, double *om_final,
                      int64_t final_stride, hipStream_t st)
{
    if (n <= 0 || nrhs <= 0) return;
    const int64_t gx = std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_lu_accept, dim3((unsigned)gx, (unsigned)nrhs), dim3(256), 0, st, n, X, ldx, D, ldd, out, ldo, om_in, act_in, om_cand,
                       om_out, act_out, om_final, final_stride);
}

}  // namespace kvx
