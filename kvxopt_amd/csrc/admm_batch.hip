// The ADMM iteration of admm.hip for a batch: B data sets (q_b, l_b, u_b) on one scaled A and P, one rho vector and one kept
// factor of S = P + sigma I + A' diag(rho) A (kvx_admm_batch_*, admm_batch_api.cpp).  State and data are column-major, member b
// in column b (ld = n or m): the layout kvx_chol_solve_async_dev takes for nrhs = B, so an iteration is
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
// a launch still runs every shuffle (a frozen member contributes empty sums), and nothing of the member is written.  Per row,
// column and member the kernels call the functions of admm_device.hpp that admm.hip calls: one text defines the 24 numbers.
#include "admm_batch.hpp"
#include "admm_device.hpp"

namespace kvx {
namespace {

static inline unsigned strips_of(int64_t B, int strip) { return (unsigned)((B + strip - 1) / strip); }

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

// group_dot for a strip: out[s] = sum_e Mx[e] * w[Mi[e] + (b0 + s) ld] over e in [e0, e1), lane `sub` of G taking e0 + sub,
// e0 + sub + G, ...
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

// row_dot for a strip: out[s] = (A w_s)_row, w_s = w + (b0 + s) n
template <int NB>
__device__ inline void strip_row_dot(const AdmmDev &a, const RowGroup &g, const double *__restrict__ w, int64_t b0, unsigned act,
                                     double (&out)[NB])
{
    if (g.wide) strip_dot<64, NB>(g.e0, g.e1, g.sub, a.Ti, a.Tx, w, a.n, b0, act, out);
    else strip_dot<16, NB>(g.e0, g.e1, g.sub, a.Ti, a.Tx, w, a.n, b0, act, out);
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
    out[i + bm * b.a.m] = scaled_bound(raw[i + bm * b.a.m], b.a.E + i, upper);
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

// workgroups x in [0, nbs + nbl): the rows of A (row_group); the rest: 256 entries of x each
__global__ __launch_bounds__(256) void k_admm_batch_update(AdmmBatchDev b, unsigned nbs, unsigned nbl)
{
    const AdmmDev &a = b.a;
    const int64_t b0 = (int64_t)blockIdx.y * ADMM_STRIP;
    const unsigned act = strip_mask<ADMM_STRIP>(b, b0);
    if (blockIdx.x < nbs + nbl) {
        const RowGroup g = row_group(a, nbs, blockIdx.x, threadIdx.x);
        double zt[ADMM_STRIP];
        strip_row_dot<ADMM_STRIP>(a, g, b.xt, b0, act, zt);
        if (g.lead()) {
#pragma unroll
            for (int s = 0; s < ADMM_STRIP; s++)
                if ((act >> s) & 1u) {
                    const int64_t t = g.row + (b0 + s) * a.m;
                    update_row(a.alpha, a.rho[g.row], b.l[t], b.u[t], zt[s], b.z + t, b.y + t, b.dy + t);
                }
        }
    } else {
        const int64_t j = (int64_t)(blockIdx.x - nbs - nbl) * 256 + threadIdx.x;
        if (j < a.n) {
#pragma unroll
            for (int s = 0; s < ADMM_STRIP; s++)
                if ((act >> s) & 1u) {
                    const int64_t t = j + (b0 + s) * a.n;
                    update_x(a.alpha, b.xt[t], b.x + t, b.dx + t);
                }
        }
    }
}

// ---- residuals: 24 numbers per member -----------------------------------------------------------------------------------------
// workgroups x in [0, nbs + nbl): the rows of A (row_group); the rest: 16 columns each; y: the strip of members.  part: the 24 x nb
// block of member b at part + b * ADMM_NRES * nb.
__global__ __launch_bounds__(256) void k_admm_batch_residuals(AdmmBatchDev b, unsigned nbs, unsigned nbl, double *__restrict__ part)
{
    __shared__ double sh[4 * 14];
    const AdmmDev &a = b.a;
    const int64_t nb = gridDim.x;
    const int64_t b0 = (int64_t)blockIdx.y * ADMM_RSTRIP;
    const unsigned act = strip_mask<ADMM_RSTRIP>(b, b0);
    if (blockIdx.x < nbs + nbl) {
        const RowGroup g = row_group(a, nbs, blockIdx.x, threadIdx.x);
        double ax[ADMM_RSTRIP], adx[ADMM_RSTRIP];
        strip_row_dot<ADMM_RSTRIP>(a, g, b.x, b0, act, ax);
        strip_row_dot<ADMM_RSTRIP>(a, g, b.dx, b0, act, adx);
#pragma unroll
        for (int s = 0; s < ADMM_RSTRIP; s++) {
            if (!((act >> s) & 1u)) continue;                           // uniform over the workgroup
            double v[10];
            reduce_identity<10, ROW_LSUM>(v);
            if (g.lead()) {
                const int64_t i = g.row, t = i + (b0 + s) * a.m;
                residual_row(b.z[t], b.l[t], b.u[t], b.dy[t], a.E[i], a.Einv[i], a.cinv, ax[s], adx[s], v);
            }
            block_reduce<10, ROW_LSUM>(v, sh, RK, part + (b0 + s) * ADMM_NRES * nb, nb, blockIdx.x);
            __syncthreads();                                            // sh is free for the next member
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
            double v[14];
            reduce_identity<14, COL_LSUM>(v);
            if (live && sub == 0) {
                const int64_t t = j + (b0 + s) * a.n;
                residual_col(b.q[t], b.x[t], b.dx[t], a.D[j], a.Dinv[j], a.cinv, px[s], pdx[s], aty[s], atd[s], v);
            }
            block_reduce<14, COL_LSUM>(v, sh, CK, part + (b0 + s) * ADMM_NRES * nb, nb, blockIdx.x);
            __syncthreads();                                            // sh is free for the next member
        }
    }
}

// second stage: workgroup (k, b), one wavefront: entry k of member b over the workgroups that hold it.  The numbers of a frozen
// member stay what its last check left.
__global__ __launch_bounds__(64) void k_admm_batch_reduce2(AdmmBatchDev b, const double *__restrict__ part, int64_t nbr, int64_t nb,
                                                          double *__restrict__ res)
{
    const int k = blockIdx.x;
    const int64_t bm = blockIdx.y;
    const bool on = b.run[bm] != 0;
    int64_t b0, b1;
    residual_range(k, nbr, nb, &b0, &b1);
    const double acc = wave_reduce2(part + (bm * ADMM_NRES + k) * nb, b0, on ? b1 : b0, (SUMMASK >> k) & 1u);
    if (on && threadIdx.x == 0) res[bm * ADMM_NRES + k] = acc;
}

}  // namespace

void launch_admm_batch_scale_q(hipStream_t st, const AdmmBatchDev &b, double c, const double *raw)
{
    if (b.a.n > 0 && b.B > 0) hipLaunchKernelGGL(k_admm_batch_scale_q, dim3(AdmmGrid(b.a).nbx, (unsigned)b.B), dim3(256), 0, st, b, c, raw);
}

void launch_admm_batch_scale_bound(hipStream_t st, const AdmmBatchDev &b, bool upper, const double *raw)
{
    if (b.a.m > 0 && b.B > 0) hipLaunchKernelGGL(k_admm_batch_scale_bound, dim3(AdmmGrid(b.a).nbm, (unsigned)b.B), dim3(256), 0, st, b, upper, raw);
}

void launch_admm_batch_rhs(hipStream_t st, const AdmmBatchDev &b)
{
    if (b.a.n > 0 && b.B > 0)
        hipLaunchKernelGGL(k_admm_batch_rhs, dim3(AdmmGrid(b.a).nbc, strips_of(b.B, ADMM_STRIP)), dim3(256), 0, st, b);
}

void launch_admm_batch_update(hipStream_t st, const AdmmBatchDev &b)
{
    const AdmmGrid g(b.a);
    if (g.rows() + g.nbx > 0 && b.B > 0)
        hipLaunchKernelGGL(k_admm_batch_update, dim3(g.rows() + g.nbx, strips_of(b.B, ADMM_STRIP)), dim3(256), 0, st, b, g.nbs, g.nbl);
}

void launch_admm_batch_residuals(hipStream_t st, const AdmmBatchDev &b, double *part, double *res)
{
    const AdmmGrid g(b.a);
    const unsigned nb = g.rows() + g.nbc;
    if (b.B <= 0) return;
    if (nb > 0) hipLaunchKernelGGL(k_admm_batch_residuals, dim3(nb, strips_of(b.B, ADMM_RSTRIP)), dim3(256), 0, st, b, g.nbs, g.nbl, part);
    hipLaunchKernelGGL(k_admm_batch_reduce2, dim3(ADMM_NRES, (unsigned)b.B), dim3(64), 0, st, b, part, (int64_t)g.rows(), (int64_t)nb, res);
}
}  // namespace kvx
