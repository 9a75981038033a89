// Kernels of the general-cone KKT assembly (cone_api.cpp) -- S = Gs' Gs with Gs = pack2(W^-T G), what the reference's
// misc.kkt_chol forms with dense BLAS (misc.py:1267-1277) -- and the vector helpers of the general-cone driver (kvxopt_amd/cone.py).
// Every kernel writes each output once (gathers in a fixed order, no floating-point atomics): two assemblies of the same
// operands give the same bits.
#include "cone.hpp"

namespace kvx {
namespace {

static inline unsigned grid_of(int64_t n, int bs = 256)
{
    int64_t b = (n + bs - 1) / bs;
    if (b > 4096) b = 4096;
    if (b < 1) b = 1;
    return (unsigned)b;
}

#define CONE_LOOP(i, n) \
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

__global__ void k_cone_gather(int64_t n, const int64_t *__restrict__ idx, const double *__restrict__ src, double *__restrict__ dst)
{
    CONE_LOOP(i, n) dst[i] = src[idx[i]];
}

__global__ void k_cone_scatter(int64_t n, const int64_t *__restrict__ idx, const double *__restrict__ src, double *__restrict__ dst)
{
    CONE_LOOP(i, n) dst[idx[i]] = src[i];
}

__global__ void k_cone_move(int64_t n, const int64_t *__restrict__ sidx, const double *__restrict__ src, const int64_t *__restrict__ didx,
                            int64_t doff, double *__restrict__ dst)
{
    CONE_LOOP(i, n) dst[didx[i] - doff] = src[sidx[i]];
}

__global__ void k_cone_weights(int64_t ml, int64_t mq, const int32_t *__restrict__ rcone, const double *__restrict__ di,
                               const double *__restrict__ beta, double *__restrict__ w)
{
    CONE_LOOP(r, ml + mq) {
        if (r < ml) w[r] = di[r] * di[r];
        else {
            const double b = beta[rcone[r - ml]];
            w[r] = 1.0 / (b * b);
        }
    }
}

__global__ void k_cone_vnorm(int64_t nq, const int64_t *__restrict__ qoff, const double *__restrict__ v, double *__restrict__ nv2)
{
    CONE_LOOP(k, nq) {
        double a = 0.0;
        for (int64_t r = qoff[k]; r < qoff[k + 1]; r++) a = __builtin_fma(v[r], v[r], a);
        nv2[k] = a;
    }
}

// vrow: index of the row in the 'q' section of v; vhead: 1 when the row is the first of its cone (J v = (v0, -v1, ...))
__global__ void k_cone_pq(int64_t npairs, const int64_t *__restrict__ ptr, const int64_t *__restrict__ pos, const int64_t *__restrict__ vrow,
                          const int32_t *__restrict__ vhead, const double *__restrict__ Gx, const double *__restrict__ v,
                          double *__restrict__ p, double *__restrict__ q)
{
    CONE_LOOP(t, npairs) {
        double ap = 0.0, aq = 0.0;
        for (int64_t e = ptr[t]; e < ptr[t + 1]; e++) {
            const double g = Gx[pos[e]], vr = v[vrow[e]];
            aq = __builtin_fma(g, vr, aq);
            ap = __builtin_fma(g, vhead[e] ? vr : -vr, ap);
        }
        p[t] = ap;
        q[t] = aq;
    }
}

typedef double d4 __attribute__((ext_vector_type(4)));

// C_b = Y_b' Y_b, Y_b: mp_b x c_b column-major at yoff_b; C_b: c_b x c_b column-major at goff_b, lower triangle written.
// v_mfma_f64_16x16x4_f64: lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15], and holds D[(l >> 4) + 4 q][l & 15].
// A = Y(rows r.., columns i0..)' and B = Y(rows r.., columns j0..): both operands are columns of Y read down their rows.
__global__ __launch_bounds__(256) void k_cone_gram(int64_t ntiles, const int32_t *__restrict__ tblk, const int32_t *__restrict__ ti,
                                                   const int32_t *__restrict__ tj, const int64_t *__restrict__ yoff,
                                                   const int64_t *__restrict__ mpv, const int64_t *__restrict__ ncol,
                                                   const int64_t *__restrict__ goff, const double *__restrict__ Y, double *__restrict__ C)
{
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= ntiles) return;                                    // (whole wave: no MFMA with inactive lanes)
    const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    const int b = tblk[t];
    const int64_t mp = mpv[b], c = ncol[b];
    const int64_t i0 = 16 * (int64_t)ti[t], j0 = 16 * (int64_t)tj[t];
    const bool ia = i0 + lr < c, ja = j0 + lr < c;
    const double *Yi = Y + yoff[b] + mp * (ia ? i0 + lr : 0);
    const double *Yj = Y + yoff[b] + mp * (ja ? j0 + lr : 0);
    d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
    int64_t r = 0;
    for (; r + 16 <= mp; r += 16) {                             // four k-steps, loads first
        double av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            av[u] = ia ? Yi[r + 4 * u + lk] : 0.0;
            bv[u] = ja ? Yj[r + 4 * u + lk] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
    }
    for (; r < mp; r += 4) {
        const bool rk = r + lk < mp;
        const double av = (ia && rk) ? Yi[r + lk] : 0.0;
        const double bv = (ja && rk) ? Yj[r + lk] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
    const int64_t col = j0 + lr;
#pragma unroll
    for (int qq = 0; qq < 4; qq++) {
        const int64_t row = i0 + lk + 4 * qq;
        if (row < c && col < c && row >= col) C[goff[b] + row + c * col] = acc[qq];
    }
}

// HAS_H: the entry's value of H (hidx[e] >= 0: its position in Hx) is added last -- cones, then blocks, then H.  Without it the
// floating-point operations and their order are those of the plain assembly.
template <bool HAS_H>
__global__ void k_cone_pgather(int64_t pnz, const int64_t *__restrict__ qptr, const int32_t *__restrict__ qk, const int64_t *__restrict__ qa,
                               const int64_t *__restrict__ qb, const double *__restrict__ p, const double *__restrict__ q,
                               const double *__restrict__ nv2, const double *__restrict__ beta, const int64_t *__restrict__ sptr,
                               const int64_t *__restrict__ sidx, const double *__restrict__ C, const int64_t *__restrict__ hidx,
                               const double *__restrict__ Hx, double *__restrict__ Px)
{
    CONE_LOOP(e, pnz) {
        double acc = 0.0;
        for (int64_t u = qptr[e]; u < qptr[e + 1]; u++) {
            const int k = qk[u];
            const double pa = p[qa[u]], pb = p[qb[u]], qa_ = q[qa[u]], qb_ = q[qb[u]];
            const double bk = beta[k];
            acc += (4.0 * nv2[k] * pa * pb - 2.0 * (pa * qb_ + qa_ * pb)) / (bk * bk);
        }
        for (int64_t u = sptr[e]; u < sptr[e + 1]; u++) acc += C[sidx[u]];
        if (HAS_H) {
            const int64_t hp = hidx[e];
            if (hp >= 0) acc += Hx[hp];
        }
        Px[e] = acc;
    }
}

__global__ __launch_bounds__(256) void k_nts_colscale(const int64_t *__restrict__ off2, const int64_t *__restrict__ off1, double *__restrict__ x,
                                                      const double *__restrict__ w)
{
    const int64_t o2 = off2[blockIdx.x], o1 = off1[blockIdx.x];
    const int64_t m = off1[blockIdx.x + 1] - o1;
    for (int64_t e = threadIdx.x; e < m * m; e += blockDim.x) x[o2 + e] *= sqrt(w[o1 + e / m]);
}

}  // namespace

void launch_cone_gather(hipStream_t st, int64_t n, const int64_t *idx, const double *src, double *dst)
{ if (n > 0) hipLaunchKernelGGL(k_cone_gather, dim3(grid_of(n)), dim3(256), 0, st, n, idx, src, dst); }

void launch_cone_scatter(hipStream_t st, int64_t n, const int64_t *idx, const double *src, double *dst)
{ if (n > 0) hipLaunchKernelGGL(k_cone_scatter, dim3(grid_of(n)), dim3(256), 0, st, n, idx, src, dst); }

void launch_cone_move(hipStream_t st, int64_t n, const int64_t *sidx, const double *src, const int64_t *didx, int64_t doff, double *dst)
{ if (n > 0) hipLaunchKernelGGL(k_cone_move, dim3(grid_of(n)), dim3(256), 0, st, n, sidx, src, didx, doff, dst); }

void launch_cone_weights(hipStream_t st, int64_t ml, int64_t mq, const int32_t *rcone, const double *di, const double *beta, double *w)
{ if (ml + mq > 0) hipLaunchKernelGGL(k_cone_weights, dim3(grid_of(ml + mq)), dim3(256), 0, st, ml, mq, rcone, di, beta, w); }

void launch_cone_vnorm(hipStream_t st, int64_t nq, const int64_t *qoff, const double *v, double *nv2)
{ if (nq > 0) hipLaunchKernelGGL(k_cone_vnorm, dim3(grid_of(nq)), dim3(256), 0, st, nq, qoff, v, nv2); }

void launch_cone_pq(hipStream_t st, int64_t npairs, const int64_t *ptr, const int64_t *pos, const int64_t *vrow, const int32_t *vhead,
                    const double *Gx, const double *v, double *p, double *q)
{ if (npairs > 0) hipLaunchKernelGGL(k_cone_pq, dim3(grid_of(npairs)), dim3(256), 0, st, npairs, ptr, pos, vrow, vhead, Gx, v, p, q); }

void launch_cone_gram(hipStream_t st, int64_t ntiles, const int32_t *tblk, const int32_t *ti, const int32_t *tj, const int64_t *yoff,
                      const int64_t *mp, const int64_t *ncol, const int64_t *goff, const double *Y, double *C)
{
    if (ntiles > 0)
        hipLaunchKernelGGL(k_cone_gram, dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, st, ntiles, tblk, ti, tj, yoff, mp, ncol, goff, Y, C);
}

void launch_cone_pgather(hipStream_t st, int64_t pnz, const int64_t *qptr, const int32_t *qk, const int64_t *qa, const int64_t *qb,
                         const double *p, const double *q, const double *nv2, const double *beta, const int64_t *sptr,
                         const int64_t *sidx, const double *C, const int64_t *hidx, const double *Hx, double *Px)
{
    if (pnz <= 0) return;
    if (hidx)
        hipLaunchKernelGGL(k_cone_pgather<true>, dim3(grid_of(pnz)), dim3(256), 0, st, pnz, qptr, qk, qa, qb, p, q, nv2, beta, sptr, sidx, C,
                           hidx, Hx, Px);
    else
        hipLaunchKernelGGL(k_cone_pgather<false>, dim3(grid_of(pnz)), dim3(256), 0, st, pnz, qptr, qk, qa, qb, p, q, nv2, beta, sptr, sidx, C,
                           hidx, Hx, Px);
}

void launch_nts_colscale(hipStream_t st, int64_t ns, const int64_t *off2, const int64_t *off1, double *x, const double *w)
{ if (ns > 0) hipLaunchKernelGGL(k_nts_colscale, dim3((unsigned)ns), dim3(256), 0, st, off2, off1, x, w); }

}  // namespace kvx
