// k_qp_batch: one workgroup (256 threads, four wavefronts) carries one small dense QP from its starting point to its status
// (qp_batch.hpp).  It is a device restatement of _ipm.coneqp_start / _ipm.coneqp_loop on the orthant with refinement 0:
// coneprog.py:2044-2105 (start), 2167-2234 (residuals, stopping test), 2243-2316 (scaling, f4_no_ir), 2357-2456 (the two
// directions), 2459-2547 (step and scaling update, misc.py:444-464), and the Newton solve of misc.kkt_chol2 (misc.py:1489-1563)
// with dense Cholesky factors of S = P + G' diag(di^2) G and, for p > 0, of K = X'X with X = L^-1 A'.
//
// Everything a member iterates on lives in LDS: S (leading dimension n | 1, odd, so that a walk along a row changes bank), its
// factor in place, X and K (their region holds the staged rows of diag(di) G while S is assembled, when X and K are not live),
// and the n-, p- and ml-vectors.  P, q, G, h, A, b are read from HBM / L2; G is column-major and read with lanes along its
// rows.  Every sum has a fixed order: a thread's partial sum runs over its indices ascending, a wavefront adds by an xor
// butterfly, the four wavefront sums are added 0..3 -- so a member's bytes depend on nothing but its own data.  No atomics, no
// communication between workgroups.  Every loop is bounded by maxiters, n, ml or p; every branch around a barrier is taken on
// values all threads read from the same LDS words, so it is workgroup-uniform.  A NaN or Inf never passes a pivot test
// (!(pivot > 0 && pivot < inf) fails) and makes every comparison of the stopping test false, so such a member ends with exit 3,
// 2 or 1.
#include "qp_batch.hpp"
#include "batch_kkt.hpp"

#include <cmath>

namespace kvx {
namespace {

using namespace batchdev;                     // the reductions, row_dot, gemv_t_add, chol_lds; the KKT core and the orthant
static_assert(NT == QPB_THREADS, "the shared helpers are written for the workgroup of k_qp_batch");

struct Layout {                               // offsets in doubles from the LDS base; every part starts on 16 bytes
    int ldn, ldp;
    int S, XK, X, K, x, dx, rx, y, dy, ry, s, z, d, di, lm, ds, dz, rz, ws3, red, total;
};

__host__ __device__ inline Layout layout(int n, int ml, int p)
{
    Layout L;
    L.ldn = n | 1;
    L.ldp = p | 1;
    int o = 0;
    L.S = o; o += even(n * L.ldn);
    const int xsz = even(p * L.ldn), ksz = even(p * L.ldp), tsz = even(QPB_TILE * L.ldn);
    L.XK = L.X = o; L.K = o + xsz; o += (xsz + ksz > tsz ? xsz + ksz : tsz);
    const int nv = even(n), pv = even(p), mv = even(ml);
    L.x = o; o += nv; L.dx = o; o += nv; L.rx = o; o += nv;
    L.y = o; o += pv; L.dy = o; o += pv; L.ry = o; o += pv;
    L.s = o; o += mv; L.z = o; o += mv; L.d = o; o += mv; L.di = o; o += mv; L.lm = o; o += mv;
    L.ds = o; o += mv; L.dz = o; o += mv; L.rz = o; o += mv; L.ws3 = o; o += mv;
    L.red = o; o += NW * NRED;
    L.total = o;
    return L;
}

struct Member : KktMem {                      // one member's data in HBM and its vectors and matrices in LDS
    int ml;
    const double *P, *q, *G, *h, *b;
    double *x, *dx, *rx, *y, *dy, *ry, *s, *z, *d, *di, *lm, *ds, *dz, *rz, *ws3, *red;
};

// The KKT factorisation in the scaling di (misc.py:1436-1487): S = P + G' diag(di^2) G, its factor L in place, and for p > 0
// X, K and its factor (batch_kkt.hpp).  false on a failed pivot.  Barriers before (the caller's) and after.
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

// misc.py:1489-1563 on the LDS vectors (vx, vy, vz) = (bx, by, bz): on return ux, uy, W uz.  Barriers before (the caller's)
// and after.
__device__ __forceinline__ void kkt_solve(const Member &M, double *vx, double *vy, double *vz)
{
    orth_kkt_before(M.G, M.ml, M.n, M.di, vx, vz);
    kkt_reduced_solve(M, false, vx, vy);
    orth_kkt_after(M.G, M.ml, M.n, M.di, vx, vz);
}

__global__ void __launch_bounds__(QPB_THREADS) k_qp_batch(QpBatchArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, n = a.n, ml = a.ml, p = a.p;
    const int64_t bm = blockIdx.x;
    const Layout L = layout(n, ml, p);
    Member M;
    M.n = n; M.ml = ml; M.p = p; M.ldn = L.ldn; M.ldp = L.ldp;
    M.P = a.P + bm * a.sP; M.q = a.c + bm * a.sc; M.G = a.G + bm * a.sG; M.h = a.h + bm * a.sh;
    M.A = p ? a.A + bm * a.sA : nullptr; M.b = p ? a.b + bm * a.sb : nullptr;
    M.S = lds + L.S; M.T = lds + L.XK; M.X = lds + L.X; M.K = lds + L.K;
    M.x = lds + L.x; M.dx = lds + L.dx; M.rx = lds + L.rx; M.y = lds + L.y; M.dy = lds + L.dy; M.ry = lds + L.ry;
    M.s = lds + L.s; M.z = lds + L.z; M.d = lds + L.d; M.di = lds + L.di; M.lm = lds + L.lm; M.ds = lds + L.ds; M.dz = lds + L.dz;
    M.rz = lds + L.rz; M.ws3 = lds + L.ws3; M.red = lds + L.red;
    double *xo = a.x + bm * n, *yo = p ? a.y + bm * p : nullptr, *so = a.s + bm * ml, *zo = a.z + bm * ml, *st = a.stats + bm * QPB_NSTAT;

    // ---- starting point (coneprog.py:2044-2105): W = I, [P A' G'; A 0 0; G 0 -I][x; y; z] = [-q; b; h], s = -z
    for (int k = tid; k < ml; k += NT) { M.d[k] = 1.0; M.di[k] = 1.0; M.z[k] = M.h[k]; }
    if (tid < n) M.x[tid] = -M.q[tid];
    if (tid < p) M.y[tid] = M.b[tid];
    __syncthreads();
    if (!factor(M)) {                                      // solvers.qp: ValueError("Rank(A) < p or Rank([P; A; G]) < n")
        for (int k = tid; k < ml; k += NT) { so[k] = 0.0; zo[k] = 0.0; }
        if (tid < n) xo[tid] = 0.0;
        if (tid < p) yo[tid] = 0.0;
        if (tid < QPB_NSTAT) st[tid] = NAN;
        if (tid == 0) { a.iters[bm] = 0; a.exitc[bm] = QPB_RANK; }
        return;
    }
    kkt_solve(M, M.x, M.y, M.z);
    double r0[3] = {0.0, 0.0, 0.0};                        // |q|^2, |b|^2, |h|^2 of resx0, resy0, resz0 (coneprog.py:1977-1979)
    if (tid < n) r0[0] = M.q[tid] * M.q[tid];
    if (tid < p) r0[1] = M.b[tid] * M.b[tid];
    {
        double mx[2] = {-INFINITY, -INFINITY}, nr[2] = {0.0, 0.0};
        for (int k = tid; k < ml; k += NT) {
            const double zk = M.z[k], sk = -zk, hk = M.h[k];
            M.s[k] = sk;
            mx[0] = fmax(mx[0], -sk); mx[1] = fmax(mx[1], -zk);
            nr[0] += sk * sk; nr[1] += zk * zk;
            r0[2] += hk * hk;
        }
        blk_reduce<2, true>(mx, M.red);
        blk_reduce<2, false>(nr, M.red);
        blk_reduce<3, false>(r0, M.red);
        const bool ps = mx[0] >= -1e-8 * fmax(sqrt(nr[0]), 1.0), pz = mx[1] >= -1e-8 * fmax(sqrt(nr[1]), 1.0);
        for (int k = tid; k < ml; k += NT) {               // each thread shifts the entries it wrote itself
            if (ps) M.s[k] += 1.0 + mx[0];
            if (pz) M.z[k] += 1.0 + mx[1];
        }
    }
    const double resx0 = fmax(1.0, sqrt(r0[0])), resy0 = fmax(1.0, sqrt(r0[1])), resz0 = fmax(1.0, sqrt(r0[2]));
    double gap;
    {
        double g[1] = {0.0};
        for (int k = tid; k < ml; k += NT) g[0] += M.s[k] * M.z[k];
        blk_reduce<1, false>(g, M.red);                    // its barriers also publish x, y, s, z
        gap = g[0];
    }

    int code = QPB_MAXITERS, iters = 0;
    double relgap = NAN, pcost = NAN, dcost = NAN, pres = NAN, dres = NAN;
    for (;; iters++) {
        // ---- residuals and objectives (coneprog.py:2167-2203)
        double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};               // x'(Px + q), x'q, |rx|^2, |ry|^2, |rz|^2, y'ry, z'rz
        if (tid < n) {
            double t = 0.0;
            for (int j = 0; j < n; j++) t += (j <= tid ? M.P[tid + j * n] : M.P[j + tid * n]) * M.x[j];
            t += M.q[tid];
            M.rx[tid] = t;
            v[0] = M.x[tid] * t;
            v[1] = M.x[tid] * M.q[tid];
        }
        if (tid < p) {
            const double t = row_dot(M.A, p, n, tid, M.x) - M.b[tid];
            M.ry[tid] = t;
            v[3] = t * t;
            v[5] = M.y[tid] * t;
        }
        for (int k = tid; k < ml; k += NT) {
            const double t = (M.s[k] - M.h[k]) + row_dot(M.G, ml, n, k, M.x);
            M.rz[k] = t;
            v[4] += t * t;
            v[6] += M.z[k] * t;
        }
        __syncthreads();
        if (p > 0) gemv_t_add(M.A, p, n, M.y, nullptr, 1.0, M.rx);
        __syncthreads();
        gemv_t_add(M.G, ml, n, M.z, nullptr, 1.0, M.rx);
        __syncthreads();
        if (tid < n) v[2] = M.rx[tid] * M.rx[tid];
        blk_reduce<7, false>(v, M.red);
        const double f0 = 0.5 * (v[0] + v[1]);
        pcost = f0;
        dcost = f0 + v[5] + v[6] - gap;
        relgap = pcost < 0.0 ? gap / -pcost : (dcost > 0.0 ? gap / dcost : NAN);
        pres = fmax(sqrt(v[3]) / resy0, sqrt(v[4]) / resz0);
        dres = sqrt(v[2]) / resx0;
        if (iters == a.maxiters) { code = QPB_MAXITERS; break; }
        if (pres <= a.feastol && dres <= a.feastol && (gap <= a.abstol || relgap <= a.reltol)) { code = QPB_OPTIMAL; break; }

        // ---- scaling of the first iteration (misc.py:284-287), the factorisation
        if (iters == 0) orth_first_scaling(ml, M.s, M.z, M.d, M.di, M.lm);
        __syncthreads();
        if (!factor(M)) { code = iters == 0 ? QPB_RANK : QPB_SINGULAR; break; }

        // ---- the affine-scaling and the combined direction (coneprog.py:2357-2456, f4_no_ir :2288-2316)
        const double mu = gap / ml;
        double sigma = 0.0, step = 0.0;
        for (int i = 0; i < 2; i++) {
            const bool corr = a.correction != 0;
            for (int k = tid; k < ml; k += NT) {
                const double lk = M.lm[k];
                double t = -lk * lk + sigma * mu;
                if (corr && i == 1) t -= M.ws3[k];
                t /= lk;
                M.ds[k] = t;
                M.dz[k] = -M.rz[k] - M.d[k] * t;
            }
            if (tid < n) M.dx[tid] = -M.rx[tid];
            if (tid < p) M.dy[tid] = -M.ry[tid];
            __syncthreads();
            kkt_solve(M, M.dx, M.dy, M.dz);
            double dsdz[1] = {0.0}, mx[2] = {-INFINITY, -INFINITY};
            for (int k = tid; k < ml; k += NT) {
                const double lk = M.lm[k], zk = M.dz[k], sk = M.ds[k] - zk, pr = sk * zk;
                dsdz[0] += pr;
                if (corr && i == 0) M.ws3[k] = pr;
                const double s2 = sk / lk, z2 = zk / lk;
                M.ds[k] = s2; M.dz[k] = z2;
                mx[0] = fmax(mx[0], -s2); mx[1] = fmax(mx[1], -z2);
            }
            blk_reduce<1, false>(dsdz, M.red);
            blk_reduce<2, true>(mx, M.red);
            const double t = fmax(0.0, fmax(mx[0], mx[1]));
            step = t == 0.0 ? 1.0 : (i == 0 ? fmin(1.0, 1.0 / t) : fmin(1.0, 0.99 / t));
            if (i == 0) {
                const double u = fmin(1.0, fmax(0.0, 1.0 - step + dsdz[0] / gap * (step * step)));
                sigma = u * u * u;
            }
        }

        // ---- the step, the scaling update (misc.py:444-464), s and z of the next iteration (coneprog.py:2459-2547)
        if (tid < n) M.x[tid] += step * M.dx[tid];
        if (tid < p) M.y[tid] += step * M.dy[tid];
        double g[1] = {orth_update(ml, step, M.ds, M.dz, M.d, M.di, M.lm, M.s, M.z)};
        blk_reduce<1, false>(g, M.red);
        gap = g[0];
    }

    // ---- the member's result (coneprog.py:2213-2234, 2261-2275); after a first factorisation that failed: zeros
    const bool rank = code == QPB_RANK;
    double mx[2] = {-INFINITY, -INFINITY};
    for (int k = tid; k < ml; k += NT) {
        const double sk = M.s[k], zk = M.z[k];
        so[k] = rank ? 0.0 : sk; zo[k] = rank ? 0.0 : zk;
        mx[0] = fmax(mx[0], -sk); mx[1] = fmax(mx[1], -zk);
    }
    if (tid < n) xo[tid] = rank ? 0.0 : M.x[tid];
    if (tid < p) yo[tid] = rank ? 0.0 : M.y[tid];
    blk_reduce<2, true>(mx, M.red);
    if (tid == 0) {
        const double out[QPB_NSTAT] = {gap, relgap, pcost, dcost, pres, dres, -mx[0], -mx[1]};
#pragma unroll
        for (int k = 0; k < QPB_NSTAT; k++) st[k] = rank ? NAN : out[k];
        a.iters[bm] = rank ? 0 : iters;
        a.exitc[bm] = code;
    }
}

}  // namespace

size_t qp_batch_lds_bytes(int n, int ml, int p) { return (size_t)layout(n, ml, p).total * sizeof(double); }

hipError_t launch_qp_batch(hipStream_t st, const QpBatchArgs &a)
{
    // per device, so asked of the current one at every launch
    const hipError_t e = hipFuncSetAttribute((const void *)k_qp_batch, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    k_qp_batch<<<dim3((unsigned)a.B), dim3(QPB_THREADS), qp_batch_lds_bytes(a.n, a.ml, a.p), st>>>(a);
    return hipGetLastError();
}

}  // namespace kvx
