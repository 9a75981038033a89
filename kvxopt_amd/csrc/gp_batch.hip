// k_gp_batch: one workgroup (256 threads, four wavefronts) carries one small dense geometric program from x = 0 to its status
// (gp_batch.hpp).  It is a device restatement of cvx._cpl at refinement 0 on cp's epigraph form: cvxprog.py:625-755 (residuals,
// phi, stopping test), 757-840 (scaling, factorisation, the restore after a relaxed line search), 858-883 (f4_no_ir), 925-1080
// (the two directions), 1081-1261 (the relaxed and the standard line search with the saved state), 1264-1355 (step and scaling
// update, misc.py:444-464), the evaluator of cvxprog.gp (cvxprog.py:2109-2150) and the Newton solve of misc.kkt_chol2
// (misc.py:1489-1563) with dense Cholesky factors of S = H + J' diag(di^2) J and, for p > 0, of K = X'X with X = L^-1 A'.
//
// The variable is (x, t), t in column n, so the system has order n + 1 <= 64.  The mnl + 1 log-sum-exp rows (the objective,
// f_0 - t, first) and the ml rows of G are one orthant block of N rows with the scaling d, di.  J = [Df; G] is never held: with
// y = exp(u) / sum exp(u) per block in LDS, J'v on the nonlinear rows is F'(y o v_block) with -v_0 in column n, and J u is per
// block sum_k y_k (F_k u), minus u_t on row 0.  H is never held either: S receives the staged rows di_k G_k, dnli_i Df_i and the
// centred factors sqrt(z_i y_k) (F_k - Df_i) of cvxprog.py:2135-2150 through kkt_s_add_rows; a one-term block has y = 1 and
// Df_i = F_k, so its factors are exact zeros.  The block gradients a tile of factors needs are formed beside the tile, in the
// region X and K take once S is factored.
//
// Everything a member iterates on lives in LDS.  F, g, G, h, b are read from HBM / L2.  A member's HBM scratch holds A with a
// zero column n (kkt_equalities reads n + 1 columns) and the saved state of the line search, which is written at most once per
// iteration and read only on a restore; a thread reads back only what it wrote itself.  Every sum has a fixed order: a thread's
// partial sum runs over its indices ascending, a wavefront adds by an xor butterfly, the four wavefront sums are added 0..3 --
// so a member's bytes depend on nothing but its own data.  No atomics, no communication between workgroups.  Every loop is
// bounded by maxiters, n, N, p, l, K_i, or by the count of halvings of a line search (GPB_MAX_HALVINGS: the reference has no
// bound and would spin on a NaN); every branch around a barrier is taken on values all threads read from the same LDS words,
// so it is workgroup-uniform.  A NaN or Inf never passes a pivot test (!(pivot > 0 && pivot < inf) fails).
#include "gp_batch.hpp"
#include "batch_kkt.hpp"
#include "gp_batch_device.hpp"

#include <cmath>

namespace kvx {
namespace {

using namespace gpdev;
constexpr double BETA = 0.5, ALPHA = 0.01, STEP = 0.99;     // cvxprog.py:384-388, 424
constexpr int MAX_RELAXED_ITERS = 8, EXPON = 3;

struct Layout {                               // offsets in doubles from the LDS base; every part starts on 16 bytes
    int ne, N, ldn, ldp;
    int S, XK, X, K, Gs, x, dx, rx, newx, newrx, y, dy, ry, newy, s, z, d, di, lm, lmsq, ds, dz, ds2, dz2, rz, ws, news, newz, f,
        newf, yv, yn, w, off, blk, red, total;
};

__host__ __device__ inline Layout layout(int n, int m, int l, int ml, int p)
{
    Layout L;
    L.ne = n + 1;
    L.N = m + ml;
    L.ldn = L.ne | 1;
    L.ldp = p | 1;
    int o = 0;
    L.S = o; o += even(L.ne * L.ldn);
    const int xsz = even(p * L.ldn), ksz = even(p * L.ldp), tsz = even(GPB_TILE * L.ldn);
    L.XK = L.X = o; L.K = o + xsz; L.Gs = o + tsz; o += (xsz + ksz > 2 * tsz ? xsz + ksz : 2 * tsz);
    const int nv = even(L.ne), pv = even(p), mv = even(L.N), bv = even(m), lv = even(l);
    L.x = o; o += nv; L.dx = o; o += nv; L.rx = o; o += nv; L.newx = o; o += nv; L.newrx = o; o += nv;
    L.y = o; o += pv; L.dy = o; o += pv; L.ry = o; o += pv; L.newy = o; o += pv;
    L.s = o; o += mv; L.z = o; o += mv; L.d = o; o += mv; L.di = o; o += mv; L.lm = o; o += mv; L.lmsq = o; o += mv;
    L.ds = o; o += mv; L.dz = o; o += mv; L.ds2 = o; o += mv; L.dz2 = o; o += mv; L.rz = o; o += mv; L.ws = o; o += mv;
    L.news = o; o += mv; L.newz = o; o += mv;
    L.f = o; o += bv; L.newf = o; o += bv;
    L.yv = o; o += lv; L.yn = o; o += lv; L.w = o; o += lv;
    L.off = o; o += even(m + 1) / 2;          // ints: the first term of every block and l
    L.blk = o; o += even(l) / 2;              // ints: the block of every term
    o = even(o);
    L.red = o; o += NW * NRED;
    L.total = o;
    return L;
}

struct Saved {                                // offsets in doubles into a member's HBM scratch
    int A, x, dx, rx, y, dy, ry, d, di, s, z, ds, dz, ds2, dz2, lm, lmsq, rz, total;
};

__host__ __device__ inline Saved saved(int n, int m, int ml, int p)
{
    Saved V;
    const int nv = even(n + 1), pv = even(p), mv = even(m + ml);
    int o = 0;
    V.A = o; o += even(p * (n + 1));
    V.x = o; o += nv; V.dx = o; o += nv; V.rx = o; o += nv;
    V.y = o; o += pv; V.dy = o; o += pv; V.ry = o; o += pv;
    V.d = o; o += mv; V.di = o; o += mv; V.s = o; o += mv; V.z = o; o += mv; V.ds = o; o += mv; V.dz = o; o += mv;
    V.ds2 = o; o += mv; V.dz2 = o; o += mv; V.lm = o; o += mv; V.lmsq = o; o += mv; V.rz = o; o += mv;
    V.total = o;
    return V;
}

struct Member : GpMem {                       // KktMem::n is the order n + 1 of the system; A is the padded copy in the scratch
    int N;
    const double *h, *b;
    double *x, *dx, *rx, *y, *dy, *ry, *s, *z, *d, *di, *lm, *lmsq, *ds, *dz, *ds2, *dz2, *rz, *ws, *f, *red;
};

// dst[k] := src[k], k < count, every thread its own indices: the way to and from the HBM scratch.  No barrier.
__device__ __forceinline__ void copy_own(double *dst, const double *src, int count)
{
    for (int k = threadIdx.x; k < count; k += NT) dst[k] = src[k];
}

// The KKT factorisation at (x, z) in the scaling di (misc.py:1436-1487): S = H + J' diag(di^2) J from staged rows
// (gp_batch_device.hpp), its factor L in place, and for p > 0 X, K and its factor (batch_kkt.hpp).  false on a failed pivot.
// Barriers before (the caller's) and after.
__device__ __forceinline__ bool factor(const Member &M)
{
    gp_assemble<true>(M, M.z, M.di, false);
    return chol_lds(M.S, M.ldn, M.n) && kkt_equalities(M);
}

// misc.py:1489-1563 on the LDS vectors (vx, vy, vz) = (bx, by, bz): on return ux, uy, W uz.  Barriers before (the caller's)
// and after.
__device__ __forceinline__ void kkt_solve(const Member &M, double *vx, double *vy, double *vz)
{
    for (int k = threadIdx.x; k < M.N; k += NT) vz[k] *= M.di[k];
    __syncthreads();
    jt_add<true>(M, M.yv, vz, M.di, 1.0, vx);
    kkt_reduced_solve(M, false, vx, vy);
    j_mul<true>(M, M.yv, vx, M.ws);
    for (int k = threadIdx.x; k < M.N; k += NT) vz[k] = M.di[k] * M.ws[k] - vz[k];
    __syncthreads();
}

__global__ void __launch_bounds__(GPB_THREADS) k_gp_batch(GpBatchArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, nx = a.n, m = a.m, l = a.l, ml = a.ml, p = a.p;
    const int64_t bm = blockIdx.x;
    const Layout L = layout(nx, m, l, ml, p);
    const Saved V = saved(nx, m, ml, p);
    const int ne = L.ne, N = L.N;
    double *const sv = a.scratch + bm * V.total;
    int *const off = reinterpret_cast<int *>(lds + L.off), *const blk = reinterpret_cast<int *>(lds + L.blk);
    Member M;
    M.n = ne; M.p = p; M.ldn = L.ldn; M.ldp = L.ldp; M.nx = nx; M.m = m; M.ml = ml; M.N = N; M.l = l;
    M.F = a.F + bm * a.sF; M.g = a.c + bm * a.sc;
    M.G = ml ? a.G + bm * a.sG : nullptr; M.h = ml ? a.h + bm * a.sh : nullptr;
    M.A = sv + V.A; M.b = p ? a.b + bm * a.sb : nullptr;
    M.off = off; M.blk = blk;
    M.S = lds + L.S; M.T = lds + L.XK; M.X = lds + L.X; M.K = lds + L.K; M.Gs = lds + L.Gs;
    M.x = lds + L.x; M.dx = lds + L.dx; M.rx = lds + L.rx; M.y = lds + L.y; M.dy = lds + L.dy; M.ry = lds + L.ry;
    M.s = lds + L.s; M.z = lds + L.z; M.d = lds + L.d; M.di = lds + L.di; M.lm = lds + L.lm; M.lmsq = lds + L.lmsq;
    M.ds = lds + L.ds; M.dz = lds + L.dz; M.ds2 = lds + L.ds2; M.dz2 = lds + L.dz2; M.rz = lds + L.rz; M.ws = lds + L.ws;
    M.f = lds + L.f; M.yv = lds + L.yv; M.w = lds + L.w; M.red = lds + L.red;
    double *const newx = lds + L.newx, *const newrx = lds + L.newrx, *const newy = lds + L.newy, *const news = lds + L.news,
                 *const newz = lds + L.newz, *const newf = lds + L.newf, *const yn = lds + L.yn;
    double *xo = a.x + bm * nx, *yo = p ? a.y + bm * p : nullptr, *so = a.s + bm * N, *zo = a.z + bm * N, *st = a.stats + bm * GPB_NSTAT;

    // ---- the blocks, A with its zero column, the starting point x = 0, t = 0, y = 0, s = z = 1 (cvxprog.py:557-570)
    gp_blocks(a, off, blk);
    if (p > 0) {
        const double *A = a.A + bm * a.sA;
        for (int e = tid; e < p * ne; e += NT) sv[V.A + e] = e < p * nx ? A[e] : 0.0;
    }
    if (tid < ne) M.x[tid] = 0.0;
    if (tid < p) M.y[tid] = 0.0;
    for (int k = tid; k < N; k += NT) { M.s[k] = 1.0; M.z[k] = 1.0; }
    __syncthreads();

    int code = GPB_MAXITERS, iters = 0, relaxed_iters = 0;
    double gap = NAN, relgap = NAN, pcost = NAN, dcost = NAN, pres = NAN, dres = NAN;
    double resx0 = 1.0, resznl0 = 1.0, pres0 = 1.0, dres0 = 1.0, theta1 = 0.0, theta2 = 0.0, theta3 = 0.0;
    double phi0 = 0.0, dphi0 = 0.0, gap0 = 0.0, step0 = 0.0, dsdz0 = 0.0, sigma0 = 0.0, eta0 = 0.0;
    for (;; iters++) {
        // ---- f, the weights of Df and H at x; residuals and objectives (cvxprog.py:625-727)
        lse_eval<true>(M, M.x, M.f, M.yv);
        double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};               // |rx|^2, |ry|^2, |rznl|^2, |rzl|^2, y'ry, z'rz, s'z
        if (tid < ne) M.rx[tid] = tid == nx ? 1.0 : 0.0;                 // c = e_n
        if (tid < p) {
            const double t = row_dot(M.A, p, nx, tid, M.x) - M.b[tid];
            M.ry[tid] = t;
            v[1] = t * t;
            v[4] = M.y[tid] * t;
        }
        for (int k = tid; k < N; k += NT) {
            const double t = k < m ? M.s[k] + M.f[k] : (M.s[k] - M.h[k - m]) + row_dot(M.G, ml, nx, k - m, M.x);
            M.rz[k] = t;
            if (k < m) v[2] += t * t;
            else v[3] += t * t;
            v[5] += M.z[k] * t;
            v[6] += M.s[k] * M.z[k];
        }
        __syncthreads();
        if (p > 0) gemv_t_add(M.A, p, ne, M.y, nullptr, 1.0, M.rx);
        __syncthreads();
        jt_add<true>(M, M.yv, M.z, nullptr, 1.0, M.rx);
        if (tid < ne) v[0] = M.rx[tid] * M.rx[tid];
        blk_reduce<7, false>(v, M.red);
        gap = v[6];
        double resx = sqrt(v[0]), resznl = sqrt(v[2]);
        pcost = M.x[nx];
        dcost = pcost + v[4] + v[5] - gap;
        relgap = pcost < 0.0 ? gap / -pcost : (dcost > 0.0 ? gap / dcost : NAN);
        pres = sqrt(v[1] + v[2] + v[3]);
        dres = resx;
        if (iters == 0) {
            resx0 = fmax(1.0, resx); resznl0 = fmax(1.0, resznl);
            pres0 = fmax(1.0, pres); dres0 = fmax(1.0, dres);
            gap0 = gap;
            theta1 = 1.0 / gap0; theta2 = 1.0 / resx0; theta3 = 1.0 / resznl0;
        }
        double phi = theta1 * gap + theta2 * resx + theta3 * resznl;
        pres /= pres0; dres /= dres0;
        if (iters == a.maxiters) { code = GPB_MAXITERS; break; }
        if (pres <= a.feastol && dres <= a.feastol && (gap <= a.abstol || relgap <= a.reltol)) { code = GPB_OPTIMAL; break; }

        // ---- scaling of the first iteration (misc.py:284-287), lmbda o lmbda, the factorisation (cvxprog.py:757-840)
        if (iters == 0) orth_first_scaling(N, M.s, M.z, M.d, M.di, M.lm);
        for (int k = tid; k < N; k += NT) M.lmsq[k] = M.lm[k] * M.lm[k];   // a thread squares the entries it wrote itself
        __syncthreads();
        bool failed = false;
        for (int attempt = 0; !factor(M); attempt++) {
            if (iters == 0) { code = GPB_RANK; failed = true; break; }
            if (attempt == 1 || !(0 < relaxed_iters && relaxed_iters < MAX_RELAXED_ITERS)) { code = GPB_SINGULAR; failed = true; break; }
            // the failure may come from a relaxed line search: restore the saved state, ask for a standard line search, factor again
            phi = phi0; gap = gap0;
            __syncthreads();                               // every thread has read the failed pivot
            copy_own(M.d, sv + V.d, N); copy_own(M.di, sv + V.di, N);
            copy_own(M.x, sv + V.x, ne); copy_own(M.y, sv + V.y, p); copy_own(M.s, sv + V.s, N); copy_own(M.z, sv + V.z, N);
            copy_own(M.lm, sv + V.lm, N);
            copy_own(sv + V.lmsq, M.lmsq, N);              // as the reference has it (cvxprog.py:807): lmbdasq stays
            copy_own(M.rx, sv + V.rx, ne); copy_own(M.ry, sv + V.ry, p); copy_own(M.rz, sv + V.rz, N);
            double r[2] = {0.0, 0.0};
            if (tid < ne) r[0] = M.rx[tid] * M.rx[tid];    // own entries
            for (int k = tid; k < m; k += NT) r[1] += M.rz[k] * M.rz[k];
            blk_reduce<2, false>(r, M.red);                // its barriers also publish the restored state
            resx = sqrt(r[0]); resznl = sqrt(r[1]);
            relaxed_iters = -1;
            lse_eval<true>(M, M.x, M.f, M.yv);
        }
        if (failed) break;

        // ---- the affine-scaling and the combined direction (cvxprog.py:925-1080), each with its line search (:1081-1261)
        double sigma = 0.0, eta = 0.0, step = 0.0;
        bool gaveup = false;
        for (int i = 0; i < 2 && !gaveup; i++) {
            const double mu = gap / N;
            for (int k = tid; k < N; k += NT) {            // ds = -lmbdasq + sigma mu e, then f4_no_ir (cvxprog.py:858-883)
                const double t = (-M.lmsq[k] + sigma * mu) / M.lm[k];
                M.ds[k] = t;
                M.dz[k] = (-1.0 + eta) * M.rz[k] - M.d[k] * t;
            }
            if (tid < ne) M.dx[tid] = (-1.0 + eta) * M.rx[tid];
            if (tid < p) M.dy[tid] = (-1.0 + eta) * M.ry[tid];
            __syncthreads();
            kkt_solve(M, M.dx, M.dy, M.dz);
            double sd[1] = {0.0}, mx[2] = {-INFINITY, -INFINITY};
            for (int k = tid; k < N; k += NT) {
                const double lk = M.lm[k], zk = M.dz[k], sk = M.ds[k] - zk;
                sd[0] += sk * zk;
                M.dz2[k] = M.di[k] * zk; M.ds2[k] = M.d[k] * sk;
                const double s2 = sk / lk, z2 = zk / lk;
                M.ds[k] = s2; M.dz[k] = z2;
                mx[0] = fmax(mx[0], -s2); mx[1] = fmax(mx[1], -z2);
            }
            blk_reduce<1, false>(sd, M.red);
            blk_reduce<2, true>(mx, M.red);
            double dsdz = sd[0];
            const double t = fmax(0.0, fmax(mx[0], mx[1]));
            step = t == 0.0 ? 1.0 : fmin(1.0, STEP / t);
            phi = theta1 * gap + theta2 * resx + theta3 * resznl;
            double dphi = i == 0 ? -phi : -theta1 * (1.0 - sigma) * gap - theta2 * (1.0 - eta) * resx - theta3 * (1.0 - eta) * resznl;

            int halvings = 0;
            for (;;) {
                if (tid < ne) newx[tid] = M.x[tid] + step * M.dx[tid];
                if (tid < p) newy[tid] = M.y[tid] + step * M.dy[tid];
                for (int k = tid; k < N; k += NT) {
                    newz[k] = M.z[k] + step * M.dz2[k];
                    news[k] = M.s[k] + step * M.ds2[k];
                }
                if (tid < ne) newrx[tid] = tid == nx ? 1.0 : 0.0;
                __syncthreads();
                lse_eval<true>(M, newx, newf, yn);
                if (p > 0) gemv_t_add(M.A, p, ne, newy, nullptr, 1.0, newrx);
                __syncthreads();
                jt_add<true>(M, yn, newz, nullptr, 1.0, newrx);
                double r[2] = {0.0, 0.0};
                if (tid < ne) r[0] = newrx[tid] * newrx[tid];
                for (int k = tid; k < m; k += NT) { const double u = news[k] + newf[k]; r[1] += u * u; }
                blk_reduce<2, false>(r, M.red);
                const double newgap = (1.0 - (1.0 - sigma) * step) * gap + step * step * dsdz;
                const double newphi = theta1 * newgap + theta2 * sqrt(r[0]) + theta3 * sqrt(r[1]);
                bool halve = false;
                if (i == 0) {
                    if (newgap <= (1.0 - ALPHA * step) * gap &&
                             ((0 <= relaxed_iters && relaxed_iters < MAX_RELAXED_ITERS) || newphi <= phi + ALPHA * step * dphi)) {
                        const double q = newgap / gap;
                        double q3 = q;
#pragma unroll
                        for (int e = 1; e < EXPON; e++) q3 *= q;
                        sigma = fmin(q, q3);
                        eta = 0.0;
                        break;
                    }
                    halve = true;
                } else if (relaxed_iters == -1) {                          // a standard line search
                    if (newphi <= phi + ALPHA * step * dphi) break;
                    halve = true;
                } else if (relaxed_iters == 0) {
                    if (!(newphi <= phi + ALPHA * step * dphi)) {    // no sufficient decrease: save the state
                        phi0 = phi; dphi0 = dphi; gap0 = gap; step0 = step;
                        dsdz0 = dsdz; sigma0 = sigma; eta0 = eta;
                        copy_own(sv + V.d, M.d, N); copy_own(sv + V.di, M.di, N);
                        copy_own(sv + V.x, M.x, ne); copy_own(sv + V.dx, M.dx, ne); copy_own(sv + V.y, M.y, p); copy_own(sv + V.dy, M.dy, p);
                        copy_own(sv + V.s, M.s, N); copy_own(sv + V.z, M.z, N); copy_own(sv + V.ds, M.ds, N); copy_own(sv + V.dz, M.dz, N);
                        copy_own(sv + V.ds2, M.ds2, N); copy_own(sv + V.dz2, M.dz2, N);
                        copy_own(sv + V.lm, M.lm, N); copy_own(sv + V.lmsq, M.lmsq, N);
                        copy_own(sv + V.rx, M.rx, ne); copy_own(sv + V.ry, M.ry, p); copy_own(sv + V.rz, M.rz, N);
                        relaxed_iters = 1;
                    }
                    break;
                } else if (relaxed_iters < MAX_RELAXED_ITERS) {
                    relaxed_iters = newphi <= phi0 + ALPHA * step0 * dphi0 ? 0 : relaxed_iters + 1;
                    break;
                } else {                                                   // relaxed_iters == MAX_RELAXED_ITERS
                    if (newphi <= phi0 + ALPHA * step0 * dphi0) { relaxed_iters = 0; break; }
                    // resume the last saved line search; every thread is past its reads of this trial (blk_reduce)
                    phi = phi0; dphi = dphi0; gap = gap0; step = step0;
                    dsdz = dsdz0; sigma = sigma0; eta = eta0;
                    copy_own(M.d, sv + V.d, N); copy_own(M.di, sv + V.di, N);
                    copy_own(M.x, sv + V.x, ne); copy_own(M.dx, sv + V.dx, ne); copy_own(M.y, sv + V.y, p); copy_own(M.dy, sv + V.dy, p);
                    copy_own(M.s, sv + V.s, N); copy_own(M.z, sv + V.z, N); copy_own(M.ds, sv + V.ds, N); copy_own(M.dz, sv + V.dz, N);
                    copy_own(M.ds2, sv + V.ds2, N); copy_own(M.dz2, sv + V.dz2, N);
                    copy_own(M.lm, sv + V.lm, N);
                    relaxed_iters = -1;
                    __syncthreads();
                }
                if (halve) {
                    step *= BETA;
                    if (++halvings == GPB_MAX_HALVINGS) { gaveup = true; break; }
                }
            }
        }
        if (gaveup) { code = GPB_LINESEARCH; break; }

        // ---- the step, the scaling update (misc.py:444-464), s and z of the next iteration (cvxprog.py:1264-1355)
        if (tid < ne) M.x[tid] += step * M.dx[tid];
        if (tid < p) M.y[tid] += step * M.dy[tid];
        (void)orth_update(N, step, M.ds, M.dz, M.d, M.di, M.lm, M.s, M.z);       // the gap is s'z at the top of the loop
        __syncthreads();
    }

    // ---- the member's result (cvxprog.py:729-755); after a first factorisation that failed: zeros
    const bool rank = code == GPB_RANK;
    double mx[2] = {-INFINITY, -INFINITY};
    for (int k = tid; k < N; k += NT) {
        const double sk = M.s[k], zk = M.z[k];
        so[k] = rank ? 0.0 : sk; zo[k] = rank ? 0.0 : zk;
        mx[0] = fmax(mx[0], -sk); mx[1] = fmax(mx[1], -zk);
    }
    if (tid < nx) xo[tid] = rank ? 0.0 : M.x[tid];
    if (tid < p) yo[tid] = rank ? 0.0 : M.y[tid];
    blk_reduce<2, true>(mx, M.red);
    if (tid == 0) {
        const double out[GPB_NSTAT] = {gap, relgap, pcost, dcost, pres, dres, -mx[0], -mx[1]};
#pragma unroll
        for (int k = 0; k < GPB_NSTAT; k++) st[k] = rank ? NAN : out[k];
        a.iters[bm] = rank ? 0 : iters;
        a.exitc[bm] = code;
    }
}

}  // namespace

size_t gp_batch_lds_bytes(int n, int m, int l, int ml, int p) { return (size_t)layout(n, m, l, ml, p).total * sizeof(double); }

int64_t gp_batch_scratch_doubles(int n, int m, int ml, int p) { return saved(n, m, ml, p).total; }

hipError_t launch_gp_batch(hipStream_t st, const GpBatchArgs &a)
{
    // per device, so asked of the current one at every launch
    const hipError_t e = hipFuncSetAttribute((const void *)k_gp_batch, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    k_gp_batch<<<dim3((unsigned)a.B), dim3(GPB_THREADS), gp_batch_lds_bytes(a.n, a.m, a.l, a.ml, a.p), st>>>(a);
    return hipGetLastError();
}

}  // namespace kvx
