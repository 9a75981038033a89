// k_lp_batch: one workgroup (256 threads, four wavefronts) carries one small dense LP from its starting point to its status or
// its infeasibility certificate (lp_batch.hpp).  It is a device restatement of _ipm.conelp_start / _ipm.conelp_loop on the
// orthant with refinement 0: coneprog.py:662-842 (start with W = I, the two pushes, the optimal-at-iteration-0 return), 861-1024
// (residuals, the three stopping tests and their scalings), 1031-1190 (scaling, the constant system, f6_no_ir), 1248-1333 (the
// two directions), 1336-1436 (step and scaling update, misc.py:444-464), and the Newton solve of misc.kkt_chol2
// (misc.py:1395-1563) with dense Cholesky factors of S = G' diag(di^2) G and, for p > 0, of K = X'X with X = L^-1 A'.  When the
// first factorisation of S (the one with W = I) fails and p > 0, S := S + A'A from then on and every solve adds A'by to bx
// (F['singular'], misc.py:1433-1458, 1526-1527); the flag belongs to the member.
//
// Everything a member iterates on lives in LDS, laid out as in qp_batch.hip: S, its factor in place, X and K (their region holds
// the staged rows of diag(di) G while S is assembled), four n-vectors (x, dx, rx, x1), four p-vectors and ten ml-vectors
// (s, z, d, di, lmbda, ds, dz, rz, ws3, z1); th = W^-T h is recomputed as di h where it is used.  c, G, h, A, b are read from
// HBM / L2.  The scalars tau, kappa, dg, lmbda_g, dtau, dkappa, sigma, step are computed by every thread from the same reduced
// values, so every branch around a barrier is workgroup-uniform.  Sums have the fixed order of batch_device.hpp: a member's
// bytes depend on nothing but its own data.  No atomics, no communication between workgroups.  Every loop is bounded by
// maxiters, n, ml or p.  A NaN or Inf never passes a pivot test and makes every comparison of the stopping tests false, so such
// a member ends with exit 3, 2 or 1.
#include "lp_batch.hpp"
#include "batch_device.hpp"

#include <cmath>

namespace kvx {
namespace {

using namespace batchdev;
static_assert(NT == LPB_THREADS, "the shared helpers are written for the workgroup of k_lp_batch");

struct Layout {                               // offsets in doubles from the LDS base; every part starts on 16 bytes
    int ldn, ldp;
    int S, XK, X, K, x, dx, rx, x1, y, dy, ry, y1, s, z, d, di, lm, ds, dz, rz, ws3, z1, red, total;
};

__host__ __device__ inline Layout layout(int n, int ml, int p)
{
    Layout L;
    L.ldn = n | 1;
    L.ldp = p | 1;
    int o = 0;
    L.S = o; o += even(n * L.ldn);
    const int xsz = even(p * L.ldn), ksz = even(p * L.ldp), tsz = even(LPB_TILE * L.ldn);
    L.XK = L.X = o; L.K = o + xsz; o += (xsz + ksz > tsz ? xsz + ksz : tsz);
    const int nv = even(n), pv = even(p), mv = even(ml);
    L.x = o; o += nv; L.dx = o; o += nv; L.rx = o; o += nv; L.x1 = o; o += nv;
    L.y = o; o += pv; L.dy = o; o += pv; L.ry = o; o += pv; L.y1 = o; o += pv;
    L.s = o; o += mv; L.z = o; o += mv; L.d = o; o += mv; L.di = o; o += mv; L.lm = o; o += mv;
    L.ds = o; o += mv; L.dz = o; o += mv; L.rz = o; o += mv; L.ws3 = o; o += mv; L.z1 = o; o += mv;
    L.red = o; o += NW * NRED;
    L.total = o;
    return L;
}

struct Member {                               // one member's data in HBM and its vectors and matrices in LDS
    int n, ml, p, ldn, ldp;
    const double *c, *G, *h, *A, *b;
    double *S, *T, *X, *K, *x, *dx, *rx, *x1, *y, *dy, *ry, *y1, *s, *z, *d, *di, *lm, *ds, *dz, *rz, *ws3, *z1, *red;
};

// The lower triangle of S = G' diag(di^2) G [+ A'A] in LDS.  Barriers before (the caller's) and after.
__device__ void assemble(const Member &M, bool sing)
{
    const int tid = threadIdx.x, n = M.n, ml = M.ml, p = M.p, ldn = M.ldn;
    const int cnt = tri_count(n);
    for (int e = tid; e < cnt; e += NT) {
        int i, j;
        if (!tri_map(e, n, i, j)) continue;
        double acc = 0.0;
        if (sing)
            for (int a = 0; a < p; a++) acc += M.A[a + (int64_t)i * p] * M.A[a + (int64_t)j * p];
        M.S[i + j * ldn] = acc;
    }
    for (int k0 = 0; k0 < ml; k0 += LPB_TILE) {
        const int kt = min((int)LPB_TILE, ml - k0);
        __syncthreads();                                   // the staged rows of the previous step have been read
        for (int e = tid; e < LPB_TILE * n; e += NT) {
            const int kk = e & (LPB_TILE - 1), c = e / LPB_TILE;
            if (kk < kt) M.T[kk * ldn + c] = M.di[k0 + kk] * M.G[k0 + kk + (int64_t)c * ml];
        }
        __syncthreads();
        for (int e = tid; e < cnt; e += NT) {
            int i, j;
            if (!tri_map(e, n, i, j)) continue;
            double acc = 0.0;
            for (int kk = 0; kk < kt; kk++) acc += M.T[kk * ldn + i] * M.T[kk * ldn + j];
            M.S[i + j * ldn] += acc;
        }
    }
    __syncthreads();
}

// The KKT factorisation in the scaling di (misc.py:1395-1487): S, its factor L in place, and for p > 0 X = L^-1 A', K = X'X and
// its factor.  first: the member's first factorisation, where a failed factor of S with p > 0 sets `sing` and is repeated on
// S + A'A.  false on a failed pivot.  Barriers before (the caller's) and after.
__device__ bool factor(const Member &M, bool &sing, bool first)
{
    const int tid = threadIdx.x, n = M.n, p = M.p, ldn = M.ldn, ldp = M.ldp;
    assemble(M, sing);
    if (!chol_lds(M.S, ldn, n)) {
        if (!first || p == 0) return false;
        sing = true;
        __syncthreads();                                   // every thread has read the failed pivot
        assemble(M, true);
        if (!chol_lds(M.S, ldn, n)) return false;
    }
    if (p == 0) return true;
    const int lane = tid & 63, w = tid >> 6;
    for (int a = w; a < p; a += NW) {                      // the staged rows are dead: X may take their place
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

// misc.py:1489-1563 on the LDS vectors (vx, vy, vz) = (bx, by, bz): on return ux, uy, W uz.  Barriers before (the caller's)
// and after.
__device__ void kkt_solve(const Member &M, bool sing, double *vx, double *vy, double *vz)
{
    const int tid = threadIdx.x, n = M.n, ml = M.ml, p = M.p, lane = tid & 63, w = tid >> 6;
    for (int k = tid; k < ml; k += NT) vz[k] *= M.di[k];                                   // z := W^-T bz
    __syncthreads();
    gemv_t_add(M.G, ml, n, vz, M.di, 1.0, vx);                                             // x += G' W^-1 z
    __syncthreads();
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
    for (int k = tid; k < ml; k += NT) vz[k] = M.di[k] * row_dot(M.G, ml, n, k, vx) - vz[k];   // W uz = W^-T (G ux - bz)
    __syncthreads();
}

// coneprog.py:861-896: rx = hrx - tau c with hrx = -A'y - G'z, ry = hry - tau b with hry = A x, rz = hrz - tau h with
// hrz = s + G x, left in M.rx, M.ry, M.rz.  r: the squared norms of hrx, rx, hry, ry, hrz, rz, then c'x, b'y, h'z.  Barriers
// before (the caller's) and after.
__device__ void residuals(const Member &M, double tau, double (&r)[9])
{
    const int tid = threadIdx.x, n = M.n, ml = M.ml, p = M.p;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
    if (tid < n) M.rx[tid] = 0.0;
    if (tid < p) {
        const double t = row_dot(M.A, p, n, tid, M.x), bk = M.b[tid], u = t - tau * bk;
        M.ry[tid] = u;
        v[2] = t * t; v[3] = u * u;
        w[1] = bk * M.y[tid];
    }
    for (int k = tid; k < ml; k += NT) {
        const double t = row_dot(M.G, ml, n, k, M.x) + M.s[k], hk = M.h[k], u = t - tau * hk;
        M.rz[k] = u;
        v[4] += t * t; v[5] += u * u;
        w[2] += hk * M.z[k];
    }
    __syncthreads();
    if (p > 0) gemv_t_add(M.A, p, n, M.y, nullptr, -1.0, M.rx);
    __syncthreads();
    gemv_t_add(M.G, ml, n, M.z, nullptr, -1.0, M.rx);
    __syncthreads();
    if (tid < n) {
        const double t = M.rx[tid], ck = M.c[tid], u = t - tau * ck;
        M.rx[tid] = u;
        v[0] = t * t; v[1] = u * u;
        w[0] = ck * M.x[tid];
    }
    blk_reduce<6, false>(v, M.red);
    blk_reduce<3, false>(w, M.red);                        // its barriers also publish rx
#pragma unroll
    for (int k = 0; k < 6; k++) r[k] = v[k];
#pragma unroll
    for (int k = 0; k < 3; k++) r[6 + k] = w[k];
}

__global__ void __launch_bounds__(LPB_THREADS) k_lp_batch(LpBatchArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, n = a.n, ml = a.ml, p = a.p;
    const int64_t bm = blockIdx.x;
    const Layout L = layout(n, ml, p);
    Member M;
    M.n = n; M.ml = ml; M.p = p; M.ldn = L.ldn; M.ldp = L.ldp;
    M.c = a.c + bm * a.sc; M.G = a.G + bm * a.sG; M.h = a.h + bm * a.sh;
    M.A = p ? a.A + bm * a.sA : nullptr; M.b = p ? a.b + bm * a.sb : nullptr;
    M.S = lds + L.S; M.T = lds + L.XK; M.X = lds + L.X; M.K = lds + L.K;
    M.x = lds + L.x; M.dx = lds + L.dx; M.rx = lds + L.rx; M.x1 = lds + L.x1;
    M.y = lds + L.y; M.dy = lds + L.dy; M.ry = lds + L.ry; M.y1 = lds + L.y1;
    M.s = lds + L.s; M.z = lds + L.z; M.d = lds + L.d; M.di = lds + L.di; M.lm = lds + L.lm; M.ds = lds + L.ds; M.dz = lds + L.dz;
    M.rz = lds + L.rz; M.ws3 = lds + L.ws3; M.z1 = lds + L.z1; M.red = lds + L.red;
    double *xo = a.x + bm * n, *yo = p ? a.y + bm * p : nullptr, *so = a.s + bm * ml, *zo = a.z + bm * ml, *st = a.stats + bm * LPB_NSTAT;

    int code = LPB_RANK, iters = 0;                        // solvers.lp: ValueError("Rank(A) < p or Rank([G; A]) < n")
    bool sing = false, at0 = false;
    double tau = 1.0, kappa = 1.0, dg = 1.0, dgi = 1.0, lg = 1.0, gap = NAN, lam2 = 0.0;
    double relgap = NAN, pcost = NAN, dcost = NAN, pres = NAN, dres = NAN, pinfres = NAN, dinfres = NAN;
    double sp = 0.0, sd = 0.0;                             // what x, s and y, z are scaled by at the end; NaN: not returned
    double resx0 = 1.0, resy0 = 1.0, resz0 = 1.0;

    // ---- starting point (coneprog.py:662-842): W = I; [0 A' G'; A 0 0; G 0 -I] [x; .; -s] = [0; b; h] and
    //      [0 A' G'; A 0 0; G 0 -I] [.; y; z] = [-c; 0; 0]
    for (int k = tid; k < ml; k += NT) { M.d[k] = 1.0; M.di[k] = 1.0; M.s[k] = M.h[k]; M.z[k] = 0.0; }
    if (tid < n) { M.x[tid] = 0.0; M.dx[tid] = -M.c[tid]; }
    if (tid < p) { M.dy[tid] = M.b[tid]; M.y[tid] = 0.0; }
    __syncthreads();
    bool run = factor(M, sing, true);
    if (run) {
        kkt_solve(M, sing, M.x, M.dy, M.s);
        kkt_solve(M, sing, M.dx, M.y, M.z);
        double mx[2] = {-INFINITY, -INFINITY}, nr[4] = {0.0, 0.0, 0.0, 0.0}, r0[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (tid < n) { const double ck = M.c[tid]; r0[0] = ck * ck; r0[3] = ck * M.x[tid]; }
        if (tid < p) { const double bk = M.b[tid]; r0[1] = bk * bk; r0[4] = bk * M.y[tid]; }
        for (int k = tid; k < ml; k += NT) {
            const double sk = -M.s[k], zk = M.z[k], hk = M.h[k];
            M.s[k] = sk;
            mx[0] = fmax(mx[0], -sk); mx[1] = fmax(mx[1], -zk);
            nr[0] += sk * sk; nr[1] += zk * zk; nr[2] += sk * zk; nr[3] += hk * zk;
            r0[2] += hk * hk;
        }
        blk_reduce<2, true>(mx, M.red);
        blk_reduce<4, false>(nr, M.red);
        blk_reduce<5, false>(r0, M.red);
        resx0 = fmax(1.0, sqrt(r0[0])); resy0 = fmax(1.0, sqrt(r0[1])); resz0 = fmax(1.0, sqrt(r0[2]));
        gap = nr[2];
        {
            const double pc = r0[3], dc = -r0[4] - nr[3];
            const double rg = pc < 0.0 ? gap / -pc : (dc > 0.0 ? gap / dc : NAN);
            at0 = mx[0] <= 0.0 && mx[1] <= 0.0 && (gap <= a.abstol || rg <= a.reltol);
        }
        if (!at0) {                                        // both pushes into the cone (coneprog.py:806-842)
            const bool ps = mx[0] >= -1e-8 * fmax(sqrt(nr[0]), 1.0), pz = mx[1] >= -1e-8 * fmax(sqrt(nr[1]), 1.0);
            double g[1] = {0.0};
            for (int k = tid; k < ml; k += NT) {           // each thread shifts the entries it wrote itself
                if (ps) M.s[k] += 1.0 + mx[0];
                if (pz) M.z[k] += 1.0 + mx[1];
                g[0] += M.s[k] * M.z[k];
            }
            blk_reduce<1, false>(g, M.red);
            gap = g[0];
        }
        __syncthreads();
    }

    for (; run; iters++) {
        // ---- residuals, objectives and the three stopping tests (coneprog.py:861-1024)
        double r[9];
        residuals(M, tau, r);
        const double hresx = sqrt(r[0]), resx = sqrt(r[1]) / tau, hresy = sqrt(r[2]), resy = sqrt(r[3]) / tau;
        const double hresz = sqrt(r[4]), resz = sqrt(r[5]) / tau, cx = r[6], by = r[7], hz = r[8];
        if (iters > 0) { const double t = sqrt(lam2) / tau; gap = t * t; }
        const double rt = kappa + cx + by + hz;
        pcost = cx / tau; dcost = -(by + hz) / tau;
        relgap = pcost < 0.0 ? gap / -pcost : (dcost > 0.0 ? gap / dcost : NAN);
        pres = fmax(resy / resy0, resz / resz0);
        dres = resx / resx0;
        pinfres = hz + by < 0.0 ? hresx / resx0 / (-hz - by) : NAN;
        dinfres = cx < 0.0 ? fmax(hresy / resy0, hresz / resz0) / (-cx) : NAN;
        if (at0) { code = LPB_OPTIMAL; pinfres = dinfres = NAN; sp = sd = 1.0; break; }       // coneprog.py:757-804: as they are
        if (iters == a.maxiters) { code = LPB_MAXITERS; sp = sd = 1.0 / tau; break; }
        if (pres <= a.feastol && dres <= a.feastol && (gap <= a.abstol || relgap <= a.reltol)) {
            code = LPB_OPTIMAL; pinfres = dinfres = NAN; sp = sd = 1.0 / tau; break;
        }
        if (pinfres <= a.feastol) { code = LPB_PRIMAL_INFEASIBLE; sp = NAN; sd = 1.0 / (-hz - by); break; }
        if (dinfres <= a.feastol) { code = LPB_DUAL_INFEASIBLE; sp = 1.0 / (-cx); sd = NAN; break; }

        // ---- scaling of the first iteration (misc.py:284-287, coneprog.py:1041-1043)
        if (iters == 0) {
            double g[1] = {0.0};
            for (int k = tid; k < ml; k += NT) {
                const double sk = M.s[k], zk = M.z[k], dk = sqrt(sk / zk), lk = sqrt(sk * zk);
                M.d[k] = dk; M.di[k] = 1.0 / dk; M.lm[k] = lk;
                g[0] += lk * lk;
            }
            blk_reduce<1, false>(g, M.red);
            lam2 = g[0];
            dg = sqrt(kappa / tau); dgi = sqrt(tau / kappa); lg = sqrt(tau * kappa);
        }
        __syncthreads();

        // ---- the factorisation and the constant system (coneprog.py:1066-1077): (x1, y1, z1) = dgi f3(-c, b, h)
        if (!factor(M, sing, false)) {
            if (iters == 0) code = LPB_RANK;
            else { code = LPB_SINGULAR; sp = sd = 1.0 / tau; }
            break;
        }
        for (int k = tid; k < ml; k += NT) M.z1[k] = M.h[k];
        if (tid < n) M.x1[tid] = -M.c[tid];
        if (tid < p) M.y1[tid] = M.b[tid];
        __syncthreads();
        kkt_solve(M, sing, M.x1, M.y1, M.z1);
        double z1z1;
        {
            double g[1] = {0.0};
            for (int k = tid; k < ml; k += NT) { const double t = dgi * M.z1[k]; M.z1[k] = t; g[0] += t * t; }
            if (tid < n) M.x1[tid] *= dgi;
            if (tid < p) M.y1[tid] *= dgi;
            blk_reduce<1, false>(g, M.red);
            z1z1 = g[0];
        }

        // ---- the two directions (coneprog.py:1248-1333) through f6_no_ir (:1130-1195)
        const double mu = (lam2 + lg * lg) / (1 + ml);
        double sigma = 0.0, wkappa3 = 0.0, step = 0.0, tt = 0.0, tk = 0.0;
        for (int i = 0; i < 2; i++) {
            for (int k = tid; k < ml; k += NT) {
                const double lk = M.lm[k];
                double t = lk * lk;
                if (i == 1) t += M.ws3[k] - sigma * mu;
                t = -t / lk;
                M.ds[k] = t;
                M.dz[k] = -((1.0 - sigma) * M.rz[k] + M.d[k] * t);
            }
            if (tid < n) M.dx[tid] = (1.0 - sigma) * M.rx[tid];
            if (tid < p) M.dy[tid] = -((1.0 - sigma) * M.ry[tid]);
            double dkappa = lg * lg;
            if (i == 1) dkappa += wkappa3 - sigma * mu;
            __syncthreads();
            kkt_solve(M, sing, M.dx, M.dy, M.dz);
            dkappa = -dkappa / lg;
            double dot[3] = {0.0, 0.0, 0.0};               // c'dx, b'dy, th'dz with th = W^-T h
            if (tid < n) dot[0] = M.c[tid] * M.dx[tid];
            if (tid < p) dot[1] = M.b[tid] * M.dy[tid];
            for (int k = tid; k < ml; k += NT) dot[2] += M.di[k] * M.h[k] * M.dz[k];
            blk_reduce<3, false>(dot, M.red);
            const double dtau = dgi * ((1.0 - sigma) * rt + dkappa / dgi + dot[0] + dot[1] + dot[2]) / (1.0 + z1z1);
            if (tid < n) M.dx[tid] += dtau * M.x1[tid];
            if (tid < p) M.dy[tid] += dtau * M.y1[tid];
            double mx[2] = {-INFINITY, -INFINITY};
            for (int k = tid; k < ml; k += NT) {
                const double lk = M.lm[k], zk = M.dz[k] + dtau * M.z1[k], sk = M.ds[k] - zk;
                if (i == 0) M.ws3[k] = sk * zk;
                const double s2 = sk / lk, z2 = zk / lk;
                M.ds[k] = s2; M.dz[k] = z2;
                mx[0] = fmax(mx[0], -s2); mx[1] = fmax(mx[1], -z2);
            }
            dkappa -= dtau;
            if (i == 0) wkappa3 = dtau * dkappa;
            blk_reduce<2, true>(mx, M.red);
            tt = -dtau / lg; tk = -dkappa / lg;
            const double t = fmax(fmax(0.0, fmax(mx[0], mx[1])), fmax(tt, tk));
            step = t == 0.0 ? 1.0 : (i == 0 ? fmin(1.0, 1.0 / t) : fmin(1.0, 0.99 / t));
            if (i == 0) { const double u = 1.0 - step; sigma = u * u * u; }
        }

        // ---- the step, the scaling update (misc.py:444-464, coneprog.py:1405-1407), s and z of the next iteration
        dg *= sqrt(1.0 - step * tk) / sqrt(1.0 - step * tt);
        dgi = 1.0 / dg;
        lg *= sqrt(1.0 - step * tt) * sqrt(1.0 - step * tk);
        kappa = lg / dgi; tau = lg * dgi;
        if (tid < n) M.x[tid] += step * M.dx[tid];
        if (tid < p) M.y[tid] += step * M.dy[tid];
        double g[1] = {0.0};
        for (int k = tid; k < ml; k += NT) {
            const double lk = M.lm[k], rs = sqrt((1.0 + step * M.ds[k]) * lk), rz = sqrt((1.0 + step * M.dz[k]) * lk);
            const double dk = M.d[k] * rs / rz, dik = 1.0 / dk, ln = rs * rz;
            M.d[k] = dk; M.di[k] = dik; M.lm[k] = ln;
            M.s[k] = dk * ln; M.z[k] = dik * ln;
            g[0] += ln * ln;
        }
        blk_reduce<1, false>(g, M.red);                    // its barriers also publish x, y, s, z
        lam2 = g[0];
    }

    // ---- the member's result: x, s scaled by sp and y, z by sd (coneprog.py:925-1024, 1082-1109); NaN for the half a certificate
    //      comes without; after a first factorisation that failed: zeros
    const bool rank = code == LPB_RANK, xs = sp == sp, zs = sd == sd;
    double mx[2] = {-INFINITY, -INFINITY};
    for (int k = tid; k < ml; k += NT) {
        const double sk = sp * M.s[k], zk = sd * M.z[k];
        so[k] = rank ? 0.0 : (xs ? sk : NAN); zo[k] = rank ? 0.0 : (zs ? zk : NAN);
        mx[0] = fmax(mx[0], -sk); mx[1] = fmax(mx[1], -zk);
    }
    if (tid < n) xo[tid] = rank ? 0.0 : (xs ? sp * M.x[tid] : NAN);
    if (tid < p) yo[tid] = rank ? 0.0 : (zs ? sd * M.y[tid] : NAN);
    blk_reduce<2, true>(mx, M.red);
    if (tid == 0) {
        const bool pinf = code == LPB_PRIMAL_INFEASIBLE, dinf = code == LPB_DUAL_INFEASIBLE, cert = pinf || dinf;
        const double out[LPB_NSTAT] = {cert ? NAN : gap, cert ? NAN : relgap, pinf ? NAN : (dinf ? -1.0 : pcost),
                                       dinf ? NAN : (pinf ? 1.0 : dcost), cert ? NAN : pres, cert ? NAN : dres,
                                       xs ? -mx[0] : NAN, zs ? -mx[1] : NAN, dinf ? NAN : pinfres, pinf ? NAN : dinfres};
#pragma unroll
        for (int k = 0; k < LPB_NSTAT; k++) st[k] = rank ? NAN : out[k];
        a.iters[bm] = rank ? 0 : iters;
        a.exitc[bm] = code;
    }
}

}  // namespace

size_t lp_batch_lds_bytes(int n, int ml, int p) { return (size_t)layout(n, ml, p).total * sizeof(double); }

hipError_t launch_lp_batch(hipStream_t st, const LpBatchArgs &a)
{
    // per device, so asked of the current one at every launch
    const hipError_t e = hipFuncSetAttribute((const void *)k_lp_batch, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    k_lp_batch<<<dim3((unsigned)a.B), dim3(LPB_THREADS), lp_batch_lds_bytes(a.n, a.ml, a.p), st>>>(a);
    return hipGetLastError();
}

}  // namespace kvx
