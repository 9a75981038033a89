// conelp_member: one workgroup carries one member of a batch of small dense cone programs
//
//     minimize c'x   subject to   G x + s = h,  s in K,  A x = b
//
// from its starting point to its status or its infeasibility certificate.  It is the device restatement of _ipm.conelp_start /
// _ipm.conelp_loop with refinement 0: coneprog.py:662-842 (start with W = I, the two pushes, the optimal-at-iteration-0 return),
// 861-1024 (residuals, the three stopping tests and their scalings), 1031-1190 (scaling, the constant system, f6_no_ir),
// 1248-1333 (the two directions), 1336-1436 (step and scaling update), with the Newton solve of batch_kkt.hpp.  It is written
// once and instantiated by k_lp_batch (K = R^ml_+), k_socp_batch (K = R^ml_+ x Q x ...) and k_sdp_batch (K = R^ml_+ x S_+ x ...).
//
// The loop reaches the cone only through a policy `Cone`, the device twin of cone.py::_ConeEngine.  C.M is the member
// (a ConelpMem); a vector of the cone has M.N entries.  Unless said otherwise an operation starts after a barrier of the caller
// and ends with one.
//
//   lmbda_len()                  the length of lmbda, for mu
//   for_rows(f)                  f(row) for the rows this thread adds: row.k the entry, row.w(v) v with the row's weight in the
//                                cone's inner product, row.put(vec, v) vec[k] := v, and its mirror image.  No barrier.
//   load_h(out)                  out := h as a vector of the cone.  No barrier.
//   start()                      W := I, s := h, z := 0
//   max_step(u0, a0, u1, a1, mx) mx[0], mx[1] := the larger of themselves and max_step of a0 u0 and a1 u1, in every thread
//   push(ps, pz, mx)             s += (1 + mx[0]) e if ps, z += (1 + mx[1]) e if pz.  No barrier.
//   first_scaling()              W and lmbda from s and z; false when it fails.  No barrier at the end.
//   lam_sq()                     lmbda'lmbda
//   prepare(), assemble(sing)    what the factorisation needs of W (W^-T h), then the lower triangle of S = Gs'Gs [+ A'A]
//   kkt_before(vx, vz)           vz := W^-T vz, vx += G'W^-1 vz
//   kkt_after(vx, vz)            vz := W^-T G vx - vz
//   gemv_t(u, sign, v)           v += sign G'u.  No barrier.
//   rhs(i, sigma, mu)            ds := -(lmbda o\ (lmbda o lmbda [+ ws3 - sigma mu e])), dz := -((1 - sigma) rz + W'ds);
//                                no barrier at the end
//   th_dot(dz)                   the thread's part of (W^-T h)'dz.  No barrier.
//   combine(i, dtau, mx)         dz += dtau z1, ds -= dz, ws3 := ds o dz after the predictor (i = 0), both scaled by lmbda; mx as
//                                in max_step
//   update(step)                 the scaling update, s = W'lmbda and z = W^-1 lmbda of the next iteration.  No barrier at the end.
//
// Where two kernels form a quantity by different floating-point expressions, the policy keeps the difference: a member's bytes
// are those of the kernel that owns it.  The orthant operations below are the 'l' rows of all three policies.
//
// The scalars tau, kappa, dg, lmbda_g, dtau, dkappa, sigma, step are computed by every thread from the same reduced values, so
// every branch around a barrier is workgroup-uniform.  Sums have the fixed order of batch_device.hpp: a member's bytes depend on
// nothing but its own data.  Every loop is bounded by maxiters or by the member's dimensions.  A NaN or Inf never passes a pivot
// test and makes every comparison of the stopping tests false, so such a member ends with exit 3, 2 or 1.
#pragma once
#include "batch_host.hpp"
#include "batch_kkt.hpp"

namespace kvx {
namespace batchdev {

// What a member ends with: the `exit` of kvxopt_amd.lpbatch, socpbatch and sdpbatch.
enum { CONELP_OPTIMAL = 0, CONELP_MAXITERS = 1, CONELP_SINGULAR = 2, CONELP_RANK = 3, CONELP_PRIMAL_INFEASIBLE = 4,
       CONELP_DUAL_INFEASIBLE = 5 };
constexpr int CONELP_NSTAT = 10;

struct ConelpMem : KktMem {                   // what the loop itself reads and writes of a member: data in HBM, vectors in LDS
    int N;
    const double *c, *G, *h, *b;
    double *x, *dx, *rx, *x1, *y, *dy, *ry, *y1, *s, *z, *ds, *dz, *rz, *ws3, *z1, *red;
};

// The member's data of the batch `a`; N: the rows of G and h.
__device__ __forceinline__ void conelp_data(ConelpMem &M, const BatchArgs &a, int N)
{
    const int64_t bm = blockIdx.x;
    M.n = a.n; M.p = a.p; M.N = N;
    M.c = a.c + bm * a.sc; M.G = a.G + bm * a.sG; M.h = a.h + bm * a.sh;
    M.A = a.p ? a.A + bm * a.sA : nullptr; M.b = a.p ? a.b + bm * a.sb : nullptr;
}

// ---- rows that stand for themselves with weight 1 ('l' and 'q'), and the sum of squares of an LDS vector

struct PlainRow {
    int k;
    __device__ __forceinline__ double w(double v) const { return v; }
    __device__ __forceinline__ void put(double *vec, double v) const { vec[k] = v; }
};

template <class F>
__device__ __forceinline__ void plain_rows(int N, F f)
{
    for (int k = threadIdx.x; k < N; k += NT) f(PlainRow{k});
}

__device__ __forceinline__ double sum_sq(const double *v, int len, double *red)
{
    double g[1] = {0.0};
    for (int k = threadIdx.x; k < len; k += NT) g[0] += v[k] * v[k];
    blk_reduce<1, false>(g, red);
    return g[0];
}

// ---- the orthant: the 'l' rows 0 .. ml of a cone.  None of these has a barrier.

__device__ __forceinline__ void orth_max_step(int ml, const double *u0, double a0, const double *u1, double a1, double (&mx)[2])
{
    for (int k = threadIdx.x; k < ml; k += NT) {
        const double sk = a0 * u0[k], zk = a1 * u1[k];
        mx[0] = fmax(mx[0], -sk); mx[1] = fmax(mx[1], -zk);
    }
}

__device__ __forceinline__ void orth_push(int ml, bool ps, bool pz, const double (&mx)[2], double *s, double *z)
{
    for (int k = threadIdx.x; k < ml; k += NT) {
        if (ps) s[k] += 1.0 + mx[0];
        if (pz) z[k] += 1.0 + mx[1];
    }
}

// DZ: also dz, in one expression with d ds; a cone that scales ds as a whole forms dz itself
template <bool DZ>
__device__ __forceinline__ void orth_rhs(int ml, int i, double sigma, double mu, const double *lm, const double *ws3, const double *d,
                                         const double *rz, double *ds, double *dz)
{
    for (int k = threadIdx.x; k < ml; k += NT) {
        const double lk = lm[k];
        double t = lk * lk;
        if (i == 1) t += ws3[k] - sigma * mu;
        t = -t / lk;
        ds[k] = t;
        if (DZ) dz[k] = -((1.0 - sigma) * rz[k] + d[k] * t);
    }
}

__device__ __forceinline__ void orth_combine(int ml, int i, double dtau, const double *lm, const double *z1, double *ds, double *dz,
                                             double *ws3, double (&mx)[2])
{
    for (int k = threadIdx.x; k < ml; k += NT) {
        const double lk = lm[k], zk = dz[k] + dtau * z1[k], sk = ds[k] - zk;
        if (i == 0) ws3[k] = sk * zk;
        const double s2 = sk / lk, z2 = zk / lk;
        ds[k] = s2; dz[k] = z2;
        mx[0] = fmax(mx[0], -s2); mx[1] = fmax(mx[1], -z2);
    }
}

// ---- the loop

template <class Cone>
__device__ __forceinline__ bool conelp_factor(const Cone &C, bool &sing, bool first)
{
    C.prepare();
    return kkt_factor(C.M, sing, first, [&](bool sg) { C.assemble(sg); });
}

// misc.py:1489-1563 on the LDS vectors (vx, vy, vz) = (bx, by, bz): on return ux, uy, W uz
template <class Cone>
__device__ __forceinline__ void conelp_kkt_solve(const Cone &C, bool sing, double *vx, double *vy, double *vz)
{
    C.kkt_before(vx, vz);
    kkt_reduced_solve(C.M, sing, vx, vy);
    C.kkt_after(vx, vz);
}

// coneprog.py:861-896: rx = hrx - tau c with hrx = -A'y - G'z, ry = hry - tau b with hry = A x, rz = hrz - tau h with
// hrz = s + G x, left in M.rx, M.ry, M.rz.  r: the squared norms of hrx, rx, hry, ry, hrz, rz, then c'x, b'y, h'z.
template <class Cone>
__device__ __forceinline__ void conelp_residuals(const Cone &C, double tau, double (&r)[9])
{
    const auto &M = C.M;
    const int tid = threadIdx.x, n = M.n, p = M.p;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
    if (tid < n) M.rx[tid] = 0.0;
    if (tid < p) {
        const double t = row_dot(M.A, p, n, tid, M.x), bk = M.b[tid], u = t - tau * bk;
        M.ry[tid] = u;
        v[2] = t * t; v[3] = u * u;
        w[1] = bk * M.y[tid];
    }
    C.for_rows([&](auto row) {
        const int k = row.k;
        const double t = row_dot(M.G, M.N, n, k, M.x) + M.s[k], hk = M.h[k], u = t - tau * hk;
        row.put(M.rz, u);
        v[4] += row.w(t * t); v[5] += row.w(u * u);
        w[2] += row.w(hk * M.z[k]);
    });
    __syncthreads();
    if (p > 0) gemv_t_add(M.A, p, n, M.y, nullptr, -1.0, M.rx);
    __syncthreads();
    C.gemv_t(M.z, -1.0, M.rx);
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

// The member blockIdx.x of the batch `a`, whose cone is C and whose data and LDS vectors are bound in C.M.  Barrier before: the
// caller's, after it has set up the cone.
template <class Cone>
__device__ __forceinline__ void conelp_member(const Cone &C, const BatchArgs &a)
{
    const auto &M = C.M;
    const int tid = threadIdx.x, n = M.n, N = M.N, p = M.p;
    const int64_t bm = blockIdx.x;
    double *xo = a.x + bm * n, *yo = p ? a.y + bm * p : nullptr, *so = a.s + bm * N, *zo = a.z + bm * N, *st = a.stats + bm * CONELP_NSTAT;

    int code = CONELP_RANK, iters = 0;                     // the solver's ValueError("Rank(A) < p or Rank([G; A]) < n")
    bool sing = false, at0 = false;
    double tau = 1.0, kappa = 1.0, dg = 1.0, dgi = 1.0, lg = 1.0, gap = NAN, lam2 = 0.0;
    double relgap = NAN, pcost = NAN, dcost = NAN, pres = NAN, dres = NAN, pinfres = NAN, dinfres = NAN;
    double sp = 0.0, sd = 0.0;                             // what x, s and y, z are scaled by at the end; NaN: not returned
    double resx0 = 1.0, resy0 = 1.0, resz0 = 1.0;

    // ---- starting point (coneprog.py:662-842): W = I; [0 A' G'; A 0 0; G 0 -I] [x; .; -s] = [0; b; h] and
    //      [0 A' G'; A 0 0; G 0 -I] [.; y; z] = [-c; 0; 0]
    if (tid < n) { M.x[tid] = 0.0; M.dx[tid] = -M.c[tid]; }
    if (tid < p) { M.dy[tid] = M.b[tid]; M.y[tid] = 0.0; }
    C.start();
    bool run = conelp_factor(C, sing, true);
    if (run) {
        conelp_kkt_solve(C, sing, M.x, M.dy, M.s);
        conelp_kkt_solve(C, sing, M.dx, M.y, M.z);
        double mx[2] = {-INFINITY, -INFINITY}, nr[4] = {0.0, 0.0, 0.0, 0.0}, r0[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (tid < n) { const double ck = M.c[tid]; r0[0] = ck * ck; r0[3] = ck * M.x[tid]; }
        if (tid < p) { const double bk = M.b[tid]; r0[1] = bk * bk; r0[4] = bk * M.y[tid]; }
        for (int k = tid; k < N; k += NT) M.s[k] = -M.s[k];
        __syncthreads();
        C.for_rows([&](auto row) {
            const int k = row.k;
            const double sk = M.s[k], zk = M.z[k], hk = M.h[k];
            nr[0] += row.w(sk * sk); nr[1] += row.w(zk * zk); nr[2] += row.w(sk * zk); nr[3] += row.w(hk * zk);
            r0[2] += row.w(hk * hk);
        });
        blk_reduce<4, false>(nr, M.red);
        blk_reduce<5, false>(r0, M.red);
        C.max_step(M.s, 1.0, M.z, 1.0, mx);
        resx0 = fmax(1.0, sqrt(r0[0])); resy0 = fmax(1.0, sqrt(r0[1])); resz0 = fmax(1.0, sqrt(r0[2]));
        gap = nr[2];
        {
            const double pc = r0[3], dc = -r0[4] - nr[3];
            const double rg = pc < 0.0 ? gap / -pc : (dc > 0.0 ? gap / dc : NAN);
            at0 = mx[0] <= 0.0 && mx[1] <= 0.0 && (gap <= a.abstol || rg <= a.reltol);
        }
        if (!at0) {                                        // both pushes into the cone (coneprog.py:806-842): along e
            const bool ps = mx[0] >= -1e-8 * fmax(sqrt(nr[0]), 1.0), pz = mx[1] >= -1e-8 * fmax(sqrt(nr[1]), 1.0);
            C.push(ps, pz, mx);
            __syncthreads();
            double g[1] = {0.0};
            C.for_rows([&](auto row) { g[0] += row.w(M.s[row.k] * M.z[row.k]); });
            blk_reduce<1, false>(g, M.red);
            gap = g[0];
        }
        __syncthreads();
    }

    for (; run; iters++) {
        // ---- residuals, objectives and the three stopping tests (coneprog.py:861-1024)
        double r[9];
        conelp_residuals(C, tau, r);
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
        if (at0) { code = CONELP_OPTIMAL; pinfres = dinfres = NAN; sp = sd = 1.0; break; }    // coneprog.py:757-804: as they are
        if (iters == a.maxiters) { code = CONELP_MAXITERS; sp = sd = 1.0 / tau; break; }
        if (pres <= a.feastol && dres <= a.feastol && (gap <= a.abstol || relgap <= a.reltol)) {
            code = CONELP_OPTIMAL; pinfres = dinfres = NAN; sp = sd = 1.0 / tau; break;
        }
        if (pinfres <= a.feastol) { code = CONELP_PRIMAL_INFEASIBLE; sp = NAN; sd = 1.0 / (-hz - by); break; }
        if (dinfres <= a.feastol) { code = CONELP_DUAL_INFEASIBLE; sp = 1.0 / (-cx); sd = NAN; break; }

        // ---- scaling of the first iteration (misc.compute_scaling, coneprog.py:1041-1043)
        if (iters == 0) {
            if (!C.first_scaling()) { code = CONELP_RANK; break; }   // lapack.potrf's ArithmeticError in misc.compute_scaling
            __syncthreads();
            lam2 = C.lam_sq();
            dg = sqrt(kappa / tau); dgi = sqrt(tau / kappa); lg = sqrt(tau * kappa);
        }
        __syncthreads();

        // ---- the factorisation and the constant system (coneprog.py:1066-1077): (x1, y1, z1) = dgi f3(-c, b, h)
        if (!conelp_factor(C, sing, false)) {
            if (iters == 0) code = CONELP_RANK;
            else { code = CONELP_SINGULAR; sp = sd = 1.0 / tau; }
            break;
        }
        C.load_h(M.z1);
        if (tid < n) M.x1[tid] = -M.c[tid];
        if (tid < p) M.y1[tid] = M.b[tid];
        __syncthreads();
        conelp_kkt_solve(C, sing, M.x1, M.y1, M.z1);
        double z1z1;
        {
            double g[1] = {0.0};
            for (int k = tid; k < N; k += NT) M.z1[k] *= dgi;
            if (tid < n) M.x1[tid] *= dgi;
            if (tid < p) M.y1[tid] *= dgi;
            __syncthreads();
            C.for_rows([&](auto row) { const double t = M.z1[row.k]; g[0] += row.w(t * t); });
            blk_reduce<1, false>(g, M.red);
            z1z1 = g[0];
        }

        // ---- the two directions (coneprog.py:1248-1333) through f6_no_ir (:1130-1195)
        const double mu = (lam2 + lg * lg) / (1 + C.lmbda_len());    // coneprog.py:1248: 1 + cdim_diag
        double sigma = 0.0, wkappa3 = 0.0, step = 0.0, tt = 0.0, tk = 0.0;
        for (int i = 0; i < 2; i++) {
            C.rhs(i, sigma, mu);
            if (tid < n) M.dx[tid] = (1.0 - sigma) * M.rx[tid];
            if (tid < p) M.dy[tid] = -((1.0 - sigma) * M.ry[tid]);
            double dkappa = lg * lg;
            if (i == 1) dkappa += wkappa3 - sigma * mu;
            __syncthreads();
            conelp_kkt_solve(C, sing, M.dx, M.dy, M.dz);
            dkappa = -dkappa / lg;
            double dot[3] = {0.0, 0.0, 0.0};               // c'dx, b'dy, th'dz with th = W^-T h
            if (tid < n) dot[0] = M.c[tid] * M.dx[tid];
            if (tid < p) dot[1] = M.b[tid] * M.dy[tid];
            dot[2] = C.th_dot(M.dz);
            blk_reduce<3, false>(dot, M.red);
            const double dtau = dgi * ((1.0 - sigma) * rt + dkappa / dgi + dot[0] + dot[1] + dot[2]) / (1.0 + z1z1);
            if (tid < n) M.dx[tid] += dtau * M.x1[tid];
            if (tid < p) M.dy[tid] += dtau * M.y1[tid];
            double mx[2] = {-INFINITY, -INFINITY};
            C.combine(i, dtau, mx);
            dkappa -= dtau;
            if (i == 0) wkappa3 = dtau * dkappa;
            tt = -dtau / lg; tk = -dkappa / lg;
            const double t = fmax(fmax(0.0, fmax(mx[0], mx[1])), fmax(tt, tk));
            step = t == 0.0 ? 1.0 : (i == 0 ? fmin(1.0, 1.0 / t) : fmin(1.0, 0.99 / t));
            if (i == 0) { const double u = 1.0 - step; sigma = u * u * u; }
        }

        // ---- the step, the scaling update (misc.update_scaling, coneprog.py:1336-1436), s and z of the next iteration
        dg *= sqrt(1.0 - step * tk) / sqrt(1.0 - step * tt);
        dgi = 1.0 / dg;
        lg *= sqrt(1.0 - step * tt) * sqrt(1.0 - step * tk);
        kappa = lg / dgi; tau = lg * dgi;
        if (tid < n) M.x[tid] += step * M.dx[tid];
        if (tid < p) M.y[tid] += step * M.dy[tid];
        C.update(step);
        __syncthreads();
        lam2 = C.lam_sq();                                 // its barriers also publish x, y, s, z
    }

    // ---- the member's result: x, s scaled by sp and y, z by sd (coneprog.py:925-1024, 1082-1109); NaN for the half a certificate
    //      comes without; after a first factorisation that failed: zeros.  The slacks are -max_step of the scaled s and z.
    const bool rank = code == CONELP_RANK, xs = sp == sp, zs = sd == sd;
    double mx[2] = {-INFINITY, -INFINITY};
    __syncthreads();
    for (int k = tid; k < N; k += NT) {
        const double sk = sp * M.s[k], zk = sd * M.z[k];
        so[k] = rank ? 0.0 : (xs ? sk : NAN); zo[k] = rank ? 0.0 : (zs ? zk : NAN);
    }
    if (tid < n) xo[tid] = rank ? 0.0 : (xs ? sp * M.x[tid] : NAN);
    if (tid < p) yo[tid] = rank ? 0.0 : (zs ? sd * M.y[tid] : NAN);
    if (!rank) C.max_step(M.s, sp, M.z, sd, mx);
    if (tid == 0) {
        const bool pinf = code == CONELP_PRIMAL_INFEASIBLE, dinf = code == CONELP_DUAL_INFEASIBLE, cert = pinf || dinf;
        const double out[CONELP_NSTAT] = {cert ? NAN : gap, cert ? NAN : relgap, pinf ? NAN : (dinf ? -1.0 : pcost),
                                          dinf ? NAN : (pinf ? 1.0 : dcost), cert ? NAN : pres, cert ? NAN : dres,
                                          xs ? -mx[0] : NAN, zs ? -mx[1] : NAN, dinf ? NAN : pinfres, pinf ? NAN : dinfres};
#pragma unroll
        for (int k = 0; k < CONELP_NSTAT; k++) st[k] = rank ? NAN : out[k];
        a.iters[bm] = rank ? 0 : iters;
        a.exitc[bm] = code;
    }
}

}  // namespace batchdev
}  // namespace kvx
