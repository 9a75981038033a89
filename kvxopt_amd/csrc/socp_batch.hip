// k_socp_batch: one workgroup (256 threads, four wavefronts) carries one small dense second-order-cone program from its starting
// point to its status or its infeasibility certificate (socp_batch.hpp).  It is k_lp_batch (lp_batch.hip) -- the device
// restatement of _ipm.conelp_start / _ipm.conelp_loop with refinement 0 and the Newton solve of misc.kkt_chol2 -- on the cone
// K = R^ml_+ x Q^{q_0} x ...: the 'l' rows are treated as there, the 'q' rows by the reference's own operations, the ones
// csrc/kkt_q.hip carries as stand-alone kernels: misc.compute_scaling / update_scaling (misc.py:290-352, 467-580), scale, scale2,
// sprod, sinv (misc_solvers.c:144-186, 301-341, 671-700, 803-835) and max_step (misc_solvers.c:1073-1085), strung together as
// cone.py::_ConeEngine strings them (coneprog.py:1130-1195 f6_no_ir, 1248-1333, 1336-1436).
//
// W_k = beta_k (2 v_k v_k' - J) is symmetric, so W^-T = W^-1 = (1 / beta_k)(2 (J v_k)(J v_k)' - J).  S = Gs'Gs with Gs = W^-1 G
// is assembled from staged rows of Gs, 32 at a time: row i of cone k is (2 (J v_k)_i g_k - (J G_k)_i) / beta_k with the row
// vector g_k = (J v_k)'G_k, which is computed once per cone when the tile with the cone's first row is staged and kept, in a
// ring of 33 slots, while later tiles stage the rest of the cone.  (J v_k)'h_k is kept per cone for th = W^-1 h.
//
// LDS: the layout of lp_batch.hip with N = ml + sum q_k rows; v_k lies in the 'q' rows of the slot whose 'l' rows hold d; one
// more N-vector of work (W^-1 of a right-hand side); beta_k and (J v_k)'h_k in arrays of length nq; the first row of every cone
// and the cone of every row as integers; the ring of g_k behind the staged rows, in the region X and K take afterwards.
//
// A cone belongs to one wavefront at a time: its lanes run along the rows, a lane adds its rows ascending, the lanes add by
// the xor butterfly of batch_device.hpp.  The order of a cone's sums depends on its order m_k alone.  A lane reads, of what its
// wavefront writes in one pass over a cone, only the rows it wrote itself; the first row's values travel in registers.  Sums
// over all rows have the fixed order of batch_device.hpp.  No atomics, no communication between workgroups; every scalar is
// computed by every thread from the same reduced values, so every branch around a barrier is workgroup-uniform.  Every loop is
// bounded by maxiters, n, N, p or nq.  A NaN or Inf never passes a pivot test and makes every comparison of the stopping tests
// false, so such a member ends with exit 3, 2 or 1.
#include "socp_batch.hpp"
#include "batch_device.hpp"

#include <cmath>

namespace kvx {
namespace {

using namespace batchdev;
static_assert(NT == SOCPB_THREADS, "the shared helpers are written for the workgroup of k_socp_batch");
constexpr int RING = SOCPB_TILE + 1;          // a tile meets at most 32 cones, one of them begun in an earlier tile

struct Layout {                               // offsets in doubles from the LDS base; every part starts on 16 bytes
    int ldn, ldp;
    int S, XK, X, K, g, x, dx, rx, x1, y, dy, ry, y1, s, z, d, di, lm, ds, dz, rz, ws3, z1, tw, beta, hv, red, off, cone, total;
};

__host__ __device__ inline Layout layout(int n, int N, int nq, int p)
{
    Layout L;
    L.ldn = n | 1;
    L.ldp = p | 1;
    int o = 0;
    L.S = o; o += even(n * L.ldn);
    const int xsz = even(p * L.ldn), ksz = even(p * L.ldp), tsz = even(SOCPB_TILE * L.ldn), gsz = nq ? even(RING * L.ldn) : 0;
    L.XK = L.X = o; L.K = o + xsz; L.g = o + tsz; o += (xsz + ksz > tsz + gsz ? xsz + ksz : tsz + gsz);
    const int nv = even(n), pv = even(p), mv = even(N), qv = even(nq);
    L.x = o; o += nv; L.dx = o; o += nv; L.rx = o; o += nv; L.x1 = o; o += nv;
    L.y = o; o += pv; L.dy = o; o += pv; L.ry = o; o += pv; L.y1 = o; o += pv;
    L.s = o; o += mv; L.z = o; o += mv; L.d = o; o += mv; L.di = o; o += mv; L.lm = o; o += mv; L.ds = o; o += mv;
    L.dz = o; o += mv; L.rz = o; o += mv; L.ws3 = o; o += mv; L.z1 = o; o += mv; L.tw = o; o += mv;
    L.beta = o; o += qv; L.hv = o; o += qv;
    L.red = o; o += NW * NRED;
    L.off = o; o += even((nq + 2) / 2);                    // nq + 1 ints
    L.cone = o; o += even((N + 3) / 4);                    // N unsigned shorts
    L.total = o;
    return L;
}

struct Member {                               // one member's data in HBM and its vectors and matrices in LDS
    int n, ml, nq, N, p, ldn, ldp;
    const double *c, *G, *h, *A, *b;
    double *S, *T, *X, *K, *g, *x, *dx, *rx, *x1, *y, *dy, *ry, *y1, *s, *z, *d, *di, *lm, *ds, *dz, *rz, *ws3, *z1, *tw, *beta, *hv, *red;
    int *off;                                 // off[k]: the first row of cone k; off[nq] = N
    unsigned short *cone;                     // cone[r - ml]: the cone of row r >= ml
};

// r[0..K) := the sums over the rows i = 0..m-1 of a cone of what f adds for row i, the same bytes in every lane of the wavefront
template <int K, class F>
__device__ inline void cone_sum(int m, double (&r)[K], F f)
{
#pragma unroll
    for (int k = 0; k < K; k++) r[k] = 0.0;
    for (int i = threadIdx.x & 63; i < m; i += 64) f(i, r);
#pragma unroll
    for (int k = 0; k < K; k++) r[k] = wave_sum(r[k]);
}

__device__ inline double jsign(int i, double u) { return i ? -u : u; }                     // (J u)_i
__device__ inline double jnrm(double x0, double tail_sq)                                  // misc.jnrm2 as the reference forms it
{
    const double a = sqrt(tail_sq);
    return sqrt(x0 - a) * sqrt(x0 + a);
}

// out := W^-1 in (INV) or W in; in == out is allowed.  The caller's barriers stand before and after.
template <bool INV>
__device__ void wscale(const Member &M, const double *in, double *out)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int k = tid; k < M.ml; k += NT) out[k] = (INV ? M.di[k] : M.d[k]) * in[k];
    for (int c = w; c < M.nq; c += NW) {
        const int o = M.off[c], m = M.off[c + 1] - o;
        const double *v = M.d + o;
        double r[1];
        cone_sum<1>(m, r, [&](int i, double (&r)[1]) { r[0] += (INV ? jsign(i, v[i]) : v[i]) * in[o + i]; });
        const double be = M.beta[c];
        for (int i = lane; i < m; i += 64) {
            const double t = 2.0 * (INV ? jsign(i, v[i]) : v[i]) * r[0] - jsign(i, in[o + i]);
            out[o + i] = INV ? t / be : t * be;
        }
    }
}

// mx[0], mx[1] := the larger of themselves and max_step over the 'q' blocks of a1 u1 and a2 u2 (misc_solvers.c:1073-1085)
__device__ void cone_max_step(const Member &M, const double *u1, double a1, const double *u2, double a2, double (&mx)[2])
{
    for (int c = threadIdx.x >> 6; c < M.nq; c += NW) {
        const int o = M.off[c], m = M.off[c + 1] - o;
        double r[2];
        cone_sum<2>(m, r, [&](int i, double (&r)[2]) {
            if (i) { const double t1 = a1 * u1[o + i], t2 = a2 * u2[o + i]; r[0] += t1 * t1; r[1] += t2 * t2; }
        });
        mx[0] = fmax(mx[0], sqrt(r[0]) - a1 * u1[o]);
        mx[1] = fmax(mx[1], sqrt(r[1]) - a2 * u2[o]);
    }
}

// hv[k] := (J v_k)'h_k.  The caller's barriers stand before and after.
__device__ void cone_hv(const Member &M)
{
    for (int c = threadIdx.x >> 6; c < M.nq; c += NW) {
        const int o = M.off[c], m = M.off[c + 1] - o;
        double r[1];
        cone_sum<1>(m, r, [&](int i, double (&r)[1]) { r[0] += jsign(i, M.d[o + i]) * M.h[o + i]; });
        if ((threadIdx.x & 63) == 0) M.hv[c] = r[0];
    }
}

// (W^-1 h)_r from hv
__device__ inline double th_row(const Member &M, int r)
{
    if (r < M.ml) return M.di[r] * M.h[r];
    const int c = M.cone[r - M.ml], i = r - M.off[c];
    return (2.0 * jsign(i, M.d[r]) * M.hv[c] - jsign(i, M.h[r])) / M.beta[c];
}

// The lower triangle of S = Gs'Gs [+ A'A], Gs = W^-1 G, in LDS.  Barriers before (the caller's) and after.
__device__ void assemble(const Member &M, bool sing)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = M.n, ml = M.ml, N = M.N, nq = M.nq, p = M.p, ldn = M.ldn;
    const int cnt = tri_count(n);
    for (int e = tid; e < cnt; e += NT) {
        int i, j;
        if (!tri_map(e, n, i, j)) continue;
        double acc = 0.0;
        if (sing)
            for (int a = 0; a < p; a++) acc += M.A[a + (int64_t)i * p] * M.A[a + (int64_t)j * p];
        M.S[i + j * ldn] = acc;
    }
    for (int k0 = 0; k0 < N; k0 += SOCPB_TILE) {
        const int kt = min((int)SOCPB_TILE, N - k0), k1 = k0 + kt;
        // the cones whose first row lies in this tile: g_k = (J v_k)'G_k into slot k mod RING.  The cone an earlier tile began
        // keeps its slot; the at most 31 that begin here follow it, so no two live cones share one.
        int cf = nq, cl = nq;
        if (k1 > ml && nq > 0) {
            cf = k0 <= ml ? 0 : M.cone[k0 - ml] + (M.off[M.cone[k0 - ml]] < k0 ? 1 : 0);
            cl = M.cone[k1 - 1 - ml] + 1;
        }
        const int pairs = (cl - cf) * n;
        for (int e = tid; e < pairs; e += NT) {            // a small cone: one thread adds its rows ascending
            const int c = cf + e / n, col = e - (c - cf) * n, o = M.off[c], m = M.off[c + 1] - o;
            if (m > SOCPB_SERIAL) continue;
            double acc = 0.0;
            for (int i = 0; i < m; i++) acc += jsign(i, M.d[o + i]) * M.G[o + i + (int64_t)col * N];
            M.g[(c % RING) * ldn + col] = acc;
        }
        for (int e = w; e < pairs; e += NW) {              // a larger one: a wavefront
            const int c = cf + e / n, col = e - (c - cf) * n, o = M.off[c], m = M.off[c + 1] - o;
            if (m <= SOCPB_SERIAL) continue;
            double r[1];
            cone_sum<1>(m, r, [&](int i, double (&r)[1]) { r[0] += jsign(i, M.d[o + i]) * M.G[o + i + (int64_t)col * N]; });
            if (lane == 0) M.g[(c % RING) * ldn + col] = r[0];
        }
        __syncthreads();                                   // g is there, and the staged rows of the previous step have been read
        for (int e = tid; e < SOCPB_TILE * n; e += NT) {
            const int kk = e & (SOCPB_TILE - 1), col = e / SOCPB_TILE, r = k0 + kk;
            if (kk >= kt) continue;
            const double gv = M.G[r + (int64_t)col * N];
            double t;
            if (r < ml) t = M.di[r] * gv;
            else {
                const int c = M.cone[r - ml], i = r - M.off[c];
                t = (2.0 * jsign(i, M.d[r]) * M.g[(c % RING) * ldn + col] - jsign(i, gv)) / M.beta[c];
            }
            M.T[kk * ldn + col] = t;
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

// The KKT factorisation in the scaling W (misc.py:1395-1487), as in lp_batch.hip; also hv.  false on a failed pivot.  Barriers
// before (the caller's) and after.
__device__ bool factor(const Member &M, bool &sing, bool first)
{
    const int tid = threadIdx.x, n = M.n, p = M.p, ldn = M.ldn, ldp = M.ldp;
    cone_hv(M);
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
    for (int a = w; a < p; a += NW) {                      // the staged rows and g are dead: X may take their place
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
    const int tid = threadIdx.x, n = M.n, N = M.N, p = M.p, lane = tid & 63, w = tid >> 6;
    wscale<true>(M, vz, vz);                                                               // z := W^-T bz
    __syncthreads();
    wscale<true>(M, vz, M.tw);
    __syncthreads();
    gemv_t_add(M.G, N, n, M.tw, nullptr, 1.0, vx);                                         // x += G' W^-1 z
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
    for (int k = tid; k < N; k += NT) M.tw[k] = row_dot(M.G, N, n, k, vx);
    __syncthreads();
    wscale<true>(M, M.tw, M.tw);
    __syncthreads();
    for (int k = tid; k < N; k += NT) vz[k] = M.tw[k] - vz[k];                             // W uz = W^-T G ux - W^-T bz
    __syncthreads();
}

// coneprog.py:861-896 as in lp_batch.hip, on N rows.  Barriers before (the caller's) and after.
__device__ void residuals(const Member &M, double tau, double (&r)[9])
{
    const int tid = threadIdx.x, n = M.n, N = M.N, p = M.p;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
    if (tid < n) M.rx[tid] = 0.0;
    if (tid < p) {
        const double t = row_dot(M.A, p, n, tid, M.x), bk = M.b[tid], u = t - tau * bk;
        M.ry[tid] = u;
        v[2] = t * t; v[3] = u * u;
        w[1] = bk * M.y[tid];
    }
    for (int k = tid; k < N; k += NT) {
        const double t = row_dot(M.G, N, n, k, M.x) + M.s[k], hk = M.h[k], u = t - tau * hk;
        M.rz[k] = u;
        v[4] += t * t; v[5] += u * u;
        w[2] += hk * M.z[k];
    }
    __syncthreads();
    if (p > 0) gemv_t_add(M.A, p, n, M.y, nullptr, -1.0, M.rx);
    __syncthreads();
    gemv_t_add(M.G, N, n, M.z, nullptr, -1.0, M.rx);
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

// lmbda'lmbda.  Barriers before (the caller's) and after.
__device__ double lam_sq(const Member &M)
{
    double g[1] = {0.0};
    for (int k = threadIdx.x; k < M.N; k += NT) g[0] += M.lm[k] * M.lm[k];
    blk_reduce<1, false>(g, M.red);
    return g[0];
}

__global__ void __launch_bounds__(SOCPB_THREADS) k_socp_batch(SocpBatchArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = a.n, ml = a.ml, nq = a.nq, N = a.N, p = a.p;
    const int64_t bm = blockIdx.x;
    const Layout L = layout(n, N, nq, p);
    Member M;
    M.n = n; M.ml = ml; M.nq = nq; M.N = N; M.p = p; M.ldn = L.ldn; M.ldp = L.ldp;
    M.c = a.c + bm * a.sc; M.G = a.G + bm * a.sG; M.h = a.h + bm * a.sh;
    M.A = p ? a.A + bm * a.sA : nullptr; M.b = p ? a.b + bm * a.sb : nullptr;
    M.S = lds + L.S; M.T = lds + L.XK; M.X = lds + L.X; M.K = lds + L.K; M.g = lds + L.g;
    M.x = lds + L.x; M.dx = lds + L.dx; M.rx = lds + L.rx; M.x1 = lds + L.x1;
    M.y = lds + L.y; M.dy = lds + L.dy; M.ry = lds + L.ry; M.y1 = lds + L.y1;
    M.s = lds + L.s; M.z = lds + L.z; M.d = lds + L.d; M.di = lds + L.di; M.lm = lds + L.lm; M.ds = lds + L.ds; M.dz = lds + L.dz;
    M.rz = lds + L.rz; M.ws3 = lds + L.ws3; M.z1 = lds + L.z1; M.tw = lds + L.tw; M.beta = lds + L.beta; M.hv = lds + L.hv;
    M.red = lds + L.red;
    M.off = reinterpret_cast<int *>(lds + L.off);
    M.cone = reinterpret_cast<unsigned short *>(lds + L.cone);
    double *xo = a.x + bm * n, *yo = p ? a.y + bm * p : nullptr, *so = a.s + bm * N, *zo = a.z + bm * N, *st = a.stats + bm * SOCPB_NSTAT;

    // ---- the cone: the first row of every block and the block of every row
    if (tid <= nq) {
        int o = ml;
        for (int k = 0; k < tid; k++) o += a.q[k];
        M.off[tid] = o;
    }
    __syncthreads();
    for (int c = w; c < nq; c += NW) {
        const int o = M.off[c], m = M.off[c + 1] - o;
        for (int i = lane; i < m; i += 64) M.cone[o + i - ml] = (unsigned short)c;
    }

    int code = SOCPB_RANK, iters = 0;                      // solvers.socp: ValueError("Rank(A) < p or Rank([G; A]) < n")
    bool sing = false, at0 = false;
    double tau = 1.0, kappa = 1.0, dg = 1.0, dgi = 1.0, lg = 1.0, gap = NAN, lam2 = 0.0;
    double relgap = NAN, pcost = NAN, dcost = NAN, pres = NAN, dres = NAN, pinfres = NAN, dinfres = NAN;
    double sp = 0.0, sd = 0.0;                             // what x, s and y, z are scaled by at the end; NaN: not returned
    double resx0 = 1.0, resy0 = 1.0, resz0 = 1.0;

    // ---- starting point (coneprog.py:662-842): W = I, that is d = di = 1, v_k = e, beta_k = 1
    for (int k = tid; k < N; k += NT) { M.d[k] = k < ml ? 1.0 : 0.0; M.di[k] = 1.0; M.s[k] = M.h[k]; M.z[k] = 0.0; }
    if (tid < n) { M.x[tid] = 0.0; M.dx[tid] = -M.c[tid]; }
    if (tid < p) { M.dy[tid] = M.b[tid]; M.y[tid] = 0.0; }
    __syncthreads();
    if (tid < nq) { M.d[M.off[tid]] = 1.0; M.beta[tid] = 1.0; }
    __syncthreads();
    bool run = factor(M, sing, true);
    if (run) {
        kkt_solve(M, sing, M.x, M.dy, M.s);
        kkt_solve(M, sing, M.dx, M.y, M.z);
        double mx[2] = {-INFINITY, -INFINITY}, nr[4] = {0.0, 0.0, 0.0, 0.0}, r0[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (tid < n) { const double ck = M.c[tid]; r0[0] = ck * ck; r0[3] = ck * M.x[tid]; }
        if (tid < p) { const double bk = M.b[tid]; r0[1] = bk * bk; r0[4] = bk * M.y[tid]; }
        for (int k = tid; k < N; k += NT) {
            const double sk = -M.s[k], zk = M.z[k], hk = M.h[k];
            M.s[k] = sk;
            if (k < ml) { mx[0] = fmax(mx[0], -sk); mx[1] = fmax(mx[1], -zk); }
            nr[0] += sk * sk; nr[1] += zk * zk; nr[2] += sk * zk; nr[3] += hk * zk;
            r0[2] += hk * hk;
        }
        __syncthreads();
        cone_max_step(M, M.s, 1.0, M.z, 1.0, mx);
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
        if (!at0) {                                        // both pushes into the cone (coneprog.py:806-842): along e
            const bool ps = mx[0] >= -1e-8 * fmax(sqrt(nr[0]), 1.0), pz = mx[1] >= -1e-8 * fmax(sqrt(nr[1]), 1.0);
            for (int k = tid; k < ml + nq; k += NT) {
                const int r = k < ml ? k : M.off[k - ml];
                if (ps) M.s[r] += 1.0 + mx[0];
                if (pz) M.z[r] += 1.0 + mx[1];
            }
            __syncthreads();
            double g[1] = {0.0};
            for (int k = tid; k < N; k += NT) g[0] += M.s[k] * M.z[k];
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
        if (at0) { code = SOCPB_OPTIMAL; pinfres = dinfres = NAN; sp = sd = 1.0; break; }     // coneprog.py:757-804: as they are
        if (iters == a.maxiters) { code = SOCPB_MAXITERS; sp = sd = 1.0 / tau; break; }
        if (pres <= a.feastol && dres <= a.feastol && (gap <= a.abstol || relgap <= a.reltol)) {
            code = SOCPB_OPTIMAL; pinfres = dinfres = NAN; sp = sd = 1.0 / tau; break;
        }
        if (pinfres <= a.feastol) { code = SOCPB_PRIMAL_INFEASIBLE; sp = NAN; sd = 1.0 / (-hz - by); break; }
        if (dinfres <= a.feastol) { code = SOCPB_DUAL_INFEASIBLE; sp = 1.0 / (-cx); sd = NAN; break; }

        // ---- scaling of the first iteration (misc.py:284-352, coneprog.py:1041-1043)
        if (iters == 0) {
            for (int k = tid; k < ml; k += NT) {
                const double sk = M.s[k], zk = M.z[k], dk = sqrt(sk / zk);
                M.d[k] = dk; M.di[k] = 1.0 / dk; M.lm[k] = sqrt(sk * zk);
            }
            for (int c = w; c < nq; c += NW) {
                const int o = M.off[c], m = M.off[c + 1] - o;
                const double *sk = M.s + o, *zk = M.z + o;
                double q[3];                               // |s1|^2, |z1|^2, s'z
                cone_sum<3>(m, q, [&](int i, double (&q)[3]) {
                    const double u = sk[i], v = zk[i];
                    if (i) { q[0] += u * u; q[1] += v * v; }
                    q[2] += u * v;
                });
                const double s0 = sk[0], z0 = zk[0], aa = jnrm(s0, q[0]), bb = jnrm(z0, q[1]);
                const double cc = sqrt((q[2] / aa / bb + 1.0) / 2.0);
                const double v0 = (z0 / bb + s0 / aa) * (1.0 / 2.0 / cc) + 1.0, vs = 1.0 / sqrt(2.0 * v0);
                const double dd = 2.0 * cc + s0 / aa + z0 / bb;
                const double cs = (cc + z0 / bb) / dd / aa, cz = (cc + s0 / aa) / dd / bb, sab = sqrt(aa * bb);
                for (int i = lane; i < m; i += 64) {
                    if (i == 0) { M.d[o] = v0 * vs; M.lm[o] = cc * sab; }
                    else {
                        M.d[o + i] = ((-zk[i] / bb + sk[i] / aa) * (1.0 / 2.0 / cc)) * vs;
                        M.lm[o + i] = (sk[i] * cs + zk[i] * cz) * sab;
                    }
                }
                if (lane == 0) M.beta[c] = sqrt(aa / bb);
            }
            __syncthreads();
            lam2 = lam_sq(M);
            dg = sqrt(kappa / tau); dgi = sqrt(tau / kappa); lg = sqrt(tau * kappa);
        }
        __syncthreads();

        // ---- the factorisation and the constant system (coneprog.py:1066-1077): (x1, y1, z1) = dgi f3(-c, b, h)
        if (!factor(M, sing, false)) {
            if (iters == 0) code = SOCPB_RANK;
            else { code = SOCPB_SINGULAR; sp = sd = 1.0 / tau; }
            break;
        }
        for (int k = tid; k < N; k += NT) M.z1[k] = M.h[k];
        if (tid < n) M.x1[tid] = -M.c[tid];
        if (tid < p) M.y1[tid] = M.b[tid];
        __syncthreads();
        kkt_solve(M, sing, M.x1, M.y1, M.z1);
        double z1z1;
        {
            double g[1] = {0.0};
            for (int k = tid; k < N; k += NT) { const double t = dgi * M.z1[k]; M.z1[k] = t; g[0] += t * t; }
            if (tid < n) M.x1[tid] *= dgi;
            if (tid < p) M.y1[tid] *= dgi;
            blk_reduce<1, false>(g, M.red);
            z1z1 = g[0];
        }

        // ---- the two directions (coneprog.py:1248-1333) through f6_no_ir (:1130-1195)
        const double mu = (lam2 + lg * lg) / (1 + N);           // coneprog.py:1248: 1 + cdim_diag, the length of lmbda
        double sigma = 0.0, wkappa3 = 0.0, step = 0.0, tt = 0.0, tk = 0.0;
        for (int i = 0; i < 2; i++) {
            // ds := -(lmbda o\ (lmbda o lmbda [+ ws3 - sigma mu e])), dz := -((1 - sigma) rz + W'ds)
            for (int k = tid; k < ml; k += NT) {
                const double lk = M.lm[k];
                double t = lk * lk;
                if (i == 1) t += M.ws3[k] - sigma * mu;
                t = -t / lk;
                M.ds[k] = t;
                M.dz[k] = -((1.0 - sigma) * M.rz[k] + M.d[k] * t);
            }
            for (int c = w; c < nq; c += NW) {
                const int o = M.off[c], m = M.off[c + 1] - o;
                const double *lm = M.lm + o, *v = M.d + o;
                const double l0 = lm[0];
                double q[2];                               // lmbda'lmbda, |lmbda_1|^2
                cone_sum<2>(m, q, [&](int j, double (&q)[2]) { const double t = lm[j] * lm[j]; q[0] += t; if (j) q[1] += t; });
                double d0 = q[0];                          // sprod (misc_solvers.c:671-700): head lmbda'lmbda, tail 2 l0 lmbda_1
                if (i == 1) d0 += M.ws3[o] - sigma * mu;
                double u[1];                               // sinv (misc_solvers.c:803-835)
                cone_sum<1>(m, u, [&](int j, double (&u)[1]) {
                    if (j) { double t = l0 * lm[j] + lm[j] * l0; if (i == 1) t += M.ws3[o + j]; u[0] += t * lm[j]; }
                });
                const double nl = sqrt(q[1]), aq = (l0 + nl) * (l0 - nl), dq = u[0];
                double vd[1];                              // v'ds of W'ds
                cone_sum<1>(m, vd, [&](int j, double (&vd)[1]) {
                    double t;
                    if (j == 0) t = (d0 * l0 - dq) * (1.0 / aq);
                    else {
                        t = l0 * lm[j] + lm[j] * l0;
                        if (i == 1) t += M.ws3[o + j];
                        t = (t * (aq / l0) + (dq / l0 - d0) * lm[j]) * (1.0 / aq);
                    }
                    t = -t;
                    M.ds[o + j] = t;
                    vd[0] += v[j] * t;
                });
                const double be = M.beta[c];
                for (int j = lane; j < m; j += 64)
                    M.dz[o + j] = -((1.0 - sigma) * M.rz[o + j] + (2.0 * v[j] * vd[0] - jsign(j, M.ds[o + j])) * be);
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
            for (int k = tid; k < N; k += NT) dot[2] += th_row(M, k) * M.dz[k];
            blk_reduce<3, false>(dot, M.red);
            const double dtau = dgi * ((1.0 - sigma) * rt + dkappa / dgi + dot[0] + dot[1] + dot[2]) / (1.0 + z1z1);
            if (tid < n) M.dx[tid] += dtau * M.x1[tid];
            if (tid < p) M.dy[tid] += dtau * M.y1[tid];
            // dz += dtau z1, ds -= dz, ws3 := ds o dz after the predictor, both scaled by lmbda (scale2), their max_step
            double mx[2] = {-INFINITY, -INFINITY};
            for (int k = tid; k < ml; k += NT) {
                const double lk = M.lm[k], zk = M.dz[k] + dtau * M.z1[k], sk = M.ds[k] - zk;
                if (i == 0) M.ws3[k] = sk * zk;
                const double s2 = sk / lk, z2 = zk / lk;
                M.ds[k] = s2; M.dz[k] = z2;
                mx[0] = fmax(mx[0], -s2); mx[1] = fmax(mx[1], -z2);
            }
            for (int c = w; c < nq; c += NW) {
                const int o = M.off[c], m = M.off[c + 1] - o;
                const double *lm = M.lm + o;
                const double l0 = lm[0], z0 = M.dz[o] + dtau * M.z1[o], s0 = M.ds[o] - z0;
                double q[4];                               // ds'dz, |lmbda_1|^2, lmbda_1'ds_1, lmbda_1'dz_1
                cone_sum<4>(m, q, [&](int j, double (&q)[4]) {
                    const double zk = M.dz[o + j] + dtau * M.z1[o + j], sk = M.ds[o + j] - zk;
                    M.ds[o + j] = sk; M.dz[o + j] = zk;
                    q[0] += sk * zk;
                    if (j) { q[1] += lm[j] * lm[j]; q[2] += lm[j] * sk; q[3] += lm[j] * zk; }
                });
                const double nl = sqrt(q[1]), aq = sqrt(l0 + nl) * sqrt(l0 - nl);          // scale2 (misc_solvers.c:301-341)
                const double lxs = (l0 * s0 - q[2]) / aq, lxz = (l0 * z0 - q[3]) / aq;
                const double bs = -((s0 + lxs) / (l0 / aq + 1.0) / aq), bz = -((z0 + lxz) / (l0 / aq + 1.0) / aq);
                double t2[2];
                cone_sum<2>(m, t2, [&](int j, double (&t2)[2]) {
                    const double sk = M.ds[o + j], zk = M.dz[o + j];
                    if (i == 0) M.ws3[o + j] = j ? z0 * sk + s0 * zk : q[0];
                    const double s2 = (j ? sk + bs * lm[j] : lxs) * (1.0 / aq), z2 = (j ? zk + bz * lm[j] : lxz) * (1.0 / aq);
                    M.ds[o + j] = s2; M.dz[o + j] = z2;
                    if (j) { t2[0] += s2 * s2; t2[1] += z2 * z2; }
                });
                mx[0] = fmax(mx[0], sqrt(t2[0]) - lxs * (1.0 / aq));
                mx[1] = fmax(mx[1], sqrt(t2[1]) - lxz * (1.0 / aq));
            }
            dkappa -= dtau;
            if (i == 0) wkappa3 = dtau * dkappa;
            blk_reduce<2, true>(mx, M.red);
            tt = -dtau / lg; tk = -dkappa / lg;
            const double t = fmax(fmax(0.0, fmax(mx[0], mx[1])), fmax(tt, tk));
            step = t == 0.0 ? 1.0 : (i == 0 ? fmin(1.0, 1.0 / t) : fmin(1.0, 0.99 / t));
            if (i == 0) { const double u = 1.0 - step; sigma = u * u * u; }
        }

        // ---- the step, the scaling update (misc.py:444-580, coneprog.py:1336-1436), s = W'lmbda and z = W^-1 lmbda
        dg *= sqrt(1.0 - step * tk) / sqrt(1.0 - step * tt);
        dgi = 1.0 / dg;
        lg *= sqrt(1.0 - step * tt) * sqrt(1.0 - step * tk);
        kappa = lg / dgi; tau = lg * dgi;
        if (tid < n) M.x[tid] += step * M.dx[tid];
        if (tid < p) M.y[tid] += step * M.dy[tid];
        for (int k = tid; k < ml; k += NT) {
            const double lk = M.lm[k], rs = sqrt((1.0 + step * M.ds[k]) * lk), rz = sqrt((1.0 + step * M.dz[k]) * lk);
            const double dk = M.d[k] * rs / rz, dik = 1.0 / dk, ln = rs * rz;
            M.d[k] = dk; M.di[k] = dik; M.lm[k] = ln;
            M.s[k] = dk * ln; M.z[k] = dik * ln;
        }
        for (int c = w; c < nq; c += NW) {
            const int o = M.off[c], m = M.off[c + 1] - o;
            double *lm = M.lm + o, *v = M.d + o;
            const double l0 = lm[0], vk0 = v[0], e0s = 1.0 + step * M.ds[o], e0z = 1.0 + step * M.dz[o];
            // ds := e + step ds, dz := e + step dz, then scale2 with inverse 'I': the new iterates in the current scaling
            double q[3];                                   // lmbda'ds, lmbda'dz, |lmbda_1|^2
            cone_sum<3>(m, q, [&](int j, double (&q)[3]) {
                const double sk = (j ? 0.0 : 1.0) + step * M.ds[o + j], zk = (j ? 0.0 : 1.0) + step * M.dz[o + j];
                M.ds[o + j] = sk; M.dz[o + j] = zk;
                q[0] += lm[j] * sk; q[1] += lm[j] * zk;
                if (j) q[2] += lm[j] * lm[j];
            });
            const double nl = sqrt(q[2]), aq = sqrt(l0 + nl) * sqrt(l0 - nl);
            const double lxs = q[0] / aq, lxz = q[1] / aq;
            const double bs = (e0s + lxs) / (l0 / aq + 1.0) / aq, bz = (e0z + lxz) / (l0 / aq + 1.0) / aq;
            const double S0 = lxs * aq, Z0 = lxz * aq;
            double u[5];                                   // update_scaling: |s1|^2, |z1|^2, s'z, v's, v'Jz
            cone_sum<5>(m, u, [&](int j, double (&u)[5]) {
                const double sk = j ? (M.ds[o + j] + bs * lm[j]) * aq : S0, zk = j ? (M.dz[o + j] + bz * lm[j]) * aq : Z0;
                M.ds[o + j] = sk; M.dz[o + j] = zk;
                if (j) { u[0] += sk * sk; u[1] += zk * zk; }
                u[2] += sk * zk; u[3] += v[j] * sk; u[4] += jsign(j, v[j]) * zk;
            });
            const double aa = jnrm(S0, u[0]), bb = jnrm(Z0, u[1]);
            const double s0 = S0 / aa, z0 = Z0 / bb;
            const double cc = sqrt((1.0 + u[2] / aa / bb) / 2.0);
            const double vsd = u[3] / aa, vzd = u[4] / bb;
            const double vq = (vsd + vzd) / 2.0 / cc, vu = vsd - vzd;
            const double wk0 = 2.0 * vk0 * vq - (s0 + z0) / 2.0 / cc;
            const double dd = (vk0 * vu - s0 / 2.0 + z0 / 2.0) / (wk0 + 1.0);
            const double sab = sqrt(aa * bb);
            const double nv0 = 2.0 * vq * vk0 - s0 / 2.0 / cc - 0.5 / cc * z0 + 1.0, nvs = 1.0 / sqrt(2.0 * nv0);
            const double be = M.beta[c] * sqrt(aa / bb);
            double t2[2];                                  // v'lmbda and (J v)'lmbda of the new scaling
            cone_sum<2>(m, t2, [&](int j, double (&t2)[2]) {
                const double si = M.ds[o + j] / aa, zi = M.dz[o + j] / bb, vi = v[j];
                double ln, vn;
                if (j == 0) { ln = cc * sab; vn = nv0 * nvs; }
                else {
                    ln = (vi * (2.0 * (-dd * vq + 0.5 * vu)) + si * (0.5 * (1.0 - dd / cc)) + zi * (0.5 * (1.0 + dd / cc))) * sab;
                    vn = (2.0 * vq * vi + 0.5 / cc * si - 0.5 / cc * zi) * nvs;
                }
                lm[j] = ln; v[j] = vn;
                t2[0] += vn * ln; t2[1] += jsign(j, vn) * ln;
            });
            for (int j = lane; j < m; j += 64) {
                const double ln = lm[j], vn = v[j];
                M.s[o + j] = (2.0 * vn * t2[0] - jsign(j, ln)) * be;
                M.z[o + j] = (2.0 * jsign(j, vn) * t2[1] - jsign(j, ln)) / be;
            }
            if (lane == 0) M.beta[c] = be;
        }
        __syncthreads();
        lam2 = lam_sq(M);                                  // its barriers also publish x, y, s, z
    }

    // ---- the member's result: x, s scaled by sp and y, z by sd (coneprog.py:925-1024, 1082-1109); NaN for the half a certificate
    //      comes without; after a first factorisation that failed: zeros.  The slacks are -max_step of the scaled s and z.
    const bool rank = code == SOCPB_RANK, xs = sp == sp, zs = sd == sd;
    double mx[2] = {-INFINITY, -INFINITY};
    __syncthreads();
    for (int k = tid; k < N; k += NT) {
        const double sk = sp * M.s[k], zk = sd * M.z[k];
        so[k] = rank ? 0.0 : (xs ? sk : NAN); zo[k] = rank ? 0.0 : (zs ? zk : NAN);
        if (k < ml) { mx[0] = fmax(mx[0], -sk); mx[1] = fmax(mx[1], -zk); }
    }
    cone_max_step(M, M.s, sp, M.z, sd, mx);
    if (tid < n) xo[tid] = rank ? 0.0 : (xs ? sp * M.x[tid] : NAN);
    if (tid < p) yo[tid] = rank ? 0.0 : (zs ? sd * M.y[tid] : NAN);
    blk_reduce<2, true>(mx, M.red);
    if (tid == 0) {
        const bool pinf = code == SOCPB_PRIMAL_INFEASIBLE, dinf = code == SOCPB_DUAL_INFEASIBLE, cert = pinf || dinf;
        const double out[SOCPB_NSTAT] = {cert ? NAN : gap, cert ? NAN : relgap, pinf ? NAN : (dinf ? -1.0 : pcost),
                                         dinf ? NAN : (pinf ? 1.0 : dcost), cert ? NAN : pres, cert ? NAN : dres,
                                         xs ? -mx[0] : NAN, zs ? -mx[1] : NAN, dinf ? NAN : pinfres, pinf ? NAN : dinfres};
#pragma unroll
        for (int k = 0; k < SOCPB_NSTAT; k++) st[k] = rank ? NAN : out[k];
        a.iters[bm] = rank ? 0 : iters;
        a.exitc[bm] = code;
    }
}

}  // namespace

size_t socp_batch_lds_bytes(int n, int N, int nq, int p) { return (size_t)layout(n, N, nq, p).total * sizeof(double); }

hipError_t launch_socp_batch(hipStream_t st, const SocpBatchArgs &a)
{
    // per device, so asked of the current one at every launch
    const hipError_t e = hipFuncSetAttribute((const void *)k_socp_batch, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    k_socp_batch<<<dim3((unsigned)a.B), dim3(SOCPB_THREADS), socp_batch_lds_bytes(a.n, a.N, a.nq, a.p), st>>>(a);
    return hipGetLastError();
}

}  // namespace kvx
