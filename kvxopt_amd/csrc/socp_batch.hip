// k_socp_batch: one workgroup (256 threads, four wavefronts) carries one small dense second-order-cone program from its starting
// point to its status or its infeasibility certificate (socp_batch.hpp).  It is conelp_member (batch_conelp.hpp) on the cone
// K = R^ml_+ x Q^{q_0} x ...: the 'l' rows are the orthant of that header, the 'q' rows are treated by the reference's own
// operations, the ones csrc/kkt_q.hip carries as stand-alone kernels: misc.compute_scaling / update_scaling (misc.py:290-352,
// 467-580), scale, scale2, sprod, sinv (misc_solvers.c:144-186, 301-341, 671-700, 803-835) and max_step
// (misc_solvers.c:1073-1085), strung together as cone.py::_ConeEngine strings them.
//
// W_k = beta_k (2 v_k v_k' - J) is symmetric, so W^-T = W^-1 = (1 / beta_k)(2 (J v_k)(J v_k)' - J).  S = Gs'Gs with Gs = W^-1 G
// is assembled from staged rows of Gs, 32 at a time: row i of cone k is (2 (J v_k)_i g_k - (J G_k)_i) / beta_k with the row
// vector g_k = (J v_k)'G_k, which is computed once per cone when the tile with the cone's first row is staged and kept, in a
// ring of 33 slots, while later tiles stage the rest of the cone.  (J v_k)'h_k is kept per cone for th = W^-1 h.
//
// LDS: S, X and K as in batch_kkt.hpp, the n-, p- and N-vectors of conelp_member with N = ml + sum q_k rows; v_k lies in the 'q'
// rows of the slot whose 'l' rows hold d; one more N-vector of work (W^-1 of a right-hand side); beta_k and (J v_k)'h_k in arrays
// of length nq; the first row of every cone and the cone of every row as integers; the ring of g_k behind the staged rows, in the
// region X and K take afterwards.
//
// A cone belongs to one wavefront at a time: its lanes run along the rows, a lane adds its rows ascending, the lanes add by
// the xor butterfly of batch_device.hpp.  The order of a cone's sums depends on its order m_k alone.  A lane reads, of what its
// wavefront writes in one pass over a cone, only the rows it wrote itself; the first row's values travel in registers.
#include "socp_batch.hpp"
#include "batch_conelp.hpp"

#include <cmath>

namespace kvx {
namespace {

using namespace batchdev;
static_assert(NT == SOCPB_THREADS, "the shared helpers are written for the workgroup of k_socp_batch");
static_assert(CONELP_NSTAT == SOCPB_NSTAT, "the stats of conelp_member");
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

struct Member : ConelpMem {                   // N = ml + sum q_k
    int ml, nq;
    double *g, *d, *di, *lm, *tw, *beta, *hv;
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
__device__ __forceinline__ void assemble(const Member &M, bool sing)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = M.n, ml = M.ml, N = M.N, nq = M.nq, ldn = M.ldn;
    kkt_s_init(M, sing);
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
        kkt_s_add_rows(M, kt);
    }
    __syncthreads();
}

struct Cone {                                 // the cone of conelp_member: the orthant for the 'l' rows, the code here for 'q'
    const Member &M;

    __device__ __forceinline__ int lmbda_len() const { return M.N; }
    template <class F>
    __device__ __forceinline__ void for_rows(F f) const { plain_rows(M.N, f); }
    __device__ __forceinline__ void load_h(double *out) const
    {
        for (int k = threadIdx.x; k < M.N; k += NT) out[k] = M.h[k];
    }
    __device__ __forceinline__ void start() const                                   // d = di = 1, v_k = e, beta_k = 1
    {
        const int tid = threadIdx.x;
        for (int k = tid; k < M.N; k += NT) { M.d[k] = k < M.ml ? 1.0 : 0.0; M.di[k] = 1.0; M.s[k] = M.h[k]; M.z[k] = 0.0; }
        __syncthreads();
        if (tid < M.nq) { M.d[M.off[tid]] = 1.0; M.beta[tid] = 1.0; }
        __syncthreads();
    }
    __device__ __forceinline__ void max_step(const double *u0, double a0, const double *u1, double a1, double (&mx)[2]) const
    {
        orth_max_step(M.ml, u0, a0, u1, a1, mx);
        cone_max_step(M, u0, a0, u1, a1, mx);
        blk_reduce<2, true>(mx, M.red);
    }
    __device__ __forceinline__ void push(bool ps, bool pz, const double (&mx)[2]) const
    {
        orth_push(M.ml, ps, pz, mx, M.s, M.z);
        if ((int)threadIdx.x < M.nq) {
            const int r = M.off[threadIdx.x];
            if (ps) M.s[r] += 1.0 + mx[0];
            if (pz) M.z[r] += 1.0 + mx[1];
        }
    }
    __device__ __forceinline__ bool first_scaling() const                           // misc.py:284-352
    {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nq = M.nq;
        orth_first_scaling(M.ml, M.s, M.z, M.d, M.di, M.lm);
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
        return true;
    }
    __device__ __forceinline__ double lam_sq() const { return sum_sq(M.lm, M.N, M.red); }
    __device__ __forceinline__ void prepare() const { cone_hv(M); }
    __device__ __forceinline__ void assemble(bool sing) const { kvx::assemble(M, sing); }
    __device__ __forceinline__ void kkt_before(double *vx, double *vz) const
    {
        wscale<true>(M, vz, vz);                                                               // z := W^-T bz
        __syncthreads();
        wscale<true>(M, vz, M.tw);
        __syncthreads();
        gemv_t_add(M.G, M.N, M.n, M.tw, nullptr, 1.0, vx);                                       // x += G' W^-1 z
        __syncthreads();
    }
    __device__ __forceinline__ void kkt_after(double *vx, double *vz) const
    {
        const int tid = threadIdx.x, n = M.n, N = M.N;
        for (int k = tid; k < N; k += NT) M.tw[k] = row_dot(M.G, N, n, k, vx);
        __syncthreads();
        wscale<true>(M, M.tw, M.tw);
        __syncthreads();
        for (int k = tid; k < N; k += NT) vz[k] = M.tw[k] - vz[k];                             // W uz = W^-T G ux - W^-T bz
        __syncthreads();
    }
    __device__ __forceinline__ void gemv_t(const double *u, double sign, double *v) const
    {
        gemv_t_add(M.G, M.N, M.n, u, nullptr, sign, v);
    }
    __device__ __forceinline__ void rhs(int i, double sigma, double mu) const
    {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nq = M.nq;
        orth_rhs<true>(M.ml, i, sigma, mu, M.lm, M.ws3, M.d, M.rz, M.ds, M.dz);
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
    }
    __device__ __forceinline__ double th_dot(const double *dz) const
    {
        double acc = 0.0;
        for (int k = threadIdx.x; k < M.N; k += NT) acc += th_row(M, k) * dz[k];
        return acc;
    }
    __device__ __forceinline__ void combine(int i, double dtau, double (&mx)[2]) const
    {
        const int w = threadIdx.x >> 6, nq = M.nq;
        orth_combine(M.ml, i, dtau, M.lm, M.z1, M.ds, M.dz, M.ws3, mx);
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
        blk_reduce<2, true>(mx, M.red);
    }
    __device__ __forceinline__ void update(double step) const                       // misc.py:444-580; s = W'lmbda and z = W^-1 lmbda
    {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nq = M.nq;
        orth_update(M.ml, step, M.ds, M.dz, M.d, M.di, M.lm, M.s, M.z);
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
    }
};

__global__ void __launch_bounds__(SOCPB_THREADS) k_socp_batch(SocpBatchArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, ml = a.ml, nq = a.nq;
    const Layout L = layout(a.n, a.N, nq, a.p);
    Member M;
    conelp_data(M, a, a.N);
    M.ml = ml; M.nq = nq; M.ldn = L.ldn; M.ldp = L.ldp;
    M.S = lds + L.S; M.T = lds + L.XK; M.X = lds + L.X; M.K = lds + L.K; M.g = lds + L.g;
    M.x = lds + L.x; M.dx = lds + L.dx; M.rx = lds + L.rx; M.x1 = lds + L.x1;
    M.y = lds + L.y; M.dy = lds + L.dy; M.ry = lds + L.ry; M.y1 = lds + L.y1;
    M.s = lds + L.s; M.z = lds + L.z; M.d = lds + L.d; M.di = lds + L.di; M.lm = lds + L.lm; M.ds = lds + L.ds; M.dz = lds + L.dz;
    M.rz = lds + L.rz; M.ws3 = lds + L.ws3; M.z1 = lds + L.z1; M.tw = lds + L.tw; M.beta = lds + L.beta; M.hv = lds + L.hv;
    M.red = lds + L.red;
    M.off = reinterpret_cast<int *>(lds + L.off);
    M.cone = reinterpret_cast<unsigned short *>(lds + L.cone);

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
    __syncthreads();
    conelp_member(Cone{M}, a);
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
