// k_socp_batch: one workgroup (256 threads, four wavefronts) carries one small dense second-order-cone program from its starting
// point to its status or its infeasibility certificate (socp_batch.hpp).  It is conelp_member (batch_conelp.hpp) on the cone
// K = R^ml_+ x Q^{q_0} x ...: the 'l' rows are the orthant of that header, the 'q' rows are treated by the reference's own
// operations, which are batch_cone_q.hpp, included below into this file's anonymous namespace and shared with k_conelp_batch and
// k_coneqp_batch, strung together as cone.py::_ConeEngine strings them.  What stands here is this kernel's own: its layout and
// member, (J v_k)'h_k in place of a stored th, the assembly of S, the glue of the policy, the kernel and the launch.
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

#include "batch_cone_q.hpp"

// out := W^-1 in (INV) or W in; in == out is allowed.  The caller's barriers stand before and after.
template <bool INV>
__device__ void wscale(const Member &M, const double *in, double *out)
{
    for (int k = threadIdx.x; k < M.ml; k += NT) out[k] = (INV ? M.di[k] : M.d[k]) * in[k];
    cones_wscale<INV>(M, in, out);
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
        cones_max_step(M, u0, a0, u1, a1, mx);
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
        orth_first_scaling(M.ml, M.s, M.z, M.d, M.di, M.lm);
        cones_scaling(M);
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
        orth_rhs<true>(M.ml, i, sigma, mu, M.lm, M.ws3, M.d, M.rz, M.ds, M.dz);
        cones_rhs(M, i, sigma, mu);
    }
    __device__ __forceinline__ double th_dot(const double *dz) const
    {
        double acc = 0.0;
        for (int k = threadIdx.x; k < M.N; k += NT) acc += th_row(M, k) * dz[k];
        return acc;
    }
    __device__ __forceinline__ void combine(int i, double dtau, double (&mx)[2]) const
    {
        orth_combine(M.ml, i, dtau, M.lm, M.z1, M.ds, M.dz, M.ws3, mx);
        cones_combine(M, i, dtau, mx);
        blk_reduce<2, true>(mx, M.red);
    }
    __device__ __forceinline__ void update(double step) const                       // misc.py:444-580; s = W'lmbda and z = W^-1 lmbda
    {
        orth_update(M.ml, step, M.ds, M.dz, M.d, M.di, M.lm, M.s, M.z);
        cones_update(M, step);
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
