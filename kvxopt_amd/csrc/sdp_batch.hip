// k_sdp_batch: one workgroup (256 threads, four wavefronts) carries one small dense semidefinite program from its starting point
// to its status or its infeasibility certificate (sdp_batch.hpp).  It is conelp_member (batch_conelp.hpp) on the cone
// K = R^ml_+ x S^{m_0}_+ x ...: the 'l' rows are the orthant of that header, the 's' rows are treated by the reference's own
// operations, which are batch_cone_s.hpp, included below into this file's anonymous namespace and shared with k_conelp_batch and
// k_coneqp_batch, strung together as cone.py::_ConeEngine strings them.  What stands here is this kernel's own: its layout and
// member, W on its cone, the assembly of S, the glue of the policy and the kernel.
//
// Vectors of the cone lie in LDS with every 's' block as its full symmetric m x m matrix, column-major with leading dimension m:
// with a thread per entry a wavefront reads consecutive rows of one operand and at most 64 / m entries of the other, which are
// broadcasts, so a padded leading dimension buys nothing and the blocks keep the layout the results are returned in.  Every block
// operation writes both triangles from one computed value, so the blocks stay symmetric to the bit.  G and h are read in HBM
// through two tables of the Np = ml + sum m_k (m_k + 1) / 2 packed rows: prow[q], the row of the q-th lower-triangle entry, and
// pmir[q], the row of its mirror image; an off-diagonal entry counts twice in G'z and in the cone's inner product (misc.sgemv,
// misc.sdot).  The upper triangles of G and h are never read.
//
// S = Gs'Gs with Gs = W^-T G is assembled from staged rows of Gs, at most 32 at a time.  The 's' rows of block k and column j are
// rti_k' mat(G_kj) rti_k, packed with sqrt(2) on the off-diagonals; they are staged one block column b at a time, with no
// workspace in HBM: w_j = mat(G_kj) rti_k[:, b] for all columns j (m_k x n, in the 16 rows behind the staged ones), then the rows
// (a, b), a >= b, as rti_k[:, a]'w_j.  G's 's' rows are read m_k times per factorisation, from L2; the scaled rows never leave
// LDS, which keeps the Gram form and spares the _dev entry a workspace argument.
//
// Sums over all rows have the fixed order of batch_device.hpp.  Every loop of this file and of batch_cone_s.hpp is bounded by n,
// N, ns, m_k or SDPB_SWEEPS.
#include "sdp_batch.hpp"
#include "batch_conelp.hpp"

#include <cmath>

namespace kvx {
namespace {

using namespace batchdev;
static_assert(NT == SDPB_THREADS, "the shared helpers are written for the workgroup of k_sdp_batch");
static_assert(SDPB_MAX_M * SDPB_MAX_M <= NT, "a thread per entry of a block");
constexpr int MAX_M = SDPB_MAX_M, SWEEPS = SDPB_SWEEPS;      // what batch_cone_s.hpp asks of its includer
constexpr int MM = MAX_M * MAX_M;
constexpr int STAGE = SDPB_TILE + SDPB_MAX_M;      // the staged rows and, behind them, w of the block column being staged
constexpr double RT2 = 1.41421356237309504880;
static_assert(CONELP_NSTAT == SDPB_NSTAT, "the stats of conelp_member");

struct Layout {                               // offsets in doubles from the LDS base; every part starts on 16 bytes
    int ldn, ldp;
    int S, XK, X, K, x, dx, rx, x1, y, dy, ry, y1, s, z, ds, dz, rz, ws3, z1, tw, th, r, rti, lm, d, di, sgs, sgz, wk, nrm, red, blk,
        prow, pmir, flag, total;
};

__host__ __device__ inline Layout layout(int n, int ml, int N, int Nd, int Np, int ns, int p)
{
    Layout L;
    L.ldn = n | 1;
    L.ldp = p | 1;
    int o = 0;
    L.S = o; o += even(n * L.ldn);
    const int xsz = even(p * L.ldn), ksz = even(p * L.ldp), tsz = even((ns ? STAGE : SDPB_TILE) * L.ldn);
    L.XK = L.X = o; L.K = o + xsz; o += (xsz + ksz > tsz ? xsz + ksz : tsz);
    const int nv = even(n), pv = even(p), mv = even(N), sv = even(N - ml), lv = even(ml), dv = even(Nd), ev = even(Nd - ml);
    L.x = o; o += nv; L.dx = o; o += nv; L.rx = o; o += nv; L.x1 = o; o += nv;
    L.y = o; o += pv; L.dy = o; o += pv; L.ry = o; o += pv; L.y1 = o; o += pv;
    L.s = o; o += mv; L.z = o; o += mv; L.ds = o; o += mv; L.dz = o; o += mv; L.rz = o; o += mv; L.ws3 = o; o += mv;
    L.z1 = o; o += mv; L.tw = o; o += mv; L.th = o; o += mv;
    L.r = o; o += sv; L.rti = o; o += sv;
    L.lm = o; o += dv; L.d = o; o += lv; L.di = o; o += lv; L.sgs = o; o += ev; L.sgz = o; o += ev;
    L.wk = o; o += ns ? 4 * MM : 0;
    L.nrm = o; o += ns ? 2 * SDPB_MAX_M : 0;
    L.red = o; o += NW * NRED;
    L.blk = o; o += ns + 1;                                // 2 (ns + 1) ints
    L.prow = o; o += even((Np + 3) / 4);                   // Np unsigned shorts
    L.pmir = o; o += even((Np + 3) / 4);
    L.flag = o; o += 2;
    L.total = o;
    return L;
}

struct Member : ConelpMem {                   // N = ml + sum m_k^2
    int ml, ns, Nd, Np;
    double *tw, *th, *r, *rti, *lm, *d, *di, *sgs, *sgz, *wa, *wb, *wc, *wd, *nrm;
    int *bo, *bl;                             // bo[k]: the first row of block k; bl[k]: the first entry of lmbda_k; [ns]: N, Nd
    int *flag;
    const unsigned short *prow, *pmir;
    __device__ __forceinline__ int first_s() const { return ml; }
    __device__ int order(int k) const { return bl[k + 1] - bl[k]; }
};

#include "batch_cone_s.hpp"

// out := W in, W'in, W^-1 in or W^-T in (misc_solvers.c:85-240); in == out is allowed.  Barriers before (the caller's) and after.
__device__ __forceinline__ void wscale(const Member &M, const double *in, double *out, bool inv, bool trans)
{
    for (int k = threadIdx.x; k < M.ml; k += NT) out[k] = (inv ? M.di[k] : M.d[k]) * in[k];
    blocks_congr(M, inv ? M.rti : M.r, inv != trans ? 1 : 0, in, out);
    __syncthreads();
}

// The lower triangle of S = Gs'Gs [+ A'A], Gs = W^-T G packed, in LDS.  Barriers before (the caller's) and after.
__device__ __forceinline__ void assemble(const Member &M, bool sing)
{
    const int tid = threadIdx.x, n = M.n, ml = M.ml, N = M.N, ldn = M.ldn;
    kkt_s_init(M, sing);
    int fill = 0;                                          // staged rows not yet added to S
    const auto flush = [&]() {                             // S += T'T over the staged rows; the rows are free afterwards
        __syncthreads();
        kkt_s_add_rows(M, fill);
        __syncthreads();
        fill = 0;
    };
    for (int k0 = 0; k0 < ml; k0 += SDPB_TILE) {
        const int kt = min((int)SDPB_TILE, ml - k0);
        orth_stage<SDPB_TILE>(M, M.G, N, M.di, k0, kt);
        fill = kt;
        if (fill == SDPB_TILE) flush();
    }
    double *w = M.T + SDPB_TILE * ldn;
    for (int k = 0; k < M.ns; k++) {
        const int o = M.bo[k], m = M.order(k);
        const double *rti = M.rti + (o - ml);
        for (int b = 0; b < m; b++) {
            if (fill + m - b > SDPB_TILE) flush();
            for (int e = tid; e < m * n; e += NT) {        // w(u, col) = sum_v mat(G_k col)(u, v) rti(v, b), the lower triangle read
                const int u = e % m, col = e / m;
                const double *g = M.G + o + (int64_t)col * N;
                double acc = 0.0;
                for (int v = 0; v < m; v++) acc = fma(u >= v ? g[u + v * m] : g[v + u * m], rti[v + b * m], acc);
                w[u * ldn + col] = acc;
            }
            __syncthreads();
            for (int e = tid; e < (m - b) * n; e += NT) {
                const int a = b + e % (m - b), col = e / (m - b);
                double acc = 0.0;
                for (int u = 0; u < m; u++) acc = fma(rti[u + a * m], w[u * ldn + col], acc);
                M.T[(fill + a - b) * ldn + col] = a == b ? acc : acc * RT2;
            }
            fill += m - b;
            __syncthreads();                               // w is free for the next block column
        }
    }
    if (fill) flush();
    __syncthreads();
}

struct Cone {                                 // the cone of conelp_member: the orthant for the 'l' rows, the code here for 's'
    const Member &M;

    __device__ __forceinline__ int lmbda_len() const { return M.Nd; }
    template <class F>
    __device__ __forceinline__ void for_rows(F f) const
    {
        for (int q = threadIdx.x; q < M.Np; q += NT) f(PackedRow{M.prow[q], M.pmir[q], weight(M, q)});
    }
    __device__ __forceinline__ void load_h(double *out) const { load_sym(M, M.h, out); }
    __device__ __forceinline__ void start() const                                   // d = di = 1, r_k = rti_k = I
    {
        const int tid = threadIdx.x, ml = M.ml, N = M.N;
        for (int k = tid; k < ml; k += NT) { M.d[k] = 1.0; M.di[k] = 1.0; }
        for (int k = tid; k < N; k += NT) M.z[k] = 0.0;
        blocks_identity(M);
        __syncthreads();
        load_sym(M, M.h, M.s);
        __syncthreads();
    }
    __device__ __forceinline__ void max_step(const double *u0, double a0, const double *u1, double a1, double (&mx)[2]) const
    {
        orth_max_step(M.ml, u0, a0, u1, a1, mx);
        blk_reduce<2, true>(mx, M.red);
        blocks_max_step(M, u0, a0, u1, a1, mx);
    }
    __device__ __forceinline__ void push(bool ps, bool pz, const double (&mx)[2]) const
    {
        orth_push(M.ml, ps, pz, mx, M.s, M.z);
        blocks_push(M, ps, pz, mx);
    }
    __device__ __forceinline__ bool first_scaling() const                           // misc.py:284-419
    {
        orth_first_scaling(M.ml, M.s, M.z, M.d, M.di, M.lm);
        return blocks_scaling(M);
    }
    __device__ __forceinline__ double lam_sq() const { return sum_sq(M.lm, M.Nd, M.red); }
    __device__ __forceinline__ void prepare() const                                 // th = W^-T h
    {
        load_sym(M, M.h, M.th);
        __syncthreads();
        wscale(M, M.th, M.th, true, true);
    }
    __device__ __forceinline__ void assemble(bool sing) const { kvx::assemble(M, sing); }
    __device__ __forceinline__ void kkt_before(double *vx, double *vz) const
    {
        wscale(M, vz, vz, true, true);                                                         // z := W^-T bz
        wscale(M, vz, M.tw, true, false);
        gemv_t_packed(M, M.tw, 1.0, vx);                                                       // x += G' W^-1 z
        __syncthreads();
    }
    __device__ __forceinline__ void kkt_after(double *vx, double *vz) const
    {
        const int tid = threadIdx.x, n = M.n, N = M.N;
        for (int q = tid; q < M.Np; q += NT) {
            const double t = row_dot(M.G, N, n, M.prow[q], vx);
            M.tw[M.prow[q]] = t; M.tw[M.pmir[q]] = t;
        }
        __syncthreads();
        wscale(M, M.tw, M.tw, true, true);
        for (int k = tid; k < N; k += NT) vz[k] = M.tw[k] - vz[k];                             // W uz = W^-T G ux - W^-T bz
        __syncthreads();
    }
    __device__ __forceinline__ void gemv_t(const double *u, double sign, double *v) const { gemv_t_packed(M, u, sign, v); }
    __device__ __forceinline__ void rhs(int i, double sigma, double mu) const
    {
        const int tid = threadIdx.x, N = M.N;
        orth_rhs<false>(M.ml, i, sigma, mu, M.lm, M.ws3, M.d, M.rz, M.ds, M.dz);
        blocks_sinv(M, i, sigma, mu);
        __syncthreads();
        wscale(M, M.ds, M.tw, false, true);
        for (int k = tid; k < N; k += NT) M.dz[k] = -((1.0 - sigma) * M.rz[k] + M.tw[k]);
    }
    __device__ __forceinline__ double th_dot(const double *dz) const
    {
        double acc = 0.0;
        for (int q = threadIdx.x; q < M.Np; q += NT) acc += weight(M, q) * (M.th[M.prow[q]] * dz[M.prow[q]]);
        return acc;
    }
    __device__ __forceinline__ void combine(int i, double dtau, double (&mx)[2]) const
    {
        const int tid = threadIdx.x, ml = M.ml, N = M.N;
        orth_combine(ml, i, dtau, M.lm, M.z1, M.ds, M.dz, M.ws3, mx);
        for (int k = ml + tid; k < N; k += NT) {
            const double zk = M.dz[k] + dtau * M.z1[k];
            M.dz[k] = zk; M.ds[k] -= zk;
        }
        blk_reduce<2, true>(mx, M.red);                // its barriers also publish ds and dz
        blocks_combine(M, i == 0, mx);
    }
    __device__ __forceinline__ void update(double step) const                       // misc.py:444-634; s = W'lmbda and z = W^-1 lmbda
    {
        orth_update(M.ml, step, M.ds, M.dz, M.d, M.di, M.lm, M.s, M.z);
        blocks_update(M, step);
    }
};

__global__ void __launch_bounds__(SDPB_THREADS) k_sdp_batch(SdpBatchArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, ml = a.ml, ns = a.ns;
    const Layout L = layout(a.n, ml, a.N, a.Nd, a.Np, ns, a.p);
    Member M;
    conelp_data(M, a, a.N);
    M.ml = ml; M.ns = ns; M.Nd = a.Nd; M.Np = a.Np; M.ldn = L.ldn; M.ldp = L.ldp;
    M.S = lds + L.S; M.T = lds + L.XK; M.X = lds + L.X; M.K = lds + L.K;
    M.x = lds + L.x; M.dx = lds + L.dx; M.rx = lds + L.rx; M.x1 = lds + L.x1;
    M.y = lds + L.y; M.dy = lds + L.dy; M.ry = lds + L.ry; M.y1 = lds + L.y1;
    M.s = lds + L.s; M.z = lds + L.z; M.ds = lds + L.ds; M.dz = lds + L.dz; M.rz = lds + L.rz; M.ws3 = lds + L.ws3;
    M.z1 = lds + L.z1; M.tw = lds + L.tw; M.th = lds + L.th; M.r = lds + L.r; M.rti = lds + L.rti;
    M.lm = lds + L.lm; M.d = lds + L.d; M.di = lds + L.di; M.sgs = lds + L.sgs; M.sgz = lds + L.sgz;
    M.wa = lds + L.wk; M.wb = M.wa + MM; M.wc = M.wb + MM; M.wd = M.wc + MM; M.nrm = lds + L.nrm;
    M.red = lds + L.red;
    M.bo = reinterpret_cast<int *>(lds + L.blk); M.bl = M.bo + (ns + 1);
    M.flag = reinterpret_cast<int *>(lds + L.flag);
    unsigned short *prow = reinterpret_cast<unsigned short *>(lds + L.prow), *pmir = reinterpret_cast<unsigned short *>(lds + L.pmir);
    M.prow = prow; M.pmir = pmir;

    // ---- the cone: the first row and the first lmbda of every block, the packed rows and their mirror images
    if (tid <= ns) {
        int o = ml, ol = ml;
        for (int k = 0; k < tid; k++) { o += a.m[k] * a.m[k]; ol += a.m[k]; }
        M.bo[tid] = o; M.bl[tid] = ol;
    }
    for (int k = tid; k < ml; k += NT) { prow[k] = (unsigned short)k; pmir[k] = (unsigned short)k; }
    __syncthreads();
    {
        int po = ml;
        for (int k = 0; k < ns; k++) {
            const int o = M.bo[k], m = M.order(k);
            for (int e = tid; e < m * m; e += NT) {
                const int i = e % m, j = e / m;
                if (i < j) continue;
                const int q = po + j * m - (j * (j - 1)) / 2 + (i - j);
                prow[q] = (unsigned short)(o + i + j * m);
                pmir[q] = (unsigned short)(o + j + i * m);
            }
            po += (m * (m + 1)) / 2;
        }
    }
    __syncthreads();
    conelp_member(Cone{M}, a);
}

}  // namespace

size_t sdp_batch_lds_bytes(int n, int ml, int ns, const unsigned char *m, int p)
{
    int N = ml, Nd = ml, Np = ml;
    for (int k = 0; k < ns; k++) { N += m[k] * m[k]; Nd += m[k]; Np += (m[k] * (m[k] + 1)) / 2; }
    return (size_t)layout(n, ml, N, Nd, Np, ns, p).total * sizeof(double);
}

hipError_t launch_sdp_batch(hipStream_t st, const SdpBatchArgs &a)
{
    // per device, so asked of the current one at every launch
    const hipError_t e = hipFuncSetAttribute((const void *)k_sdp_batch, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    k_sdp_batch<<<dim3((unsigned)a.B), dim3(SDPB_THREADS), sdp_batch_lds_bytes(a.n, a.ml, a.ns, a.m, a.p), st>>>(a);
    return hipGetLastError();
}

}  // namespace kvx
