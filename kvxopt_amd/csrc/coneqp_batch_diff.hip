// k_coneqp_batch_diff: one workgroup (256 threads, four wavefronts) differentiates one solved member of coneqp_batch
// (coneqp_batch_diff.hpp).  It runs on the cone code k_coneqp_batch carries (batch_cone.hpp, included below into this file's
// anonymous namespace) in three parts:
//
//   the point     x, y, s, z of the solution into LDS, the Nesterov-Todd scaling from s and z (Cone::first_scaling), mu = s'z / degree
//   centring      at most `centering` times, while |lmbda o lmbda - mu e|_2 > centol mu: the residuals rx, ry, rz as coneqp_member
//                 (batch_coneqp.hpp) forms them, coneqp_factor, the direction of coneqp_member with sigma = 1 and no Mehrotra term
//                 (rhs_qp(false, mu), conelp_kkt_solve, combine_qp), the step min(1, 0.99 / t), Cone::update
//   the system    coneqp_factor at the centred point, the right-hand side of the mode, conelp_kkt_solve, uz = W^-1 (W uz), and
//                 `refinement` times the residual of the full 3 x 3 system in float64 -- W'W uz by wscale twice, P, G, A from HBM --
//                 and a solve with the same factors (the scheme of qp_batch_diff.hip)
//
// LDS: the layout of k_coneqp_batch (batch_coneqp_layout.hpp) and one more n-vector and p-vector for the kept right-hand side.
// After centring s, ds, dz, ws3, dx, dy are dead: bz, uz, W'W uz, ux, uy live there.
//
// The rules of the family hold.  Sums have the fixed order of batch_device.hpp; the centrality measure is a block reduction over
// lm in that order.  No atomics; a member's bytes depend on nothing but its own data.  Every loop is bounded by `centering`,
// `refinement`, n, N, p, nq, ns, q_k, m_k or CONEB_SWEEPS.  Every branch around a barrier is taken on values all threads hold alike:
// reduced values, or a word of HBM all threads read.  A NaN or Inf ends in exit 2 through the test of the scaling or a pivot
// test, or makes the comparison with centol false until the cap: exit 3.
#include "coneqp_batch_diff.hpp"
#include "batch_coneqp.hpp"
#include "batch_diff_device.hpp"

#include <cmath>

namespace kvx {
namespace {

using namespace batchdev;
static_assert(NT == CONEB_THREADS, "the shared helpers are written for the workgroup of k_coneqp_batch");
static_assert(CONEB_MAX_M * CONEB_MAX_M <= NT, "a thread per entry of a block");
#include "batch_cone.hpp"
#include "batch_coneqp_layout.hpp"

struct DiffLayout {                           // QpLayout and the right-hand side kept for the refinement
    QpLayout q;
    int bx, by, total;
};

__host__ __device__ inline DiffLayout diff_layout(int n, int ml, int Ms, int N, int Nd, int Np, int nq, int ns, int p)
{
    DiffLayout L;
    L.q = qp_layout(n, ml, Ms, N, Nd, Np, nq, ns, p);
    int o = L.q.total;
    L.bx = o; o += even(n);
    L.by = o; o += even(p);
    L.total = o;
    return L;
}

// v[c] += sign * sum over the packed rows j of D(row_j, c) weight_j u[row_j] for a matrix D (N x n in HBM) that is not the
// member's G: gemv_t_packed on the lower triangles of a perturbation.  The caller's barriers stand before and after.
__device__ __forceinline__ void gemv_t_packed_of(const Member &M, const double *__restrict__ D, const double *u, double sign, double *v)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c = w; c < M.n; c += NW) {
        double acc = 0.0;
        for (int j = lane; j < M.Np; j += 64) { const int r = M.prow[j]; acc += D[r + (int64_t)c * M.N] * (weight(M, j) * u[r]); }
        acc = wave_sum(acc);
        if (lane == 0) v[c] += sign * acc;
    }
}

// |lmbda o lmbda - mu e|_2 / mu in every thread: the Jordan product on the 'l' rows and the 'q' cones (head lmbda'lmbda - mu,
// tail 2 lmbda_0 lmbda_1), lmbda_k^2 - mu on the diagonal of an 's' block.  Barriers inside (blk_reduce).
__device__ __forceinline__ double centrality(const Member &M, double mu)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double acc[1] = {0.0};
    for (int k = tid; k < M.Nd; k += NT) {
        if (k >= M.ml && k < M.Ms) continue;
        const double t = M.lm[k] * M.lm[k] - mu;
        acc[0] += t * t;
    }
    for (int c = wv; c < M.nq; c += NW) {
        const int o = M.off[c], m = M.off[c + 1] - o;
        const double *lm = M.lm + o;
        const double l0 = lm[0];
        double q[2];                               // lmbda'lmbda, the squared norm of the tail 2 lmbda_0 lmbda_1
        cone_sum<2>(m, q, [&](int j, double (&q)[2]) {
            q[0] += lm[j] * lm[j];
            if (j) { const double t = 2.0 * l0 * lm[j]; q[1] += t * t; }
        });
        if (lane == 0) { const double t = q[0] - mu; acc[0] += t * t + q[1]; }
    }
    blk_reduce<1, false>(acc, M.red);
    return sqrt(acc[0]) / mu;
}

// (vx, vy, vz) := K^-1 (vx, vy, vz) with K = [P A' G'; A 0 0; G 0 -W'W] by the factors in LDS: conelp_kkt_solve leaves W uz.
// Barriers before (the caller's) and after.
__device__ __forceinline__ void kkt_solve(const Cone &C, double *vx, double *vy, double *vz)
{
    conelp_kkt_solve(C, false, vx, vy, vz);
    wscale(C.M, vz, vz, true, false);
}

__global__ void __launch_bounds__(CONEB_THREADS) k_coneqp_batch_diff(ConeqpDiffArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, n = a.n, N = a.N, p = a.p, ml = a.ml, nq = a.nq, ns = a.ns, Ms = a.Ms;
    const int64_t bm = blockIdx.x;
    const bool jvp = a.mode == QPD_JVP;
    const DiffLayout DL = diff_layout(n, ml, Ms, N, a.Nd, a.Np, nq, ns, p);
    const QpLayout &L = DL.q;
    Member M;
    conelp_data(M, a, N);
    M.P = a.P + bm * a.sP;
    M.ml = ml; M.nq = nq; M.ns = ns; M.Ms = Ms; M.Nd = a.Nd; M.Np = a.Np; M.ldn = L.ldn; M.ldp = L.ldp;
    M.S = lds + L.S; M.T = lds + L.XK; M.X = lds + L.X; M.K = lds + L.K; M.w = lds + L.w; M.g = lds + L.g;
    M.x = lds + L.x; M.dx = lds + L.dx; M.rx = lds + L.rx; M.y = lds + L.y; M.dy = lds + L.dy; M.ry = lds + L.ry;
    M.x1 = nullptr; M.y1 = nullptr; M.z1 = nullptr; M.th = nullptr;      // conelp's; nothing called here reads them
    M.s = lds + L.s; M.z = lds + L.z; M.ds = lds + L.ds; M.dz = lds + L.dz; M.rz = lds + L.rz; M.ws3 = lds + L.ws3;
    M.tw = lds + L.tw; M.r = lds + L.r; M.rti = lds + L.rti;
    M.lm = lds + L.lm; M.d = lds + L.d; M.di = lds + L.di; M.beta = lds + L.beta; M.sgs = lds + L.sgs; M.sgz = lds + L.sgz;
    M.wa = lds + L.wk; M.wb = M.wa + MM; M.wc = M.wb + MM; M.wd = M.wc + MM; M.nrm = lds + L.nrm;
    M.red = lds + L.red;
    M.off = reinterpret_cast<int *>(lds + L.off);
    M.cone = reinterpret_cast<unsigned short *>(lds + L.cone);
    M.bo = reinterpret_cast<int *>(lds + L.blk); M.bl = M.bo + (ns + 1);
    M.flag = reinterpret_cast<int *>(lds + L.flag);
    unsigned short *prow = reinterpret_cast<unsigned short *>(lds + L.prow), *pmir = reinterpret_cast<unsigned short *>(lds + L.pmir);
    M.prow = prow; M.pmir = pmir;
    // what the derivative keeps where the centring steps had their work vectors
    double *bx = lds + DL.bx, *by = lds + DL.by, *bz = M.ds, *ux = M.dx, *uy = M.dy, *uz = M.dz, *wz = M.ws3;
    const Cone C{M};

    double *uxo = a.ux + bm * n, *uyo = p ? a.uy + bm * p : nullptr, *uzo = a.uz + bm * N, *uso = jvp ? a.us + bm * N : nullptr;
    double *gP = !jvp && a.gP && a.sP ? a.gP + bm * n * n : nullptr, *gG = !jvp && a.gG && a.sG ? a.gG + bm * N * n : nullptr;
    double *gA = !jvp && p && a.gA && a.sA ? a.gA + bm * p * n : nullptr;

    int code = a.solexit[bm] != 0 ? CQD_SKIPPED : CQD_DONE;              // one word of HBM, the same for every thread
    int steps = 0;
    double cen = NAN;

    if (code == CQD_DONE) {
        // ---- the point and its scaling (misc.compute_scaling); the 'l' rows positive and finite, every part of W finite
        cone_tables(M, a, prow, pmir);
        const double *xs = a.x + bm * n, *ys = p ? a.y + bm * p : nullptr, *ss = a.s + bm * N, *zs = a.z + bm * N;
        double bad[1] = {0.0};
        if (tid < n) M.x[tid] = xs[tid];
        if (tid < p) M.y[tid] = ys[tid];
        for (int k = tid; k < N; k += NT) {
            const double sk = ss[k], zk = zs[k];
            if (k < ml && !(sk > 0.0 && sk < INFINITY && zk > 0.0 && zk < INFINITY)) bad[0] = 1.0;
            M.s[k] = sk; M.z[k] = zk;
        }
        blk_reduce<1, true>(bad, M.red);                   // its barriers also publish x, y, s, z
        if (bad[0] != 0.0 || !C.first_scaling()) code = CQD_FAILED;
    }
    double mu = NAN;
    if (code == CQD_DONE) {
        __syncthreads();
        double nf[1] = {0.0}, g[1] = {0.0};                // a part of W that is not finite; s'z
        const auto test = [&](const double *u, int len) {
            for (int k = tid; k < len; k += NT)
                if (!(fabs(u[k]) < INFINITY)) nf[0] = 1.0;
        };
        test(M.lm, a.Nd); test(M.d, Ms); test(M.di, ml); test(M.beta, nq); test(M.r, N - Ms); test(M.rti, N - Ms);
        C.for_rows([&](auto row) { g[0] += row.w(M.s[row.k] * M.z[row.k]); });
        blk_reduce<1, true>(nf, M.red);
        blk_reduce<1, false>(g, M.red);
        if (nf[0] != 0.0) code = CQD_FAILED;
        mu = g[0] / C.degree();
    }

    // ---- centring: Newton steps of coneqp with sigma = 1, no Mehrotra term and mu fixed
    if (code == CQD_DONE) {
        cen = centrality(M, mu);
        while (steps < a.centering && !(cen <= a.centol)) {
            // residuals (coneprog.py:2167-2203): rx = P x + q + A'y + G'z, ry = A x - b, rz = s + G x - h
            if (tid < n) M.rx[tid] = sym_row_dot(M.P, n, tid, M.x) + M.c[tid];
            if (tid < p) M.ry[tid] = row_dot(M.A, p, n, tid, M.x) - M.b[tid];
            C.for_rows([&](auto row) {
                const int k = row.k;
                row.put(M.rz, (M.s[k] - M.h[k]) + row_dot(M.G, N, n, k, M.x));
            });
            __syncthreads();
            if (p > 0) gemv_t_add(M.A, p, n, M.y, nullptr, 1.0, M.rx);
            __syncthreads();
            C.gemv_t(M.z, 1.0, M.rx);
            __syncthreads();
            if (!coneqp_factor(C)) { code = CQD_FAILED; break; }
            C.rhs_qp(false, mu);
            if (tid < n) M.dx[tid] = -M.rx[tid];
            if (tid < p) M.dy[tid] = -M.ry[tid];
            __syncthreads();
            conelp_kkt_solve(C, false, M.dx, M.dy, M.dz);
            double dsdz = 0.0, mx[2] = {-INFINITY, -INFINITY};
            C.combine_qp(false, dsdz, mx);
            const double t = fmax(0.0, fmax(mx[0], mx[1]));
            const double step = t == 0.0 ? 1.0 : fmin(1.0, 0.99 / t);
            if (tid < n) M.x[tid] += step * M.dx[tid];
            if (tid < p) M.y[tid] += step * M.dy[tid];
            C.update(step);
            __syncthreads();
            steps++;
            cen = centrality(M, mu);                       // its barriers also publish x, y, s, z
        }
        if (code == CQD_DONE && a.centering > 0 && !(cen <= a.centol)) code = CQD_NOT_CENTRED;
    }
    if (code == CQD_DONE) {
        __syncthreads();
        if (!coneqp_factor(C)) code = CQD_FAILED;
    }

    if (code != CQD_DONE) {
        __syncthreads();
        for (int k = tid; k < N; k += NT) { uzo[k] = 0.0; if (jvp) uso[k] = 0.0; if (a.zc) a.zc[bm * N + k] = 0.0; }
        if (tid < n) { uxo[tid] = 0.0; if (a.xc) a.xc[bm * n + tid] = 0.0; }
        if (tid < p) { uyo[tid] = 0.0; if (a.yc) a.yc[bm * p + tid] = 0.0; }
        if (gP) for (int e = tid; e < n * n; e += NT) gP[e] = 0.0;
        if (gG) for (int e = tid; e < N * n; e += NT) gG[e] = 0.0;
        if (gA) for (int e = tid; e < p * n; e += NT) gA[e] = 0.0;
        if (tid == 0) {
            a.exitc[bm] = code;
            a.centrality[bm] = code == CQD_NOT_CENTRED ? cen : NAN;
            a.steps[bm] = steps;
        }
        return;
    }

    // ---- the right-hand side at the centred x, y, z, kept in bx, by, bz for the refinement
    if (!jvp) {
        if (tid < n) bx[tid] = -a.gx[bm * n + tid];
        if (tid < p) by[tid] = 0.0;
        for (int k = tid; k < N; k += NT) bz[k] = 0.0;
    } else {
        const double *dP = a.dP ? a.dP + bm * a.sdP : nullptr, *dq = a.dq ? a.dq + bm * a.sdq : nullptr;
        const double *dG = a.dG ? a.dG + bm * a.sdG : nullptr, *dh = a.dh ? a.dh + bm * a.sdh : nullptr;
        const double *dA = p && a.dA ? a.dA + bm * a.sdA : nullptr, *db = p && a.db ? a.db + bm * a.sdb : nullptr;
        if (tid < n) bx[tid] = -((dP ? sym_row_dot(dP, n, tid, M.x) : 0.0) + (dq ? dq[tid] : 0.0));
        if (tid < p) by[tid] = (db ? db[tid] : 0.0) - (dA ? row_dot(dA, p, n, tid, M.x) : 0.0);
        C.for_rows([&](auto row) {                         // the lower triangles of dG and dh, mirrored
            const int k = row.k;
            row.put(bz, (dh ? dh[k] : 0.0) - (dG ? row_dot(dG, N, n, k, M.x) : 0.0));
        });
        __syncthreads();
        if (dG) gemv_t_packed_of(M, dG, M.z, -1.0, bx);
        __syncthreads();
        if (dA) gemv_t_add(dA, p, n, M.y, nullptr, -1.0, bx);
    }
    __syncthreads();

    // ---- u = K^-1 b, then `refinement` times u += K^-1 (b - K u)
    if (tid < n) ux[tid] = bx[tid];
    if (tid < p) uy[tid] = by[tid];
    for (int k = tid; k < N; k += NT) uz[k] = bz[k];
    __syncthreads();
    kkt_solve(C, ux, uy, uz);
    for (int it = 0; it < a.refinement; it++) {
        wscale(M, uz, wz, false, false);
        wscale(M, wz, wz, false, true);                    // W'W uz
        if (tid < n) M.rx[tid] = bx[tid] - sym_row_dot(M.P, n, tid, ux);
        if (tid < p) M.ry[tid] = by[tid] - row_dot(M.A, p, n, tid, ux);
        C.for_rows([&](auto row) {
            const int k = row.k;
            row.put(M.rz, bz[k] - (row_dot(M.G, N, n, k, ux) - wz[k]));
        });
        __syncthreads();
        if (p > 0) gemv_t_add(M.A, p, n, uy, nullptr, -1.0, M.rx);
        __syncthreads();
        C.gemv_t(uz, -1.0, M.rx);
        __syncthreads();
        kkt_solve(C, M.rx, M.ry, M.rz);
        if (tid < n) ux[tid] += M.rx[tid];
        if (tid < p) uy[tid] += M.ry[tid];
        for (int k = tid; k < N; k += NT) uz[k] += M.rz[k];
        __syncthreads();
    }
    // ds = -W'W dz by the third block row, G dx - W'W dz = bz: in W'W dz the rows that are not active multiply an entry of dz that
    // is the small difference of large numbers by a large one, and lose what the solve had gained
    if (jvp) {
        C.for_rows([&](auto row) {
            const int k = row.k;
            row.put(wz, bz[k] - row_dot(M.G, N, n, k, ux));
        });
        __syncthreads();
    }

    // ---- the member's result
    if (tid < n) { uxo[tid] = ux[tid]; if (a.xc) a.xc[bm * n + tid] = M.x[tid]; }
    if (tid < p) { uyo[tid] = uy[tid]; if (a.yc) a.yc[bm * p + tid] = M.y[tid]; }
    for (int k = tid; k < N; k += NT) {
        uzo[k] = uz[k];
        if (jvp) uso[k] = wz[k];
        if (a.zc) a.zc[bm * N + k] = M.z[k];
    }
    // Entries (i, j) and (j, i) of gP evaluate one expression, so gP is symmetric to the last bit; so are the 's' blocks of gG in
    // their rows, since z and uz are symmetric to the bit.
    if (gP)
        for (int e = tid; e < n * n; e += NT) {
            const int c = e / n, r = e - c * n, i = max(r, c), j = min(r, c);
            gP[e] = 0.5 * (ux[i] * M.x[j] + M.x[i] * ux[j]);
        }
    if (gG)
        for (int e = tid; e < N * n; e += NT) {
            const int c = e / N, k = e - c * N;
            gG[e] = uz[k] * M.x[c] + M.z[k] * ux[c];
        }
    if (gA)
        for (int e = tid; e < p * n; e += NT) {
            const int c = e / p, r = e - c * p;
            gA[e] = uy[r] * M.x[c] + M.y[r] * ux[c];
        }
    if (tid == 0) {
        a.exitc[bm] = CQD_DONE;
        a.centrality[bm] = cen;
        a.steps[bm] = steps;
    }
}

}  // namespace

size_t coneqp_batch_diff_lds_bytes(int n, int ml, int nq, const unsigned short *q, int ns, const unsigned char *m, int p)
{
    const Sizes z = sizes(ml, nq, q, ns, m);
    return (size_t)diff_layout(n, ml, z.Ms, z.N, z.Nd, z.Np, nq, ns, p).total * sizeof(double);
}

hipError_t launch_coneqp_batch_diff(hipStream_t st, const ConeqpDiffArgs &a)
{
    // per device, so asked of the current one at every launch
    const hipError_t e = hipFuncSetAttribute((const void *)k_coneqp_batch_diff, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    k_coneqp_batch_diff<<<dim3((unsigned)a.B), dim3(CONEB_THREADS), coneqp_batch_diff_lds_bytes(a.n, a.ml, a.nq, a.q, a.ns, a.m, a.p), st>>>(a);
    return hipGetLastError();
}

}  // namespace kvx
