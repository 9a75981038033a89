// The cone K = R^ml_+ x Q^{q_0} x ... x S^{m_0}_+ x ... as k_conelp_batch (conelp_batch.hip) and k_coneqp_batch
// (coneqp_batch.hip) carry it: the rows of a member and their tables, the 'q' operations, the 's' operations, W and its
// inverses, the assembly of S over staged rows of W^-T G, and the policy `Cone` through which conelp_member (batch_conelp.hpp)
// and coneqp_member (batch_coneqp.hpp) reach all of it.  conelp_batch.hip has the description of the rows and of the work.
//
// This file is text of its includer: it is included once, inside the anonymous namespace of kvx, after `using namespace
// batchdev` and the includer's static_asserts on CONEB_THREADS, so every kernel keeps its own internal copy of these functions.
// It needs conelp_batch.hpp (the CONEB_ limits), batch_conelp.hpp and <cmath>.  The 'q' and the 's' operations themselves are
// batch_cone_q.hpp and batch_cone_s.hpp, included below and shared with k_socp_batch and k_sdp_batch: what
// stands here is the layout, the member, W on the whole cone, the assembly of S, the policy and the tables.
//
// What only coneqp needs is marked "coneqp" and is not instantiated by conelp_member: Member::P, cones_rhs_qp and
// cones_combine_qp (batch_cone_q.hpp), and Cone::degree, assemble_qp, rhs_qp, combine_qp.
constexpr int MAX_M = CONEB_MAX_M, SWEEPS = CONEB_SWEEPS;    // what batch_cone_s.hpp asks of its includer
constexpr int MM = MAX_M * MAX_M;
constexpr int RING = CONEB_TILE + 1;          // a tile meets at most 32 cones, one of them begun in an earlier tile
constexpr double RT2 = 1.41421356237309504880;

struct Layout {                               // offsets in doubles from the LDS base; every part starts on 16 bytes
    int ldn, ldp;
    int S, XK, X, K, w, g, x, dx, rx, x1, y, dy, ry, y1, s, z, ds, dz, rz, ws3, z1, tw, th, r, rti, lm, d, di, beta, sgs, sgz, wk, nrm,
        red, off, blk, cone, prow, pmir, flag, total;
};

// Ms: the first 's' row, ml + sum q_k
__host__ __device__ inline Layout layout(int n, int ml, int Ms, int N, int Nd, int Np, int nq, int ns, int p)
{
    Layout L;
    L.ldn = n | 1;
    L.ldp = p | 1;
    int o = 0;
    L.S = o; o += even(n * L.ldn);
    const int xsz = even(p * L.ldn), ksz = even(p * L.ldp), tsz = even(CONEB_TILE * L.ldn), wsz = ns ? even(CONEB_MAX_M * L.ldn) : 0,
              gsz = nq ? even(RING * L.ldn) : 0;
    L.XK = L.X = o; L.K = o + xsz; L.w = o + tsz; L.g = o + tsz + wsz;
    o += (xsz + ksz > tsz + wsz + gsz ? xsz + ksz : tsz + wsz + gsz);
    const int nv = even(n), pv = even(p), mv = even(N), sv = even(N - Ms), lv = even(ml), cv = even(Ms), dv = even(Nd), ev = even(Nd - Ms);
    L.x = o; o += nv; L.dx = o; o += nv; L.rx = o; o += nv; L.x1 = o; o += nv;
    L.y = o; o += pv; L.dy = o; o += pv; L.ry = o; o += pv; L.y1 = o; o += pv;
    L.s = o; o += mv; L.z = o; o += mv; L.ds = o; o += mv; L.dz = o; o += mv; L.rz = o; o += mv; L.ws3 = o; o += mv;
    L.z1 = o; o += mv; L.tw = o; o += mv; L.th = o; o += mv;
    L.r = o; o += sv; L.rti = o; o += sv;
    L.lm = o; o += dv; L.d = o; o += cv; L.di = o; o += lv; L.beta = o; o += even(nq); L.sgs = o; o += ev; L.sgz = o; o += ev;
    L.wk = o; o += ns ? 4 * MM : 0;
    L.nrm = o; o += ns ? 2 * CONEB_MAX_M : 0;
    L.red = o; o += NW * NRED;
    L.off = o; o += even((nq + 2) / 2);                    // nq + 1 ints
    L.blk = o; o += even(ns + 1);                          // 2 (ns + 1) ints
    L.cone = o; o += even((Ms - ml + 3) / 4);              // sum q_k unsigned shorts
    L.prow = o; o += even((Np + 3) / 4);                   // Np unsigned shorts
    L.pmir = o; o += even((Np + 3) / 4);
    L.flag = o; o += 2;
    L.total = o;
    return L;
}

struct Member : ConelpMem {                   // N = ml + sum q_k + sum m_k^2
    int ml, nq, ns, Ms, Nd, Np;
    double *w, *g, *tw, *th, *r, *rti, *lm, *d, *di, *beta, *sgs, *sgz, *wa, *wb, *wc, *wd, *nrm;
    int *off;                                 // off[k]: the first row of cone k; off[nq] = Ms
    unsigned short *cone;                     // cone[r - ml]: the cone of the 'q' row r
    int *bo, *bl;                             // bo[k]: the first row of block k; bl[k]: the first entry of lmbda_k; [ns]: N, Nd
    int *flag;
    const unsigned short *prow, *pmir;
    __device__ __forceinline__ int first_s() const { return Ms; }
    __device__ __forceinline__ int order(int k) const { return bl[k + 1] - bl[k]; }
    const double *P;                          // coneqp: n x n in HBM, column-major, its lower triangle read; c is q
};

#include "batch_cone_q.hpp"                   // the 'q' cones: d holds v_k in the 'q' rows, lm lmbda_k in the same rows
#include "batch_cone_s.hpp"                   // the 's' blocks

// ================================================================================================================ the whole cone

// out := W in, W'in, W^-1 in or W^-T in (misc_solvers.c:85-240); in == out is allowed.  Barriers before (the caller's) and after.
__device__ __forceinline__ void wscale(const Member &M, const double *in, double *out, bool inv, bool trans)
{
    for (int k = threadIdx.x; k < M.ml; k += NT) out[k] = (inv ? M.di[k] : M.d[k]) * in[k];
    if (inv) cones_wscale<true>(M, in, out);
    else cones_wscale<false>(M, in, out);
    blocks_congr(M, inv ? M.rti : M.r, inv != trans ? 1 : 0, in, out);
    __syncthreads();
}

// The lower triangle of S = S0 + Gs'Gs, Gs = W^-T G packed, in LDS; start() writes the lower triangle of S0 and has no barrier.
// Barriers before (the caller's) and after.
template <class Start>
__device__ __forceinline__ void assemble_from(const Member &M, Start start)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = M.n, ml = M.ml, Ms = M.Ms, N = M.N, nq = M.nq, ldn = M.ldn;
    start();
    int fill = 0;                                          // staged rows not yet added to S
    const auto flush = [&]() {                             // S += T'T over the staged rows; the rows are free afterwards
        __syncthreads();
        kkt_s_add_rows(M, fill);
        __syncthreads();
        fill = 0;
    };
    // ---- the 'l' and 'q' rows, in tiles of 32 from row 0
    for (int k0 = 0; k0 < Ms; k0 += CONEB_TILE) {
        const int kt = min((int)CONEB_TILE, Ms - k0), k1 = k0 + kt;
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
            if (m > CONEB_SERIAL) continue;
            double acc = 0.0;
            for (int i = 0; i < m; i++) acc += jsign(i, M.d[o + i]) * M.G[o + i + (int64_t)col * N];
            M.g[(c % RING) * ldn + col] = acc;
        }
        for (int e = wv; e < pairs; e += NW) {             // a larger one: a wavefront
            const int c = cf + e / n, col = e - (c - cf) * n, o = M.off[c], m = M.off[c + 1] - o;
            if (m <= CONEB_SERIAL) continue;
            double r[1];
            cone_sum<1>(m, r, [&](int i, double (&r)[1]) { r[0] += jsign(i, M.d[o + i]) * M.G[o + i + (int64_t)col * N]; });
            if (lane == 0) M.g[(c % RING) * ldn + col] = r[0];
        }
        __syncthreads();                                   // g is there; the staged rows are free (the flush of the tile before)
        for (int e = tid; e < CONEB_TILE * n; e += NT) {
            const int kk = e & (CONEB_TILE - 1), col = e / CONEB_TILE, r = k0 + kk;
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
        fill = kt;
        if (fill == CONEB_TILE) flush();
    }
    // ---- the 's' rows, a block column at a time, appended to the tile the 'q' rows left
    for (int k = 0; k < M.ns; k++) {
        const int o = M.bo[k], m = M.order(k);
        const double *rti = M.rti + (o - Ms);
        for (int b = 0; b < m; b++) {
            if (fill + m - b > CONEB_TILE) flush();
            for (int e = tid; e < m * n; e += NT) {        // w(u, col) = sum_v mat(G_k col)(u, v) rti(v, b), the lower triangle read
                const int u = e % m, col = e / m;
                const double *g = M.G + o + (int64_t)col * N;
                double acc = 0.0;
                for (int v = 0; v < m; v++) acc = fma(u >= v ? g[u + v * m] : g[v + u * m], rti[v + b * m], acc);
                M.w[u * ldn + col] = acc;
            }
            __syncthreads();
            for (int e = tid; e < (m - b) * n; e += NT) {
                const int a = b + e % (m - b), col = e / (m - b);
                double acc = 0.0;
                for (int u = 0; u < m; u++) acc = fma(rti[u + a * m], M.w[u * ldn + col], acc);
                M.T[(fill + a - b) * ldn + col] = a == b ? acc : acc * RT2;
            }
            fill += m - b;
            __syncthreads();                               // w is free for the next block column
        }
    }
    if (fill) flush();
    __syncthreads();
}

// The lower triangle of S = Gs'Gs [+ A'A] of conelp (misc.kkt_chol2).  Barriers before (the caller's) and after.
__device__ __forceinline__ void assemble(const Member &M, bool sing)
{
    assemble_from(M, [&]() { kkt_s_init(M, sing); });
}

// ================================================================================================================ coneqp
// What coneqp_member (batch_coneqp.hpp) needs beyond the operations above; conelp_member instantiates none of it.

// The lower triangle of S = P + Gs'Gs (misc.kkt_chol with H = P): S starts from the lower triangle of P in HBM, as k_qp_batch
// starts it.  Barriers before (the caller's) and after.
__device__ __forceinline__ void assemble_qp(const Member &M)
{
    assemble_from(M, [&]() {
        const int n = M.n;
        for (int e = threadIdx.x; e < n * n; e += NT) {
            const int j = e / n, i = e - j * n;
            if (i >= j) M.S[i + j * M.ldn] = M.P[i + j * n];
        }
    });
}

struct Cone {                                 // the cone of conelp_member: per operation the orthant, the 'q' code, the 's' code
    const Member &M;

    __device__ __forceinline__ int lmbda_len() const { return M.Nd; }
    template <class F>
    __device__ __forceinline__ void for_rows(F f) const
    {
        for (int j = threadIdx.x; j < M.Np; j += NT) f(PackedRow{M.prow[j], M.pmir[j], weight(M, j)});
    }
    __device__ __forceinline__ void load_h(double *out) const { load_sym(M, M.h, out); }
    __device__ __forceinline__ void start() const                                   // d = di = 1, v_k = e, beta_k = 1, r_k = rti_k = I
    {
        const int tid = threadIdx.x, ml = M.ml, Ms = M.Ms, N = M.N;
        for (int k = tid; k < Ms; k += NT) M.d[k] = k < ml ? 1.0 : 0.0;
        for (int k = tid; k < ml; k += NT) M.di[k] = 1.0;
        for (int k = tid; k < N; k += NT) M.z[k] = 0.0;
        blocks_identity(M);
        __syncthreads();
        if (tid < M.nq) { M.d[M.off[tid]] = 1.0; M.beta[tid] = 1.0; }
        load_sym(M, M.h, M.s);
        __syncthreads();
    }
    __device__ __forceinline__ void max_step(const double *u0, double a0, const double *u1, double a1, double (&mx)[2]) const
    {
        orth_max_step(M.ml, u0, a0, u1, a1, mx);
        cones_max_step(M, u0, a0, u1, a1, mx);
        blocks_max_step(M, u0, a0, u1, a1, mx);
        blk_reduce<2, true>(mx, M.red);
    }
    __device__ __forceinline__ void push(bool ps, bool pz, const double (&mx)[2]) const
    {
        const int tid = threadIdx.x;
        orth_push(M.ml, ps, pz, mx, M.s, M.z);
        if (tid < M.nq) {
            const int r = M.off[tid];
            if (ps) M.s[r] += 1.0 + mx[0];
            if (pz) M.z[r] += 1.0 + mx[1];
        }
        blocks_push(M, ps, pz, mx);
    }
    __device__ __forceinline__ bool first_scaling() const                           // misc.py:284-419
    {
        orth_first_scaling(M.ml, M.s, M.z, M.d, M.di, M.lm);
        cones_scaling(M);
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
        for (int j = tid; j < M.Np; j += NT) {
            const double t = row_dot(M.G, N, n, M.prow[j], vx);
            M.tw[M.prow[j]] = t; M.tw[M.pmir[j]] = t;
        }
        __syncthreads();
        wscale(M, M.tw, M.tw, true, true);
        for (int k = tid; k < N; k += NT) vz[k] = M.tw[k] - vz[k];                             // W uz = W^-T G ux - W^-T bz
        __syncthreads();
    }
    __device__ __forceinline__ void gemv_t(const double *u, double sign, double *v) const { gemv_t_packed(M, u, sign, v); }
    __device__ __forceinline__ void rhs(int i, double sigma, double mu) const
    {
        const int tid = threadIdx.x, ns = M.ns, Ms = M.Ms, N = M.N;
        orth_rhs<true>(M.ml, i, sigma, mu, M.lm, M.ws3, M.d, M.rz, M.ds, M.dz);
        cones_rhs(M, i, sigma, mu);
        if (ns == 0) return;
        blocks_sinv(M, i, sigma, mu);
        __syncthreads();
        blocks_congr(M, M.r, 1, M.ds, M.tw);           // W'ds
        for (int k = Ms + tid; k < N; k += NT) M.dz[k] = -((1.0 - sigma) * M.rz[k] + M.tw[k]);
    }
    __device__ __forceinline__ double th_dot(const double *dz) const
    {
        double acc = 0.0;
        for (int j = threadIdx.x; j < M.Np; j += NT) acc += weight(M, j) * (M.th[M.prow[j]] * dz[M.prow[j]]);
        return acc;
    }
    __device__ __forceinline__ void combine(int i, double dtau, double (&mx)[2]) const
    {
        const int tid = threadIdx.x, Ms = M.Ms, N = M.N;
        orth_combine(M.ml, i, dtau, M.lm, M.z1, M.ds, M.dz, M.ws3, mx);
        cones_combine(M, i, dtau, mx);
        for (int k = Ms + tid; k < N; k += NT) {
            const double zk = M.dz[k] + dtau * M.z1[k];
            M.dz[k] = zk; M.ds[k] -= zk;
        }
        __syncthreads();
        blocks_combine(M, i == 0, mx);
        blk_reduce<2, true>(mx, M.red);                // the maximum over the three kinds
    }
    __device__ __forceinline__ void update(double step) const                       // misc.py:444-634; s = W'lmbda and z = W^-1 lmbda
    {
        orth_update(M.ml, step, M.ds, M.dz, M.d, M.di, M.lm, M.s, M.z);
        cones_update(M, step);
        blocks_update(M, step);
    }

    // ---- coneqp: what coneqp_member asks for beyond the operations above (batch_coneqp.hpp has the protocol)
    __device__ __forceinline__ int degree() const { return M.ml + M.nq + (M.Nd - M.Ms); }       // ml + nq + sum m_k
    __device__ __forceinline__ void assemble_qp() const { kvx::assemble_qp(M); }
    __device__ __forceinline__ void rhs_qp(bool ws, double smu) const
    {
        const int tid = threadIdx.x, ns = M.ns, Ms = M.Ms, N = M.N;
        for (int k = tid; k < M.ml; k += NT) {             // the 'l' rows as k_qp_batch forms them
            const double lk = M.lm[k];
            double t = -lk * lk + smu;
            if (ws) t -= M.ws3[k];
            t /= lk;
            M.ds[k] = t;
            M.dz[k] = -M.rz[k] - M.d[k] * t;
        }
        cones_rhs_qp(M, ws, smu);
        if (ns == 0) return;
        for (int k = 0; k < ns; k++) {                 // sinv with the diagonal lmbda_k (misc_solvers.c:845-882)
            const int o = M.bo[k], m = M.order(k);
            const double *lm = M.lm + M.bl[k];
            for (int e = tid; e < m * m; e += NT) {
                const int ii = e % m, jj = e / m;
                double t = ii == jj ? -lm[ii] * lm[ii] + smu : 0.0;
                if (ws) t -= M.ws3[o + e];
                M.ds[o + e] = t / ((lm[ii] + lm[jj]) / 2.0);
            }
        }
        __syncthreads();
        blocks_congr(M, M.r, 1, M.ds, M.tw);           // W'ds
        for (int k = Ms + tid; k < N; k += NT) M.dz[k] = -M.rz[k] - M.tw[k];
    }
    // ds -= dz; dot := ds'dz in every thread; ws3 := ds o dz (save); both scaled by lmbda; mx as in max_step.  As in combine the
    // eigenvectors replace the 's' blocks and the eigenvalues stand in sgs, sgz for update().  z1 is not read.
    __device__ __forceinline__ void combine_qp(bool save, double &dot, double (&mx)[2]) const
    {
        const int tid = threadIdx.x, Ms = M.Ms, N = M.N;
        double acc[1] = {0.0};
        for (int k = tid; k < M.ml; k += NT) {             // the 'l' rows as k_qp_batch forms them
            const double lk = M.lm[k], zk = M.dz[k], sk = M.ds[k] - zk, pr = sk * zk;
            acc[0] += pr;
            if (save) M.ws3[k] = pr;
            const double s2 = sk / lk, z2 = zk / lk;
            M.ds[k] = s2; M.dz[k] = z2;
            mx[0] = fmax(mx[0], -s2); mx[1] = fmax(mx[1], -z2);
        }
        cones_combine_qp(M, save, acc[0], mx);
        for (int k = Ms + tid; k < N; k += NT) {
            const double zk = M.dz[k], sk = M.ds[k] - zk;
            M.ds[k] = sk;
            acc[0] += sk * zk;                             // both triangles: an off-diagonal entry counts twice
        }
        __syncthreads();
        blocks_combine(M, save, mx);
        blk_reduce<2, true>(mx, M.red);                // the maximum over the three kinds
        blk_reduce<1, false>(acc, M.red);
        dot = acc[0];
    }
};

// The tables of the cone, at the top of a kernel once M has its sizes and its LDS pointers.  a: the kernel's arguments, of which
// the cone orders a.q and the block orders a.m are read; prow, pmir: M.prow, M.pmir as they are written.  Barriers: none
// before, one after.
template <class Args>
__device__ __forceinline__ void cone_tables(Member &M, const Args &a, unsigned short *prow, unsigned short *pmir)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, ml = M.ml, nq = M.nq, ns = M.ns, Ms = M.Ms;
    // ---- the cone: the first row of every 'q' cone and the cone of every 'q' row; the first row and the first lmbda of every
    //      's' block; the packed rows and their mirror images
    if (tid <= nq) {
        int o = ml;
        for (int k = 0; k < tid; k++) o += a.q[k];
        M.off[tid] = o;
    }
    if (tid <= ns) {
        int o = Ms, ol = Ms;
        for (int k = 0; k < tid; k++) { o += a.m[k] * a.m[k]; ol += a.m[k]; }
        M.bo[tid] = o; M.bl[tid] = ol;
    }
    for (int k = tid; k < Ms; k += NT) { prow[k] = (unsigned short)k; pmir[k] = (unsigned short)k; }
    __syncthreads();
    for (int c = wv; c < nq; c += NW) {
        const int o = M.off[c], m = M.off[c + 1] - o;
        for (int i = lane; i < m; i += 64) M.cone[o + i - ml] = (unsigned short)c;
    }
    {
        int po = Ms;
        for (int k = 0; k < ns; k++) {
            const int o = M.bo[k], m = M.order(k);
            for (int e = tid; e < m * m; e += NT) {
                const int i = e % m, j = e / m;
                if (i < j) continue;
                const int pq = po + j * m - (j * (j - 1)) / 2 + (i - j);
                prow[pq] = (unsigned short)(o + i + j * m);
                pmir[pq] = (unsigned short)(o + j + i * m);
            }
            po += (m * (m + 1)) / 2;
        }
    }
    __syncthreads();
}

// The cone's sizes as the kernel and the layout take them
struct Sizes { int Ms, N, Nd, Np; };
Sizes sizes(int ml, int nq, const unsigned short *q, int ns, const unsigned char *m)
{
    Sizes z = {ml, 0, 0, 0};
    for (int k = 0; k < nq; k++) z.Ms += q[k];
    z.N = z.Nd = z.Np = z.Ms;
    for (int k = 0; k < ns; k++) { z.N += m[k] * m[k]; z.Nd += m[k]; z.Np += (m[k] * (m[k] + 1)) / 2; }
    return z;
}
