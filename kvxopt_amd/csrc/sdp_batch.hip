// k_sdp_batch: one workgroup (256 threads, four wavefronts) carries one small dense semidefinite program from its starting point
// to its status or its infeasibility certificate (sdp_batch.hpp).  It is conelp_member (batch_conelp.hpp) on the cone
// K = R^ml_+ x S^{m_0}_+ x ...: the 'l' rows are the orthant of that header, the 's' rows are treated by the reference's own
// operations, the ones csrc/kkt_s.hip carries as stand-alone kernels: misc.compute_scaling / update_scaling (misc.py:354-419,
// 582-634), scale, scale2, sprod, sinv, sdot and max_step (misc_solvers.c:188-240, 343-397, 700-770, 845-882, 1029-1046,
// 1086-1160), strung together as cone.py::_ConeEngine strings them.
//
// Vectors of the cone lie in LDS with every 's' block as its full symmetric m x m matrix, column-major with leading dimension m:
// with a thread per entry a wavefront reads consecutive rows of one operand and at most 64 / m entries of the other, which are
// broadcasts, so a padded leading dimension buys nothing and the blocks keep the layout the results are returned in.  Every block
// operation writes both triangles from one computed value, so the blocks stay symmetric to the bit.  G and h are read in HBM
// through two tables of the Np = ml + sum m_k (m_k + 1) / 2 packed rows: prow[q], the row of the q-th lower-triangle entry, and
// pmir[q], the row of its mirror image; an off-diagonal entry counts twice in G'z and in the cone's inner product (misc.sgemv,
// misc.sdot).  The upper triangles of G and h are never read.
//
// A block belongs to the workgroup, one block after the other: a thread per entry in the m x m products, the Cholesky factors and
// the congruences, and in the one-sided Jacobi iteration (round-robin order of kkt_s.hip) sixteen lanes per column pair, so the
// eight pairs of a round of an order-16 block take half the workgroup and the other half carries a second matrix: the scaled ds
// and dz, or s and z, are diagonalised together, between the same barriers.  A pair's three inner products are an xor butterfly
// over its sixteen lanes, taken from the first of them, so a block's result depends on its entries and its order alone; a matrix that has converged takes no
// further rotation while its partner finishes.  Whether a sweep rotated anything is a flag that the rotating pairs set, never
// a count.  Symmetric eigenvalues come from the same iteration on x + 1.5 |x|_F I (kkt_s.hip's shift).
//
// S = Gs'Gs with Gs = W^-T G is assembled from staged rows of Gs, at most 32 at a time.  The 's' rows of block k and column j are
// rti_k' mat(G_kj) rti_k, packed with sqrt(2) on the off-diagonals; they are staged one block column b at a time, with no
// workspace in HBM: w_j = mat(G_kj) rti_k[:, b] for all columns j (m_k x n, in the 16 rows behind the staged ones), then the rows
// (a, b), a >= b, as rti_k[:, a]'w_j.  G's 's' rows are read m_k times per factorisation, from L2; the scaled rows never leave
// LDS, which keeps the Gram form and spares the _dev entry a workspace argument.
//
// Sums over all rows have the fixed order of batch_device.hpp.  Every loop of this file is bounded by n, N, ns, m_k or
// SDPB_SWEEPS.  A block that is not finite is not iterated on.
#include "sdp_batch.hpp"
#include "batch_conelp.hpp"

#include <cmath>

namespace kvx {
namespace {

using namespace batchdev;
static_assert(NT == SDPB_THREADS, "the shared helpers are written for the workgroup of k_sdp_batch");
static_assert(SDPB_MAX_M * SDPB_MAX_M <= NT, "a thread per entry of a block");
constexpr int MM = SDPB_MAX_M * SDPB_MAX_M;
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
    __device__ int order(int k) const { return bl[k + 1] - bl[k]; }
};

// The sum over the sixteen lanes of a column pair, the same bytes in each: an xor butterfly, then the first lane's sum for all.
// The butterfly alone does not give that: the compiler contracts a product that feeds its first addition into
// fma(x, x, partner's rounded product), two partners then hold sums that differ in the last bit, al - be of two columns of nearly
// equal norm gives them different rotations, and rows of one column pair turn by different angles.
__device__ inline double sum16(double v)
{
#pragma unroll
    for (int o = 8; o; o >>= 1) v += __shfl_xor(v, o);
    return __shfl(v, (threadIdx.x & 63) & ~15);
}

// ---- the dense kernels of a block: m x m matrices in LDS, column-major, leading dimension m; each ends with a barrier.
// They are functions of their own, called from many places, so their pointer arguments arrive as generic pointers; every one of
// them points into LDS, and the kernels say so (lds_d, lds_i): their loads and stores are then LDS instructions, not flat ones.
typedef __attribute__((address_space(3))) double lds_d;
typedef __attribute__((address_space(3))) int lds_i;
__device__ inline lds_d *in_lds(double *p) { return (lds_d *)p; }
__device__ inline const lds_d *in_lds(const double *p) { return (const lds_d *)p; }

// C := op(A) op(B); ta / tb: 0 plain, 1 transposed.  C must not alias A or B.
__device__ void mm(double *C_, const double *A_, int ta, const double *B_, int tb, int m)
{
    lds_d *C = in_lds(C_);
    const lds_d *A = in_lds(A_), *B = in_lds(B_);
    for (int e = threadIdx.x; e < m * m; e += NT) {
        const int i = e % m, j = e / m;
        double acc = 0.0;
        for (int p = 0; p < m; p++) acc = fma(ta ? A[p + i * m] : A[i + p * m], tb ? B[j + p * m] : B[p + j * m], acc);
        C[e] = acc;
    }
    __syncthreads();
}

// In-place lower Cholesky factor; the strict upper triangle is set to zero.  false, for every thread, on a pivot that is <= 0 or
// not finite.
__device__ bool chol_blk(double *A_, int m)
{
    lds_d *A = in_lds(A_);
    const int tid = threadIdx.x;
    for (int j = 0; j < m; j++) {
        const double piv = A[j + j * m];
        if (!(piv > 0.0 && piv < INFINITY)) return false;
        const double l = sqrt(piv);
        __syncthreads();                                   // every thread has read the pivot
        if (tid >= j && tid < m) A[tid + j * m] = tid == j ? l : A[tid + j * m] / l;
        __syncthreads();
        for (int e = tid; e < m * m; e += NT) {
            const int i = e % m, c = e / m;
            if (c > j && i >= c) A[e] -= A[i + j * m] * A[c + j * m];
        }
        __syncthreads();
    }
    for (int e = tid; e < m * m; e += NT)
        if (e % m < e / m) A[e] = 0.0;
    __syncthreads();
    return true;
}

// X := L^-T X for the lower triangular L: thread c owns column c of X
__device__ void trsm_lt(const double *L_, double *X_, int m)
{
    const lds_d *L = in_lds(L_);
    if ((int)threadIdx.x < m) {
        lds_d *x = in_lds(X_) + threadIdx.x * m;
        for (int i = m - 1; i >= 0; i--) {
            double v = x[i];
            for (int p = i + 1; p < m; p++) v = fma(-L[p + i * m], x[p], v);
            x[i] = v / L[i + i * m];
        }
    }
    __syncthreads();
}

// out := R'X R (form 0) or R X R' (form 1) with X the symmetric matrix of the lower triangle of the block X (misc_solvers.c:188-240);
// both triangles of out are written, from one value.  out == X is allowed; T: m^2 of work.
__device__ void congr(const double *R_, int form, const double *X_, double *out_, double *T_, int m)
{
    const lds_d *R = in_lds(R_), *X = in_lds(X_);
    lds_d *out = in_lds(out_), *T = in_lds(T_);
    for (int e = threadIdx.x; e < m * m; e += NT) {
        const int i = e % m, j = e / m;
        double acc = 0.0;
        for (int p = 0; p < m; p++) acc = fma(i >= p ? X[i + p * m] : X[p + i * m], form ? R[j + p * m] : R[p + j * m], acc);
        T[e] = acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < m * m; e += NT) {
        const int i = e % m, j = e / m, a = max(i, j), b = min(i, j);
        double acc = 0.0;
        for (int p = 0; p < m; p++) acc = fma(form ? R[a + p * m] : R[p + a * m], T[p + b * m], acc);
        out[e] = acc;
    }
    __syncthreads();
}

// out := R diag(l) R', both triangles from one value (W'diag(lmbda) and W^-1 diag(lmbda): coneprog.py:1413-1433)
__device__ void rdr(const double *R_, const double *l_, double *out_, int m)
{
    const lds_d *R = in_lds(R_), *l = in_lds(l_);
    lds_d *out = in_lds(out_);
    for (int e = threadIdx.x; e < m * m; e += NT) {
        const int i = e % m, j = e / m, a = max(i, j), b = min(i, j);
        double acc = 0.0;
        for (int p = 0; p < m; p++) acc = fma(R[a + p * m] * l[p], R[b + p * m], acc);
        out[e] = acc;
    }
}

// One-sided Jacobi (Hestenes) on the columns of A0 and, by the other half of the workgroup, of A1 (either may be null), in the
// round-robin order of kkt_s.hip: on return the columns are mutually orthogonal, A_out = A_in V; V0, V1 (optional) accumulate the
// rotations from the identity.  Group g = tid / 16 takes pair g % 8 of matrix g / 8, lane l of the group row l.
__device__ void jacobi2(double *A0, double *V0, double *A1, double *V1, int m, int *flag_)
{
    const int tid = threadIdx.x, g = tid >> 4, l = tid & 15, pk = g & 7;
    const bool has = ((g >> 3) ? A1 : A0) != nullptr, acc = ((g >> 3) ? V1 : V0) != nullptr;
    lds_d *A = in_lds((g >> 3) ? A1 : A0), *V = in_lds((g >> 3) ? V1 : V0);
    lds_i *flag = (lds_i *)flag_;
    for (int e = tid; e < m * m; e += NT) {
        const double v = (e % m == e / m) ? 1.0 : 0.0;
        if (V0) in_lds(V0)[e] = v;
        if (V1) in_lds(V1)[e] = v;
    }
    __syncthreads();
    if (m < 2) return;
    const int n = m + (m & 1);                             // players of the round-robin (a dummy when m is odd)
    const double tol = 2.220446049250313e-16 * sqrt((double)m);       // dgesvj's default: sqrt(m) eps
    for (int sweep = 0; sweep < SDPB_SWEEPS; sweep++) {
        if (tid == 0) flag[0] = 0;
        __syncthreads();
        for (int r = 0; r < n - 1; r++) {
            int p = 0, q = 0;
            bool act = has && pk < n / 2;
            if (act) {
                if (pk == 0) { p = n - 1; q = r; }
                else { p = (r + pk) % (n - 1); q = (r - pk + (n - 1)) % (n - 1); }
                if (p > q) { const int t = p; p = q; q = t; }
                act = q < m;
                if (!act) p = q = 0;
            }
            const bool row = act && l < m;
            const double x = row ? A[l + p * m] : 0.0, y = row ? A[l + q * m] : 0.0;
            const double al = sum16(x * x), be = sum16(y * y), ga = sum16(x * y);
            if (act && !(fabs(ga) <= tol * sqrt(al * be) || ga == 0.0)) {
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                if (row) {
                    A[l + p * m] = c * x - s * y;
                    A[l + q * m] = s * x + c * y;
                    if (acc) {
                        const double vx = V[l + p * m], vy = V[l + q * m];
                        V[l + p * m] = c * vx - s * vy;
                        V[l + q * m] = s * vx + c * vy;
                    }
                }
                if (l == 0) flag[0] = 1;                   // a flag: every rotating pair stores the same value
            }
            __syncthreads();
        }
        const int rot = flag[0];
        __syncthreads();
        if (!rot) break;
    }
}

// After jacobi2: sig[rank] = |a_j| - shift, U(:, rank) = a_j / |a_j|, Vo(:, rank) = v_j (U, Vo optional), ranks by descending
// (desc) or ascending norm, ties by column index.  A null: the block was not finite and was not iterated on, NaN everywhere.
// nrm: 16 doubles.
__device__ void collect(const double *A_, const double *V_, int m, bool desc, double shift, double *nrm_, double *sig_, double *U_,
                        double *Vo_)
{
    const int tid = threadIdx.x;
    const bool U = U_ != nullptr, Vo = Vo_ != nullptr;
    const lds_d *A = in_lds(A_), *V = in_lds(V_);
    lds_d *nrm = in_lds(nrm_), *sig = in_lds(sig_), *Uo = in_lds(U_), *Vout = in_lds(Vo_);
    if (A_ == nullptr) {
        for (int e = tid; e < m * m; e += NT) {
            if (U) Uo[e] = NAN;
            if (Vo) Vout[e] = NAN;
            if (e < m) sig[e] = NAN;
        }
        __syncthreads();
        return;
    }
    if (tid < m) {
        double acc = 0.0;
        for (int i = 0; i < m; i++) acc = fma(A[i + tid * m], A[i + tid * m], acc);
        nrm[tid] = sqrt(acc);
    }
    __syncthreads();
    for (int e = tid; e < m * m; e += NT) {
        const int i = e % m, j = e / m;
        const double sj = nrm[j];
        int rk = 0;
        for (int t = 0; t < m; t++) {
            const double st = nrm[t];
            rk += (desc ? (st > sj || (st == sj && t < j)) : (st < sj || (st == sj && t < j))) ? 1 : 0;
        }
        if (U) Uo[i + rk * m] = A[e] * (sj > 0.0 ? 1.0 / sj : 0.0);
        if (Vo) Vout[i + rk * m] = V[e];
        if (i == 0) sig[rk] = sj - shift;
    }
    __syncthreads();
}

// The eigenvalues (ascending) of a0 X0 and a1 X1 into sig0 and sig1 and, with Q0, Q1, their eigenvectors there (Q may be X): the
// 's' part of misc.max_step (misc_solvers.c:1086-1160).  Barriers before (the caller's) and after.
__device__ __forceinline__ void eig2(const Member &M, const double *X0, double a0, const double *X1, double a1, int m, double *sig0, double *sig1,
                     double *Q0, double *Q1)
{
    double f[2] = {0.0, 0.0};
    for (int e = threadIdx.x; e < m * m; e += NT) {
        const double v0 = a0 * X0[e], v1 = a1 * X1[e];
        M.wa[e] = v0; M.wb[e] = v1;
        f[0] = fma(v0, v0, f[0]); f[1] = fma(v1, v1, f[1]);
    }
    blk_reduce<2, false>(f, M.red);
    const double f0 = sqrt(f[0]), f1 = sqrt(f[1]);
    const bool ok0 = f0 < INFINITY, ok1 = f1 < INFINITY;                 // false for a NaN as well
    const double c0 = f0 > 0.0 ? 1.5 * f0 : 1.0, c1 = f1 > 0.0 ? 1.5 * f1 : 1.0;
    if ((int)threadIdx.x < m) { M.wa[threadIdx.x * (m + 1)] += c0; M.wb[threadIdx.x * (m + 1)] += c1; }
    jacobi2(ok0 ? M.wa : nullptr, nullptr, ok1 ? M.wb : nullptr, nullptr, m, M.flag);
    collect(ok0 ? M.wa : nullptr, nullptr, m, false, c0, M.nrm, sig0, Q0, nullptr);
    collect(ok1 ? M.wb : nullptr, nullptr, m, false, c1, M.nrm + SDPB_MAX_M, sig1, Q1, nullptr);
}

// mx[0], mx[1] := the larger of themselves and -lambda_min over the 's' blocks of a0 u0 and a1 u1, by every thread
__device__ __forceinline__ void blocks_max_step(const Member &M, const double *u0, double a0, const double *u1, double a1, double (&mx)[2])
{
    for (int k = 0; k < M.ns; k++) {
        const int o = M.bo[k], ol = M.bl[k] - M.ml, m = M.order(k);
        eig2(M, u0 + o, a0, u1 + o, a1, m, M.sgs + ol, M.sgz + ol, nullptr, nullptr);
        mx[0] = fmax(mx[0], -M.sgs[ol]);
        mx[1] = fmax(mx[1], -M.sgz[ol]);
    }
}

// out := W in, W'in, W^-1 in or W^-T in (misc_solvers.c:85-240); in == out is allowed.  Barriers before (the caller's) and after.
__device__ __forceinline__ void wscale(const Member &M, const double *in, double *out, bool inv, bool trans)
{
    for (int k = threadIdx.x; k < M.ml; k += NT) out[k] = (inv ? M.di[k] : M.d[k]) * in[k];
    for (int k = 0; k < M.ns; k++) {
        const int o = M.bo[k];
        congr((inv ? M.rti : M.r) + (o - M.ml), inv != trans ? 1 : 0, in + o, out + o, M.wa, M.order(k));
    }
    __syncthreads();
}

// 1 for a diagonal or an 'l' row, 2 for an off-diagonal one: its weight in G'z and in the inner product of the cone
__device__ inline double weight(const Member &M, int q) { return M.prow[q] != M.pmir[q] ? 2.0 : 1.0; }

// v[c] += sign * sum over the packed rows q of G(row_q, c) weight_q u[row_q] (misc.sgemv, trans 'T'): a wavefront per column
__device__ __forceinline__ void gemv_t_packed(const Member &M, const double *u, double sign, double *v)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c = w; c < M.n; c += NW) {
        double acc = 0.0;
        for (int q = lane; q < M.Np; q += 64) { const int r = M.prow[q]; acc += M.G[r + (int64_t)c * M.N] * (weight(M, q) * u[r]); }
        acc = wave_sum(acc);
        if (lane == 0) v[c] += sign * acc;
    }
}

// out := the vector of the cone whose lower triangles are those of the HBM vector v, both triangles written
__device__ __forceinline__ void load_sym(const Member &M, const double *v, double *out)
{
    for (int q = threadIdx.x; q < M.Np; q += NT) { const double t = v[M.prow[q]]; out[M.prow[q]] = t; out[M.pmir[q]] = t; }
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
// misc.compute_scaling on the 's' blocks (misc.py:354-419): r_k, rti_k and lmbda_k from s_k and z_k.  false when an s_k or z_k is
// not positive definite.  Barriers before (the caller's) and after.
__device__ __forceinline__ bool blocks_scaling(const Member &M)
{
    for (int k = 0; k < M.ns; k++) {
        const int o = M.bo[k], ol = M.bl[k], m = M.order(k);
        double *r = M.r + (o - M.ml), *rti = M.rti + (o - M.ml);
        for (int e = threadIdx.x; e < m * m; e += NT) { M.wa[e] = M.s[o + e]; M.wb[e] = M.z[o + e]; }
        __syncthreads();
        if (!chol_blk(M.wa, m) || !chol_blk(M.wb, m)) return false;
        mm(M.wc, M.wb, 1, M.wa, 0, m);                     // Lz'Ls = U diag(lmbda) V'
        jacobi2(M.wc, nullptr, nullptr, nullptr, m, M.flag);
        collect(M.wc, nullptr, m, true, 0.0, M.nrm, M.lm + ol, M.wd, nullptr);
        mm(rti, M.wb, 0, M.wd, 0, m);                      // rti = Lz U diag(lmbda)^-1/2
        trsm_lt(M.wb, M.wd, m);                            // r = Lz^-T U diag(lmbda)^1/2
        for (int e = threadIdx.x; e < m * m; e += NT) {
            const double a = sqrt(M.lm[ol + e / m]);
            r[e] = M.wd[e] * a;
            rti[e] = rti[e] / a;
        }
        __syncthreads();
    }
    return true;
}


struct PackedRow {                            // a packed row of the cone: its entry, its mirror image, its weight
    int k, mir;
    double wq;
    __device__ __forceinline__ double w(double v) const { return wq * v; }
    __device__ __forceinline__ void put(double *vec, double v) const { vec[k] = v; vec[mir] = v; }
};

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
        const int tid = threadIdx.x, ml = M.ml, ns = M.ns, N = M.N;
        for (int k = tid; k < ml; k += NT) { M.d[k] = 1.0; M.di[k] = 1.0; }
        for (int k = tid; k < N; k += NT) M.z[k] = 0.0;
        for (int k = 0; k < ns; k++) {
            const int o = M.bo[k] - ml, m = M.order(k);
            for (int e = tid; e < m * m; e += NT) { const double v = (e % m == e / m) ? 1.0 : 0.0; M.r[o + e] = v; M.rti[o + e] = v; }
        }
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
        const int tid = threadIdx.x, ns = M.ns;
        orth_push(M.ml, ps, pz, mx, M.s, M.z);
        for (int k = 0; k < ns; k++) {
            const int m = M.order(k), r = M.bo[k] + tid * (m + 1);
            if (tid < m) {
                if (ps) M.s[r] += 1.0 + mx[0];
                if (pz) M.z[r] += 1.0 + mx[1];
            }
        }
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
        const int tid = threadIdx.x, ns = M.ns, N = M.N;
        orth_rhs<false>(M.ml, i, sigma, mu, M.lm, M.ws3, M.d, M.rz, M.ds, M.dz);
        for (int k = 0; k < ns; k++) {                 // sinv with the diagonal lmbda_k (misc_solvers.c:845-882)
            const int o = M.bo[k], m = M.order(k);
            const double *lm = M.lm + M.bl[k];
            for (int e = tid; e < m * m; e += NT) {
                const int ii = e % m, jj = e / m;
                double t = ii == jj ? lm[ii] * lm[ii] : 0.0;
                if (i == 1) t += M.ws3[o + e] - (ii == jj ? sigma * mu : 0.0);
                M.ds[o + e] = -(t / ((lm[ii] + lm[jj]) / 2.0));
            }
        }
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
        const int tid = threadIdx.x, ml = M.ml, ns = M.ns, N = M.N;
        orth_combine(ml, i, dtau, M.lm, M.z1, M.ds, M.dz, M.ws3, mx);
        for (int k = ml + tid; k < N; k += NT) {
            const double zk = M.dz[k] + dtau * M.z1[k];
            M.dz[k] = zk; M.ds[k] -= zk;
        }
        blk_reduce<2, true>(mx, M.red);                // its barriers also publish ds and dz
        for (int k = 0; k < ns; k++) {
            const int o = M.bo[k], ol = M.bl[k], m = M.order(k);
            double *ds = M.ds + o, *dz = M.dz + o;
            const double *lm = M.lm + ol;
            if (i == 0) {                              // sprod (misc_solvers.c:700-742): (ds dz + dz ds) / 2
                for (int e = tid; e < m * m; e += NT) {
                    const int ii = e % m, jj = e / m, aa = max(ii, jj), bb = min(ii, jj);
                    double acc = 0.0;
                    for (int q = 0; q < m; q++) acc += ds[aa + q * m] * dz[q + bb * m] + dz[aa + q * m] * ds[q + bb * m];
                    M.ws3[o + e] = 0.5 * acc;
                }
                __syncthreads();
            }
            for (int e = tid; e < m * m; e += NT) {    // scale2 (misc_solvers.c:343-397)
                const double cc = sqrt(lm[e % m]) * sqrt(lm[e / m]);
                ds[e] = ds[e] / cc; dz[e] = dz[e] / cc;
            }
            __syncthreads();
            // the eigenvalues in sgs, sgz; the eigenvectors replace the blocks (coneprog.py:1308-1321); the update consumes both
            eig2(M, ds, 1.0, dz, 1.0, m, M.sgs + (ol - ml), M.sgz + (ol - ml), ds, dz);
            mx[0] = fmax(mx[0], -M.sgs[ol - ml]);
            mx[1] = fmax(mx[1], -M.sgz[ol - ml]);
        }
    }
    __device__ __forceinline__ void update(double step) const                       // misc.py:444-634; s = W'lmbda and z = W^-1 lmbda
    {
        const int tid = threadIdx.x, ml = M.ml, ns = M.ns;
        orth_update(ml, step, M.ds, M.dz, M.d, M.di, M.lm, M.s, M.z);
        for (int k = 0; k < ns; k++) {
            const int o = M.bo[k], ol = M.bl[k], m = M.order(k);
            double *r = M.r + (o - ml), *rti = M.rti + (o - ml), *lm = M.lm + ol;
            const double *sgs = M.sgs + (ol - ml), *sgz = M.sgz + (ol - ml);
            // Ls = diag(lmbda)^1/2 Qs diag(lmbda)^1/2 diag((1 + step sigs) / lmbda)^1/2, Lz likewise (coneprog.py:1356-1390)
            for (int e = tid; e < m * m; e += NT) {
                const int ii = e % m, jj = e / m;
                const double cc = sqrt(lm[ii]) * sqrt(lm[jj]);
                M.wa[e] = (M.ds[o + e] * cc) * sqrt((1.0 + step * sgs[jj]) / lm[jj]);
                M.wb[e] = (M.dz[o + e] * cc) * sqrt((1.0 + step * sgz[jj]) / lm[jj]);
            }
            __syncthreads();
            mm(M.wc, r, 0, M.wa, 0, m);                    // r := r Ls, rti := rti Lz
            mm(M.wd, rti, 0, M.wb, 0, m);
            for (int e = tid; e < m * m; e += NT) { r[e] = M.wc[e]; rti[e] = M.wd[e]; }
            __syncthreads();
            mm(M.wc, M.wb, 1, M.wa, 0, m);                 // Lz'Ls = U diag(lmbda+) V'
            {
                double f[1] = {0.0};
                for (int e = tid; e < m * m; e += NT) f[0] = fma(M.wc[e], M.wc[e], f[0]);
                blk_reduce<1, false>(f, M.red);
                const bool ok = sqrt(f[0]) < INFINITY;
                jacobi2(ok ? M.wc : nullptr, ok ? M.wd : nullptr, nullptr, nullptr, m, M.flag);
                collect(ok ? M.wc : nullptr, M.wd, m, true, 0.0, M.nrm, lm, M.wa, M.wb);      // U in wa, V in wb
            }
            mm(M.wc, r, 0, M.wb, 0, m);                    // r := r V diag(lmbda+)^-1/2, rti := rti U diag(lmbda+)^-1/2
            mm(M.wd, rti, 0, M.wa, 0, m);
            for (int e = tid; e < m * m; e += NT) {
                const double aa = 1.0 / sqrt(lm[e / m]);
                r[e] = M.wc[e] * aa; rti[e] = M.wd[e] * aa;
            }
            __syncthreads();
            rdr(r, lm, M.s + o, m);
            rdr(rti, lm, M.z + o, m);
            __syncthreads();
        }
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
