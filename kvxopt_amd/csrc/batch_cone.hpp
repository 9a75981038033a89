// The cone K = R^ml_+ x Q^{q_0} x ... x S^{m_0}_+ x ... as k_conelp_batch (conelp_batch.hip) and k_coneqp_batch
// (coneqp_batch.hip) carry it: the rows of a member and their tables, the 'q' operations, the 's' operations, W and its
// inverses, the assembly of S over staged rows of W^-T G, and the policy `Cone` through which conelp_member (batch_conelp.hpp)
// and coneqp_member (batch_coneqp.hpp) reach all of it.  conelp_batch.hip has the description of the rows and of the work.
//
// This file is text of its includer: it is included once, inside the anonymous namespace of kvx, after `using namespace
// batchdev` and the includer's static_asserts on CONEB_THREADS, so every kernel keeps its own internal copy of these functions.
// It needs conelp_batch.hpp (the CONEB_ limits), batch_conelp.hpp and <cmath>.  k_socp_batch and k_sdp_batch keep their own
// copies of the 'q' and 's' code: their members' bytes are pinned by digests.
//
// What only coneqp needs is marked "coneqp" and is not instantiated by conelp_member: Member::P, cones_rhs_qp, cones_combine_qp,
// and Cone::degree, assemble_qp, rhs_qp, combine_qp.
constexpr int MM = CONEB_MAX_M * CONEB_MAX_M;
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
    __device__ __forceinline__ int order(int k) const { return bl[k + 1] - bl[k]; }
    const double *P;                          // coneqp: n x n in HBM, column-major, its lower triangle read; c is q
};

// ================================================================================================================ 'q' cones
// d holds v_k in the 'q' rows, lm lmbda_k in the same rows.

// r[0..K) := the sums over the rows i = 0..m-1 of a cone of what f adds for row i, the same bytes in every lane of the wavefront
template <int K, class F>
__device__ __forceinline__ void cone_sum(int m, double (&r)[K], F f)
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

// out := W^-1 in (INV) or W in on the 'q' rows; W_k is symmetric; in == out is allowed.  No barrier.
template <bool INV>
__device__ __forceinline__ void cones_wscale(const Member &M, const double *in, double *out)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
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
__device__ __forceinline__ void cones_max_step(const Member &M, const double *u1, double a1, const double *u2, double a2, double (&mx)[2])
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

// misc.compute_scaling on the 'q' blocks (misc.py:290-352): v_k, beta_k and lmbda_k from s_k and z_k.  No barrier.
__device__ __forceinline__ void cones_scaling(const Member &M)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nq = M.nq;
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
}

// The 'q' rows of the right-hand side: ds by sprod and sinv (misc_solvers.c:671-700, 803-835), dz with W'ds.  No barrier.
__device__ __forceinline__ void cones_rhs(const Member &M, int i, double sigma, double mu)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nq = M.nq;
    for (int c = w; c < nq; c += NW) {
        const int o = M.off[c], m = M.off[c + 1] - o;
        const double *lm = M.lm + o, *v = M.d + o;
        const double l0 = lm[0];
        double q[2];                               // lmbda'lmbda, |lmbda_1|^2
        cone_sum<2>(m, q, [&](int j, double (&q)[2]) { const double t = lm[j] * lm[j]; q[0] += t; if (j) q[1] += t; });
        double d0 = q[0];                          // sprod: head lmbda'lmbda, tail 2 l0 lmbda_1
        if (i == 1) d0 += M.ws3[o] - sigma * mu;
        double u[1];                               // sinv
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

// The 'q' rows of combine: dz += dtau z1, ds -= dz, ws3 = ds o dz (i = 0), scale2 (misc_solvers.c:301-341), max_step.  No barrier.
__device__ __forceinline__ void cones_combine(const Member &M, int i, double dtau, double (&mx)[2])
{
    const int w = threadIdx.x >> 6, nq = M.nq;
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
        const double nl = sqrt(q[1]), aq = sqrt(l0 + nl) * sqrt(l0 - nl);
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
}

// misc.update_scaling on the 'q' blocks (misc.py:467-580), then s = W'lmbda and z = W^-1 lmbda.  No barrier.
__device__ __forceinline__ void cones_update(const Member &M, double step)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nq = M.nq;
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

// ================================================================================================================ 's' blocks

// The sum over the sixteen lanes of a column pair, the same bytes in each: an xor butterfly, then the first lane's sum for all.
// The butterfly alone does not give that: the compiler contracts a product that feeds its first addition into
// fma(x, x, partner's rounded product), two partners then hold sums that differ in the last bit, and rows of one column pair
// turn by different angles.
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

// out := R'X R (form 0) or R X R' (form 1) with X the symmetric matrix of the lower triangle of the block X
// (misc_solvers.c:188-240); both triangles of out are written, from one value.  out == X is allowed; T: m^2 of work.
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
    for (int sweep = 0; sweep < CONEB_SWEEPS; sweep++) {
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
__device__ __forceinline__ void eig2(const Member &M, const double *X0, double a0, const double *X1, double a1, int m, double *sig0,
                                     double *sig1, double *Q0, double *Q1)
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
    collect(ok1 ? M.wb : nullptr, nullptr, m, false, c1, M.nrm + CONEB_MAX_M, sig1, Q1, nullptr);
}

// mx[0], mx[1] := the larger of themselves and -lambda_min over the 's' blocks of a0 u0 and a1 u1, by every thread.  Barriers
// before (the caller's) and after.
__device__ __forceinline__ void blocks_max_step(const Member &M, const double *u0, double a0, const double *u1, double a1, double (&mx)[2])
{
    for (int k = 0; k < M.ns; k++) {
        const int o = M.bo[k], ol = M.bl[k] - M.Ms, m = M.order(k);
        eig2(M, u0 + o, a0, u1 + o, a1, m, M.sgs + ol, M.sgz + ol, nullptr, nullptr);
        mx[0] = fmax(mx[0], -M.sgs[ol]);
        mx[1] = fmax(mx[1], -M.sgz[ol]);
    }
}

// misc.compute_scaling on the 's' blocks (misc.py:354-419): r_k, rti_k and lmbda_k from s_k and z_k.  false when an s_k or z_k is
// not positive definite.  Barriers before (the caller's) and after.
__device__ __forceinline__ bool blocks_scaling(const Member &M)
{
    for (int k = 0; k < M.ns; k++) {
        const int o = M.bo[k], ol = M.bl[k], m = M.order(k);
        double *r = M.r + (o - M.Ms), *rti = M.rti + (o - M.Ms);
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

// ================================================================================================================ the whole cone

// out := W in, W'in, W^-1 in or W^-T in (misc_solvers.c:85-240); in == out is allowed.  Barriers before (the caller's) and after.
__device__ __forceinline__ void wscale(const Member &M, const double *in, double *out, bool inv, bool trans)
{
    for (int k = threadIdx.x; k < M.ml; k += NT) out[k] = (inv ? M.di[k] : M.d[k]) * in[k];
    if (inv) cones_wscale<true>(M, in, out);
    else cones_wscale<false>(M, in, out);
    for (int k = 0; k < M.ns; k++) {
        const int o = M.bo[k];
        congr((inv ? M.rti : M.r) + (o - M.Ms), inv != trans ? 1 : 0, in + o, out + o, M.wa, M.order(k));
    }
    __syncthreads();
}

// 1 for a diagonal, an 'l' or a 'q' row, 2 for an off-diagonal one: its weight in G'z and in the inner product of the cone
__device__ __forceinline__ double weight(const Member &M, int j) { return M.prow[j] != M.pmir[j] ? 2.0 : 1.0; }

// v[c] += sign * sum over the packed rows j of G(row_j, c) weight_j u[row_j] (misc.sgemv, trans 'T'): a wavefront per column
__device__ __forceinline__ void gemv_t_packed(const Member &M, const double *u, double sign, double *v)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c = w; c < M.n; c += NW) {
        double acc = 0.0;
        for (int j = lane; j < M.Np; j += 64) { const int r = M.prow[j]; acc += M.G[r + (int64_t)c * M.N] * (weight(M, j) * u[r]); }
        acc = wave_sum(acc);
        if (lane == 0) v[c] += sign * acc;
    }
}

// out := the vector of the cone whose lower triangles are those of the HBM vector v, both triangles written
__device__ __forceinline__ void load_sym(const Member &M, const double *v, double *out)
{
    for (int j = threadIdx.x; j < M.Np; j += NT) { const double t = v[M.prow[j]]; out[M.prow[j]] = t; out[M.pmir[j]] = t; }
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

// The 'q' rows of coneqp's right-hand side (coneprog.py:2376-2392, f4_no_ir :2288-2300): ds := lmbda o\ (-lmbda o lmbda + smu e
// [- ws3]) by sprod and sinv as in cones_rhs, dz := -rz - W'ds: rz enters whole, there is no (1 - sigma).  ws: with the
// Mehrotra term.  No barrier.
__device__ __forceinline__ void cones_rhs_qp(const Member &M, bool ws, double smu)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nq = M.nq;
    for (int c = w; c < nq; c += NW) {
        const int o = M.off[c], m = M.off[c + 1] - o;
        const double *lm = M.lm + o, *v = M.d + o;
        const double l0 = lm[0];
        double q[2];                               // lmbda'lmbda, |lmbda_1|^2
        cone_sum<2>(m, q, [&](int j, double (&q)[2]) { const double t = lm[j] * lm[j]; q[0] += t; if (j) q[1] += t; });
        double d0 = -q[0] + smu;                   // the head of -lmbda o lmbda + smu e [- ws3]
        if (ws) d0 -= M.ws3[o];
        const auto tail = [&](int j) {             // its row j > 0
            double t = -(l0 * lm[j] + lm[j] * l0);
            if (ws) t -= M.ws3[o + j];
            return t;
        };
        double u[1];                               // sinv
        cone_sum<1>(m, u, [&](int j, double (&u)[1]) { if (j) u[0] += tail(j) * lm[j]; });
        const double nl = sqrt(q[1]), aq = (l0 + nl) * (l0 - nl), dq = u[0];
        double vd[1];                              // v'ds of W'ds
        cone_sum<1>(m, vd, [&](int j, double (&vd)[1]) {
            const double t = j == 0 ? (d0 * l0 - dq) * (1.0 / aq) : (tail(j) * (aq / l0) + (dq / l0 - d0) * lm[j]) * (1.0 / aq);
            M.ds[o + j] = t;
            vd[0] += v[j] * t;
        });
        const double be = M.beta[c];
        for (int j = lane; j < m; j += 64) M.dz[o + j] = -M.rz[o + j] - (2.0 * v[j] * vd[0] - jsign(j, M.ds[o + j])) * be;
    }
}

// The 'q' rows of coneqp's combine: ds -= dz, dot += the wavefront's ds'dz (in its lane 0), ws3 = ds o dz (save), scale2
// (misc_solvers.c:301-341), max_step.  It is cones_combine without dtau: z1 is not read.  No barrier.
__device__ __forceinline__ void cones_combine_qp(const Member &M, bool save, double &dot, double (&mx)[2])
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nq = M.nq;
    for (int c = w; c < nq; c += NW) {
        const int o = M.off[c], m = M.off[c + 1] - o;
        const double *lm = M.lm + o;
        const double l0 = lm[0], z0 = M.dz[o], s0 = M.ds[o] - z0;
        double q[4];                               // ds'dz, |lmbda_1|^2, lmbda_1'ds_1, lmbda_1'dz_1
        cone_sum<4>(m, q, [&](int j, double (&q)[4]) {
            const double zk = M.dz[o + j], sk = M.ds[o + j] - zk;
            M.ds[o + j] = sk;
            q[0] += sk * zk;
            if (j) { q[1] += lm[j] * lm[j]; q[2] += lm[j] * sk; q[3] += lm[j] * zk; }
        });
        if (lane == 0) dot += q[0];
        const double nl = sqrt(q[1]), aq = sqrt(l0 + nl) * sqrt(l0 - nl);
        const double lxs = (l0 * s0 - q[2]) / aq, lxz = (l0 * z0 - q[3]) / aq;
        const double bs = -((s0 + lxs) / (l0 / aq + 1.0) / aq), bz = -((z0 + lxz) / (l0 / aq + 1.0) / aq);
        double t2[2];
        cone_sum<2>(m, t2, [&](int j, double (&t2)[2]) {
            const double sk = M.ds[o + j], zk = M.dz[o + j];
            if (save) M.ws3[o + j] = j ? z0 * sk + s0 * zk : q[0];
            const double s2 = (j ? sk + bs * lm[j] : lxs) * (1.0 / aq), z2 = (j ? zk + bz * lm[j] : lxz) * (1.0 / aq);
            M.ds[o + j] = s2; M.dz[o + j] = z2;
            if (j) { t2[0] += s2 * s2; t2[1] += z2 * z2; }
        });
        mx[0] = fmax(mx[0], sqrt(t2[0]) - lxs * (1.0 / aq));
        mx[1] = fmax(mx[1], sqrt(t2[1]) - lxz * (1.0 / aq));
    }
}

struct PackedRow {                            // a packed row of the cone: its entry, its mirror image, its weight
    int k, mir;
    double wq;
    __device__ __forceinline__ double w(double v) const { return wq * v; }
    __device__ __forceinline__ void put(double *vec, double v) const { vec[k] = v; vec[mir] = v; }
};

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
        const int tid = threadIdx.x, ml = M.ml, Ms = M.Ms, ns = M.ns, N = M.N;
        for (int k = tid; k < Ms; k += NT) M.d[k] = k < ml ? 1.0 : 0.0;
        for (int k = tid; k < ml; k += NT) M.di[k] = 1.0;
        for (int k = tid; k < N; k += NT) M.z[k] = 0.0;
        for (int k = 0; k < ns; k++) {
            const int o = M.bo[k] - Ms, m = M.order(k);
            for (int e = tid; e < m * m; e += NT) { const double v = (e % m == e / m) ? 1.0 : 0.0; M.r[o + e] = v; M.rti[o + e] = v; }
        }
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
        const int tid = threadIdx.x, ns = M.ns;
        orth_push(M.ml, ps, pz, mx, M.s, M.z);
        if (tid < M.nq) {
            const int r = M.off[tid];
            if (ps) M.s[r] += 1.0 + mx[0];
            if (pz) M.z[r] += 1.0 + mx[1];
        }
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
        for (int k = 0; k < ns; k++) {                 // W'ds
            const int o = M.bo[k];
            congr(M.r + (o - Ms), 1, M.ds + o, M.tw + o, M.wa, M.order(k));
        }
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
        const int tid = threadIdx.x, Ms = M.Ms, ns = M.ns, N = M.N;
        orth_combine(M.ml, i, dtau, M.lm, M.z1, M.ds, M.dz, M.ws3, mx);
        cones_combine(M, i, dtau, mx);
        for (int k = Ms + tid; k < N; k += NT) {
            const double zk = M.dz[k] + dtau * M.z1[k];
            M.dz[k] = zk; M.ds[k] -= zk;
        }
        __syncthreads();
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
            eig2(M, ds, 1.0, dz, 1.0, m, M.sgs + (ol - Ms), M.sgz + (ol - Ms), ds, dz);
            mx[0] = fmax(mx[0], -M.sgs[ol - Ms]);
            mx[1] = fmax(mx[1], -M.sgz[ol - Ms]);
        }
        blk_reduce<2, true>(mx, M.red);                // the maximum over the three kinds
    }
    __device__ __forceinline__ void update(double step) const                       // misc.py:444-634; s = W'lmbda and z = W^-1 lmbda
    {
        const int tid = threadIdx.x, Ms = M.Ms, ns = M.ns;
        orth_update(M.ml, step, M.ds, M.dz, M.d, M.di, M.lm, M.s, M.z);
        cones_update(M, step);
        for (int k = 0; k < ns; k++) {
            const int o = M.bo[k], ol = M.bl[k], m = M.order(k);
            double *r = M.r + (o - Ms), *rti = M.rti + (o - Ms), *lm = M.lm + ol;
            const double *sgs = M.sgs + (ol - Ms), *sgz = M.sgz + (ol - Ms);
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
        for (int k = 0; k < ns; k++) {                 // W'ds
            const int o = M.bo[k];
            congr(M.r + (o - Ms), 1, M.ds + o, M.tw + o, M.wa, M.order(k));
        }
        for (int k = Ms + tid; k < N; k += NT) M.dz[k] = -M.rz[k] - M.tw[k];
    }
    // ds -= dz; dot := ds'dz in every thread; ws3 := ds o dz (save); both scaled by lmbda; mx as in max_step.  As in combine the
    // eigenvectors replace the 's' blocks and the eigenvalues stand in sgs, sgz for update().  z1 is not read.
    __device__ __forceinline__ void combine_qp(bool save, double &dot, double (&mx)[2]) const
    {
        const int tid = threadIdx.x, Ms = M.Ms, ns = M.ns, N = M.N;
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
        for (int k = 0; k < ns; k++) {
            const int o = M.bo[k], ol = M.bl[k], m = M.order(k);
            double *ds = M.ds + o, *dz = M.dz + o;
            const double *lm = M.lm + ol;
            if (save) {                                // sprod (misc_solvers.c:700-742): (ds dz + dz ds) / 2
                for (int e = tid; e < m * m; e += NT) {
                    const int ii = e % m, jj = e / m, aa = max(ii, jj), bb = min(ii, jj);
                    double t = 0.0;
                    for (int q = 0; q < m; q++) t += ds[aa + q * m] * dz[q + bb * m] + dz[aa + q * m] * ds[q + bb * m];
                    M.ws3[o + e] = 0.5 * t;
                }
                __syncthreads();
            }
            for (int e = tid; e < m * m; e += NT) {    // scale2 (misc_solvers.c:343-397)
                const double cc = sqrt(lm[e % m]) * sqrt(lm[e / m]);
                ds[e] = ds[e] / cc; dz[e] = dz[e] / cc;
            }
            __syncthreads();
            eig2(M, ds, 1.0, dz, 1.0, m, M.sgs + (ol - Ms), M.sgz + (ol - Ms), ds, dz);
            mx[0] = fmax(mx[0], -M.sgs[ol - Ms]);
            mx[1] = fmax(mx[1], -M.sgz[ol - Ms]);
        }
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
