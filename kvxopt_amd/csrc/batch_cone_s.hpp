// The 's' (semidefinite cone) operations of the batch interior-point kernels, each written once: k_sdp_batch (sdp_batch.hip)
// and, through batch_cone.hpp, k_conelp_batch and k_coneqp_batch run them.  They are the reference's own operations, the ones
// csrc/kkt_s.hip carries as stand-alone kernels: misc.compute_scaling / update_scaling (misc.py:354-419, 582-634), scale, scale2,
// sprod, sinv, sdot and max_step (misc_solvers.c:188-240, 343-397, 700-770, 845-882, 1029-1046, 1086-1160).
//
// This file is text of its includer: it is included once, inside the anonymous namespace of kvx, after `using namespace
// batchdev` (NT, NW, wave_sum, blk_reduce) and after the includer's `constexpr int MAX_M` (the largest order of a block,
// MAX_M * MAX_M <= NT) and `constexpr int SWEEPS` (the cap on the sweeps of one Jacobi iteration), so every kernel keeps its own
// internal copy of these functions.  It needs <cmath>.
//
// A function that reads a member is a template on the member type and uses only what every includer's Member has: n, N, G, ml,
// ns, Np, bo, bl, order(k), r, rti, lm, s, z, ds, dz, ws3, sgs, sgz, the four work matrices wa .. wd, nrm (2 MAX_M doubles), red,
// flag, prow, pmir, and first_s(), the first 's' row: r, rti, sgs and sgz are indexed from it.
//
// A block is its full symmetric m x m matrix in LDS, column-major with leading dimension m, and belongs to the workgroup, one
// block after the other: a thread per entry in the products, the Cholesky factors and the congruences, and in the one-sided
// Jacobi iteration (round-robin order of kkt_s.hip) sixteen lanes per column pair, so the eight pairs of a round of an order-16
// block take half the workgroup and the other half carries a second matrix between the same barriers.  Every block operation
// writes both triangles from one computed value, so the blocks stay symmetric to the bit.  A block that is not finite is not
// iterated on.  The loops over blocks are the same for every thread.

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
// rotations from the identity.  Group g = tid / 16 takes pair g % 8 of matrix g / 8, lane l of the group row l.  A pair's three
// inner products are taken by sum16, so a block's result depends on its entries and its order alone; a matrix that has
// converged takes no further rotation while its partner finishes.  Whether a sweep rotated anything is a flag that the
// rotating pairs set, never a count.
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
    for (int sweep = 0; sweep < SWEEPS; sweep++) {
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

// ---- what reads a member

// The eigenvalues (ascending) of a0 X0 and a1 X1 into sig0 and sig1 and, with Q0, Q1, their eigenvectors there (Q may be X): the
// 's' part of misc.max_step (misc_solvers.c:1086-1160), by the same iteration on x + 1.5 |x|_F I (kkt_s.hip's shift).  Barriers
// before (the caller's) and after.
template <class Mem>
__device__ __forceinline__ void eig2(const Mem &M, const double *X0, double a0, const double *X1, double a1, int m, double *sig0,
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
    collect(ok1 ? M.wb : nullptr, nullptr, m, false, c1, M.nrm + MAX_M, sig1, Q1, nullptr);
}

// mx[0], mx[1] := the larger of themselves and -lambda_min over the 's' blocks of a0 u0 and a1 u1, by every thread.  Barriers
// before (the caller's) and after.
template <class Mem>
__device__ __forceinline__ void blocks_max_step(const Mem &M, const double *u0, double a0, const double *u1, double a1, double (&mx)[2])
{
    for (int k = 0; k < M.ns; k++) {
        const int o = M.bo[k], ol = M.bl[k] - M.first_s(), m = M.order(k);
        eig2(M, u0 + o, a0, u1 + o, a1, m, M.sgs + ol, M.sgz + ol, nullptr, nullptr);
        mx[0] = fmax(mx[0], -M.sgs[ol]);
        mx[1] = fmax(mx[1], -M.sgz[ol]);
    }
}

// misc.compute_scaling on the 's' blocks (misc.py:354-419): r_k, rti_k and lmbda_k from s_k and z_k.  false when an s_k or z_k is
// not positive definite.  Barriers before (the caller's) and after.
template <class Mem>
__device__ __forceinline__ bool blocks_scaling(const Mem &M)
{
    for (int k = 0; k < M.ns; k++) {
        const int o = M.bo[k], ol = M.bl[k], m = M.order(k);
        double *r = M.r + (o - M.first_s()), *rti = M.rti + (o - M.first_s());
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

// out_k := R_k'X_k R_k (form 0) or R_k X_k R_k' (form 1) on every 's' block, X = in, R the member's r or rti: W, W', W^-1 or W^-T
// on the 's' rows (misc_solvers.c:188-240); in == out is allowed.  Every block ends with a barrier (congr).
template <class Mem>
__device__ __forceinline__ void blocks_congr(const Mem &M, const double *R, int form, const double *in, double *out)
{
    for (int k = 0; k < M.ns; k++) {
        const int o = M.bo[k];
        congr(R + (o - M.first_s()), form, in + o, out + o, M.wa, M.order(k));
    }
}

// 1 for a diagonal row or a row of another kind, 2 for an off-diagonal one: its weight in G'z and in the inner product of the cone
template <class Mem>
__device__ __forceinline__ double weight(const Mem &M, int j) { return M.prow[j] != M.pmir[j] ? 2.0 : 1.0; }

// v[c] += sign * sum over the packed rows j of G(row_j, c) weight_j u[row_j] (misc.sgemv, trans 'T'): a wavefront per column
template <class Mem>
__device__ __forceinline__ void gemv_t_packed(const Mem &M, const double *u, double sign, double *v)
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
template <class Mem>
__device__ __forceinline__ void load_sym(const Mem &M, const double *v, double *out)
{
    for (int j = threadIdx.x; j < M.Np; j += NT) { const double t = v[M.prow[j]]; out[M.prow[j]] = t; out[M.pmir[j]] = t; }
}

struct PackedRow {                            // a packed row of the cone: its entry, its mirror image, its weight
    int k, mir;
    double wq;
    __device__ __forceinline__ double w(double v) const { return wq * v; }
    __device__ __forceinline__ void put(double *vec, double v) const { vec[k] = v; vec[mir] = v; }
};

// ---- the 's' rows of the policy's operations

// r_k = rti_k = I.  No barrier.
template <class Mem>
__device__ __forceinline__ void blocks_identity(const Mem &M)
{
    const int tid = threadIdx.x, ns = M.ns;
    for (int k = 0; k < ns; k++) {
        const int o = M.bo[k] - M.first_s(), m = M.order(k);
        for (int e = tid; e < m * m; e += NT) { const double v = (e % m == e / m) ? 1.0 : 0.0; M.r[o + e] = v; M.rti[o + e] = v; }
    }
}

// s_k += (1 + mx[0]) I (ps), z_k += (1 + mx[1]) I (pz).  No barrier.
template <class Mem>
__device__ __forceinline__ void blocks_push(const Mem &M, bool ps, bool pz, const double (&mx)[2])
{
    const int tid = threadIdx.x, ns = M.ns;
    for (int k = 0; k < ns; k++) {
        const int m = M.order(k), r = M.bo[k] + tid * (m + 1);
        if (tid < m) {
            if (ps) M.s[r] += 1.0 + mx[0];
            if (pz) M.z[r] += 1.0 + mx[1];
        }
    }
}

// The 's' rows of ds of the right-hand side: sinv with the diagonal lmbda_k (misc_solvers.c:845-882).  No barrier.
template <class Mem>
__device__ __forceinline__ void blocks_sinv(const Mem &M, int i, double sigma, double mu)
{
    const int tid = threadIdx.x, ns = M.ns;
    for (int k = 0; k < ns; k++) {
        const int o = M.bo[k], m = M.order(k);
        const double *lm = M.lm + M.bl[k];
        for (int e = tid; e < m * m; e += NT) {
            const int ii = e % m, jj = e / m;
            double t = ii == jj ? lm[ii] * lm[ii] : 0.0;
            if (i == 1) t += M.ws3[o + e] - (ii == jj ? sigma * mu : 0.0);
            M.ds[o + e] = -(t / ((lm[ii] + lm[jj]) / 2.0));
        }
    }
}

// The 's' rows of combine once ds and dz are there: ws3 = ds o dz (save), both scaled by lmbda, mx as in blocks_max_step.  The
// eigenvalues stand in sgs, sgz and the eigenvectors replace the blocks (coneprog.py:1308-1321); blocks_update consumes both.
// Barriers before (the caller's) and after.
template <class Mem>
__device__ __forceinline__ void blocks_combine(const Mem &M, bool save, double (&mx)[2])
{
    const int tid = threadIdx.x, ns = M.ns, Ms = M.first_s();
    for (int k = 0; k < ns; k++) {
        const int o = M.bo[k], ol = M.bl[k], m = M.order(k);
        double *ds = M.ds + o, *dz = M.dz + o;
        const double *lm = M.lm + ol;
        if (save) {                                // sprod (misc_solvers.c:700-742): (ds dz + dz ds) / 2
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
        eig2(M, ds, 1.0, dz, 1.0, m, M.sgs + (ol - Ms), M.sgz + (ol - Ms), ds, dz);
        mx[0] = fmax(mx[0], -M.sgs[ol - Ms]);
        mx[1] = fmax(mx[1], -M.sgz[ol - Ms]);
    }
}

// misc.update_scaling on the 's' blocks (misc.py:582-634), then s = W'lmbda and z = W^-1 lmbda.  Barriers before (the caller's)
// and after.
template <class Mem>
__device__ __forceinline__ void blocks_update(const Mem &M, double step)
{
    const int tid = threadIdx.x, ns = M.ns, Ms = M.first_s();
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
