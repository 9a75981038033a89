// The 'q' (second-order cone) operations of the batch interior-point kernels, each written once: k_socp_batch (socp_batch.hip)
// and, through batch_cone.hpp, k_conelp_batch and k_coneqp_batch run them.  They are the reference's own operations, the ones
// csrc/kkt_q.hip carries as stand-alone kernels: misc.compute_scaling / update_scaling (misc.py:290-352, 467-580), scale, scale2,
// sprod, sinv (misc_solvers.c:144-186, 301-341, 671-700, 803-835) and max_step (misc_solvers.c:1073-1085).
//
// This file is text of its includer: it is included once, inside the anonymous namespace of kvx, after `using namespace
// batchdev` (NT, NW, wave_sum), so every kernel keeps its own internal copy of these functions.  It needs <cmath>.
//
// A function that reads a member is a template on the member type and uses only what every includer's Member has: nq, off
// (off[k]: the first row of cone k; off[nq]: the row behind the last), d (v_k in the 'q' rows), lm (lmbda_k in the same rows),
// beta, s, z, ds, dz, rz, ws3, z1.
//
// A cone belongs to one wavefront at a time: its lanes run along the rows, a lane adds its rows ascending, the lanes add by the
// xor butterfly of batch_device.hpp.  The order of a cone's sums depends on its order m_k alone.  A lane reads, of what its
// wavefront writes in one pass over a cone, only the rows it wrote itself; the first row's values travel in registers.  No
// function here has a barrier.

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

// out := W^-1 in (INV) or W in on the 'q' rows; W_k is symmetric; in == out is allowed
template <bool INV, class Mem>
__device__ __forceinline__ void cones_wscale(const Mem &M, const double *in, double *out)
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
template <class Mem>
__device__ __forceinline__ void cones_max_step(const Mem &M, const double *u1, double a1, const double *u2, double a2, double (&mx)[2])
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

// misc.compute_scaling on the 'q' blocks (misc.py:290-352): v_k, beta_k and lmbda_k from s_k and z_k
template <class Mem>
__device__ __forceinline__ void cones_scaling(const Mem &M)
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

// The 'q' rows of the right-hand side: ds by sprod and sinv (misc_solvers.c:671-700, 803-835), dz with W'ds
template <class Mem>
__device__ __forceinline__ void cones_rhs(const Mem &M, int i, double sigma, double mu)
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

// The 'q' rows of combine: dz += dtau z1, ds -= dz, ws3 = ds o dz (i = 0), scale2 (misc_solvers.c:301-341), max_step
template <class Mem>
__device__ __forceinline__ void cones_combine(const Mem &M, int i, double dtau, double (&mx)[2])
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

// misc.update_scaling on the 'q' blocks (misc.py:467-580), then s = W'lmbda and z = W^-1 lmbda
template <class Mem>
__device__ __forceinline__ void cones_update(const Mem &M, double step)
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

// ---- coneqp: instantiated by coneqp_member (batch_coneqp.hpp) alone

// The 'q' rows of coneqp's right-hand side (coneprog.py:2376-2392, f4_no_ir :2288-2300): ds := lmbda o\ (-lmbda o lmbda + smu e
// [- ws3]) by sprod and sinv as in cones_rhs, dz := -rz - W'ds: rz enters whole, there is no (1 - sigma).  ws: with the
// Mehrotra term.
template <class Mem>
__device__ __forceinline__ void cones_rhs_qp(const Mem &M, bool ws, double smu)
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
// (misc_solvers.c:301-341), max_step.  It is cones_combine without dtau: z1 is not read.
template <class Mem>
__device__ __forceinline__ void cones_combine_qp(const Mem &M, bool save, double &dot, double (&mx)[2])
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
