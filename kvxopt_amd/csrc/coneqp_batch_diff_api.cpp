// kvx_coneqp_batch_vjp / kvx_coneqp_batch_jvp and their _dev forms (include/kvxhip.h): the limits of k_coneqp_batch_diff
// (coneqp_batch_diff.hip), which are those of kvx_coneqp_batch_solve, the placement of its cone, its launch, and after a
// reverse-mode launch k_batch_outer_sum (qp_batch_diff.hip) for every matrix the members share, on the centred x, y, z the kernel
// leaves in pooled buffers.  The host entries go up, launch and come down through the pooled buffers of batch_host.hpp.
#include "batch_host.hpp"
#include "coneqp_batch_diff.hpp"

using namespace kvx;
using namespace kvx::batchhost;

namespace {

// the cone into the kernel's arguments; the orders are in range (check)
void place(ConeqpDiffArgs &a, int64_t nq, const int64_t *q, int64_t ns, const int64_t *m)
{
    a.nq = (int)nq;
    a.ns = (int)ns;
    a.Ms = a.ml;
    for (int64_t k = 0; k < CONEB_MAX_NQ; k++) a.q[k] = k < nq ? (unsigned short)q[k] : 0;
    for (int64_t k = 0; k < CONEB_MAX_NS; k++) a.m[k] = k < ns ? (unsigned char)m[k] : 0;
    for (int64_t k = 0; k < nq; k++) a.Ms += (int)q[k];
    a.N = a.Nd = a.Np = a.Ms;
    for (int64_t k = 0; k < ns; k++) {
        a.N += (int)(m[k] * m[k]);
        a.Nd += (int)m[k];
        a.Np += (int)((m[k] * (m[k] + 1)) / 2);
    }
}

// What all four entries check before a device is asked for; on success the cone is placed in `a`
int check(const char *who, ConeqpDiffArgs &a, int64_t nq, const int64_t *q, int64_t ns, const int64_t *m)
{
    if (a.B < 1 || a.B > 2147483647) return refuse(who, "1 <= B <= 2147483647 is required");
    if (a.n < 1 || a.n > CONEB_MAX_N) return refuse(who, "1 <= n <= 64 is required");
    if (a.ml < 0 || a.ml > CONEB_MAX_ROWS) return refuse(who, "0 <= ml <= 384 is required");
    if (nq < 0 || nq > CONEB_MAX_NQ) return refuse(who, "0 <= nq <= 128 is required");
    if (nq > 0 && !q) return refuse(who, "the cone orders q are NULL");
    if (ns < 0 || ns > CONEB_MAX_NS) return refuse(who, "0 <= ns <= 32 is required");
    if (ns > 0 && !m) return refuse(who, "the block orders m are NULL");
    int64_t N = a.ml;
    for (int64_t k = 0; k < nq; k++) {
        if (q[k] < 1 || q[k] > CONEB_MAX_ROWS) return refuse(who, "every cone order is at least 1 and at most 384");
        N += q[k];
    }
    for (int64_t k = 0; k < ns; k++) {
        if (m[k] < 1 || m[k] > CONEB_MAX_M) return refuse(who, "every block order is at least 1 and at most 16");
        N += m[k] * m[k];
    }
    if (N < 1 || N > CONEB_MAX_ROWS) return refuse(who, "1 <= N = ml + sum(q) + sum(m^2) <= 384 is required");
    if (a.p < 0 || a.p > a.n) return refuse(who, "0 <= p <= n is required");
    if (a.refinement < 0 || a.refinement > QPD_MAX_REFINEMENT) return refuse(who, "0 <= refinement <= 3 is required");
    if (a.centering < 0 || a.centering > CQD_MAX_CENTERING) return refuse(who, "0 <= centering <= 16 is required");
    if (!(a.centol > 0.0)) return refuse(who, "centol must be a positive scalar");
    place(a, nq, q, ns, m);
    if (coneqp_batch_diff_lds_bytes(a.n, a.ml, a.nq, a.q, a.ns, a.m, a.p) > 160 * 1024)
        return refuse(who, "the member needs more than 160 KiB of LDS");
    const bool jvp = a.mode == QPD_JVP, eq = a.p > 0;
    if (!a.P || !a.c || !a.G || !a.h || (eq && (!a.A || !a.b))) return refuse(who, "a data pointer is NULL");
    if (!a.x || !a.s || !a.z || (eq && !a.y) || !a.solexit) return refuse(who, "a solution pointer is NULL");
    if (!jvp && !a.gx) return refuse(who, "the cotangent pointer is NULL");
    if (!a.ux || !a.uz || (eq && !a.uy) || (jvp && !a.us) || !a.centrality || !a.steps || !a.exitc)
        return refuse(who, "a result pointer is NULL");
    const int64_t n = a.n, p = a.p;
    const Part parts[] = {{"P", a.sP, n * n}, {"q", a.sc, n}, {"G", a.sG, N * n}, {"h", a.sh, N}, {"A", a.sA, p * n}, {"b", a.sb, p},
                          {"dP", jvp && a.dP ? a.sdP : 0, n * n}, {"dq", jvp && a.dq ? a.sdq : 0, n},
                          {"dG", jvp && a.dG ? a.sdG : 0, N * n}, {"dh", jvp && a.dh ? a.sdh : 0, N},
                          {"dA", jvp && eq && a.dA ? a.sdA : 0, p * n}, {"db", jvp && eq && a.db ? a.sdb : 0, p}};
    for (const auto &t : parts)
        if (t.stride != 0 && t.stride < t.size)
            return refuse(who, std::string("the member stride of ") + t.name + " is 0 or at least its size");
    return KVX_OK;
}

// The launches of one call on device pointers and their synchronisation: the members, then the sums for the matrices all
// members share, which read the centred point from pooled buffers that live until the synchronisation.
int launch(ConeqpDiffArgs d)
{
    const bool vjp = d.mode == QPD_VJP;
    const bool sumP = vjp && d.gP && !d.sP, sumG = vjp && d.gG && !d.sG, sumA = vjp && d.p > 0 && d.gA && !d.sA;
    Buffers buf;
    int rc;
    if (sumP || sumG || sumA) {
        if ((rc = buf.get(&d.xc, d.n * d.B)) || (sumG && (rc = buf.get(&d.zc, d.N * d.B))) || (sumA && (rc = buf.get(&d.yc, d.p * d.B))))
            return rc;
    }
    HIPCHK(launch_coneqp_batch_diff(nullptr, d));
    if (sumP) HIPCHK(launch_batch_outer_sum(nullptr, d.B, d.n, d.n, d.ux, d.xc, d.xc, d.ux, 0.5, true, d.exitc, d.gP));
    if (sumG) HIPCHK(launch_batch_outer_sum(nullptr, d.B, d.N, d.n, d.uz, d.xc, d.zc, d.ux, 1.0, false, d.exitc, d.gG));
    if (sumA) HIPCHK(launch_batch_outer_sum(nullptr, d.B, d.p, d.n, d.uy, d.xc, d.yc, d.ux, 1.0, false, d.exitc, d.gA));
    HIPCHK(hipStreamSynchronize(nullptr));
    return KVX_OK;
}

int run_host(const ConeqpDiffArgs &h)
{
    const int64_t B = h.B, n = h.n, N = h.N, p = h.p;
    const bool jvp = h.mode == QPD_JVP;
    const auto extent = [&](int64_t stride, int64_t size) { return stride ? (B - 1) * stride + size : size; };
    const auto members = [&](int64_t stride, int64_t size) { return stride ? B * size : size; };      // of a matrix gradient
    ConeqpDiffArgs d = h;
    Buffers buf;
    int rc;
    const auto up = [&](const double *ConeqpDiffArgs::*f, int64_t count) { return h.*f ? buf.up(&(d.*f), h.*f, count) : KVX_OK; };
    const auto get = [&](double *ConeqpDiffArgs::*f, int64_t count) { return h.*f ? buf.get(&(d.*f), count) : KVX_OK; };
    const double *xin = nullptr, *yin = nullptr, *sin = nullptr, *zin = nullptr, *ein = nullptr;
    double *eout = nullptr, *sout = nullptr;                       // int64 travels in 8-byte slots of the same pool
    if ((rc = buf.up(&d.P, h.P, extent(h.sP, n * n))) || (rc = buf.up(&d.c, h.c, extent(h.sc, n))) ||
        (rc = buf.up(&d.G, h.G, extent(h.sG, N * n))) || (rc = buf.up(&d.h, h.h, extent(h.sh, N))) ||
        (p > 0 && ((rc = buf.up(&d.A, h.A, extent(h.sA, p * n))) || (rc = buf.up(&d.b, h.b, extent(h.sb, p))))) ||
        (rc = buf.up(&xin, h.x, n * B)) || (p > 0 && (rc = buf.up(&yin, h.y, p * B))) || (rc = buf.up(&sin, h.s, N * B)) ||
        (rc = buf.up(&zin, h.z, N * B)) || (rc = buf.up(&ein, reinterpret_cast<const double *>(h.solexit), B)) ||
        (rc = buf.get(&eout, B)) || (rc = buf.get(&sout, B)) || (rc = buf.get(&d.centrality, B)))
        return rc;
    d.x = const_cast<double *>(xin); d.y = const_cast<double *>(yin); d.s = const_cast<double *>(sin); d.z = const_cast<double *>(zin);
    d.solexit = reinterpret_cast<const int64_t *>(ein);
    d.exitc = reinterpret_cast<int64_t *>(eout);
    d.steps = reinterpret_cast<int64_t *>(sout);
    if (jvp) {
        if ((rc = up(&ConeqpDiffArgs::dP, extent(h.sdP, n * n))) || (rc = up(&ConeqpDiffArgs::dq, extent(h.sdq, n))) ||
            (rc = up(&ConeqpDiffArgs::dG, extent(h.sdG, N * n))) || (rc = up(&ConeqpDiffArgs::dh, extent(h.sdh, N))) ||
            (p > 0 && ((rc = up(&ConeqpDiffArgs::dA, extent(h.sdA, p * n))) || (rc = up(&ConeqpDiffArgs::db, extent(h.sdb, p))))) ||
            (rc = get(&ConeqpDiffArgs::us, N * B)))
            return rc;
    } else {
        if ((rc = up(&ConeqpDiffArgs::gx, n * B)) || (rc = get(&ConeqpDiffArgs::gP, members(h.sP, n * n))) ||
            (rc = get(&ConeqpDiffArgs::gG, members(h.sG, N * n))) || (p > 0 && (rc = get(&ConeqpDiffArgs::gA, members(h.sA, p * n)))))
            return rc;
    }
    if ((rc = get(&ConeqpDiffArgs::ux, n * B)) || (p > 0 && (rc = get(&ConeqpDiffArgs::uy, p * B))) || (rc = get(&ConeqpDiffArgs::uz, N * B)))
        return rc;
    if ((rc = launch(d))) return rc;
    if ((rc = down(h.ux, d.ux, n * B)) || (p > 0 && (rc = down(h.uy, d.uy, p * B))) || (rc = down(h.uz, d.uz, N * B)) ||
        (rc = down(h.exitc, d.exitc, B)) || (rc = down(h.steps, d.steps, B)) || (rc = down(h.centrality, d.centrality, B)))
        return rc;
    if (jvp) return down(h.us, d.us, N * B);
    if ((h.gP && (rc = down(h.gP, d.gP, members(h.sP, n * n)))) || (h.gG && (rc = down(h.gG, d.gG, members(h.sG, N * n)))) ||
        (p > 0 && h.gA && (rc = down(h.gA, d.gA, members(h.sA, p * n)))))
        return rc;
    return KVX_OK;
}

int run(const char *who, bool resident, ConeqpDiffArgs a, int64_t nq, const int64_t *q, int64_t ns, const int64_t *m)
{
    int rc = check(who, a, nq, q, ns, m);
    if (rc || (rc = need_device(who))) return rc;
    return resident ? launch(a) : run_host(a);
}

// The arguments all four entries share, as the C ABI passes them
ConeqpDiffArgs pack_diff(int mode, int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *q, int64_t sq,
                         const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb,
                         const double *x, const double *y, const double *s, const double *z, const int64_t *exitcode,
                         int64_t refinement, int64_t centering, double centol, double *ux, double *uy, double *uz, double *centrality,
                         int64_t *steps, int64_t *gexit)
{
    ConeqpDiffArgs a = pack<ConeqpDiffArgs>(B, n, ml, p, q, sq, G, sG, h, sh, A, sA, b, sb, refinement, 0.0, 0.0, 0.0,
                                            const_cast<double *>(x), const_cast<double *>(y), const_cast<double *>(s),
                                            const_cast<double *>(z), nullptr, nullptr, gexit);
    a.P = P; a.sP = sP; a.solexit = exitcode; a.mode = mode; a.refinement = a.maxiters;
    a.centering = (int)(centering < -1 ? -1 : (centering > 1000000000 ? 1000000000 : centering));
    a.centol = centol;
    a.ux = ux; a.uy = uy; a.uz = uz; a.centrality = centrality; a.steps = steps;
    return a;
}

}  // namespace

#define CQD_PROBLEM                                                                                                                  \
    int64_t B, int64_t n, int64_t ml, int64_t nq, const int64_t *qdims, int64_t ns, const int64_t *m, int64_t p, const double *P,   \
        int64_t sP, const double *q, int64_t sq, const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, \
        const double *b, int64_t sb, const double *x, const double *y, const double *s, const double *z, const int64_t *exitcode,   \
        int64_t refinement, int64_t centering, double centol

namespace {

int vjp(const char *who, bool resident, CQD_PROBLEM, const double *gx, double *ux, double *uy, double *uz, double *gP, double *gG,
        double *gA, double *centrality, int64_t *steps, int64_t *gexit)
{
    return guarded([&] {
        ConeqpDiffArgs a = pack_diff(QPD_VJP, B, n, ml, p, P, sP, q, sq, G, sG, h, sh, A, sA, b, sb, x, y, s, z, exitcode, refinement,
                                     centering, centol, ux, uy, uz, centrality, steps, gexit);
        a.gx = gx; a.gP = gP; a.gG = gG; a.gA = gA;
        return run(who, resident, a, nq, qdims, ns, m);
    });
}

int jvp(const char *who, bool resident, CQD_PROBLEM, const double *dP, int64_t sdP, const double *dq, int64_t sdq, const double *dG,
        int64_t sdG, const double *dh, int64_t sdh, const double *dA, int64_t sdA, const double *db, int64_t sdb, double *dx, double *dy,
        double *dz, double *ds, double *centrality, int64_t *steps, int64_t *gexit)
{
    return guarded([&] {
        ConeqpDiffArgs a = pack_diff(QPD_JVP, B, n, ml, p, P, sP, q, sq, G, sG, h, sh, A, sA, b, sb, x, y, s, z, exitcode, refinement,
                                     centering, centol, dx, dy, dz, centrality, steps, gexit);
        a.dP = dP; a.sdP = sdP; a.dq = dq; a.sdq = sdq; a.dG = dG; a.sdG = sdG; a.dh = dh; a.sdh = sdh;
        a.dA = dA; a.sdA = sdA; a.db = db; a.sdb = sdb; a.us = ds;
        return run(who, resident, a, nq, qdims, ns, m);
    });
}

}  // namespace

#define CQD_PROBLEM_ARGS                                                                                                             \
    B, n, ml, nq, qdims, ns, m, p, P, sP, q, sq, G, sG, h, sh, A, sA, b, sb, x, y, s, z, exitcode, refinement, centering, centol

extern "C" {

int kvx_coneqp_batch_vjp(CQD_PROBLEM, const double *gx, double *ux, double *uy, double *uz, double *gP, double *gG, double *gA,
                         double *centrality, int64_t *steps, int64_t *gexit)
{
    return vjp("kvx_coneqp_batch_vjp", false, CQD_PROBLEM_ARGS, gx, ux, uy, uz, gP, gG, gA, centrality, steps, gexit);
}

int kvx_coneqp_batch_vjp_dev(CQD_PROBLEM, const double *gx, double *ux, double *uy, double *uz, double *gP, double *gG, double *gA,
                             double *centrality, int64_t *steps, int64_t *gexit)
{
    return vjp("kvx_coneqp_batch_vjp_dev", true, CQD_PROBLEM_ARGS, gx, ux, uy, uz, gP, gG, gA, centrality, steps, gexit);
}

int kvx_coneqp_batch_jvp(CQD_PROBLEM, const double *dP, int64_t sdP, const double *dq, int64_t sdq, const double *dG, int64_t sdG,
                         const double *dh, int64_t sdh, const double *dA, int64_t sdA, const double *db, int64_t sdb, double *dx,
                         double *dy, double *dz, double *ds, double *centrality, int64_t *steps, int64_t *gexit)
{
    return jvp("kvx_coneqp_batch_jvp", false, CQD_PROBLEM_ARGS, dP, sdP, dq, sdq, dG, sdG, dh, sdh, dA, sdA, db, sdb, dx, dy, dz, ds,
               centrality, steps, gexit);
}

int kvx_coneqp_batch_jvp_dev(CQD_PROBLEM, const double *dP, int64_t sdP, const double *dq, int64_t sdq, const double *dG, int64_t sdG,
                             const double *dh, int64_t sdh, const double *dA, int64_t sdA, const double *db, int64_t sdb, double *dx,
                             double *dy, double *dz, double *ds, double *centrality, int64_t *steps, int64_t *gexit)
{
    return jvp("kvx_coneqp_batch_jvp_dev", true, CQD_PROBLEM_ARGS, dP, sdP, dq, sdq, dG, sdG, dh, sdh, dA, sdA, db, sdb, dx, dy, dz, ds,
               centrality, steps, gexit);
}

int64_t kvx_coneqp_batch_diff_lds_bytes(int64_t n, int64_t ml, int64_t nq, const int64_t *qdims, int64_t ns, const int64_t *m, int64_t p,
                                        int64_t *forward)
{
    ConeqpDiffArgs a = {};
    a.B = 1; a.n = (int)(n < -1 ? -1 : (n > 1000 ? 1000 : n)); a.ml = (int)(ml < -1 ? -1 : (ml > 100000 ? 100000 : ml));
    a.p = (int)(p < -1 ? -1 : (p > 1000 ? 1000 : p));
    if (a.n < 1 || a.n > CONEB_MAX_N || a.ml < 0 || a.ml > CONEB_MAX_ROWS || nq < 0 || nq > CONEB_MAX_NQ || (nq > 0 && !qdims) || ns < 0 ||
        ns > CONEB_MAX_NS || (ns > 0 && !m) || a.p < 0 || a.p > a.n)
        return -1;
    int64_t N = a.ml;
    for (int64_t k = 0; k < nq; k++) { if (qdims[k] < 1 || qdims[k] > CONEB_MAX_ROWS) return -1; N += qdims[k]; }
    for (int64_t k = 0; k < ns; k++) { if (m[k] < 1 || m[k] > CONEB_MAX_M) return -1; N += m[k] * m[k]; }
    if (N < 1 || N > CONEB_MAX_ROWS) return -1;
    place(a, nq, qdims, ns, m);
    if (forward) *forward = (int64_t)coneqp_batch_lds_bytes(a.n, a.ml, a.nq, a.q, a.ns, a.m, a.p);
    return (int64_t)coneqp_batch_diff_lds_bytes(a.n, a.ml, a.nq, a.q, a.ns, a.m, a.p);
}

}  // extern "C"
