// kvx_qp_batch_vjp / kvx_qp_batch_jvp and their _dev forms (include/kvxhip.h): the limits of k_qp_batch_diff
// (qp_batch_diff.hip), its launch, and after a reverse-mode launch k_batch_outer_sum for every matrix the members share.  The
// host entries go up, launch and come down through the pooled buffers of batch_host.hpp; q, h, b of the problem do not enter.
#include "batch_host.hpp"
#include "qp_batch_diff.hpp"

using namespace kvx;
using namespace kvx::batchhost;

namespace {

// What all four entries check before a device is asked for
int check(const char *who, const QpDiffArgs &a)
{
    if (a.B < 1 || a.B > 2147483647) return refuse(who, "1 <= B <= 2147483647 is required");
    if (a.n < 1 || a.n > QPB_MAX_N) return refuse(who, "1 <= n <= 64 is required");
    if (a.ml < 1 || a.ml > QPB_MAX_ML) return refuse(who, "1 <= ml <= 512 is required");
    if (a.p < 0 || a.p > a.n) return refuse(who, "0 <= p <= n is required");
    if (a.refinement < 0 || a.refinement > QPD_MAX_REFINEMENT) return refuse(who, "0 <= refinement <= 3 is required");
    const bool jvp = a.mode == QPD_JVP, eq = a.p > 0;
    if (!a.P || !a.G || (eq && !a.A)) return refuse(who, "a data pointer is NULL");
    if (!a.x || !a.s || !a.z || (eq && !a.y) || !a.solexit) return refuse(who, "a solution pointer is NULL");
    if (!jvp && !a.gx) return refuse(who, "the cotangent pointer is NULL");
    if (!a.ux || !a.uz || (eq && !a.uy) || (jvp && !a.us) || !a.exitc) return refuse(who, "a result pointer is NULL");
    const int64_t n = a.n, ml = a.ml, p = a.p;
    const Part parts[] = {{"P", a.sP, n * n}, {"G", a.sG, ml * n}, {"A", a.sA, p * n},
                          {"dP", jvp && a.dP ? a.sdP : 0, n * n}, {"dq", jvp && a.dq ? a.sdq : 0, n},
                          {"dG", jvp && a.dG ? a.sdG : 0, ml * n}, {"dh", jvp && a.dh ? a.sdh : 0, ml},
                          {"dA", jvp && eq && a.dA ? a.sdA : 0, p * n}, {"db", jvp && eq && a.db ? a.sdb : 0, p}};
    for (const auto &t : parts)
        if (t.stride != 0 && t.stride < t.size)
            return refuse(who, std::string("the member stride of ") + t.name + " is 0 or at least its size");
    if (qp_batch_diff_lds_bytes(a.n, a.ml, a.p) > qp_batch_lds_bytes(a.n, a.ml, a.p))
        return refuse(who, "the member does not fit where qp_batch fits");
    return KVX_OK;
}

// The launches of one call on device pointers: the members, then the sums for the matrices all members share
hipError_t launch(const QpDiffArgs &d)
{
    hipError_t e = launch_qp_batch_diff(nullptr, d);
    if (e != hipSuccess || d.mode != QPD_VJP) return e;
    if (d.gP && !d.sP) e = launch_batch_outer_sum(nullptr, d.B, d.n, d.n, d.ux, d.x, d.x, d.ux, 0.5, true, d.exitc, d.gP);
    if (e == hipSuccess && d.gG && !d.sG) e = launch_batch_outer_sum(nullptr, d.B, d.ml, d.n, d.uz, d.x, d.z, d.ux, 1.0, false, d.exitc, d.gG);
    if (e == hipSuccess && d.p > 0 && d.gA && !d.sA) e = launch_batch_outer_sum(nullptr, d.B, d.p, d.n, d.uy, d.x, d.y, d.ux, 1.0, false, d.exitc, d.gA);
    return e;
}

int run_host(const QpDiffArgs &h)
{
    const int64_t B = h.B, n = h.n, ml = h.ml, p = h.p;
    const bool jvp = h.mode == QPD_JVP;
    const auto extent = [&](int64_t stride, int64_t size) { return stride ? (B - 1) * stride + size : size; };
    const auto members = [&](int64_t stride, int64_t size) { return stride ? B * size : size; };      // of a matrix gradient
    QpDiffArgs d = h;
    Buffers buf;
    int rc;
    const auto up = [&](const double *QpDiffArgs::*f, int64_t count) { return h.*f ? buf.up(&(d.*f), h.*f, count) : KVX_OK; };
    const auto get = [&](double *QpDiffArgs::*f, int64_t count) { return h.*f ? buf.get(&(d.*f), count) : KVX_OK; };
    const double *xin = nullptr, *yin = nullptr, *sin = nullptr, *zin = nullptr, *ein = nullptr;
    double *eout = nullptr;                                        // int64 travels in 8-byte slots of the same pool
    if ((rc = up(&QpDiffArgs::P, extent(h.sP, n * n))) || (rc = buf.up(&d.G, h.G, extent(h.sG, ml * n))) ||
        (p > 0 && (rc = buf.up(&d.A, h.A, extent(h.sA, p * n)))) || (rc = buf.up(&xin, h.x, n * B)) ||
        (p > 0 && (rc = buf.up(&yin, h.y, p * B))) || (rc = buf.up(&sin, h.s, ml * B)) || (rc = buf.up(&zin, h.z, ml * B)) ||
        (rc = buf.up(&ein, reinterpret_cast<const double *>(h.solexit), B)) || (rc = buf.get(&eout, B)))
        return rc;
    d.x = const_cast<double *>(xin); d.y = const_cast<double *>(yin); d.s = const_cast<double *>(sin); d.z = const_cast<double *>(zin);
    d.solexit = reinterpret_cast<const int64_t *>(ein);
    d.exitc = reinterpret_cast<int64_t *>(eout);
    if (jvp) {
        if ((rc = up(&QpDiffArgs::dP, extent(h.sdP, n * n))) || (rc = up(&QpDiffArgs::dq, extent(h.sdq, n))) ||
            (rc = up(&QpDiffArgs::dG, extent(h.sdG, ml * n))) || (rc = up(&QpDiffArgs::dh, extent(h.sdh, ml))) ||
            (p > 0 && ((rc = up(&QpDiffArgs::dA, extent(h.sdA, p * n))) || (rc = up(&QpDiffArgs::db, extent(h.sdb, p))))) ||
            (rc = get(&QpDiffArgs::us, ml * B)))
            return rc;
    } else {
        if ((rc = up(&QpDiffArgs::gx, n * B)) || (rc = get(&QpDiffArgs::gP, members(h.sP, n * n))) ||
            (rc = get(&QpDiffArgs::gG, members(h.sG, ml * n))) || (p > 0 && (rc = get(&QpDiffArgs::gA, members(h.sA, p * n)))))
            return rc;
    }
    if ((rc = get(&QpDiffArgs::ux, n * B)) || (p > 0 && (rc = get(&QpDiffArgs::uy, p * B))) || (rc = get(&QpDiffArgs::uz, ml * B)))
        return rc;
    HIPCHK(launch(d));
    HIPCHK(hipStreamSynchronize(nullptr));
    if ((rc = down(h.ux, d.ux, n * B)) || (p > 0 && (rc = down(h.uy, d.uy, p * B))) || (rc = down(h.uz, d.uz, ml * B)) ||
        (rc = down(h.exitc, d.exitc, B)))
        return rc;
    if (jvp) return down(h.us, d.us, ml * B);
    if ((h.gP && (rc = down(h.gP, d.gP, members(h.sP, n * n)))) || (h.gG && (rc = down(h.gG, d.gG, members(h.sG, ml * n)))) ||
        (p > 0 && h.gA && (rc = down(h.gA, d.gA, members(h.sA, p * n)))))
        return rc;
    return KVX_OK;
}

int run(const char *who, bool resident, const QpDiffArgs &a)
{
    int rc = check(who, a);
    if (rc || (rc = need_device(who))) return rc;
    return resident ? solve_dev(a, launch) : run_host(a);
}

// The arguments all four entries share, as the C ABI passes them
QpDiffArgs pack_diff(int mode, int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *G, int64_t sG,
                     const double *A, int64_t sA, const double *x, const double *y, const double *s, const double *z,
                     const int64_t *exitcode, int64_t refinement, double *ux, double *uy, double *uz, int64_t *gexit)
{
    QpDiffArgs a = pack<QpDiffArgs>(B, n, ml, p, nullptr, 0, G, sG, nullptr, 0, A, sA, nullptr, 0, refinement, 0.0, 0.0, 0.0,
                                    const_cast<double *>(x), const_cast<double *>(y), const_cast<double *>(s), const_cast<double *>(z),
                                    nullptr, nullptr, gexit);
    a.P = P; a.sP = sP; a.solexit = exitcode; a.mode = mode; a.refinement = a.maxiters;
    a.ux = ux; a.uy = uy; a.uz = uz;
    return a;
}

QpDiffArgs pack_vjp(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *G, int64_t sG, const double *A,
                    int64_t sA, const double *x, const double *y, const double *s, const double *z, const int64_t *exitcode,
                    int64_t refinement, const double *gx, double *ux, double *uy, double *uz, double *gP, double *gG, double *gA,
                    int64_t *gexit)
{
    QpDiffArgs a = pack_diff(QPD_VJP, B, n, ml, p, P, sP, G, sG, A, sA, x, y, s, z, exitcode, refinement, ux, uy, uz, gexit);
    a.gx = gx; a.gP = gP; a.gG = gG; a.gA = gA;
    return a;
}

QpDiffArgs pack_jvp(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *G, int64_t sG, const double *A,
                    int64_t sA, const double *x, const double *y, const double *s, const double *z, const int64_t *exitcode,
                    int64_t refinement, const double *dP, int64_t sdP, const double *dq, int64_t sdq, const double *dG, int64_t sdG,
                    const double *dh, int64_t sdh, const double *dA, int64_t sdA, const double *db, int64_t sdb, double *dx, double *dy,
                    double *dz, double *ds, int64_t *gexit)
{
    QpDiffArgs a = pack_diff(QPD_JVP, B, n, ml, p, P, sP, G, sG, A, sA, x, y, s, z, exitcode, refinement, dx, dy, dz, gexit);
    a.dP = dP; a.sdP = sdP; a.dq = dq; a.sdq = sdq; a.dG = dG; a.sdG = sdG; a.dh = dh; a.sdh = sdh;
    a.dA = dA; a.sdA = sdA; a.db = db; a.sdb = sdb; a.us = ds;
    return a;
}

}  // namespace

extern "C" {

int kvx_qp_batch_vjp(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *G, int64_t sG,
                     const double *A, int64_t sA, const double *x, const double *y, const double *s, const double *z,
                     const int64_t *exitcode, int64_t refinement, const double *gx, double *ux, double *uy, double *uz, double *gP,
                     double *gG, double *gA, int64_t *gexit)
{
    return guarded([&] {
        return run("kvx_qp_batch_vjp", false,
                   pack_vjp(B, n, ml, p, P, sP, G, sG, A, sA, x, y, s, z, exitcode, refinement, gx, ux, uy, uz, gP, gG, gA, gexit));
    });
}

int kvx_qp_batch_vjp_dev(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *G, int64_t sG,
                         const double *A, int64_t sA, const double *x, const double *y, const double *s, const double *z,
                         const int64_t *exitcode, int64_t refinement, const double *gx, double *ux, double *uy, double *uz, double *gP,
                         double *gG, double *gA, int64_t *gexit)
{
    return guarded([&] {
        return run("kvx_qp_batch_vjp_dev", true,
                   pack_vjp(B, n, ml, p, P, sP, G, sG, A, sA, x, y, s, z, exitcode, refinement, gx, ux, uy, uz, gP, gG, gA, gexit));
    });
}

int kvx_qp_batch_jvp(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *G, int64_t sG,
                     const double *A, int64_t sA, const double *x, const double *y, const double *s, const double *z,
                     const int64_t *exitcode, int64_t refinement, const double *dP, int64_t sdP, const double *dq, int64_t sdq,
                     const double *dG, int64_t sdG, const double *dh, int64_t sdh, const double *dA, int64_t sdA, const double *db,
                     int64_t sdb, double *dx, double *dy, double *dz, double *ds, int64_t *gexit)
{
    return guarded([&] {
        return run("kvx_qp_batch_jvp", false,
                   pack_jvp(B, n, ml, p, P, sP, G, sG, A, sA, x, y, s, z, exitcode, refinement, dP, sdP, dq, sdq, dG, sdG, dh, sdh, dA,
                            sdA, db, sdb, dx, dy, dz, ds, gexit));
    });
}

int kvx_qp_batch_jvp_dev(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *G, int64_t sG,
                         const double *A, int64_t sA, const double *x, const double *y, const double *s, const double *z,
                         const int64_t *exitcode, int64_t refinement, const double *dP, int64_t sdP, const double *dq, int64_t sdq,
                         const double *dG, int64_t sdG, const double *dh, int64_t sdh, const double *dA, int64_t sdA, const double *db,
                         int64_t sdb, double *dx, double *dy, double *dz, double *ds, int64_t *gexit)
{
    return guarded([&] {
        return run("kvx_qp_batch_jvp_dev", true,
                   pack_jvp(B, n, ml, p, P, sP, G, sG, A, sA, x, y, s, z, exitcode, refinement, dP, sdP, dq, sdq, dG, sdG, dh, sdh, dA,
                            sdA, db, sdb, dx, dy, dz, ds, gexit));
    });
}

int64_t kvx_qp_batch_diff_lds_bytes(int64_t n, int64_t ml, int64_t p, int64_t *forward)
{
    if (n < 1 || n > QPB_MAX_N || ml < 1 || ml > QPB_MAX_ML || p < 0 || p > n) return -1;
    if (forward) *forward = (int64_t)qp_batch_lds_bytes((int)n, (int)ml, (int)p);
    return (int64_t)qp_batch_diff_lds_bytes((int)n, (int)ml, (int)p);
}

}  // extern "C"
