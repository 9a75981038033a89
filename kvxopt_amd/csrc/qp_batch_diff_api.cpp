// kvx_qp_batch_vjp / kvx_qp_batch_jvp and their _dev forms (include/kvxhip.h): the limits of k_qp_batch_diff
// (qp_batch_diff.hip), its launch, and after a reverse-mode launch k_batch_outer_sum for every matrix the members share.  The
// host entries go up, launch and come down through diff_host of batch_host.hpp; q, h, b of the problem do not enter.
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
    if (int rc = check_diff(who, a, a.ml, a.mode == QPD_JVP, false)) return rc;
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

int run(const char *who, bool resident, const QpDiffArgs &a)
{
    int rc = check(who, a);
    if (rc || (rc = need_device(who))) return rc;
    const auto synced = [](const QpDiffArgs &d) { return solve_dev(d, launch); };
    return resident ? synced(a) : diff_host(a, a.ml, a.mode == QPD_JVP, false, synced);
}

}  // namespace

#define QPD_PROBLEM                                                                                                                  \
    int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *G, int64_t sG, const double *A, int64_t sA, \
        const double *x, const double *y, const double *s, const double *z, const int64_t *exitcode, int64_t refinement
// the same, passed on to pack_diff: q, h and b do not enter
#define QPD_PROBLEM_ARGS B, n, ml, p, P, sP, nullptr, 0, G, sG, nullptr, 0, A, sA, nullptr, 0, x, y, s, z, exitcode, refinement

namespace {

int vjp(const char *who, bool resident, QPD_PROBLEM, const double *gx, double *ux, double *uy, double *uz, double *gP, double *gG,
        double *gA, int64_t *gexit)
{
    return guarded([&] {
        QpDiffArgs a = pack_diff<QpDiffArgs>(QPD_VJP, QPD_PROBLEM_ARGS, ux, uy, uz, gexit);
        set_vjp(a, gx, gP, gG, gA);
        return run(who, resident, a);
    });
}

int jvp(const char *who, bool resident, QPD_PROBLEM, const double *dP, int64_t sdP, const double *dq, int64_t sdq, const double *dG,
        int64_t sdG, const double *dh, int64_t sdh, const double *dA, int64_t sdA, const double *db, int64_t sdb, double *dx, double *dy,
        double *dz, double *ds, int64_t *gexit)
{
    return guarded([&] {
        QpDiffArgs a = pack_diff<QpDiffArgs>(QPD_JVP, QPD_PROBLEM_ARGS, dx, dy, dz, gexit);
        set_jvp(a, dP, sdP, dq, sdq, dG, sdG, dh, sdh, dA, sdA, db, sdb, ds);
        return run(who, resident, a);
    });
}

}  // namespace

#define QPD_PASSED B, n, ml, p, P, sP, G, sG, A, sA, x, y, s, z, exitcode, refinement

extern "C" {

int kvx_qp_batch_vjp(QPD_PROBLEM, const double *gx, double *ux, double *uy, double *uz, double *gP, double *gG, double *gA, int64_t *gexit)
{
    return vjp("kvx_qp_batch_vjp", false, QPD_PASSED, gx, ux, uy, uz, gP, gG, gA, gexit);
}

int kvx_qp_batch_vjp_dev(QPD_PROBLEM, const double *gx, double *ux, double *uy, double *uz, double *gP, double *gG, double *gA,
                         int64_t *gexit)
{
    return vjp("kvx_qp_batch_vjp_dev", true, QPD_PASSED, gx, ux, uy, uz, gP, gG, gA, gexit);
}

int kvx_qp_batch_jvp(QPD_PROBLEM, const double *dP, int64_t sdP, const double *dq, int64_t sdq, const double *dG, int64_t sdG,
                     const double *dh, int64_t sdh, const double *dA, int64_t sdA, const double *db, int64_t sdb, double *dx, double *dy,
                     double *dz, double *ds, int64_t *gexit)
{
    return jvp("kvx_qp_batch_jvp", false, QPD_PASSED, dP, sdP, dq, sdq, dG, sdG, dh, sdh, dA, sdA, db, sdb, dx, dy, dz, ds, gexit);
}

int kvx_qp_batch_jvp_dev(QPD_PROBLEM, const double *dP, int64_t sdP, const double *dq, int64_t sdq, const double *dG, int64_t sdG,
                         const double *dh, int64_t sdh, const double *dA, int64_t sdA, const double *db, int64_t sdb, double *dx,
                         double *dy, double *dz, double *ds, int64_t *gexit)
{
    return jvp("kvx_qp_batch_jvp_dev", true, QPD_PASSED, dP, sdP, dq, sdq, dG, sdG, dh, sdh, dA, sdA, db, sdb, dx, dy, dz, ds, gexit);
}

int64_t kvx_qp_batch_diff_lds_bytes(int64_t n, int64_t ml, int64_t p, int64_t *forward)
{
    if (n < 1 || n > QPB_MAX_N || ml < 1 || ml > QPB_MAX_ML || p < 0 || p > n) return -1;
    if (forward) *forward = (int64_t)qp_batch_lds_bytes((int)n, (int)ml, (int)p);
    return (int64_t)qp_batch_diff_lds_bytes((int)n, (int)ml, (int)p);
}

}  // extern "C"
