// kvx_coneqp_batch_vjp / kvx_coneqp_batch_jvp and their _dev forms (include/kvxhip.h): the limits of k_coneqp_batch_diff
// (coneqp_batch_diff.hip), which are those of kvx_coneqp_batch_solve, the placement of its cone, its launch, and after a
// reverse-mode launch k_batch_outer_sum (qp_batch_diff.hip) for every matrix the members share, on the centred x, y, z the kernel
// leaves in pooled buffers.  The host entries go up, launch and come down through diff_host of batch_host.hpp.
#include "batch_cone_host.hpp"
#include "coneqp_batch_diff.hpp"

using namespace kvx;
using namespace kvx::batchhost;

namespace {

// What all four entries check before a device is asked for; on success the cone is placed in `a`
int check(const char *who, ConeqpDiffArgs &a, int64_t nq, const int64_t *q, int64_t ns, const int64_t *m)
{
    int64_t N = 0;
    if (const char *why = cone_limits(a.B, a.n, a.ml, nq, q, ns, m, a.p, &N)) return refuse(who, why);
    if (a.refinement < 0 || a.refinement > QPD_MAX_REFINEMENT) return refuse(who, "0 <= refinement <= 3 is required");
    if (a.centering < 0 || a.centering > CQD_MAX_CENTERING) return refuse(who, "0 <= centering <= 16 is required");
    if (!(a.centol > 0.0)) return refuse(who, "centol must be a positive scalar");
    place_cone(a, nq, q, ns, m);
    if (coneqp_batch_diff_lds_bytes(a.n, a.ml, a.nq, a.q, a.ns, a.m, a.p) > 160 * 1024)
        return refuse(who, "the member needs more than 160 KiB of LDS");
    return check_diff(who, a, N, a.mode == QPD_JVP, true, a.centrality && a.steps);
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

// centrality and the centring steps of every member; int64 travels in 8-byte slots of the same pool
struct Centring {
    int get(Buffers &buf, ConeqpDiffArgs &d, int64_t B) const
    {
        double *steps = nullptr;
        int rc;
        if ((rc = buf.get(&steps, B)) || (rc = buf.get(&d.centrality, B))) return rc;
        d.steps = reinterpret_cast<int64_t *>(steps);
        return KVX_OK;
    }
    int down(const ConeqpDiffArgs &h, const ConeqpDiffArgs &d, int64_t B) const
    {
        int rc = batchhost::down(h.steps, d.steps, B);
        return rc ? rc : batchhost::down(h.centrality, d.centrality, B);
    }
};

int run(const char *who, bool resident, ConeqpDiffArgs a, int64_t nq, const int64_t *q, int64_t ns, const int64_t *m)
{
    int rc = check(who, a, nq, q, ns, m);
    if (rc || (rc = need_device(who))) return rc;
    return resident ? launch(a) : diff_host(a, a.N, a.mode == QPD_JVP, true, launch, Centring());
}

// The arguments all four entries share, as the C ABI passes them
ConeqpDiffArgs pack_cone(ConeqpDiffArgs a, int64_t centering, double centol, double *centrality, int64_t *steps)
{
    a.centering = (int)(centering < -1 ? -1 : (centering > 1000000000 ? 1000000000 : centering));
    a.centol = centol;
    a.centrality = centrality; a.steps = steps;
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
        ConeqpDiffArgs a = pack_cone(pack_diff<ConeqpDiffArgs>(QPD_VJP, B, n, ml, p, P, sP, q, sq, G, sG, h, sh, A, sA, b, sb, x, y, s, z,
                                                               exitcode, refinement, ux, uy, uz, gexit),
                                     centering, centol, centrality, steps);
        set_vjp(a, gx, gP, gG, gA);
        return run(who, resident, a, nq, qdims, ns, m);
    });
}

int jvp(const char *who, bool resident, CQD_PROBLEM, const double *dP, int64_t sdP, const double *dq, int64_t sdq, const double *dG,
        int64_t sdG, const double *dh, int64_t sdh, const double *dA, int64_t sdA, const double *db, int64_t sdb, double *dx, double *dy,
        double *dz, double *ds, double *centrality, int64_t *steps, int64_t *gexit)
{
    return guarded([&] {
        ConeqpDiffArgs a = pack_cone(pack_diff<ConeqpDiffArgs>(QPD_JVP, B, n, ml, p, P, sP, q, sq, G, sG, h, sh, A, sA, b, sb, x, y, s, z,
                                                               exitcode, refinement, dx, dy, dz, gexit),
                                     centering, centol, centrality, steps);
        set_jvp(a, dP, sdP, dq, sdq, dG, sdG, dh, sdh, dA, sdA, db, sdb, ds);
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
    int64_t N = 0;
    if (cone_limits(a.B, a.n, a.ml, nq, qdims, ns, m, a.p, &N)) return -1;
    place_cone(a, nq, qdims, ns, m);
    if (forward) *forward = (int64_t)coneqp_batch_lds_bytes(a.n, a.ml, a.nq, a.q, a.ns, a.m, a.p);
    return (int64_t)coneqp_batch_diff_lds_bytes(a.n, a.ml, a.nq, a.q, a.ns, a.m, a.p);
}

}  // extern "C"
