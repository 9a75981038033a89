// kvx_coneqp_batch_solve / kvx_coneqp_batch_solve_dev (include/kvxhip.h): the limits of k_coneqp_batch (coneqp_batch.hip), the
// placement of its cone, and its launch through the host entry that the batch solvers share (batch_host.hpp).  The limits are
// those of kvx_conelp_batch_solve without its rank condition on the packed dimension: P may supply the rank, and a member without
// it ends with exit 3.  q travels as the c of BatchArgs; P is the QP's own.  The cone orders and the block orders are host arrays
// for both entries: they travel to the kernel with its arguments.  There is no workspace.
#include "batch_cone_host.hpp"
#include "coneqp_batch.hpp"

using namespace kvx;
using namespace kvx::batchhost;

namespace {

// What both entries check before a device is asked for; on success the cone is placed in `a`
int check(const char *who, ConeqpBatchArgs &a, int64_t nq, const int64_t *q, int64_t ns, const int64_t *m)
{
    int64_t N = 0;
    if (const char *why = cone_limits(a.B, a.n, a.ml, nq, q, ns, m, a.p, &N)) return refuse(who, why);
    place_cone(a, nq, q, ns, m);
    if (coneqp_batch_lds_bytes(a.n, a.ml, a.nq, a.q, a.ns, a.m, a.p) > 160 * 1024)
        return refuse(who, "the member needs more than 160 KiB of LDS");
    const Part P = {"P", a.sP, (int64_t)a.n * a.n};
    return check_common(who, a, N, "q", &P, a.P != nullptr);
}

int solve(const char *who, bool resident, ConeqpBatchArgs a, int64_t nq, const int64_t *q, int64_t ns, const int64_t *m)
{
    int rc = check(who, a, nq, q, ns, m);
    if (rc || (rc = need_device(who))) return rc;
    const auto launch = [](const ConeqpBatchArgs &d) { return launch_coneqp_batch(nullptr, d); };
    return resident ? solve_dev(a, launch)
                    : solve_host(a, a.N, CONEQPB_NSTAT, launch, &ConeqpBatchArgs::P, a.sP, (int64_t)a.n * a.n);
}

ConeqpBatchArgs pack_qp(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *q, int64_t sq,
                        const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b,
                        int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol, int use_correction, double *x,
                        double *y, double *s, double *z, double *stats, int64_t *iterations, int64_t *exitcode)
{
    ConeqpBatchArgs a = pack<ConeqpBatchArgs>(B, n, ml, p, q, sq, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, x, y, s,
                                              z, stats, iterations, exitcode);
    a.P = P; a.sP = sP; a.correction = use_correction != 0;
    return a;
}

}  // namespace

extern "C" {

int kvx_coneqp_batch_solve(int64_t B, int64_t n, int64_t ml, int64_t nq, const int64_t *qdims, int64_t ns, const int64_t *m, int64_t p,
                           const double *P, int64_t sP, const double *q, int64_t sq, const double *G, int64_t sG, const double *h,
                           int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb, int64_t maxiters, double abstol,
                           double reltol, double feastol, int use_correction, double *x, double *y, double *s, double *z, double *stats,
                           int64_t *iterations, int64_t *exitcode)
{
    return guarded([&] {
        return solve("kvx_coneqp_batch_solve", false,
                     pack_qp(B, n, ml, p, P, sP, q, sq, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, use_correction, x, y,
                             s, z, stats, iterations, exitcode),
                     nq, qdims, ns, m);
    });
}

int kvx_coneqp_batch_solve_dev(int64_t B, int64_t n, int64_t ml, int64_t nq, const int64_t *qdims, int64_t ns, const int64_t *m,
                               int64_t p, const double *P, int64_t sP, const double *q, int64_t sq, const double *G, int64_t sG,
                               const double *h, int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb, int64_t maxiters,
                               double abstol, double reltol, double feastol, int use_correction, double *x, double *y, double *s,
                               double *z, double *stats, int64_t *iterations, int64_t *exitcode)
{
    return guarded([&] {
        return solve("kvx_coneqp_batch_solve_dev", true,
                     pack_qp(B, n, ml, p, P, sP, q, sq, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, use_correction, x, y,
                             s, z, stats, iterations, exitcode),
                     nq, qdims, ns, m);
    });
}

}  // extern "C"
