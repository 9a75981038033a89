// kvx_conelp_batch_solve / kvx_conelp_batch_solve_dev (include/kvxhip.h): the limits of k_conelp_batch (conelp_batch.hip), the
// placement of its cone, and its launch through the host entry that the batch solvers share (batch_host.hpp).  The cone orders
// and the block orders are host arrays for both entries: they travel to the kernel with its arguments.  The kernel stages the
// scaled rows of G in LDS, so there is no workspace.
#include "batch_cone_host.hpp"
#include "conelp_batch.hpp"

using namespace kvx;
using namespace kvx::batchhost;

namespace {

// What both entries check before a device is asked for; on success the cone is placed in `a`
int check(const char *who, ConelpBatchArgs &a, int64_t nq, const int64_t *q, int64_t ns, const int64_t *m)
{
    int64_t N = 0;
    if (const char *why = cone_limits(a.B, a.n, a.ml, nq, q, ns, m, a.p, &N)) return refuse(who, why);
    place_cone(a, nq, q, ns, m);
    if (a.p + a.Np < a.n) return refuse(who, "p + ml + sum(q) + sum(m (m + 1) / 2) >= n is required");
    if (conelp_batch_lds_bytes(a.n, a.ml, a.nq, a.q, a.ns, a.m, a.p) > 160 * 1024)
        return refuse(who, "the member needs more than 160 KiB of LDS");
    return check_common(who, a, N);
}

int solve(const char *who, bool resident, ConelpBatchArgs a, int64_t nq, const int64_t *q, int64_t ns, const int64_t *m)
{
    int rc = check(who, a, nq, q, ns, m);
    if (rc || (rc = need_device(who))) return rc;
    const auto launch = [](const ConelpBatchArgs &d) { return launch_conelp_batch(nullptr, d); };
    return resident ? solve_dev(a, launch) : solve_host(a, a.N, CONEB_NSTAT, launch);
}

}  // namespace

extern "C" {

int kvx_conelp_batch_solve(int64_t B, int64_t n, int64_t ml, int64_t nq, const int64_t *q, int64_t ns, const int64_t *m, int64_t p,
                           const double *c, int64_t sc, const double *G, int64_t sG, const double *h, int64_t sh, const double *A,
                           int64_t sA, const double *b, int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol,
                           double *x, double *y, double *s, double *z, double *stats, int64_t *iterations, int64_t *exitcode)
{
    return guarded([&] {
        return solve("kvx_conelp_batch_solve", false,
                     pack<ConelpBatchArgs>(B, n, ml, p, c, sc, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, x, y, s,
                                           z, stats, iterations, exitcode),
                     nq, q, ns, m);
    });
}

int kvx_conelp_batch_solve_dev(int64_t B, int64_t n, int64_t ml, int64_t nq, const int64_t *q, int64_t ns, const int64_t *m, int64_t p,
                               const double *c, int64_t sc, const double *G, int64_t sG, const double *h, int64_t sh, const double *A,
                               int64_t sA, const double *b, int64_t sb, int64_t maxiters, double abstol, double reltol,
                               double feastol, double *x, double *y, double *s, double *z, double *stats, int64_t *iterations,
                               int64_t *exitcode)
{
    return guarded([&] {
        return solve("kvx_conelp_batch_solve_dev", true,
                     pack<ConelpBatchArgs>(B, n, ml, p, c, sc, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, x, y, s,
                                           z, stats, iterations, exitcode),
                     nq, q, ns, m);
    });
}

}  // extern "C"
