// kvx_lp_batch_solve / kvx_lp_batch_solve_dev (include/kvxhip.h): the limits of k_lp_batch (lp_batch.hip) and its launch through
// the host entry that the batch solvers share (batch_host.hpp).
#include "batch_host.hpp"
#include "lp_batch.hpp"

using namespace kvx;
using namespace kvx::batchhost;

namespace {

// What both entries check before a device is asked for
int check(const char *who, const LpBatchArgs &a)
{
    if (a.B < 1 || a.B > 2147483647) return refuse(who, "1 <= B <= 2147483647 is required");
    if (a.n < 1 || a.n > LPB_MAX_N) return refuse(who, "1 <= n <= 64 is required");
    if (a.ml < 1 || a.ml > LPB_MAX_ML) return refuse(who, "1 <= ml <= 512 is required");
    if (a.p < 0 || a.p > a.n) return refuse(who, "0 <= p <= n is required");
    if (a.p + a.ml < a.n) return refuse(who, "p + ml >= n is required");
    return check_common(who, a, a.ml);
}

int solve(const char *who, bool resident, const LpBatchArgs &a)
{
    int rc = check(who, a);
    if (rc || (rc = need_device(who))) return rc;
    const auto launch = [](const LpBatchArgs &d) { return launch_lp_batch(nullptr, d); };
    return resident ? solve_dev(a, launch) : solve_host(a, a.ml, LPB_NSTAT, launch);
}

}  // namespace

extern "C" {

int kvx_lp_batch_solve(int64_t B, int64_t n, int64_t ml, int64_t p, const double *c, int64_t sc, const double *G, int64_t sG,
                       const double *h, int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb, int64_t maxiters,
                       double abstol, double reltol, double feastol, double *x, double *y, double *s, double *z, double *stats,
                       int64_t *iterations, int64_t *exitcode)
{
    return guarded([&] {
        return solve("kvx_lp_batch_solve", false,
                     pack<LpBatchArgs>(B, n, ml, p, c, sc, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, x, y, s, z,
                                       stats, iterations, exitcode));
    });
}

int kvx_lp_batch_solve_dev(int64_t B, int64_t n, int64_t ml, int64_t p, const double *c, int64_t sc, const double *G, int64_t sG,
                           const double *h, int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb, int64_t maxiters,
                           double abstol, double reltol, double feastol, double *x, double *y, double *s, double *z, double *stats,
                           int64_t *iterations, int64_t *exitcode)
{
    return guarded([&] {
        return solve("kvx_lp_batch_solve_dev", true,
                     pack<LpBatchArgs>(B, n, ml, p, c, sc, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, x, y, s, z,
                                       stats, iterations, exitcode));
    });
}

}  // extern "C"
