// kvx_socp_batch_solve / kvx_socp_batch_solve_dev (include/kvxhip.h): the limits of k_socp_batch (socp_batch.hip), the placement
// of its cone, and its launch through the host entry that the batch solvers share (batch_host.hpp).  The cone orders are a host
// array for both entries: they travel to the kernel with its arguments.
#include "batch_host.hpp"
#include "socp_batch.hpp"

using namespace kvx;
using namespace kvx::batchhost;

namespace {

// What both entries check before a device is asked for
int check(const char *who, const SocpBatchArgs &a, int64_t nq, const int64_t *q)
{
    if (a.B < 1 || a.B > 2147483647) return refuse(who, "1 <= B <= 2147483647 is required");
    if (a.n < 1 || a.n > SOCPB_MAX_N) return refuse(who, "1 <= n <= 64 is required");
    if (a.ml < 0 || a.ml > SOCPB_MAX_ROWS) return refuse(who, "0 <= ml <= 512 is required");
    if (nq < 0 || nq > SOCPB_MAX_NQ) return refuse(who, "0 <= nq <= 128 is required");
    if (nq > 0 && !q) return refuse(who, "the cone orders q are NULL");
    int64_t N = a.ml;
    for (int64_t k = 0; k < nq; k++) {
        if (q[k] < 1 || q[k] > SOCPB_MAX_ROWS) return refuse(who, "every cone order is at least 1 and at most 512");
        N += q[k];
    }
    if (N < 1 || N > SOCPB_MAX_ROWS) return refuse(who, "1 <= N = ml + sum(q) <= 512 is required");
    if (a.p < 0 || a.p > a.n) return refuse(who, "0 <= p <= n is required");
    if (a.p + N < a.n) return refuse(who, "p + N >= n is required");
    if (socp_batch_lds_bytes(a.n, (int)N, (int)nq, a.p) > 160 * 1024) return refuse(who, "the member needs more than 160 KiB of LDS");
    return check_common(who, a, N);
}

// the checked cone into the kernel's arguments
void place(SocpBatchArgs &a, int64_t nq, const int64_t *q)
{
    a.nq = (int)nq;
    a.N = a.ml;
    for (int64_t k = 0; k < SOCPB_MAX_NQ; k++) a.q[k] = k < nq ? (unsigned short)q[k] : 0;
    for (int64_t k = 0; k < nq; k++) a.N += (int)q[k];
}

int solve(const char *who, bool resident, SocpBatchArgs a, int64_t nq, const int64_t *q)
{
    int rc = check(who, a, nq, q);
    if (rc || (rc = need_device(who))) return rc;
    place(a, nq, q);
    const auto launch = [](const SocpBatchArgs &d) { return launch_socp_batch(nullptr, d); };
    return resident ? solve_dev(a, launch) : solve_host(a, a.N, SOCPB_NSTAT, launch);
}

}  // namespace

extern "C" {

int kvx_socp_batch_solve(int64_t B, int64_t n, int64_t ml, int64_t nq, const int64_t *q, int64_t p, const double *c, int64_t sc,
                         const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b,
                         int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol, double *x, double *y, double *s,
                         double *z, double *stats, int64_t *iterations, int64_t *exitcode)
{
    return guarded([&] {
        return solve("kvx_socp_batch_solve", false,
                     pack<SocpBatchArgs>(B, n, ml, p, c, sc, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, x, y, s, z,
                                        stats, iterations, exitcode),
                     nq, q);
    });
}

int kvx_socp_batch_solve_dev(int64_t B, int64_t n, int64_t ml, int64_t nq, const int64_t *q, int64_t p, const double *c, int64_t sc,
                             const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b,
                             int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol, double *x, double *y,
                             double *s, double *z, double *stats, int64_t *iterations, int64_t *exitcode)
{
    return guarded([&] {
        return solve("kvx_socp_batch_solve_dev", true,
                     pack<SocpBatchArgs>(B, n, ml, p, c, sc, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, x, y, s, z,
                                        stats, iterations, exitcode),
                     nq, q);
    });
}

}  // extern "C"
