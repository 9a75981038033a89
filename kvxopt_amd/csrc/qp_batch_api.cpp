// kvx_qp_batch_solve / kvx_qp_batch_solve_dev (include/kvxhip.h): the limits of k_qp_batch (qp_batch.hip) and its launch through
// the host entry that the batch solvers share (batch_host.hpp).  q travels as the c of BatchArgs; P is the QP's own.
#include "batch_host.hpp"
#include "qp_batch.hpp"

using namespace kvx;
using namespace kvx::batchhost;

namespace {

// What both entries check before a device is asked for
int check(const char *who, const QpBatchArgs &a)
{
    if (a.B < 1 || a.B > 2147483647) return refuse(who, "1 <= B <= 2147483647 is required");
    if (a.n < 1 || a.n > QPB_MAX_N) return refuse(who, "1 <= n <= 64 is required");
    if (a.ml < 1 || a.ml > QPB_MAX_ML) return refuse(who, "1 <= ml <= 512 is required");
    if (a.p < 0 || a.p > a.n) return refuse(who, "0 <= p <= n is required");
    const Part P = {"P", a.sP, (int64_t)a.n * a.n};
    return check_common(who, a, a.ml, "q", &P, a.P != nullptr);
}

int solve(const char *who, bool resident, const QpBatchArgs &a)
{
    int rc = check(who, a);
    if (rc || (rc = need_device(who))) return rc;
    const auto launch = [](const QpBatchArgs &d) { return launch_qp_batch(nullptr, d); };
    return resident ? solve_dev(a, launch) : solve_host(a, a.ml, QPB_NSTAT, launch, &QpBatchArgs::P, a.sP, (int64_t)a.n * a.n);
}

QpBatchArgs pack_qp(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *q, int64_t sq,
                    const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb,
                    int64_t maxiters, double abstol, double reltol, double feastol, int use_correction, double *x, double *y, double *s,
                    double *z, double *stats, int64_t *iterations, int64_t *exitcode)
{
    QpBatchArgs a = pack<QpBatchArgs>(B, n, ml, p, q, sq, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, x, y, s, z, stats,
                                      iterations, exitcode);
    a.P = P; a.sP = sP; a.correction = use_correction != 0;
    return a;
}

}  // namespace

extern "C" {

int kvx_qp_batch_solve(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *q, int64_t sq,
                       const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb,
                       int64_t maxiters, double abstol, double reltol, double feastol, int use_correction, double *x, double *y, double *s,
                       double *z, double *stats, int64_t *iterations, int64_t *exitcode)
{
    return guarded([&] {
        return solve("kvx_qp_batch_solve", false,
                     pack_qp(B, n, ml, p, P, sP, q, sq, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, use_correction, x, y,
                             s, z, stats, iterations, exitcode));
    });
}

int kvx_qp_batch_solve_dev(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *q, int64_t sq,
                           const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b,
                           int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol, int use_correction, double *x,
                           double *y, double *s, double *z, double *stats, int64_t *iterations, int64_t *exitcode)
{
    return guarded([&] {
        return solve("kvx_qp_batch_solve_dev", true,
                     pack_qp(B, n, ml, p, P, sP, q, sq, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, use_correction, x, y,
                             s, z, stats, iterations, exitcode));
    });
}

}  // extern "C"
