// kvx_coneqp_batch_solve / kvx_coneqp_batch_solve_dev (include/kvxhip.h): the limits of k_coneqp_batch (coneqp_batch.hip), the
// placement of its cone, and its launch through the host entry that the batch solvers share (batch_host.hpp).  The limits are
// those of kvx_conelp_batch_solve without its rank condition on the packed dimension: P may supply the rank, and a member without
// it ends with exit 3.  q travels as the c of BatchArgs; P is the QP's own.  The cone orders and the block orders are host arrays
// for both entries: they travel to the kernel with its arguments.  There is no workspace.
#include "batch_host.hpp"
#include "coneqp_batch.hpp"

using namespace kvx;
using namespace kvx::batchhost;

namespace {

// the cone into the kernel's arguments; the orders are in range (check)
void place(ConeqpBatchArgs &a, int64_t nq, const int64_t *q, int64_t ns, const int64_t *m)
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

// What both entries check before a device is asked for; on success the cone is placed in `a`
int check(const char *who, ConeqpBatchArgs &a, int64_t nq, const int64_t *q, int64_t ns, const int64_t *m)
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
    place(a, nq, q, ns, m);
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
