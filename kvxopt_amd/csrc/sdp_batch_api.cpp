// kvx_sdp_batch_solve / kvx_sdp_batch_solve_dev (include/kvxhip.h): the limits of k_sdp_batch (sdp_batch.hip), the placement of
// its cone, and its launch through the host entry that the batch solvers share (batch_host.hpp).  The block orders are a host
// array for both entries: they travel to the kernel with its arguments.  The kernel stages the scaled 's' rows of G in LDS, so
// there is no workspace.
#include "batch_host.hpp"
#include "sdp_batch.hpp"

using namespace kvx;
using namespace kvx::batchhost;

namespace {

// What both entries check before a device is asked for
int check(const char *who, const SdpBatchArgs &a, int64_t ns, const int64_t *m)
{
    if (a.B < 1 || a.B > 2147483647) return refuse(who, "1 <= B <= 2147483647 is required");
    if (a.n < 1 || a.n > SDPB_MAX_N) return refuse(who, "1 <= n <= 64 is required");
    if (a.ml < 0 || a.ml > SDPB_MAX_ROWS) return refuse(who, "0 <= ml <= 384 is required");
    if (ns < 0 || ns > SDPB_MAX_NS) return refuse(who, "0 <= ns <= 32 is required");
    if (ns > 0 && !m) return refuse(who, "the block orders m are NULL");
    int64_t N = a.ml, Np = a.ml;
    unsigned char orders[SDPB_MAX_NS] = {};
    for (int64_t k = 0; k < ns; k++) {
        if (m[k] < 1 || m[k] > SDPB_MAX_M) return refuse(who, "every block order is at least 1 and at most 16");
        N += m[k] * m[k];
        Np += (m[k] * (m[k] + 1)) / 2;
        orders[k] = (unsigned char)m[k];
    }
    if (N < 1 || N > SDPB_MAX_ROWS) return refuse(who, "1 <= N = ml + sum(m^2) <= 384 is required");
    if (a.p < 0 || a.p > a.n) return refuse(who, "0 <= p <= n is required");
    if (a.p + Np < a.n) return refuse(who, "p + ml + sum(m (m + 1) / 2) >= n is required");
    if (sdp_batch_lds_bytes(a.n, a.ml, (int)ns, orders, a.p) > 160 * 1024) return refuse(who, "the member needs more than 160 KiB of LDS");
    return check_common(who, a, N);
}

// the checked cone into the kernel's arguments
void place(SdpBatchArgs &a, int64_t ns, const int64_t *m)
{
    a.ns = (int)ns;
    a.N = a.Nd = a.Np = a.ml;
    for (int64_t k = 0; k < SDPB_MAX_NS; k++) a.m[k] = k < ns ? (unsigned char)m[k] : 0;
    for (int64_t k = 0; k < ns; k++) {
        a.N += (int)(m[k] * m[k]);
        a.Nd += (int)m[k];
        a.Np += (int)((m[k] * (m[k] + 1)) / 2);
    }
}

int solve(const char *who, bool resident, SdpBatchArgs a, int64_t ns, const int64_t *m)
{
    int rc = check(who, a, ns, m);
    if (rc || (rc = need_device(who))) return rc;
    place(a, ns, m);
    const auto launch = [](const SdpBatchArgs &d) { return launch_sdp_batch(nullptr, d); };
    return resident ? solve_dev(a, launch) : solve_host(a, a.N, SDPB_NSTAT, launch);
}

}  // namespace

extern "C" {

int kvx_sdp_batch_solve(int64_t B, int64_t n, int64_t ml, int64_t ns, const int64_t *m, int64_t p, const double *c, int64_t sc,
                         const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b,
                         int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol, double *x, double *y, double *s,
                         double *z, double *stats, int64_t *iterations, int64_t *exitcode)
{
    return guarded([&] {
        return solve("kvx_sdp_batch_solve", false,
                     pack<SdpBatchArgs>(B, n, ml, p, c, sc, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, x, y, s, z,
                                       stats, iterations, exitcode),
                     ns, m);
    });
}

int kvx_sdp_batch_solve_dev(int64_t B, int64_t n, int64_t ml, int64_t ns, const int64_t *m, int64_t p, const double *c, int64_t sc,
                             const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b,
                             int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol, double *x, double *y,
                             double *s, double *z, double *stats, int64_t *iterations, int64_t *exitcode)
{
    return guarded([&] {
        return solve("kvx_sdp_batch_solve_dev", true,
                     pack<SdpBatchArgs>(B, n, ml, p, c, sc, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, x, y, s, z,
                                       stats, iterations, exitcode),
                     ns, m);
    });
}

}  // extern "C"
