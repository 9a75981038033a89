// kvx_sdp_batch_solve / kvx_sdp_batch_solve_dev (include/kvxhip.h): the argument checks, which need no device, the transfers
// of the host entry, and the one launch of k_sdp_batch (sdp_batch.hip).  The block orders are a host array for both entries:
// they travel to the kernel with its arguments.  The kernel stages the scaled 's' rows of G in LDS, so there is no workspace.
#include "batch_host.hpp"
#include "sdp_batch.hpp"

using namespace kvx;
using namespace kvx::batchhost;

namespace {

// What both entries check before a device is asked for.  size: doubles of one member; stride 0 (shared) or >= size.
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
    if (!a.c || !a.G || !a.h || (a.p > 0 && (!a.A || !a.b))) return refuse(who, "a data pointer is NULL");
    if (!a.x || !a.s || !a.z || !a.stats || !a.iters || !a.exitc || (a.p > 0 && !a.y)) return refuse(who, "a result pointer is NULL");
    const int64_t n = a.n, p = a.p;
    const struct { const char *name; int64_t stride, size; } parts[] = {
        {"c", a.sc, n}, {"G", a.sG, N * n}, {"h", a.sh, N}, {"A", a.sA, p * n}, {"b", a.sb, p}};
    for (const auto &t : parts)
        if (t.stride != 0 && t.stride < t.size)
            return refuse(who, std::string("the member stride of ") + t.name + " is 0 or at least its size");
    if (a.maxiters < 1) return refuse(who, "maxiters must be a positive integer");
    if (!(a.feastol > 0.0)) return refuse(who, "feastol must be a positive scalar");
    if (!(a.reltol > 0.0) && !(a.abstol > 0.0)) return refuse(who, "at least one of reltol and abstol must be positive");
    return KVX_OK;
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

int solve_dev_impl(SdpBatchArgs a, int64_t ns, const int64_t *m)
{
    int rc = check("kvx_sdp_batch_solve_dev", a, ns, m);
    if (rc || (rc = need_device("kvx_sdp_batch_solve_dev"))) return rc;
    place(a, ns, m);
    HIPCHK(launch_sdp_batch(nullptr, a));
    HIPCHK(hipStreamSynchronize(nullptr));
    return KVX_OK;
}

int solve_impl(SdpBatchArgs h, int64_t ns, const int64_t *m)
{
    int rc = check("kvx_sdp_batch_solve", h, ns, m);
    if (rc || (rc = need_device("kvx_sdp_batch_solve"))) return rc;
    place(h, ns, m);
    const int64_t B = h.B, n = h.n, N = h.N, p = h.p;
    const auto extent = [&](int64_t stride, int64_t size) { return stride ? (B - 1) * stride + size : size; };
    SdpBatchArgs d = h;
    Buffers buf;
    double *iters = nullptr, *exitc = nullptr;                     // int64 results travel in 8-byte slots of the same pool
    if ((rc = buf.up(&d.c, h.c, extent(h.sc, n))) || (rc = buf.up(&d.G, h.G, extent(h.sG, N * n))) ||
        (rc = buf.up(&d.h, h.h, extent(h.sh, N))) ||
        (p > 0 && ((rc = buf.up(&d.A, h.A, extent(h.sA, p * n))) || (rc = buf.up(&d.b, h.b, extent(h.sb, p))))) ||
        (rc = buf.get(&d.x, n * B)) || (rc = buf.get(&d.y, p * B)) || (rc = buf.get(&d.s, N * B)) || (rc = buf.get(&d.z, N * B)) ||
        (rc = buf.get(&d.stats, SDPB_NSTAT * B)) || (rc = buf.get(&iters, B)) || (rc = buf.get(&exitc, B)))
        return rc;
    d.iters = reinterpret_cast<int64_t *>(iters);
    d.exitc = reinterpret_cast<int64_t *>(exitc);
    HIPCHK(launch_sdp_batch(nullptr, d));
    HIPCHK(hipStreamSynchronize(nullptr));
    if ((rc = down(h.x, d.x, n * B)) || (rc = down(h.y, d.y, p * B)) || (rc = down(h.s, d.s, N * B)) || (rc = down(h.z, d.z, N * B)) ||
        (rc = down(h.stats, d.stats, SDPB_NSTAT * B)) || (rc = down(h.iters, d.iters, B)) || (rc = down(h.exitc, d.exitc, B)))
        return rc;
    return KVX_OK;
}

SdpBatchArgs pack(int64_t B, int64_t n, int64_t ml, int64_t p, const double *c, int64_t sc, const double *G, int64_t sG, const double *h,
                   int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb, int64_t maxiters, double abstol, double reltol,
                   double feastol, double *x, double *y, double *s, double *z, double *stats, int64_t *iterations, int64_t *exitcode)
{
    const auto small = [](int64_t v) { return (int)(v < -1 ? -1 : (v > 1000000000 ? 1000000000 : v)); };    // the checks see the range
    SdpBatchArgs a = {};
    a.B = B; a.n = small(n); a.ml = small(ml); a.p = small(p);
    a.c = c; a.G = G; a.h = h; a.A = A; a.b = b;
    a.sc = sc; a.sG = sG; a.sh = sh; a.sA = sA; a.sb = sb;
    a.maxiters = small(maxiters); a.abstol = abstol; a.reltol = reltol; a.feastol = feastol;
    a.x = x; a.y = y; a.s = s; a.z = z; a.stats = stats; a.iters = iterations; a.exitc = exitcode;
    return a;
}

}  // namespace

extern "C" {

int kvx_sdp_batch_solve(int64_t B, int64_t n, int64_t ml, int64_t ns, const int64_t *m, int64_t p, const double *c, int64_t sc,
                         const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b,
                         int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol, double *x, double *y, double *s,
                         double *z, double *stats, int64_t *iterations, int64_t *exitcode)
{
    return guarded([&] {
        return solve_impl(pack(B, n, ml, p, c, sc, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, x, y, s, z, stats,
                               iterations, exitcode), ns, m);
    });
}

int kvx_sdp_batch_solve_dev(int64_t B, int64_t n, int64_t ml, int64_t ns, const int64_t *m, int64_t p, const double *c, int64_t sc,
                             const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b,
                             int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol, double *x, double *y,
                             double *s, double *z, double *stats, int64_t *iterations, int64_t *exitcode)
{
    return guarded([&] {
        return solve_dev_impl(pack(B, n, ml, p, c, sc, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, x, y, s, z,
                                   stats, iterations, exitcode), ns, m);
    });
}

}  // extern "C"
