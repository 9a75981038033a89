// kvx_qp_batch_solve / kvx_qp_batch_solve_dev (include/kvxhip.h): the argument checks, which need no device, the transfers of
// the host entry, and the one launch of k_qp_batch (qp_batch.hip).
#include "batch_host.hpp"
#include "qp_batch.hpp"

using namespace kvx;
using namespace kvx::batchhost;

namespace {

// What both entries check before a device is asked for.  size: doubles of one member; stride 0 (shared) or >= size.
int check(const char *who, const QpBatchArgs &a)
{
    if (a.B < 1 || a.B > 2147483647) return refuse(who, "1 <= B <= 2147483647 is required");
    if (a.n < 1 || a.n > QPB_MAX_N) return refuse(who, "1 <= n <= 64 is required");
    if (a.ml < 1 || a.ml > QPB_MAX_ML) return refuse(who, "1 <= ml <= 512 is required");
    if (a.p < 0 || a.p > a.n) return refuse(who, "0 <= p <= n is required");
    if (!a.P || !a.q || !a.G || !a.h || (a.p > 0 && (!a.A || !a.b))) return refuse(who, "a data pointer is NULL");
    if (!a.x || !a.s || !a.z || !a.stats || !a.iters || !a.exitc || (a.p > 0 && !a.y)) return refuse(who, "a result pointer is NULL");
    const int64_t n = a.n, ml = a.ml, p = a.p;
    const struct { const char *name; int64_t stride, size; } parts[] = {
        {"P", a.sP, n * n}, {"q", a.sq, n}, {"G", a.sG, ml * n}, {"h", a.sh, ml}, {"A", a.sA, p * n}, {"b", a.sb, p}};
    for (const auto &t : parts)
        if (t.stride != 0 && t.stride < t.size)
            return refuse(who, std::string("the member stride of ") + t.name + " is 0 or at least its size");
    if (a.maxiters < 1) return refuse(who, "maxiters must be a positive integer");
    if (!(a.feastol > 0.0)) return refuse(who, "feastol must be a positive scalar");
    if (!(a.reltol > 0.0) && !(a.abstol > 0.0)) return refuse(who, "at least one of reltol and abstol must be positive");
    return KVX_OK;
}

int solve_dev_impl(const QpBatchArgs &a)
{
    int rc = check("kvx_qp_batch_solve_dev", a);
    if (rc || (rc = need_device("kvx_qp_batch_solve_dev"))) return rc;
    HIPCHK(launch_qp_batch(nullptr, a));
    HIPCHK(hipStreamSynchronize(nullptr));
    return KVX_OK;
}

int solve_impl(const QpBatchArgs &h)
{
    int rc = check("kvx_qp_batch_solve", h);
    if (rc || (rc = need_device("kvx_qp_batch_solve"))) return rc;
    const int64_t B = h.B, n = h.n, ml = h.ml, p = h.p;
    const auto extent = [&](int64_t stride, int64_t size) { return stride ? (B - 1) * stride + size : size; };
    QpBatchArgs d = h;
    Buffers buf;
    double *iters = nullptr, *exitc = nullptr;                     // int64 results travel in 8-byte slots of the same pool
    if ((rc = buf.up(&d.P, h.P, extent(h.sP, n * n))) || (rc = buf.up(&d.q, h.q, extent(h.sq, n))) ||
        (rc = buf.up(&d.G, h.G, extent(h.sG, ml * n))) || (rc = buf.up(&d.h, h.h, extent(h.sh, ml))) ||
        (p > 0 && ((rc = buf.up(&d.A, h.A, extent(h.sA, p * n))) || (rc = buf.up(&d.b, h.b, extent(h.sb, p))))) ||
        (rc = buf.get(&d.x, n * B)) || (rc = buf.get(&d.y, p * B)) || (rc = buf.get(&d.s, ml * B)) || (rc = buf.get(&d.z, ml * B)) ||
        (rc = buf.get(&d.stats, QPB_NSTAT * B)) || (rc = buf.get(&iters, B)) || (rc = buf.get(&exitc, B)))
        return rc;
    d.iters = reinterpret_cast<int64_t *>(iters);
    d.exitc = reinterpret_cast<int64_t *>(exitc);
    HIPCHK(launch_qp_batch(nullptr, d));
    HIPCHK(hipStreamSynchronize(nullptr));
    if ((rc = down(h.x, d.x, n * B)) || (rc = down(h.y, d.y, p * B)) || (rc = down(h.s, d.s, ml * B)) || (rc = down(h.z, d.z, ml * B)) ||
        (rc = down(h.stats, d.stats, QPB_NSTAT * B)) || (rc = down(h.iters, d.iters, B)) || (rc = down(h.exitc, d.exitc, B)))
        return rc;
    return KVX_OK;
}

QpBatchArgs pack(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *q, int64_t sq, const double *G,
                 int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb, int64_t maxiters,
                 double abstol, double reltol, double feastol, int use_correction, double *x, double *y, double *s, double *z,
                 double *stats, int64_t *iterations, int64_t *exitcode)
{
    const auto small = [](int64_t v) { return (int)(v < -1 ? -1 : (v > 1000000000 ? 1000000000 : v)); };    // the checks see the range
    QpBatchArgs a;
    a.B = B; a.n = small(n); a.ml = small(ml); a.p = small(p);
    a.P = P; a.q = q; a.G = G; a.h = h; a.A = A; a.b = b;
    a.sP = sP; a.sq = sq; a.sG = sG; a.sh = sh; a.sA = sA; a.sb = sb;
    a.maxiters = small(maxiters); a.abstol = abstol; a.reltol = reltol; a.feastol = feastol; a.correction = use_correction != 0;
    a.x = x; a.y = y; a.s = s; a.z = z; a.stats = stats; a.iters = iterations; a.exitc = exitcode;
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
        return solve_impl(pack(B, n, ml, p, P, sP, q, sq, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, use_correction,
                               x, y, s, z, stats, iterations, exitcode));
    });
}

int kvx_qp_batch_solve_dev(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *q, int64_t sq,
                           const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b,
                           int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol, int use_correction, double *x,
                           double *y, double *s, double *z, double *stats, int64_t *iterations, int64_t *exitcode)
{
    return guarded([&] {
        return solve_dev_impl(pack(B, n, ml, p, P, sP, q, sq, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol,
                                   use_correction, x, y, s, z, stats, iterations, exitcode));
    });
}

}  // extern "C"
