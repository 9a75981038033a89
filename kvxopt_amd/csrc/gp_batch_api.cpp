// kvx_gp_batch_solve / kvx_gp_batch_solve_dev (include/kvxhip.h): the limits of k_gp_batch (gp_batch.hip) and its launch on the
// pieces the batch solvers share (batch_host.hpp: the refusal, the question for a device, the packed arguments, the pooled
// copies).  g travels as the c of BatchArgs; F is the program's own.  The block sizes K are a host array for both entries: they
// travel to the kernel with its arguments; the limits of a member and their placement are gphost::place_blocks of gp_batch.hpp,
// which the derivative's entries (gp_batch_diff_api.cpp) call too.  check_common and solve_host are not used: here g has l entries and not n, G and h
// have ml >= 0 rows where s and z have N = mnl + 1 + ml, and a member has a workspace in HBM, which the host entry allocates
// and the _dev entry is given.
#include "batch_host.hpp"
#include "gp_batch.hpp"

using namespace kvx;
using namespace kvx::batchhost;

namespace {

// What both entries check before a device is asked for; on success the blocks are placed in `a`
int check(const char *who, GpBatchArgs &a, int64_t mnl, const int64_t *K, bool resident)
{
    if (int rc = gphost::place_blocks(who, a, mnl, K)) return rc;
    if (gp_batch_lds_bytes(a.n, a.m, a.l, a.ml, a.p) > 160 * 1024) return refuse(who, "the member needs more than 160 KiB of LDS");
    if (!a.F || !a.c || (a.ml > 0 && (!a.G || !a.h)) || (a.p > 0 && (!a.A || !a.b))) return refuse(who, "a data pointer is NULL");
    if (!a.x || !a.s || !a.z || !a.stats || !a.iters || !a.exitc || (a.p > 0 && !a.y)) return refuse(who, "a result pointer is NULL");
    if (resident && !a.scratch) return refuse(who, "the scratch pointer is NULL");
    const int64_t n = a.n, ml = a.ml, p = a.p, l = a.l;
    const Part parts[] = {{"F", a.sF, l * n}, {"g", a.sc, l}, {"G", a.sG, ml * n}, {"h", a.sh, ml}, {"A", a.sA, p * n}, {"b", a.sb, p}};
    for (const auto &t : parts)
        if (t.stride != 0 && t.stride < t.size)
            return refuse(who, std::string("the member stride of ") + t.name + " is 0 or at least its size");
    if (a.maxiters < 1) return refuse(who, "maxiters must be a positive integer");
    if (!(a.feastol > 0.0)) return refuse(who, "feastol must be a positive scalar");
    if (!(a.reltol > 0.0) && !(a.abstol > 0.0)) return refuse(who, "at least one of reltol and abstol must be positive");
    return KVX_OK;
}

// The checked batch `h` of host pointers: the data goes up, the scratch is taken from the pool, one launch and a
// synchronisation, the results come down, and the copies return to the pool on every path.
int solve_host_gp(const GpBatchArgs &h)
{
    const int64_t B = h.B, n = h.n, ml = h.ml, p = h.p, l = h.l, N = h.m + ml;
    const auto extent = [&](int64_t stride, int64_t size) { return stride ? (B - 1) * stride + size : size; };
    GpBatchArgs d = h;
    Buffers buf;
    int rc;
    double *iters = nullptr, *exitc = nullptr;                     // int64 results travel in 8-byte slots of the same pool
    if ((rc = buf.up(&d.F, h.F, extent(h.sF, l * n))) || (rc = buf.up(&d.c, h.c, extent(h.sc, l))) ||
        (ml > 0 && ((rc = buf.up(&d.G, h.G, extent(h.sG, ml * n))) || (rc = buf.up(&d.h, h.h, extent(h.sh, ml))))) ||
        (p > 0 && ((rc = buf.up(&d.A, h.A, extent(h.sA, p * n))) || (rc = buf.up(&d.b, h.b, extent(h.sb, p))))) ||
        (rc = buf.get(&d.scratch, B * gp_batch_scratch_doubles(h.n, h.m, h.ml, h.p))) || (rc = buf.get(&d.x, n * B)) ||
        (rc = buf.get(&d.y, p * B)) || (rc = buf.get(&d.s, N * B)) || (rc = buf.get(&d.z, N * B)) ||
        (rc = buf.get(&d.stats, (int64_t)GPB_NSTAT * B)) || (rc = buf.get(&iters, B)) || (rc = buf.get(&exitc, B)))
        return rc;
    d.iters = reinterpret_cast<int64_t *>(iters);
    d.exitc = reinterpret_cast<int64_t *>(exitc);
    HIPCHK(launch_gp_batch(nullptr, d));
    HIPCHK(hipStreamSynchronize(nullptr));
    if ((rc = down(h.x, d.x, n * B)) || (rc = down(h.y, d.y, p * B)) || (rc = down(h.s, d.s, N * B)) || (rc = down(h.z, d.z, N * B)) ||
        (rc = down(h.stats, d.stats, (int64_t)GPB_NSTAT * B)) || (rc = down(h.iters, d.iters, B)) || (rc = down(h.exitc, d.exitc, B)))
        return rc;
    return KVX_OK;
}

int solve(const char *who, bool resident, GpBatchArgs a, int64_t mnl, const int64_t *K)
{
    int rc = check(who, a, mnl, K, resident);
    if (rc || (rc = need_device(who))) return rc;
    return resident ? solve_dev(a, [](const GpBatchArgs &d) { return launch_gp_batch(nullptr, d); }) : solve_host_gp(a);
}

GpBatchArgs pack_gp(int64_t B, int64_t n, int64_t ml, int64_t p, const double *F, int64_t sF, const double *g, int64_t sg, const double *G,
                    int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb, int64_t maxiters,
                    double abstol, double reltol, double feastol, double *x, double *y, double *s, double *z, double *stats,
                    int64_t *iterations, int64_t *exitcode, double *scratch)
{
    GpBatchArgs a = pack<GpBatchArgs>(B, n, ml, p, g, sg, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, x, y, s, z, stats,
                                      iterations, exitcode);
    a.F = F; a.sF = sF; a.scratch = scratch;
    return a;
}

}  // namespace

extern "C" {

int64_t kvx_gp_batch_scratch_doubles(int64_t n, int64_t mnl, int64_t ml, int64_t p)
{
    if (n < 1 || n > GPB_MAX_N || mnl < 0 || ml < 0 || mnl + 1 + ml > GPB_MAX_ROWS || p < 0 || p > n) return -1;
    return gp_batch_scratch_doubles((int)n, (int)mnl + 1, (int)ml, (int)p);
}

int kvx_gp_batch_solve(int64_t B, int64_t n, int64_t mnl, const int64_t *K, int64_t ml, int64_t p, const double *F, int64_t sF,
                       const double *g, int64_t sg, const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA,
                       const double *b, int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol, double *x, double *y,
                       double *s, double *z, double *stats, int64_t *iterations, int64_t *exitcode)
{
    return guarded([&] {
        return solve("kvx_gp_batch_solve", false,
                     pack_gp(B, n, ml, p, F, sF, g, sg, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, x, y, s, z, stats,
                             iterations, exitcode, nullptr),
                     mnl, K);
    });
}

int kvx_gp_batch_solve_dev(int64_t B, int64_t n, int64_t mnl, const int64_t *K, int64_t ml, int64_t p, const double *F, int64_t sF,
                           const double *g, int64_t sg, const double *G, int64_t sG, const double *h, int64_t sh, const double *A,
                           int64_t sA, const double *b, int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol,
                           double *x, double *y, double *s, double *z, double *stats, int64_t *iterations, int64_t *exitcode,
                           double *scratch)
{
    return guarded([&] {
        return solve("kvx_gp_batch_solve_dev", true,
                     pack_gp(B, n, ml, p, F, sF, g, sg, G, sG, h, sh, A, sA, b, sb, maxiters, abstol, reltol, feastol, x, y, s, z, stats,
                             iterations, exitcode, scratch),
                     mnl, K);
    });
}

}  // extern "C"
