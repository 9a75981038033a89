// kvx_gp_batch_vjp / kvx_gp_batch_jvp and their _dev forms (include/kvxhip.h): the limits of k_gp_batch_diff
// (gp_batch_diff.hip), its launch, and after a reverse-mode launch k_batch_outer_sum for every matrix the members share.  The
// refusal, the question for a device, the pooled copies and solve_dev are those of batch_host.hpp, the limits of a member those
// of gp_batch.hpp.  check_diff, pack_diff and diff_host are not used, for the reasons gp_batch_api.cpp has: they know P (n x n)
// and q (n) where this program has F (l x n) and g (l); they take one `rows` for G, h, s and z, where G has ml >= 0 rows (and
// may be NULL) beside s, z, uz of N = mnl + 1 + ml; and a reverse-mode call has an l-vector result (dl/dg) and a workspace.
// g enters, for y; h and b of the problem do not.
#include "batch_host.hpp"
#include "gp_batch_diff.hpp"

using namespace kvx;
using namespace kvx::batchhost;

namespace {

bool wants_a(const GpDiffArgs &a) { return a.mode == GPD_VJP && a.gF && !a.sF; }      // a shared F: its sum needs a = zeta y

// What all four entries check before a device is asked for; on success the blocks are placed in `a`
int check(const char *who, GpDiffArgs &a, int64_t mnl, const int64_t *K, bool resident)
{
    if (int rc = gphost::place_blocks(who, a, mnl, K)) return rc;
    if (a.refinement < 0 || a.refinement > GPD_MAX_REFINEMENT) return refuse(who, "0 <= refinement <= 3 is required");
    if (gp_batch_diff_lds_bytes(a.n, a.m, a.l, a.ml, a.p) > 160 * 1024) return refuse(who, "the member needs more than 160 KiB of LDS");
    const bool jvp = a.mode == GPD_JVP, eq = a.p > 0, in = a.ml > 0;
    if (!a.F || !a.c || (in && !a.G) || (eq && !a.A)) return refuse(who, "a data pointer is NULL");
    if (!a.x || !a.s || !a.z || (eq && !a.y) || !a.solexit) return refuse(who, "a solution pointer is NULL");
    if (!jvp && !a.gx) return refuse(who, "the cotangent pointer is NULL");
    if (!a.ux || !a.uz || (eq && !a.uy) || (jvp && !a.us) || (!jvp && !a.gg) || !a.exitc) return refuse(who, "a result pointer is NULL");
    if (resident && wants_a(a) && !a.ga) return refuse(who, "the workspace pointer is NULL");
    const int64_t n = a.n, ml = a.ml, p = a.p, l = a.l;
    const Part parts[] = {{"F", a.sF, l * n}, {"g", a.sc, l}, {"G", in ? a.sG : 0, ml * n}, {"A", eq ? a.sA : 0, p * n},
                          {"dF", jvp && a.dF ? a.sdF : 0, l * n}, {"dg", jvp && a.dg ? a.sdg : 0, l},
                          {"dG", jvp && in && a.dG ? a.sdG : 0, ml * n}, {"dh", jvp && in && a.dh ? a.sdh : 0, ml},
                          {"dA", jvp && eq && a.dA ? a.sdA : 0, p * n}, {"db", jvp && eq && a.db ? a.sdb : 0, p}};
    for (const auto &t : parts)
        if (t.stride != 0 && t.stride < t.size)
            return refuse(who, std::string("the member stride of ") + t.name + " is 0 or at least its size");
    return KVX_OK;
}

// The launches of one call on device pointers: the members, then the sums for the matrices all members share.  The rows of G
// are the last ml of the N rows of uz and z.
hipError_t launch(const GpDiffArgs &d)
{
    hipError_t e = launch_gp_batch_diff(nullptr, d);
    if (e != hipSuccess || d.mode != GPD_VJP) return e;
    const int N = d.m + d.ml;
    if (wants_a(d)) e = launch_batch_outer_sum(nullptr, d.B, d.l, d.n, d.ga, d.ux, d.gg, d.x, 1.0, false, d.exitc, d.gF);
    if (e == hipSuccess && d.ml > 0 && d.gG && !d.sG)
        e = launch_batch_outer_sum(nullptr, d.B, d.ml, d.n, d.uz + d.m, d.x, d.z + d.m, d.ux, 1.0, false, d.exitc, d.gG, N);
    if (e == hipSuccess && d.p > 0 && d.gA && !d.sA)
        e = launch_batch_outer_sum(nullptr, d.B, d.p, d.n, d.uy, d.x, d.y, d.ux, 1.0, false, d.exitc, d.gA);
    return e;
}

int synced(const GpDiffArgs &d) { return solve_dev(d, launch); }

// The checked batch `h` of host pointers: the data and the solution go up, then the inputs of the mode; the results and the
// workspace are taken from the pool; the launches and a synchronisation; the results come down.  The copies return to the pool
// on every path.
int diff_host_gp(const GpDiffArgs &h)
{
    const int64_t B = h.B, n = h.n, ml = h.ml, p = h.p, l = h.l, N = h.m + ml;
    const bool jvp = h.mode == GPD_JVP;
    const auto extent = [&](int64_t stride, int64_t size) { return stride ? (B - 1) * stride + size : size; };
    const auto members = [&](int64_t stride, int64_t size) { return stride ? B * size : size; };      // of a matrix gradient
    GpDiffArgs d = h;
    Buffers buf;
    int rc;
    const auto up = [&](const double *GpDiffArgs::*f, int64_t count) { return h.*f ? buf.up(&(d.*f), h.*f, count) : KVX_OK; };
    const auto get = [&](double *GpDiffArgs::*f, int64_t count) { return h.*f ? buf.get(&(d.*f), count) : KVX_OK; };
    const double *xin = nullptr, *yin = nullptr, *sin = nullptr, *zin = nullptr, *ein = nullptr;
    double *eout = nullptr;                                        // int64 travels in 8-byte slots of the same pool
    if ((rc = buf.up(&d.F, h.F, extent(h.sF, l * n))) || (rc = buf.up(&d.c, h.c, extent(h.sc, l))) ||
        (ml > 0 && (rc = buf.up(&d.G, h.G, extent(h.sG, ml * n)))) || (p > 0 && (rc = buf.up(&d.A, h.A, extent(h.sA, p * n)))) ||
        (rc = buf.up(&xin, h.x, n * B)) || (p > 0 && (rc = buf.up(&yin, h.y, p * B))) || (rc = buf.up(&sin, h.s, N * B)) ||
        (rc = buf.up(&zin, h.z, N * B)) || (rc = buf.up(&ein, reinterpret_cast<const double *>(h.solexit), B)) ||
        (rc = buf.get(&eout, B)))
        return rc;
    d.x = const_cast<double *>(xin); d.y = const_cast<double *>(yin); d.s = const_cast<double *>(sin); d.z = const_cast<double *>(zin);
    d.solexit = reinterpret_cast<const int64_t *>(ein);
    d.exitc = reinterpret_cast<int64_t *>(eout);
    if (jvp) {
        if ((rc = up(&GpDiffArgs::dF, extent(h.sdF, l * n))) || (rc = up(&GpDiffArgs::dg, extent(h.sdg, l))) ||
            (ml > 0 && ((rc = up(&GpDiffArgs::dG, extent(h.sdG, ml * n))) || (rc = up(&GpDiffArgs::dh, extent(h.sdh, ml))))) ||
            (p > 0 && ((rc = up(&GpDiffArgs::dA, extent(h.sdA, p * n))) || (rc = up(&GpDiffArgs::db, extent(h.sdb, p))))) ||
            (rc = get(&GpDiffArgs::us, N * B)))
            return rc;
    } else {
        d.ga = nullptr;
        if ((rc = up(&GpDiffArgs::gx, n * B)) || (rc = get(&GpDiffArgs::gg, l * B)) || (wants_a(h) && (rc = buf.get(&d.ga, l * B))) ||
            (rc = get(&GpDiffArgs::gF, members(h.sF, l * n))) || (ml > 0 && (rc = get(&GpDiffArgs::gG, members(h.sG, ml * n)))) ||
            (p > 0 && (rc = get(&GpDiffArgs::gA, members(h.sA, p * n)))))
            return rc;
    }
    if ((rc = get(&GpDiffArgs::ux, n * B)) || (p > 0 && (rc = get(&GpDiffArgs::uy, p * B))) || (rc = get(&GpDiffArgs::uz, N * B))) return rc;
    if ((rc = synced(d))) return rc;
    if ((rc = down(h.ux, d.ux, n * B)) || (p > 0 && (rc = down(h.uy, d.uy, p * B))) || (rc = down(h.uz, d.uz, N * B)) ||
        (rc = down(h.exitc, d.exitc, B)))
        return rc;
    if (jvp) return down(h.us, d.us, N * B);
    if ((rc = down(h.gg, d.gg, l * B)) || (h.gF && (rc = down(h.gF, d.gF, members(h.sF, l * n)))) ||
        (ml > 0 && h.gG && (rc = down(h.gG, d.gG, members(h.sG, ml * n)))) ||
        (p > 0 && h.gA && (rc = down(h.gA, d.gA, members(h.sA, p * n)))))
        return rc;
    return KVX_OK;
}

int run(const char *who, bool resident, GpDiffArgs a, int64_t mnl, const int64_t *K)
{
    int rc = check(who, a, mnl, K, resident);
    if (rc || (rc = need_device(who))) return rc;
    return resident ? synced(a) : diff_host_gp(a);
}

}  // namespace

#define GPD_PROBLEM                                                                                                                   \
    int64_t B, int64_t n, int64_t mnl, const int64_t *K, int64_t ml, int64_t p, const double *F, int64_t sF, const double *g, int64_t sg, \
        const double *G, int64_t sG, const double *A, int64_t sA, const double *x, const double *y, const double *s, const double *z,    \
        const int64_t *exitcode, int64_t refinement
#define GPD_PASSED B, n, mnl, K, ml, p, F, sF, g, sg, G, sG, A, sA, x, y, s, z, exitcode, refinement

namespace {

// The arguments all four entries share, as the C ABI passes them; h and b do not enter
GpDiffArgs pack_gp_diff(int mode, GPD_PROBLEM, double *ux, double *uy, double *uz, int64_t *gexit)
{
    GpDiffArgs a = pack<GpDiffArgs>(B, n, ml, p, g, sg, G, sG, nullptr, 0, A, sA, nullptr, 0, refinement, 0.0, 0.0, 0.0,
                                    const_cast<double *>(x), const_cast<double *>(y), const_cast<double *>(s), const_cast<double *>(z),
                                    nullptr, nullptr, gexit);
    a.F = F; a.sF = sF; a.solexit = exitcode; a.mode = mode; a.refinement = a.maxiters;
    a.ux = ux; a.uy = uy; a.uz = uz;
    return a;
}

int vjp(const char *who, bool resident, GPD_PROBLEM, const double *gx, double *ux, double *uy, double *uz, double *gg, double *gF,
        double *gG, double *gA, double *work, int64_t *gexit)
{
    return guarded([&] {
        GpDiffArgs a = pack_gp_diff(GPD_VJP, GPD_PASSED, ux, uy, uz, gexit);
        a.gx = gx; a.gg = gg; a.gF = gF; a.gG = gG; a.gA = gA; a.ga = work;
        return run(who, resident, a, mnl, K);
    });
}

int jvp(const char *who, bool resident, GPD_PROBLEM, const double *dF, int64_t sdF, const double *dg, int64_t sdg, const double *dG,
        int64_t sdG, const double *dh, int64_t sdh, const double *dA, int64_t sdA, const double *db, int64_t sdb, double *dx, double *dy,
        double *dz, double *ds, int64_t *gexit)
{
    return guarded([&] {
        GpDiffArgs a = pack_gp_diff(GPD_JVP, GPD_PASSED, dx, dy, dz, gexit);
        a.dF = dF; a.sdF = sdF; a.dg = dg; a.sdg = sdg; a.dG = dG; a.sdG = sdG; a.dh = dh; a.sdh = sdh;
        a.dA = dA; a.sdA = sdA; a.db = db; a.sdb = sdb; a.us = ds;
        return run(who, resident, a, mnl, K);
    });
}

}  // namespace

extern "C" {

int kvx_gp_batch_vjp(GPD_PROBLEM, const double *gx, double *ux, double *uy, double *uz, double *gg, double *gF, double *gG, double *gA,
                     int64_t *gexit)
{
    return vjp("kvx_gp_batch_vjp", false, GPD_PASSED, gx, ux, uy, uz, gg, gF, gG, gA, nullptr, gexit);
}

int kvx_gp_batch_vjp_dev(GPD_PROBLEM, const double *gx, double *ux, double *uy, double *uz, double *gg, double *gF, double *gG,
                         double *gA, double *work, int64_t *gexit)
{
    return vjp("kvx_gp_batch_vjp_dev", true, GPD_PASSED, gx, ux, uy, uz, gg, gF, gG, gA, work, gexit);
}

int kvx_gp_batch_jvp(GPD_PROBLEM, const double *dF, int64_t sdF, const double *dg, int64_t sdg, const double *dG, int64_t sdG,
                     const double *dh, int64_t sdh, const double *dA, int64_t sdA, const double *db, int64_t sdb, double *dx, double *dy,
                     double *dz, double *ds, int64_t *gexit)
{
    return jvp("kvx_gp_batch_jvp", false, GPD_PASSED, dF, sdF, dg, sdg, dG, sdG, dh, sdh, dA, sdA, db, sdb, dx, dy, dz, ds, gexit);
}

int kvx_gp_batch_jvp_dev(GPD_PROBLEM, const double *dF, int64_t sdF, const double *dg, int64_t sdg, const double *dG, int64_t sdG,
                         const double *dh, int64_t sdh, const double *dA, int64_t sdA, const double *db, int64_t sdb, double *dx,
                         double *dy, double *dz, double *ds, int64_t *gexit)
{
    return jvp("kvx_gp_batch_jvp_dev", true, GPD_PASSED, dF, sdF, dg, sdg, dG, sdG, dh, sdh, dA, sdA, db, sdb, dx, dy, dz, ds, gexit);
}

int64_t kvx_gp_batch_diff_lds_bytes(int64_t n, int64_t mnl, const int64_t *K, int64_t ml, int64_t p, int64_t *forward)
{
    if (n < 1 || n > GPB_MAX_N || mnl < 0 || ml < 0 || mnl + 1 + ml > GPB_MAX_ROWS || p < 0 || p > n || !K) return -1;
    int64_t l = 0;
    for (int64_t i = 0; i <= mnl; i++) {
        if (K[i] < 1 || K[i] > GPB_MAX_L) return -1;
        l += K[i];
    }
    if (l > GPB_MAX_L) return -1;
    if (forward) *forward = (int64_t)gp_batch_lds_bytes((int)n, (int)mnl + 1, (int)l, (int)ml, (int)p);
    return (int64_t)gp_batch_diff_lds_bytes((int)n, (int)mnl + 1, (int)l, (int)ml, (int)p);
}

}  // extern "C"
