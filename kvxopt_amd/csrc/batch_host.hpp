// What the batch solvers share outside their kernels (qp_batch, lp_batch, socp_batch, sdp_batch, conelp_batch, coneqp_batch,
// gp_batch, and the derivative entries of qp_batch_diff and coneqp_batch_diff): the part of the kernel arguments that is the same
// for all, and for the host entries (*_batch_api.cpp, *_batch_diff_api.cpp) the refusal with its message, the checks of pointers,
// strides and options, the question for a device, the arguments packed from the C ABI, and the two ladders of upload,
// allocation, launch, synchronisation and download: solve_host for a solver, diff_host for a derivative.  A host entry keeps
// its limits with their texts and its extern "C" functions; the limits and the placement of a cone are in batch_cone_host.hpp.
#pragma once
#include "../../include/kvxhip.h"
#include "abi_guard.hpp"
#include "devpool.hpp"

#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>

#define HIPCHK(call)                                                             \
    do {                                                                         \
        hipError_t e_ = (call);                                                  \
        if (e_ != hipSuccess) return KVX_EDEVICE;                                \
    } while (0)

namespace kvx {

// The arguments every batch kernel takes; a solver's own struct derives from it and stays a trivially copyable aggregate.
struct BatchArgs {
    int64_t B;
    int n, ml, p;                             // ml: the 'l' rows
    // device pointers; matrices dense and column-major per member (G rows x n; A p x n); c: the linear term of the objective
    // (q of a QP); s*: distance between two members in doubles, 0: one for all
    const double *c, *G, *h, *A, *b;
    int64_t sc, sG, sh, sA, sb;
    int maxiters;
    double abstol, reltol, feastol;
    // results: x (n x B), y (p x B), s, z (rows x B), stats (the solver's NSTAT x B), iterations and exit (B each)
    double *x, *y, *s, *z, *stats;
    int64_t *iters, *exitc;
};

namespace batchhost {

inline int refuse(const char *who, const std::string &why)
{
    set_last_error(std::string(who) + ": " + why);
    return KVX_EINVAL;
}

inline int need_device(const char *who)
{
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) {
        set_last_error(std::string(who) + ": no HIP device; the batch has no CPU fallback");
        return KVX_EDEVICE;
    }
    return KVX_OK;
}

struct Part { const char *name; int64_t stride, size; };      // size: doubles of one member; stride 0 (shared) or >= size

// What every entry checks after its own limits and before a device is asked for: the pointers, the member strides and the
// options.  rows: the rows of G and h.  linear: the name of c.  first, first_ok: a solver's own leading data (P of a QP).
inline int check_common(const char *who, const BatchArgs &a, int64_t rows, const char *linear = "c", const Part *first = nullptr,
                        bool first_ok = true)
{
    if (!first_ok || !a.c || !a.G || !a.h || (a.p > 0 && (!a.A || !a.b))) return refuse(who, "a data pointer is NULL");
    if (!a.x || !a.s || !a.z || !a.stats || !a.iters || !a.exitc || (a.p > 0 && !a.y)) return refuse(who, "a result pointer is NULL");
    const int64_t n = a.n, p = a.p;
    const Part parts[] = {first ? *first : Part{"", 0, 0}, {linear, a.sc, n}, {"G", a.sG, rows * n}, {"h", a.sh, rows},
                          {"A", a.sA, p * n}, {"b", a.sb, p}};
    for (const auto &t : parts)
        if (t.stride != 0 && t.stride < t.size)
            return refuse(who, std::string("the member stride of ") + t.name + " is 0 or at least its size");
    if (a.maxiters < 1) return refuse(who, "maxiters must be a positive integer");
    if (!(a.feastol > 0.0)) return refuse(who, "feastol must be a positive scalar");
    if (!(a.reltol > 0.0) && !(a.abstol > 0.0)) return refuse(who, "at least one of reltol and abstol must be positive");
    return KVX_OK;
}

// The common arguments as the C ABI passes them
template <class Args>
Args pack(int64_t B, int64_t n, int64_t ml, int64_t p, const double *c, int64_t sc, const double *G, int64_t sG, const double *h,
          int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb, int64_t maxiters, double abstol, double reltol,
          double feastol, double *x, double *y, double *s, double *z, double *stats, int64_t *iterations, int64_t *exitcode)
{
    const auto small = [](int64_t v) { return (int)(v < -1 ? -1 : (v > 1000000000 ? 1000000000 : v)); };    // the checks see the range
    Args a = {};
    a.B = B; a.n = small(n); a.ml = small(ml); a.p = small(p);
    a.c = c; a.G = G; a.h = h; a.A = A; a.b = b;
    a.sc = sc; a.sG = sG; a.sh = sh; a.sA = sA; a.sb = sb;
    a.maxiters = small(maxiters); a.abstol = abstol; a.reltol = reltol; a.feastol = feastol;
    a.x = x; a.y = y; a.s = s; a.z = z; a.stats = stats; a.iters = iterations; a.exitc = exitcode;
    return a;
}

struct Buffers {                              // the device copies of one host call, given back to the pool on every path
    std::vector<void *> own;
    ~Buffers() { for (void *p : own) (void)pool_free(p); }
    int get(double **d, int64_t count)
    {
        HIPCHK(pool_malloc((void **)d, (size_t)(count > 0 ? count : 1) * sizeof(double)));
        own.push_back(*d);
        return KVX_OK;
    }
    int up(const double **d, const double *h, int64_t count)
    {
        double *t = nullptr;
        int rc = get(&t, count);
        if (rc) return rc;
        if (count > 0) HIPCHK(hipMemcpy(t, h, (size_t)count * sizeof(double), hipMemcpyHostToDevice));
        *d = t;
        return KVX_OK;
    }
};

inline int down(void *h, const void *d, int64_t count)
{
    if (count > 0) HIPCHK(hipMemcpy(h, d, (size_t)count * 8, hipMemcpyDeviceToHost));
    return KVX_OK;
}

// The checked batch `a`, every pointer a device pointer (the _dev entry), through launch(args) and a synchronisation
template <class Args, class Launch>
int solve_dev(const Args &a, Launch launch)
{
    HIPCHK(launch(a));
    HIPCHK(hipStreamSynchronize(nullptr));
    return KVX_OK;
}

// The checked batch `h` of host pointers: the data goes up, launch(args) and a synchronisation, the results come down, and the
// copies return to the pool on every path.  rows: the rows of G, h, s and z; nstat: the stats of a member.  first: a solver's
// own leading data (P of a QP) with its stride and size.
template <class Args, class Launch>
int solve_host(const Args &h, int64_t rows, int64_t nstat, Launch launch, const double *Args::*first = nullptr, int64_t sfirst = 0,
               int64_t nfirst = 0)
{
    const int64_t B = h.B, n = h.n, p = h.p;
    const auto extent = [&](int64_t stride, int64_t size) { return stride ? (B - 1) * stride + size : size; };
    Args d = h;
    Buffers buf;
    int rc;
    double *iters = nullptr, *exitc = nullptr;                     // int64 results travel in 8-byte slots of the same pool
    if ((first && (rc = buf.up(&(d.*first), h.*first, extent(sfirst, nfirst)))) || (rc = buf.up(&d.c, h.c, extent(h.sc, n))) ||
        (rc = buf.up(&d.G, h.G, extent(h.sG, rows * n))) || (rc = buf.up(&d.h, h.h, extent(h.sh, rows))) ||
        (p > 0 && ((rc = buf.up(&d.A, h.A, extent(h.sA, p * n))) || (rc = buf.up(&d.b, h.b, extent(h.sb, p))))) ||
        (rc = buf.get(&d.x, n * B)) || (rc = buf.get(&d.y, p * B)) || (rc = buf.get(&d.s, rows * B)) ||
        (rc = buf.get(&d.z, rows * B)) || (rc = buf.get(&d.stats, nstat * B)) || (rc = buf.get(&iters, B)) ||
        (rc = buf.get(&exitc, B)))
        return rc;
    d.iters = reinterpret_cast<int64_t *>(iters);
    d.exitc = reinterpret_cast<int64_t *>(exitc);
    HIPCHK(launch(d));
    HIPCHK(hipStreamSynchronize(nullptr));
    if ((rc = down(h.x, d.x, n * B)) || (rc = down(h.y, d.y, p * B)) || (rc = down(h.s, d.s, rows * B)) ||
        (rc = down(h.z, d.z, rows * B)) || (rc = down(h.stats, d.stats, nstat * B)) || (rc = down(h.iters, d.iters, B)) ||
        (rc = down(h.exitc, d.exitc, B)))
        return rc;
    return KVX_OK;
}

// ---- the derivative entries (vjp, jvp).  Args: a solver's arguments with P, sP and the derivative's fields of
// qp_batch_diff.hpp under the same names; x, y, s, z are the solution, exitc the exit of the derivative.  rows: the rows of G,
// s and z.  full: q, h and b enter (they travel as c, h, b of BatchArgs).

// The pointers and the member strides; extra_ok: the entry's own result pointers are there.
template <class Args>
int check_diff(const char *who, const Args &a, int64_t rows, bool jvp, bool full, bool extra_ok = true)
{
    const bool eq = a.p > 0;
    if (!a.P || !a.G || (eq && !a.A) || (full && (!a.c || !a.h || (eq && !a.b)))) return refuse(who, "a data pointer is NULL");
    if (!a.x || !a.s || !a.z || (eq && !a.y) || !a.solexit) return refuse(who, "a solution pointer is NULL");
    if (!jvp && !a.gx) return refuse(who, "the cotangent pointer is NULL");
    if (!a.ux || !a.uz || (eq && !a.uy) || (jvp && !a.us) || !extra_ok || !a.exitc) return refuse(who, "a result pointer is NULL");
    const int64_t n = a.n, p = a.p;
    const Part parts[] = {{"P", a.sP, n * n}, {"q", full ? a.sc : 0, n}, {"G", a.sG, rows * n}, {"h", full ? a.sh : 0, rows},
                          {"A", a.sA, p * n}, {"b", full ? a.sb : 0, p},
                          {"dP", jvp && a.dP ? a.sdP : 0, n * n}, {"dq", jvp && a.dq ? a.sdq : 0, n},
                          {"dG", jvp && a.dG ? a.sdG : 0, rows * n}, {"dh", jvp && a.dh ? a.sdh : 0, rows},
                          {"dA", jvp && eq && a.dA ? a.sdA : 0, p * n}, {"db", jvp && eq && a.db ? a.sdb : 0, p}};
    for (const auto &t : parts)
        if (t.stride != 0 && t.stride < t.size)
            return refuse(who, std::string("the member stride of ") + t.name + " is 0 or at least its size");
    return KVX_OK;
}

// The arguments all four entries of a derivative share, as the C ABI passes them; q, h, b NULL where they do not enter
template <class Args>
Args pack_diff(int mode, int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *q, int64_t sq,
               const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb,
               const double *x, const double *y, const double *s, const double *z, const int64_t *exitcode, int64_t refinement,
               double *ux, double *uy, double *uz, int64_t *gexit)
{
    Args a = pack<Args>(B, n, ml, p, q, sq, G, sG, h, sh, A, sA, b, sb, refinement, 0.0, 0.0, 0.0, const_cast<double *>(x),
                        const_cast<double *>(y), const_cast<double *>(s), const_cast<double *>(z), nullptr, nullptr, gexit);
    a.P = P; a.sP = sP; a.solexit = exitcode; a.mode = mode; a.refinement = a.maxiters;
    a.ux = ux; a.uy = uy; a.uz = uz;
    return a;
}

template <class Args>
void set_vjp(Args &a, const double *gx, double *gP, double *gG, double *gA)
{
    a.gx = gx; a.gP = gP; a.gG = gG; a.gA = gA;
}

template <class Args>
void set_jvp(Args &a, const double *dP, int64_t sdP, const double *dq, int64_t sdq, const double *dG, int64_t sdG, const double *dh,
             int64_t sdh, const double *dA, int64_t sdA, const double *db, int64_t sdb, double *ds)
{
    a.dP = dP; a.sdP = sdP; a.dq = dq; a.sdq = sdq; a.dG = dG; a.sdG = sdG; a.dh = dh; a.sdh = sdh;
    a.dA = dA; a.sdA = sdA; a.db = db; a.sdb = sdb; a.us = ds;
}

struct NoExtra {                              // an entry without per-member results of its own
    template <class Args> int get(Buffers &, Args &, int64_t) const { return KVX_OK; }
    template <class Args> int down(const Args &, const Args &, int64_t) const { return KVX_OK; }
};

// The checked derivative batch `h` of host pointers: the problem data the entry names in `data` and the solution go up, then
// the inputs of the mode; the results are allocated; launch(args), which synchronises; ux, uy, uz and the exits come down, then
// us or the matrix gradients.  extra.get(buf, d, B) allocates and extra.down(h, d, B) fetches the entry's own per-member
// results.  The copies return to the pool on every path.
template <class Args, class Launch, class Extra = NoExtra>
int diff_host(const Args &h, int64_t rows, bool jvp, bool full, Launch launch, Extra extra = Extra())
{
    const int64_t B = h.B, n = h.n, p = h.p;
    const auto extent = [&](int64_t stride, int64_t size) { return stride ? (B - 1) * stride + size : size; };
    const auto members = [&](int64_t stride, int64_t size) { return stride ? B * size : size; };      // of a matrix gradient
    Args d = h;
    Buffers buf;
    int rc;
    const auto up = [&](const double *Args::*f, int64_t count) { return h.*f ? buf.up(&(d.*f), h.*f, count) : KVX_OK; };
    const auto get = [&](double *Args::*f, int64_t count) { return h.*f ? buf.get(&(d.*f), count) : KVX_OK; };
    const double *xin = nullptr, *yin = nullptr, *sin = nullptr, *zin = nullptr, *ein = nullptr;
    double *eout = nullptr;                                        // int64 travels in 8-byte slots of the same pool
    if ((rc = buf.up(&d.P, h.P, extent(h.sP, n * n))) || (full && (rc = buf.up(&d.c, h.c, extent(h.sc, n)))) ||
        (rc = buf.up(&d.G, h.G, extent(h.sG, rows * n))) || (full && (rc = buf.up(&d.h, h.h, extent(h.sh, rows)))) ||
        (p > 0 && ((rc = buf.up(&d.A, h.A, extent(h.sA, p * n))) || (full && (rc = buf.up(&d.b, h.b, extent(h.sb, p)))))) ||
        (rc = buf.up(&xin, h.x, n * B)) || (p > 0 && (rc = buf.up(&yin, h.y, p * B))) || (rc = buf.up(&sin, h.s, rows * B)) ||
        (rc = buf.up(&zin, h.z, rows * B)) || (rc = buf.up(&ein, reinterpret_cast<const double *>(h.solexit), B)) ||
        (rc = buf.get(&eout, B)) || (rc = extra.get(buf, d, B)))
        return rc;
    d.x = const_cast<double *>(xin); d.y = const_cast<double *>(yin); d.s = const_cast<double *>(sin); d.z = const_cast<double *>(zin);
    d.solexit = reinterpret_cast<const int64_t *>(ein);
    d.exitc = reinterpret_cast<int64_t *>(eout);
    if (jvp) {
        if ((rc = up(&Args::dP, extent(h.sdP, n * n))) || (rc = up(&Args::dq, extent(h.sdq, n))) ||
            (rc = up(&Args::dG, extent(h.sdG, rows * n))) || (rc = up(&Args::dh, extent(h.sdh, rows))) ||
            (p > 0 && ((rc = up(&Args::dA, extent(h.sdA, p * n))) || (rc = up(&Args::db, extent(h.sdb, p))))) ||
            (rc = get(&Args::us, rows * B)))
            return rc;
    } else {
        if ((rc = up(&Args::gx, n * B)) || (rc = get(&Args::gP, members(h.sP, n * n))) ||
            (rc = get(&Args::gG, members(h.sG, rows * n))) || (p > 0 && (rc = get(&Args::gA, members(h.sA, p * n)))))
            return rc;
    }
    if ((rc = get(&Args::ux, n * B)) || (p > 0 && (rc = get(&Args::uy, p * B))) || (rc = get(&Args::uz, rows * B))) return rc;
    if ((rc = launch(d))) return rc;
    if ((rc = down(h.ux, d.ux, n * B)) || (p > 0 && (rc = down(h.uy, d.uy, p * B))) || (rc = down(h.uz, d.uz, rows * B)) ||
        (rc = down(h.exitc, d.exitc, B)) || (rc = extra.down(h, d, B)))
        return rc;
    if (jvp) return down(h.us, d.us, rows * B);
    if ((h.gP && (rc = down(h.gP, d.gP, members(h.sP, n * n)))) || (h.gG && (rc = down(h.gG, d.gG, members(h.sG, rows * n)))) ||
        (p > 0 && h.gA && (rc = down(h.gA, d.gA, members(h.sA, p * n)))))
        return rc;
    return KVX_OK;
}

}  // namespace batchhost
}  // namespace kvx
