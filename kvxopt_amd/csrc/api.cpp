// C-ABI of libkvxhip.so (include/kvxhip.h): the entry points of the Cholesky path (set-up, schedule and solves: chol_*.cpp).
// There is NO CPU fallback: every numeric entry point needs a HIP device and returns
// KVX_EDEVICE otherwise.
#include "chol_internal.hpp"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <mutex>
#include <vector>

using namespace kvx;

static thread_local std::string g_err;

// ---- launch-graph instantiations in flight (chol_internal.hpp, LazyExec) ------------------------------------------------
namespace {
struct LazyRegistry {
    std::mutex mu;
    std::vector<std::shared_future<hipGraphExec_t>> futs;
    ~LazyRegistry()                                  // static destruction = process exit: nothing of HIP may run behind this point
    {
        std::lock_guard<std::mutex> lk(mu);
        for (auto &f : futs)
            if (f.valid()) f.wait();
    }
};
LazyRegistry &lazy_registry() { static LazyRegistry R; return R; }
}  // namespace
std::atomic<int> &lazy_exec_failures() { static std::atomic<int> n{0}; return n; }
void lazy_exec_track(const std::shared_future<hipGraphExec_t> &f)
{
    LazyRegistry &R = lazy_registry();
    std::lock_guard<std::mutex> lk(R.mu);
    // finished ones go; the list stays as short as the number of instantiations in flight
    R.futs.erase(std::remove_if(R.futs.begin(), R.futs.end(), [](const std::shared_future<hipGraphExec_t> &g) {
                     return !g.valid() || g.wait_for(std::chrono::seconds(0)) == std::future_status::ready; }), R.futs.end());
    R.futs.push_back(f);
}
extern "C" int kvx_graph_instantiate_failures(void) { return lazy_exec_failures().load(); }
namespace kvx { void set_last_error(const std::string &s) { g_err = s; } }   // (also used by lu_api.cpp, dist_api.cpp)

extern "C" {

const char *kvx_version(void) { return "kvxhip 0.1 (gfx950)"; }
const char *kvx_last_error(void) { return g_err.c_str(); }
int kvx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int kvx_current_device(void)
{
    int n = 0, d = -1;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return -1; }
    if (hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return d;
}

int kvx_set_device(int dev)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); set_err("no HIP device visible"); return KVX_EDEVICE; }
    if (dev < 0 || dev >= n) { set_err("kvx_set_device: no such device"); return KVX_EINVAL; }
    HIPCHK(hipSetDevice(dev));
    return KVX_OK;
}

void kvx_chol_default_opts(kvx_chol_opts *o)
{
    memset(o, 0, sizeof(*o));
    o->supernodal = 2;
    o->ordering = 0;
    o->postorder = 1;
    o->relax_small = 4;
    o->relax_z1 = 0.8;
    o->relax_z2 = 0.1;
    o->relax_z3 = -1.0;     // < 0: by the order of the matrix -- 0.075 (CHOLMOD's own default is 0.05: measured on MI355X, section 3 of
                            // DESIGN.md), 0.2 up to 150 000 columns (see kvx_chol_analyze)
    // (experiments: KVX_RELAX_Z1 / _Z2 / _Z3 override the defaults of every analysis in the process)
    if (const char *e = getenv("KVX_RELAX_Z1")) o->relax_z1 = atof(e);
    if (const char *e = getenv("KVX_RELAX_Z2")) o->relax_z2 = atof(e);
    if (const char *e = getenv("KVX_RELAX_Z3")) o->relax_z3 = atof(e);
    o->dbound = 0.0;
}

int kvx_chol_analyze(int64_t n, const int64_t *colptr, const int64_t *rowind, int uplo, const int64_t *perm,
                     const kvx_chol_opts *opts, kvx_chol **out)
{
    if (!out || n < 0 || (n > 0 && (!colptr || (!rowind && colptr[n] > 0)))) { set_err("bad arguments"); return KVX_EINVAL; }
    kvx_chol_opts o;
    if (opts) o = *opts; else kvx_chol_default_opts(&o);
    if (o.supernodal < 0 || o.supernodal > 2) { set_err("options['supernodal'] must be 0, 1 or 2"); return KVX_EINVAL; }
    if (o.ordering < 0 || o.ordering > 3) { set_err("ordering must be 0 (best of the library's own), 1 (natural), 2 (nested dissection) or 3 (minimum degree)"); return KVX_EINVAL; }
    kvx_chol *F = nullptr;
    try {
        F = new kvx_chol();
        F->opts = o;
        SymOpts so;
        so.ordering = o.ordering;
        so.postorder = o.postorder;
        so.relax_small = o.relax_small;
        so.relax_z1 = o.relax_z1; so.relax_z2 = o.relax_z2; so.relax_z3 = o.relax_z3;
        // Zero fraction a wide chain supernode may take on when it joins its parent.  A small factorisation is a chain of levels on an
        // idle machine: explicit zeros cost nothing there and every level saved is 50-100 us (5-pt Laplacian 200 x 200: 12 -> 9
        // levels, step 1.25 -> 1.08 ms; the KKT system of the interior-point leg, n = 50 000: 520 -> 565 iterations/s); from a few
        // 10^5 columns on the merged fronts lengthen the pivot chains at the top of the tree by more than the levels save
        // (1000 x 1000: 4.62 -> 4.81 ms with 0.2; 64^3: 17.2 -> 18.7 ms).  Crossover measured between 1.2e5 and 2.5e5 columns.
        if (so.relax_z3 < 0) so.relax_z3 = n <= 150000 ? 0.2 : 0.075;
        if (o.reserved[0] > 0) so.nd_leaf = o.reserved[0];
        if (o.reserved[1] != 0) so.leaf_cols = o.reserved[1] < 0 ? 0 : o.reserved[1];
        if (o.reserved[2] > 0) so.leaf_rows = o.reserved[2];
        so.compare_given = o.reserved[4] == 1 ? 1 : 0;
        if (o.reserved[5] > 0) so.amd_auto_max = o.reserved[5];
        if (o.reserved[6] != 0) so.nd_min_n = std::max<int64_t>(0, o.reserved[6]);      // (-1: always compute the dissection too)
        static const int64_t zero = 0;
        analyze(n, n ? colptr : &zero, rowind, uplo, perm, so, F->S);
        // options['supernodal'] (spsolvers.rst:731-736): 2 -> LL'; 0 -> LDL'; 1 -> whichever CHOLMOD would find cheaper,
        // by its own rule flops / nnz(L) >= 40 -> supernodal LL'.  The arithmetic is the supernodal LL' kernels either
        // way; an LDL' factor is the same numbers seen as L = Lc diag(Lc)^-1, D = diag(Lc)^2 (solve sys = 2..6,
        // getfactor and diag follow that form).
        F->is_ll = o.supernodal == 2 || (o.supernodal == 1 && F->S.lnz > 0 && F->S.flops / (double)F->S.lnz >= 40.0);
        F->minor = n;
    } catch (const std::invalid_argument &e) {
        delete F; set_err(e.what()); return KVX_EPERM;
    } catch (const std::bad_alloc &) {
        delete F; set_err("out of host memory"); return KVX_ENOMEM;
    } catch (const std::exception &e) {
        delete F; set_err(e.what()); return KVX_EINVAL;
    }
    *out = F;
    return KVX_OK;
}

static int kvx_chol_factorize_async_dev_impl(kvx_chol *F, const double *values_dev)
{
    if (!F) return KVX_EINVAL;
    int rc = ensure_device(F);
    if (rc) return rc;
    if ((rc = wait_for_caller(F))) return rc;
    if (F->S.nnzA > 0)
        HIPCHK(hipMemcpyAsync(F->d_Ax, values_dev, F->S.nnzA * sizeof(double), hipMemcpyDeviceToDevice, F->stream));
    return enqueue_factor(F);
}

int kvx_chol_factorize_async_dev(kvx_chol *F, const double *values_dev)
{
    return guarded([&] { return kvx_chol_factorize_async_dev_impl(F, values_dev); });
}

int kvx_chol_status(kvx_chol *F, int64_t *minor)
{
    if (!F) return KVX_EINVAL;
    return finish_factor(F, minor);
}

int kvx_chol_factorize_dev(kvx_chol *F, const double *values_dev, int64_t *minor)
{
    int rc = kvx_chol_factorize_async_dev(F, values_dev);
    if (rc) return rc;
    return finish_factor(F, minor);
}

static int kvx_chol_factorize_impl(kvx_chol *F, const double *values, int64_t *minor)
{
    if (!F) return KVX_EINVAL;
    int rc = ensure_device(F);
    if (rc) return rc;
    if (F->S.nnzA > 0)
        HIPCHK(hipMemcpyAsync(F->d_Ax, values, F->S.nnzA * sizeof(double), hipMemcpyHostToDevice, F->stream));
    rc = enqueue_factor(F);
    if (rc) return rc;
    return finish_factor(F, minor);
}

int kvx_chol_factorize(kvx_chol *F, const double *values, int64_t *minor)
{
    return guarded([&] { return kvx_chol_factorize_impl(F, values, minor); });
}

static int kvx_chol_solve_dev_impl(kvx_chol *F, int sys, double *B_dev, int64_t nrhs, int64_t ldB)
{
    if (!F) return KVX_EINVAL;
    if (!F->dev_ready) { set_err("called with symbolic factor"); return KVX_ESYMBOLIC; }
    int rc = wait_for_caller(F);
    if (rc) return rc;
    return solve_dev(F, sys, B_dev, nrhs, ldB);
}

int kvx_chol_solve_dev(kvx_chol *F, int sys, double *B_dev, int64_t nrhs, int64_t ldB)
{
    return guarded([&] { return kvx_chol_solve_dev_impl(F, sys, B_dev, nrhs, ldB); });
}

static int kvx_chol_solve_async_dev_impl(kvx_chol *F, int sys, double *B_dev, int64_t nrhs, int64_t ldB)
{
    if (!F) return KVX_EINVAL;
    if (!F->dev_ready) { set_err("called with symbolic factor"); return KVX_ESYMBOLIC; }
    int rc = wait_for_caller(F);
    if (rc) return rc;
    return solve_dev(F, sys, B_dev, nrhs, ldB, true);
}

int kvx_chol_solve_async_dev(kvx_chol *F, int sys, double *B_dev, int64_t nrhs, int64_t ldB)
{
    return guarded([&] { return kvx_chol_solve_async_dev_impl(F, sys, B_dev, nrhs, ldB); });
}

int kvx_chol_factorize_solve_async_dev(kvx_chol *F, const double *values_dev, double *B_dev, int64_t nrhs, int64_t ldB)
{
    return guarded([&] {
        if (!F) return (int)KVX_EINVAL;
        return factor_solve_dev(F, values_dev, B_dev, nrhs, ldB, true);
    });
}

int kvx_chol_factorize_solve_dev(kvx_chol *F, const double *values_dev, double *B_dev, int64_t nrhs, int64_t ldB, int64_t *minor)
{
    return guarded([&] {
        if (!F) return (int)KVX_EINVAL;
        int rc = factor_solve_dev(F, values_dev, B_dev, nrhs, ldB);
        if (minor) *minor = F->minor;
        return rc;
    });
}

static int kvx_chol_solve_impl(kvx_chol *F, int sys, double *B, int64_t nrhs, int64_t ldB)
{
    if (!F) return KVX_EINVAL;
    if (!F->dev_ready) { set_err("called with symbolic factor"); return KVX_ESYMBOLIC; }
    const int64_t n = F->S.n;
    if (sys < 0 || sys > 8) { set_err("invalid value for sys"); return KVX_EINVAL; }
    int rc = finish_factor(F, nullptr);
    if (rc == KVX_ESYMBOLIC) { set_err("called with symbolic factor"); return rc; }
    if (rc == KVX_ENOTPOSDEF) { set_err("singular matrix"); return KVX_ESINGULAR; }
    if (n == 0 || nrhs == 0) return KVX_OK;
    if (ldB < std::max<int64_t>(1, n)) { set_err("ldB must be >= max(1,n)"); return KVX_EINVAL; }
    double *d_B = nullptr;
    HIPCHK(pool_malloc((void **)&d_B, n * nrhs * sizeof(double)));
    hipError_t e = hipMemcpy2D(d_B, n * sizeof(double), B, ldB * sizeof(double), n * sizeof(double), nrhs, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = solve_dev(F, sys, d_B, nrhs, n);
        if (rc == KVX_OK)
            e = hipMemcpy2D(B, ldB * sizeof(double), d_B, n * sizeof(double), n * sizeof(double), nrhs, hipMemcpyDeviceToHost);
    }
    (void)pool_free(d_B);
    if (e != hipSuccess) { set_err(hipGetErrorString(e)); return KVX_EDEVICE; }
    return rc;
}

int kvx_chol_solve(kvx_chol *F, int sys, double *B, int64_t nrhs, int64_t ldB)
{
    return guarded([&] { return kvx_chol_solve_impl(F, sys, B, nrhs, ldB); });
}

// numeric + solve (sys 0) with HOST buffers: what cholmod.linsolve does after its analysis (cholmod.c:663-753), as the one-enqueue
// form.  The staging block of B keeps its address from call to call (the captured graph reads and writes it).
static int kvx_chol_factorize_solve_impl(kvx_chol *F, const double *values, double *B, int64_t nrhs, int64_t ldB, int64_t *minor)
{
    if (!F) return KVX_EINVAL;
    int rc = ensure_device(F);
    if (rc) return rc;
    const int64_t n = F->S.n;
    if (nrhs < 0) { set_err("nrhs out of range"); return KVX_EINVAL; }
    if (n > 0 && nrhs > 0 && ldB < n) { set_err("ldB must be >= max(1,n)"); return KVX_EINVAL; }
    double *d_vals = nullptr, *d_B = nullptr;
    HIPCHK(pool_malloc((void **)&d_vals, std::max<int64_t>(F->S.nnzA, 1) * sizeof(double)));
    if (pool_malloc((void **)&d_B, std::max<int64_t>(n * nrhs, 1) * sizeof(double)) != hipSuccess) { (void)pool_free(d_vals); set_err("out of device memory"); return KVX_ENOMEM; }
    hipError_t e = hipSuccess;
    if (F->S.nnzA > 0) e = hipMemcpy(d_vals, values, F->S.nnzA * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && n > 0 && nrhs > 0)
        e = hipMemcpy2D(d_B, n * sizeof(double), B, ldB * sizeof(double), n * sizeof(double), nrhs, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = factor_solve_dev(F, d_vals, d_B, nrhs, n);
        if (minor) *minor = F->minor;
        if (rc == KVX_OK && n > 0 && nrhs > 0)
            e = hipMemcpy2D(B, ldB * sizeof(double), d_B, n * sizeof(double), n * sizeof(double), nrhs, hipMemcpyDeviceToHost);
    }
    (void)pool_free(d_vals);
    (void)pool_free(d_B);
    if (e != hipSuccess) { set_err(hipGetErrorString(e)); return KVX_EDEVICE; }
    return rc;
}

int kvx_chol_factorize_solve(kvx_chol *F, const double *values, double *B, int64_t nrhs, int64_t ldB, int64_t *minor)
{
    return guarded([&] { return kvx_chol_factorize_solve_impl(F, values, B, nrhs, ldB, minor); });
}

static int kvx_chol_spsolve_impl(kvx_chol *F, int sys, int64_t ncol, const int64_t *Bp, const int64_t *Bi, const double *Bx,
                     int64_t **Xp, int64_t **Xi, double **Xx)
{
    if (!F || !Xp || !Xi || !Xx || ncol < 0) return KVX_EINVAL;
    const int64_t n = F->S.n;
    if (sys < 0 || sys > 8) { set_err("invalid value for sys"); return KVX_EINVAL; }
    if (!F->dev_ready) { set_err("called with symbolic factor"); return KVX_ESYMBOLIC; }
    int rc = finish_factor(F, nullptr);
    if (rc == KVX_ESYMBOLIC) { set_err("called with symbolic factor"); return rc; }
    if (rc == KVX_ENOTPOSDEF) { set_err("singular matrix"); return KVX_ESINGULAR; }
    std::vector<int64_t> xp((size_t)ncol + 1, 0), xi;
    std::vector<double> xx;
    auto deliver = [&]() -> int {
        for (int64_t j = 0; j < ncol; j++) xp[j + 1] = std::max(xp[j + 1], xp[j]);
        *Xp = (int64_t *)malloc(sizeof(int64_t) * (ncol + 1));
        *Xi = (int64_t *)malloc(sizeof(int64_t) * std::max<size_t>(xi.size(), 1));
        *Xx = (double *)malloc(sizeof(double) * std::max<size_t>(xx.size(), 1));
        if (!*Xp || !*Xi || !*Xx) { free(*Xp); free(*Xi); free(*Xx); return KVX_ENOMEM; }
        memcpy(*Xp, xp.data(), sizeof(int64_t) * (ncol + 1));
        if (!xi.empty()) { memcpy(*Xi, xi.data(), sizeof(int64_t) * xi.size()); memcpy(*Xx, xx.data(), sizeof(double) * xx.size()); }
        return KVX_OK;
    };
    // forward systems: only the reach of the columns is swept (KVX_SPSOLVE_DENSE=1: the dense column blocks below, for comparison)
    if ((sys == 2 || sys == 4) && n > 0 && ncol > 0 && F->dist_nranks == 1 && !getenv("KVX_SPSOLVE_DENSE")) {
        if ((rc = wait_for_caller(F))) return rc;
        if ((rc = spsolve_forward_reach(F, sys, ncol, Bp, Bi, Bx, xp, xi, xx))) return rc;
        return deliver();
    }
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(ncol, (int64_t)(1 << 26) / std::max<int64_t>(n, 1)));
    std::vector<double> dense;
    for (int64_t c0 = 0; c0 < ncol && n > 0; c0 += chunk) {
        int64_t nc = std::min(chunk, ncol - c0);
        dense.assign((size_t)(n * nc), 0.0);
        for (int64_t j = 0; j < nc; j++)
            for (int64_t p = Bp[c0 + j]; p < Bp[c0 + j + 1]; p++) {
                if (Bi[p] < 0 || Bi[p] >= n) { set_err("row index out of range in B"); return KVX_EINVAL; }
                dense[(size_t)(Bi[p] + j * n)] += Bx[p];
            }
        rc = kvx_chol_solve(F, sys, dense.data(), nc, n);
        if (rc) return rc;
        for (int64_t j = 0; j < nc; j++) {
            for (int64_t i = 0; i < n; i++) {
                double v = dense[(size_t)(i + j * n)];
                if (v != 0.0) { xi.push_back(i); xx.push_back(v); }
            }
            xp[(size_t)(c0 + j + 1)] = (int64_t)xi.size();
        }
    }
    return deliver();
}

int kvx_chol_spsolve(kvx_chol *F, int sys, int64_t ncol, const int64_t *Bp, const int64_t *Bi, const double *Bx,
                     int64_t **Xp, int64_t **Xi, double **Xx)
{
    return guarded([&] { return kvx_chol_spsolve_impl(F, sys, ncol, Bp, Bi, Bx, Xp, Xi, Xx); });
}

int kvx_chol_diag(kvx_chol *F, double *d)
{
    if (!F || !d) return KVX_EINVAL;
    if (!F->part.empty()) { set_err("diag: this rank holds only its own fronts of a sharded factor"); return KVX_EINVAL; }
    if (!F->dev_ready || !F->is_ll) { set_err("F must be a nonsingular supernodal Cholesky factor"); return KVX_ESYMBOLIC; }
    int rc = finish_factor(F, nullptr);
    if (rc == KVX_ENOTPOSDEF) { set_err("F must be a nonsingular supernodal Cholesky factor"); return KVX_ESINGULAR; }
    if (rc) return rc;
    if (F->S.n == 0) return KVX_OK;
    double *dd = nullptr;
    HIPCHK(pool_malloc((void **)&dd, F->S.n * sizeof(double)));
    launch_extract_diag(F->stream, F->ds, F->S.nsuper, F->d_Lx, dd);
    hipError_t e = hipStreamSynchronize(F->stream);
    if (e == hipSuccess) e = hipMemcpy(d, dd, F->S.n * sizeof(double), hipMemcpyDeviceToHost);
    (void)pool_free(dd);
    if (e != hipSuccess) { set_err(hipGetErrorString(e)); return KVX_EDEVICE; }
    return KVX_OK;
}

static int kvx_chol_get_factor_impl(kvx_chol *F, int64_t *lnz, int64_t *Lp, int64_t *Li, double *Lx)
{
    if (!F) return KVX_EINVAL;
    if (!F->part.empty()) { set_err("getfactor: this rank holds only its own fronts of a sharded factor"); return KVX_EINVAL; }
    Symbolic &S = F->S;
    // structural entries of the supernodal factor: lower trapezoid of every panel
    int64_t cnt = 0;
    for (int64_t s = 0; s < S.nsuper; s++) {
        int64_t k = S.sn_k[s], m = S.sn_m[s];
        cnt += k * m - k * (k - 1) / 2;
    }
    if (lnz) *lnz = cnt;
    if (!Lp && !Li && !Lx) return KVX_OK;
    if (!F->dev_ready) { set_err("F must be a numeric Cholesky factor"); return KVX_ESYMBOLIC; }
    int rc = finish_factor(F, nullptr);
    if (rc == KVX_ESYMBOLIC) { set_err("F must be a numeric Cholesky factor"); return rc; }
    std::vector<double> host((size_t)std::max<int64_t>(S.lsize, 1));
    if (S.lsize > 0) HIPCHK(hipMemcpy(host.data(), F->d_Lx, S.lsize * sizeof(double), hipMemcpyDeviceToHost));
    int64_t q = 0;
    for (int64_t s = 0; s < S.nsuper; s++) {
        int64_t k = S.sn_k[s], m = S.sn_m[s], f = S.super[s];
        const int32_t *rows = S.rowidx.data() + S.rowptr[s];
        for (int64_t j = 0; j < k; j++) {
            if (Lp) Lp[f + j] = q;
            // LDL' form (as cholmod_factor_to_sparse returns it): D on the diagonal, the unit diagonal of L implicit
            const double dj = host[(size_t)(S.px[s] + j + j * m)];
            for (int64_t i = j; i < m; i++) {
                if (Li) Li[q] = rows[i];
                if (Lx) {
                    const double v = host[(size_t)(S.px[s] + i + j * m)];
                    Lx[q] = F->is_ll ? v : (i == j ? v * v : v / dj);
                }
                q++;
            }
        }
    }
    if (Lp) Lp[S.n] = q;
    return KVX_OK;
}

int kvx_chol_get_factor(kvx_chol *F, int64_t *lnz, int64_t *Lp, int64_t *Li, double *Lx)
{
    return guarded([&] { return kvx_chol_get_factor_impl(F, lnz, Lp, Li, Lx); });
}

int kvx_chol_get_info(kvx_chol *F, kvx_chol_info *info)
{
    if (!F || !info) return KVX_EINVAL;
    memset(info, 0, sizeof(*info));
    Symbolic &S = F->S;
    info->n = S.n;
    info->nnz_a = S.nnzTri;
    info->lnz = S.lnz;
    info->flops = S.flops;
    info->nsuper = S.nsuper;
    info->lsize = F->lsize_total >= 0 ? F->lsize_total : S.lsize;
    info->dev_bytes = F->dev_bytes;                   // bytes of the large device buffers this handle holds (0 before the first device use)
    info->lsize_local = S.lsize;                      // panel doubles resident on THIS rank (= lsize unless the sharded layout was trimmed)
    info->nlevels = S.nlevels;
    info->max_front = S.max_m;
    info->upd_size = S.upd_size[0] + S.upd_size[1];
    info->is_numeric = (F->numeric && !F->pending) ? 1 : 0;
    info->minor = F->minor;
    info->solve_rowidx = S.sum_m;
    info->is_ll = F->is_ll ? 1 : 0;
    subtree_counts(F, info->reserved);
    return KVX_OK;
}

int kvx_chol_get_perm(kvx_chol *F, int64_t *perm)
{
    if (!F || (!perm && F->S.n > 0)) return KVX_EINVAL;
    if (F->S.n > 0) memcpy(perm, F->S.perm.data(), sizeof(int64_t) * F->S.n);
    return KVX_OK;
}

static int kvx_chol_get_supernodes_impl(kvx_chol *F, int64_t *super, int64_t *nrows, int64_t *parent, int64_t *level)
{
    if (!F) return KVX_EINVAL;
    Symbolic &S = F->S;
    if (super) memcpy(super, S.super.data(), sizeof(int64_t) * (S.nsuper + 1));
    for (int64_t s = 0; s < S.nsuper; s++) {
        if (nrows) nrows[s] = S.sn_m[s];
        if (parent) parent[s] = S.sparent[s];
        if (level) level[s] = S.depth[s];
    }
    return KVX_OK;
}

int kvx_chol_get_supernodes(kvx_chol *F, int64_t *super, int64_t *nrows, int64_t *parent, int64_t *level)
{
    return guarded([&] { return kvx_chol_get_supernodes_impl(F, super, nrows, parent, level); });
}

int kvx_chol_get_front_rows(kvx_chol *F, int64_t *rowptr, int64_t *rowidx)
{
    if (!F || !rowptr) return KVX_EINVAL;
    const Symbolic &S = F->S;
    std::copy(S.rowptr.begin(), S.rowptr.end(), rowptr);
    if (rowidx) std::copy(S.rowidx.begin(), S.rowidx.end(), rowidx);
    return KVX_OK;
}

int kvx_chol_last_timing(kvx_chol *F, double *ms_factor, double *ms_solve)
{
    if (!F) return KVX_EINVAL;
    if (F->pending) finish_factor(F, nullptr);
    if (ms_factor) *ms_factor = F->have_ftime ? F->ms_factor : -1.0;
    if (ms_solve) *ms_solve = F->have_stime ? F->ms_solve : -1.0;
    return KVX_OK;
}

int kvx_chol_last_fused_path(kvx_chol *F) { return F ? F->last_fused_path : 0; }

int kvx_chol_prof_select(kvx_chol *F, int family)
{
    if (!F || family < -1 || family > 8) return KVX_EINVAL;
    if (F->pending) finish_factor(F, nullptr);
    F->prof_family = family;
    F->prof_ms = 0;
    F->prof_launches = 0;
    F->prof_used = 0;
    return KVX_OK;
}

int kvx_chol_prof_read(kvx_chol *F, double *total_ms, int64_t *launches)
{
    if (!F) return KVX_EINVAL;
    if (F->pending) finish_factor(F, nullptr);
    if (total_ms) *total_ms = F->prof_ms;
    if (launches) *launches = F->prof_launches;
    return KVX_OK;
}

void kvx_chol_free(kvx_chol *F)
{
    if (!F) return;
    const bool tim = getenv("KVX_FREE_TIMING") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto t0 = now();
    auto lap = [&](const char *what) { if (tim) { auto t1 = now(); fprintf(stderr, "  free %-10s %.2f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count()); t0 = t1; } };
    {                                              // (also after a device set-up that failed half way: every member starts out null)
        if (F->stream) (void)hipStreamSynchronize(F->stream);
        lap("sync");
        void *ptrs[] = {F->d_k, F->d_m, F->d_first, F->d_rowidx, F->d_rel, F->d_children, F->d_perm, F->d_lists,
                        F->d_px, F->d_rowptr, F->d_ux, F->d_wx, F->d_childptr, F->d_amap, F->d_sdst, F->d_ssrc, F->d_scptr, F->d_Lx, F->d_U[0], F->d_U[1],
                        F->d_Ax, F->d_X, F->d_X0, F->d_diag, F->d_W[0], F->d_W[1], F->d_status, F->d_WK, F->d_Linv, F->d_linv_off, F->d_fd, F->d_cd, F->d_tiles};
        for (void *p : ptrs)
            if (p) (void)pool_free(p);
        lap("buffers");
        if (F->h_status) (void)hipHostFree(F->h_status);
        lap("hostfree");
        for (int i = 0; i < 4; i++)
            if (F->ev[i]) pool_event_put(F->ev[i], true);
        destroy_graphs(F);
        lap("graphs");
        for (hipEvent_t e : F->prof_ev)
            if (e) pool_event_put(e, true);
        for (int i = 0; i < 3; i++) {
            if (F->side[i]) pool_stream_put(F->side[i]);
            if (F->ev_join[i]) pool_event_put(F->ev_join[i], false);
        }
        if (F->d_iperm) (void)pool_free(F->d_iperm);
        if (F->d_inv_ptr) (void)pool_free(F->d_inv_ptr);
        if (F->d_inv_src) (void)pool_free(F->d_inv_src);
        if (F->d_keep) (void)pool_free(F->d_keep);
        if (F->d_flists) (void)pool_free(F->d_flists);
        if (F->d_chain) (void)pool_free(F->d_chain);
        dist_release(F);
        for (void *p : {(void *)F->d_subs, (void *)F->d_subs_f, (void *)F->d_subs_lvl, (void *)F->d_cd_woff, (void *)F->d_lists_sw, (void *)F->d_depth})
            if (p) (void)pool_free(p);
        if (F->ev_fork) pool_event_put(F->ev_fork, false);
        for (hipEvent_t e : F->ev_u)
            if (e) pool_event_put(e, false);
        if (F->ev_ujoin) pool_event_put(F->ev_ujoin, false);
        for (hipEvent_t e : F->ev_lvl)
            if (e) pool_event_put(e, false);
        for (int i = 0; i < 4; i++)
            if (F->ev_pipe[i]) pool_event_put(F->ev_pipe[i], false);
        if (F->ev_in) pool_event_put(F->ev_in, false);
        if (F->ev_out) pool_event_put(F->ev_out, false);
        if (F->stream) pool_stream_put(F->stream);
        lap("streams");
    }
    delete F;
    lap("delete");
}

void kvx_free(void *p) { free(p); }

int kvx_dev_malloc(void **p, int64_t bytes) { HIPCHK(pool_malloc(p, (size_t)std::max<int64_t>(bytes, 1))); return KVX_OK; }
int kvx_dev_free(void *p) { HIPCHK(pool_free(p)); return KVX_OK; }
int kvx_dev_upload(void *dst, const void *src, int64_t bytes) { if (bytes > 0) HIPCHK(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyHostToDevice)); return KVX_OK; }
int kvx_dev_download(void *dst, const void *src, int64_t bytes) { if (bytes > 0) HIPCHK(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost)); return KVX_OK; }
int kvx_dev_sync(void) { HIPCHK(hipDeviceSynchronize()); return KVX_OK; }
int kvx_dev_trim(void) { pool_release_all(); return KVX_OK; }
int kvx_dev_mem_info(int64_t *free_bytes, int64_t *total_bytes)
{
    size_t f = 0, t = 0;
    HIPCHK(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = (int64_t)f;
    if (total_bytes) *total_bytes = (int64_t)t;
    return KVX_OK;
}

}  // extern "C"
