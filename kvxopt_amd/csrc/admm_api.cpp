// C-ABI entry points of the ADMM solver behind kvxopt.osqp (include/kvxhip.h, kvx_admm_*): minimise 1/2 x'Px + q'x subject to
// l <= Ax <= u by the iteration of OSQP (Stellato et al. 2020) on one kept Cholesky factor of
//
//     S = P + sigma I + A' diag(rho) A.
//
// The plan (host only) equilibrates the data (Ruiz passes on the KKT matrix [[P, A'], [A, 0]] and the cost scaling), keeps the
// scaled A by columns and by rows, the scaled P as its lower triangle (for S) and in full (for P x), builds the kvx_atda plan of
// A with the pattern tril(P) U I -- sigma has a slot in every column -- and analyses that pattern once.  Everything after the
// plan runs in HBM: kvx_admm_iterate issues k x {k_admm_rhs, kvx_chol_solve_async_dev, k_admm_update} back to back, then the
// residual kernels, and reads 24 doubles.  No CPU fallback: without a HIP device the device entry points return KVX_EDEVICE.
//
// A handle can be kept across solves: kvx_admm_update replaces q, l, u (rescaled with the kept D, E, c; one refactorisation only
// when a row changes its rho class), kvx_admm_warm_start / kvx_admm_cold_start set the state, and kvx_admm_polish solves the
// equality-constrained QP of the guessed active set on S_pol = P + delta I + A' diag(w) A -- the analysed pattern, the same
// kvx_chol, whose numeric factor it takes over: the handle marks the ADMM factor stale and the next iteration rebuilds it.
//
// A batch (kvx_admm_batch_*, admm_batch.hip) runs B data sets (q_b, l_b, u_b) through that one factor: buffers of its own,
// column-major, one triangular solve with B right-hand sides per iteration, one host read of B x 24 numbers per check.  The kept
// problem's data, state, rho and factor are not touched (a stale factor is rebuilt once, as kvx_admm_iterate does).
#include "../../include/kvxhip.h"
#include "abi_guard.hpp"
#include "admm.hpp"
#include "admm_batch.hpp"
#include "admm_polish.hpp"
#include "devpool.hpp"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

using namespace kvx;

#define HIPCHK(call)                                                             \
    do {                                                                         \
        hipError_t e_ = (call);                                                  \
        if (e_ != hipSuccess) return KVX_EDEVICE;                                \
    } while (0)

namespace {
constexpr double OSQP_INFTY = 1e30, MIN_SCALING = 1e-4, MAX_SCALING = 1e4;
constexpr double RHO_MIN = 1e-6, RHO_MAX = 1e6, RHO_TOL = 1e-4, RHO_EQ_OVER_RHO_INEQ = 1e3;

inline double limit_scaling(double v) { return v < MIN_SCALING ? 1.0 : (v > MAX_SCALING ? MAX_SCALING : v); }
}  // namespace

struct kvx_admm {
    int64_t m = 0, n = 0, snz = 0, nfact = 0, niter = 0;
    std::vector<int64_t> Ap, Ai, Tp, Ti, Lp, Li, Fp, Fi, rs, rl, Sp, Si;
    std::vector<double> Ax, Tx, Lx, Fx, q, l, u, D, Dinv, E, Einv, rho;
    double c = 1.0, sigma = 0.0, alpha = 0.0, rho0 = 0.0;
    kvx_atda *plan = nullptr;
    kvx_chol *F = nullptr;
    bool dev = false;
    AdmmDev d{};
    double *d_Lxs = nullptr, *d_Sx = nullptr, *d_part = nullptr, *d_res = nullptr;
    std::vector<void *> owned;
    // the kept problem (admm_polish.hip): staging for raw q | x (n), l | y (m), u (m); the polish buffers, allocated at first use
    bool stale = false;                 // the kept numeric factor is that of S_pol, not of S
    bool polished = false;              // xh, zh, yh hold the result of a polish that factored
    PolishDev p{};
    double *d_stage = nullptr, *d_ppart = nullptr, *d_pres = nullptr, *d_Lxd = nullptr;
    double lxd_delta = 0.0;
    // a batch on the kept factor (admm_batch.hip): B members, buffers from kvx_admm_batch_begin (they are in `owned` as well)
    AdmmBatchDev b{};
    std::vector<void *> bowned;
    int *d_run = nullptr;
    double *d_bpart = nullptr, *d_bres = nullptr;
};

namespace {

template <class T>
int up(kvx_admm *S, const T **dst, const std::vector<T> &src)
{
    T *p = nullptr;
    HIPCHK(pool_malloc((void **)&p, std::max<size_t>(src.size(), 1) * sizeof(T)));
    S->owned.push_back(p);
    if (!src.empty()) HIPCHK(hipMemcpy(p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    *dst = p;
    return KVX_OK;
}

int zeros(kvx_admm *S, double **dst, int64_t count)
{
    const size_t bytes = (size_t)std::max<int64_t>(count, 1) * sizeof(double);
    HIPCHK(pool_malloc((void **)dst, bytes));
    S->owned.push_back(*dst);
    HIPCHK(hipMemset(*dst, 0, bytes));
    return KVX_OK;
}

bool have_device(const char *who)
{
    int nd = 0;
    if (hipGetDeviceCount(&nd) == hipSuccess && nd > 0) return true;
    set_last_error(std::string(who) + ": no HIP device; the ADMM iteration has no CPU fallback");
    return false;
}

// rho_i = 1e3 rho on rows with u - l < 1e-4 (scaled bounds), 1e-6 on rows without a finite bound, rho elsewhere
void rho_vector(const kvx_admm *S, double rho, double *out)
{
    rho = std::min(std::max(rho, RHO_MIN), RHO_MAX);
    for (int64_t i = 0; i < S->m; i++) {
        const double l = S->l[i], u = S->u[i];
        if (l <= -OSQP_INFTY * MIN_SCALING && u >= OSQP_INFTY * MIN_SCALING) out[i] = RHO_MIN;
        else if (u - l < RHO_TOL) out[i] = RHO_EQ_OVER_RHO_INEQ * rho;
        else out[i] = rho;
    }
}

int plan_impl(int64_t m, int64_t n, const int64_t *Ap, const int64_t *Ai, const double *Ax, const int64_t *Pp, const int64_t *Pi,
              const double *Px, const double *q, const double *l, const double *u, int64_t scaling, double *D_out, double *E_out,
              double *c_out, int64_t *snz_out, kvx_admm **out)
{
    if (!out) return KVX_EINVAL;
    *out = nullptr;
    if (m < 1 || n < 1 || !Ap || !q || !l || !u || scaling < 0) { set_last_error("kvx_admm_plan: bad argument"); return KVX_EINVAL; }
    if (Ap[0] != 0) return KVX_EINVAL;
    for (int64_t j = 0; j < n; j++)
        if (Ap[j + 1] < Ap[j]) return KVX_EINVAL;
    const int64_t anz = Ap[n];
    if (anz > 0 && (!Ai || !Ax)) return KVX_EINVAL;
    for (int64_t e = 0; e < anz; e++)
        if (Ai[e] < 0 || Ai[e] >= m) { set_last_error("kvx_admm_plan: row index of A out of range"); return KVX_EINVAL; }
    if (Pp) {
        if (Pp[0] != 0) return KVX_EINVAL;
        for (int64_t j = 0; j < n; j++)
            if (Pp[j + 1] < Pp[j]) return KVX_EINVAL;
        if (Pp[n] > 0 && (!Pi || !Px)) return KVX_EINVAL;
        for (int64_t e = 0; e < Pp[n]; e++)
            if (Pi[e] < 0 || Pi[e] >= n) { set_last_error("kvx_admm_plan: row index of P out of range"); return KVX_EINVAL; }
    }
    for (int64_t i = 0; i < m; i++)
        if (!(l[i] <= u[i])) { set_last_error("kvx_admm_plan: l <= u does not hold"); return KVX_EINVAL; }
    std::unique_ptr<kvx_admm, void (*)(kvx_admm *)> hold(new kvx_admm(), kvx_admm_free);
    kvx_admm *S = hold.get();
    S->m = m; S->n = n;
    S->Ap.assign(Ap, Ap + n + 1); S->Ai.assign(Ai, Ai + anz); S->Ax.assign(Ax, Ax + anz);
    S->q.assign(q, q + n);
    // tril(P) U I with rows ascending in every column; an entry stored twice is refused
    S->Lp.assign((size_t)n + 1, 0);
    {
        std::vector<std::pair<int64_t, double>> col;
        for (int64_t j = 0; j < n; j++) {
            col.clear();
            col.emplace_back(j, 0.0);
            bool diag = false;
            for (int64_t e = Pp ? Pp[j] : 0; e < (Pp ? Pp[j + 1] : 0); e++) {
                if (Pi[e] == j) {
                    if (diag) { set_last_error("kvx_admm_plan: the pattern of P holds an entry twice"); return KVX_EINVAL; }
                    diag = true;
                    col[0].second = Px[e];
                } else if (Pi[e] > j) {
                    col.emplace_back(Pi[e], Px[e]);
                }
            }
            std::sort(col.begin() + 1, col.end(), [](const std::pair<int64_t, double> &a, const std::pair<int64_t, double> &b) { return a.first < b.first; });
            for (size_t t = 0; t < col.size(); t++) {
                if (t > 1 && col[t].first == col[t - 1].first) { set_last_error("kvx_admm_plan: the pattern of P holds an entry twice"); return KVX_EINVAL; }
                S->Li.push_back(col[t].first);
                S->Lx.push_back(col[t].second);
            }
            S->Lp[j + 1] = (int64_t)S->Li.size();
        }
    }
    const int64_t lnz = S->Lp[n];
    // ---- equilibration: D, E, c
    S->D.assign((size_t)n, 1.0); S->E.assign((size_t)m, 1.0); S->c = 1.0;
    std::vector<double> dn((size_t)n), en((size_t)m);
    for (int64_t pass = 0; pass < scaling; pass++) {
        std::fill(dn.begin(), dn.end(), 0.0);
        std::fill(en.begin(), en.end(), 0.0);
        for (int64_t j = 0; j < n; j++) {                               // column norms of [[P, A'], [A, 0]]
            for (int64_t e = S->Lp[j]; e < S->Lp[j + 1]; e++) {
                const double a = std::fabs(S->Lx[e]);
                dn[j] = std::max(dn[j], a);
                dn[S->Li[e]] = std::max(dn[S->Li[e]], a);
            }
            for (int64_t e = S->Ap[j]; e < S->Ap[j + 1]; e++) {
                const double a = std::fabs(S->Ax[e]);
                dn[j] = std::max(dn[j], a);
                en[S->Ai[e]] = std::max(en[S->Ai[e]], a);
            }
        }
        for (int64_t j = 0; j < n; j++) dn[j] = 1.0 / std::sqrt(limit_scaling(dn[j]));
        for (int64_t i = 0; i < m; i++) en[i] = 1.0 / std::sqrt(limit_scaling(en[i]));
        for (int64_t j = 0; j < n; j++) {
            for (int64_t e = S->Lp[j]; e < S->Lp[j + 1]; e++) S->Lx[e] = (dn[S->Li[e]] * S->Lx[e]) * dn[j];
            for (int64_t e = S->Ap[j]; e < S->Ap[j + 1]; e++) S->Ax[e] = (en[S->Ai[e]] * S->Ax[e]) * dn[j];
            S->q[j] *= dn[j];
            S->D[j] *= dn[j];
        }
        for (int64_t i = 0; i < m; i++) S->E[i] *= en[i];
        // cost scaling: 1 / max(mean column norm of P, |q|_inf), both limited as the norms above
        std::fill(dn.begin(), dn.end(), 0.0);
        for (int64_t j = 0; j < n; j++)
            for (int64_t e = S->Lp[j]; e < S->Lp[j + 1]; e++) {
                const double a = std::fabs(S->Lx[e]);
                dn[j] = std::max(dn[j], a);
                dn[S->Li[e]] = std::max(dn[S->Li[e]], a);
            }
        double sum = 0.0, qn = 0.0;
        for (int64_t j = 0; j < n; j++) { sum += dn[j]; qn = std::max(qn, std::fabs(S->q[j])); }
        const double g = 1.0 / limit_scaling(std::max(sum / (double)n, limit_scaling(qn)));
        for (int64_t e = 0; e < lnz; e++) S->Lx[e] *= g;
        for (int64_t j = 0; j < n; j++) S->q[j] *= g;
        S->c *= g;
    }
    S->Dinv.resize((size_t)n); S->Einv.resize((size_t)m);
    for (int64_t j = 0; j < n; j++) S->Dinv[j] = 1.0 / S->D[j];
    for (int64_t i = 0; i < m; i++) S->Einv[i] = 1.0 / S->E[i];
    S->l.resize((size_t)m); S->u.resize((size_t)m);
    for (int64_t i = 0; i < m; i++) {
        S->l[i] = l[i] <= -OSQP_INFTY * MIN_SCALING ? -OSQP_INFTY : S->E[i] * l[i];
        S->u[i] = u[i] >= OSQP_INFTY * MIN_SCALING ? OSQP_INFTY : S->E[i] * u[i];
    }
    // ---- A by rows (columns ascending inside a row), the two row classes
    S->Tp.assign((size_t)m + 1, 0);
    for (int64_t e = 0; e < anz; e++) S->Tp[S->Ai[e] + 1]++;
    for (int64_t i = 0; i < m; i++) S->Tp[i + 1] += S->Tp[i];
    S->Ti.resize((size_t)anz); S->Tx.resize((size_t)anz);
    {
        std::vector<int64_t> fill(S->Tp.begin(), S->Tp.end() - 1);
        for (int64_t j = 0; j < n; j++)
            for (int64_t e = S->Ap[j]; e < S->Ap[j + 1]; e++) {
                const int64_t t = fill[S->Ai[e]]++;
                S->Ti[t] = j;
                S->Tx[t] = S->Ax[e];
            }
    }
    for (int64_t i = 0; i < m; i++) (S->Tp[i + 1] - S->Tp[i] >= ADMM_ROW_WAVE ? S->rl : S->rs).push_back(i);
    // ---- the full symmetric P by columns (rows ascending): column j = row j of the strict lower triangle, then column j of it
    S->Fp.assign((size_t)n + 1, 0);
    for (int64_t j = 0; j < n; j++)
        for (int64_t e = S->Lp[j]; e < S->Lp[j + 1]; e++) {
            S->Fp[j + 1]++;
            if (S->Li[e] != j) S->Fp[S->Li[e] + 1]++;
        }
    for (int64_t j = 0; j < n; j++) S->Fp[j + 1] += S->Fp[j];
    S->Fi.resize((size_t)S->Fp[n]); S->Fx.resize((size_t)S->Fp[n]);
    {
        std::vector<int64_t> fill(S->Fp.begin(), S->Fp.end() - 1);
        for (int64_t j = 0; j < n; j++)                                  // the entries (i, j), i > j, seen as (j, i): ascending j in column i
            for (int64_t e = S->Lp[j]; e < S->Lp[j + 1]; e++)
                if (S->Li[e] != j) { const int64_t t = fill[S->Li[e]]++; S->Fi[t] = j; S->Fx[t] = S->Lx[e]; }
        for (int64_t j = 0; j < n; j++)
            for (int64_t e = S->Lp[j]; e < S->Lp[j + 1]; e++) { const int64_t t = fill[j]++; S->Fi[t] = S->Li[e]; S->Fx[t] = S->Lx[e]; }
    }
    // ---- S on a fixed pattern, analysed once
    int rc = kvx_atda_plan(m, n, S->Ap.data(), S->Ai.data(), S->Lp.data(), S->Li.data(), &S->plan);
    if (rc) return rc;
    if ((rc = kvx_atda_pattern(S->plan, &S->snz, nullptr, nullptr))) return rc;
    S->Sp.resize((size_t)n + 1); S->Si.resize((size_t)S->snz);
    if ((rc = kvx_atda_pattern(S->plan, nullptr, S->Sp.data(), S->Si.data()))) return rc;
    if ((rc = kvx_chol_analyze(n, S->Sp.data(), S->Si.data(), 'L', nullptr, nullptr, &S->F))) return rc;
    if (D_out) std::copy(S->D.begin(), S->D.end(), D_out);
    if (E_out) std::copy(S->E.begin(), S->E.end(), E_out);
    if (c_out) *c_out = S->c;
    if (snz_out) *snz_out = S->snz;
    *out = hold.release();
    return KVX_OK;
}

// rho vector to the device, S assembled on its pattern and factored
int refactor(kvx_admm *S, double rho)
{
    S->rho0 = std::min(std::max(rho, RHO_MIN), RHO_MAX);
    S->rho.resize((size_t)S->m);
    rho_vector(S, rho, S->rho.data());
    HIPCHK(hipMemcpy(const_cast<double *>(S->d.rho), S->rho.data(), (size_t)S->m * sizeof(double), hipMemcpyHostToDevice));
    int rc = kvx_atda_assemble_dev(S->plan, S->d.Ax, S->d.rho, S->d_Lxs, S->d_Sx);
    if (rc) return rc;
    int64_t minor = 0;
    rc = kvx_chol_factorize_dev(S->F, S->d_Sx, &minor);
    if (rc == KVX_ENOTPOSDEF) set_last_error("kvx_admm: P + sigma I + A' diag(rho) A is not positive definite: the problem is not convex");
    if (rc) return rc;
    S->nfact++;
    S->stale = false;
    return KVX_OK;
}

int setup_impl(kvx_admm *S, double sigma, double rho, double alpha)
{
    if (!S) return KVX_EINVAL;
    if (!(sigma > 0.0) || !(rho > 0.0) || !(alpha > 0.0 && alpha < 2.0)) {
        set_last_error("kvx_admm_setup_dev: sigma > 0, rho > 0 and 0 < alpha < 2 are required");
        return KVX_EINVAL;
    }
    if (!have_device("kvx_admm_setup_dev")) return KVX_EDEVICE;
    if (S->dev) { set_last_error("kvx_admm_setup_dev: called twice"); return KVX_EINVAL; }
    AdmmDev &d = S->d;
    d.m = S->m; d.n = S->n; d.ns = (int64_t)S->rs.size(); d.nl = (int64_t)S->rl.size();
    d.sigma = S->sigma = sigma; d.alpha = S->alpha = alpha; d.cinv = 1.0 / S->c;
    int rc = 0;
#define UP(dst, src) if ((rc = up(S, &d.dst, S->src))) return rc
    UP(Ap, Ap); UP(Ai, Ai); UP(Ax, Ax); UP(Tp, Tp); UP(Ti, Ti); UP(Tx, Tx); UP(Fp, Fp); UP(Fi, Fi); UP(Fx, Fx); UP(rs, rs); UP(rl, rl);
    UP(q, q); UP(l, l); UP(u, u); UP(D, D); UP(Dinv, Dinv); UP(E, E); UP(Einv, Einv);
#undef UP
    double *rho_dev = nullptr;
    if ((rc = zeros(S, &rho_dev, S->m))) return rc;
    d.rho = rho_dev;
    if ((rc = zeros(S, &d.x, S->n)) || (rc = zeros(S, &d.z, S->m)) || (rc = zeros(S, &d.y, S->m)) || (rc = zeros(S, &d.dx, S->n)) ||
        (rc = zeros(S, &d.dy, S->m)) || (rc = zeros(S, &d.xt, S->n)) || (rc = zeros(S, &S->d_Sx, S->snz)) ||
        (rc = zeros(S, &S->d_part, ADMM_NRES * admm_residual_blocks(d))) || (rc = zeros(S, &S->d_res, ADMM_NRES)))
        return rc;
    std::vector<double> lxs(S->Lx);                                     // tril(P) + sigma I on the pattern the plan was given
    for (int64_t j = 0; j < S->n; j++) lxs[S->Lp[j]] += sigma;
    const double *p = nullptr;
    if ((rc = up(S, &p, lxs))) return rc;
    S->d_Lxs = const_cast<double *>(p);
    S->dev = true;
    return refactor(S, rho);
}

int iterate_impl(kvx_admm *S, int64_t k, double *out)
{
    if (!S || k < 0 || !out) return KVX_EINVAL;
    if (!have_device("kvx_admm_iterate")) return KVX_EDEVICE;
    if (!S->dev) { set_last_error("kvx_admm_iterate: kvx_admm_setup_dev has not run"); return KVX_EINVAL; }
    const int64_t ld = std::max<int64_t>(1, S->n);
    if (S->stale && k > 0) {                                            // a polish took the factor over: S at the current rho again
        const int rc = refactor(S, S->rho0);
        if (rc) return rc;
    }
    for (int64_t it = 0; it < k; it++) {
        launch_admm_rhs(nullptr, S->d);
        const int rc = kvx_chol_solve_async_dev(S->F, 0, S->d.xt, 1, ld);
        if (rc) return rc;
        launch_admm_update(nullptr, S->d);
    }
    S->niter += k;
    launch_admm_residuals(nullptr, S->d, S->d_part, S->d_res);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, S->d_res, ADMM_NRES * sizeof(double), hipMemcpyDeviceToHost));
    return KVX_OK;
}

int fetch(double *dst, const double *src_dev, int64_t count)
{
    if (dst && count > 0) HIPCHK(hipMemcpy(dst, src_dev, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
    return KVX_OK;
}

// ---- the kept problem: update, warm start, polish ---------------------------------------------------------------------------
inline int rho_class(double l, double u)                                 // the three classes of rho_vector: free, equality, other
{
    if (l <= -OSQP_INFTY * MIN_SCALING && u >= OSQP_INFTY * MIN_SCALING) return 0;
    return u - l < RHO_TOL ? 1 : 2;
}

int need_setup(kvx_admm *S, const char *who)
{
    if (!have_device(who)) return KVX_EDEVICE;
    if (!S->dev) { set_last_error(std::string(who) + ": kvx_admm_setup_dev has not run"); return KVX_EINVAL; }
    return KVX_OK;
}

int stage_buffer(kvx_admm *S)
{
    if (S->d_stage) return KVX_OK;
    return zeros(S, &S->d_stage, S->n + 2 * S->m);
}

int update_impl(kvx_admm *S, const double *q, const double *l, const double *u)
{
    if (!S) return KVX_EINVAL;
    const int64_t m = S->m, n = S->n;
    std::vector<double> ln, un;
    bool changed = false;
    if (l || u) {                                                       // the scaled bounds on the host too: they give the rho classes
        ln = S->l; un = S->u;
        for (int64_t i = 0; i < m; i++) {
            if (l) ln[i] = l[i] <= -OSQP_INFTY * MIN_SCALING ? -OSQP_INFTY : S->E[i] * l[i];
            if (u) un[i] = u[i] >= OSQP_INFTY * MIN_SCALING ? OSQP_INFTY : S->E[i] * u[i];
            if (!(ln[i] <= un[i])) { set_last_error("kvx_admm_update: l <= u does not hold"); return KVX_EINVAL; }
            changed = changed || rho_class(ln[i], un[i]) != rho_class(S->l[i], S->u[i]);
        }
    }
    int rc = need_setup(S, "kvx_admm_update");
    if (rc || (rc = stage_buffer(S))) return rc;
    double *sq = S->d_stage, *sl = S->d_stage + n, *su = S->d_stage + n + m;
    if (q) {
        HIPCHK(hipMemcpy(sq, q, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
        launch_admm_scale_q(nullptr, S->d, S->c, sq, const_cast<double *>(S->d.q));
        for (int64_t j = 0; j < n; j++) S->q[j] = (S->c * S->D[j]) * q[j];
    }
    if (l) {
        HIPCHK(hipMemcpy(sl, l, (size_t)m * sizeof(double), hipMemcpyHostToDevice));
        launch_admm_scale_bound(nullptr, S->d, false, sl, const_cast<double *>(S->d.l));
        S->l.swap(ln);
    }
    if (u) {
        HIPCHK(hipMemcpy(su, u, (size_t)m * sizeof(double), hipMemcpyHostToDevice));
        launch_admm_scale_bound(nullptr, S->d, true, su, const_cast<double *>(S->d.u));
        S->u.swap(un);
    }
    HIPCHK(hipGetLastError());
    S->polished = false;
    return changed ? refactor(S, S->rho0) : (int)KVX_OK;               // same pattern, same analysis
}

int warm_start_impl(kvx_admm *S, const double *x, const double *y)
{
    if (!S) return KVX_EINVAL;
    int rc = need_setup(S, "kvx_admm_warm_start");
    if (rc || (rc = stage_buffer(S))) return rc;
    const int64_t m = S->m, n = S->n;
    if (x) {
        HIPCHK(hipMemcpy(S->d_stage, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
        launch_admm_warm_x(nullptr, S->d, S->d_stage);
    }
    if (y) {
        HIPCHK(hipMemcpy(S->d_stage + n, y, (size_t)m * sizeof(double), hipMemcpyHostToDevice));
        launch_admm_warm_y(nullptr, S->d, S->c, S->d_stage + n);
    }
    HIPCHK(hipMemsetAsync(S->d.dx, 0, (size_t)n * sizeof(double), nullptr));
    HIPCHK(hipMemsetAsync(S->d.dy, 0, (size_t)m * sizeof(double), nullptr));
    HIPCHK(hipGetLastError());
    return KVX_OK;
}

int cold_start_impl(kvx_admm *S)
{
    if (!S) return KVX_EINVAL;
    const int rc = need_setup(S, "kvx_admm_cold_start");
    if (rc) return rc;
    const size_t nb = (size_t)S->n * sizeof(double), mb = (size_t)S->m * sizeof(double);
    HIPCHK(hipMemsetAsync(S->d.x, 0, nb, nullptr));
    HIPCHK(hipMemsetAsync(S->d.dx, 0, nb, nullptr));
    HIPCHK(hipMemsetAsync(S->d.z, 0, mb, nullptr));
    HIPCHK(hipMemsetAsync(S->d.y, 0, mb, nullptr));
    HIPCHK(hipMemsetAsync(S->d.dy, 0, mb, nullptr));
    return KVX_OK;
}

// the buffers of the polish, and tril(P) + delta I on the pattern the plan was given
int polish_buffers(kvx_admm *S, double delta)
{
    PolishDev &p = S->p;
    int rc = 0;
    if (!p.act) {
        double *act = nullptr;                                          // m int64 flags in a buffer of the same width
        if ((rc = zeros(S, &p.w, S->m)) || (rc = zeros(S, &p.b, S->m)) || (rc = zeros(S, &p.xh, S->n)) || (rc = zeros(S, &p.zh, S->m)) ||
            (rc = zeros(S, &p.yh, S->m)) || (rc = zeros(S, &p.e2, S->m)) || (rc = zeros(S, &p.we2, S->m)) || (rc = zeros(S, &p.rhs, S->n)) ||
            (rc = zeros(S, &S->d_ppart, POLISH_NRES * polish_part_stride(S->d))) || (rc = zeros(S, &S->d_pres, POLISH_NRES)) ||
            (rc = zeros(S, &S->d_Lxd, (int64_t)S->Lx.size())) || (rc = zeros(S, &act, S->m)))
            return rc;
        static_assert(sizeof(int64_t) == sizeof(double), "the flags share the allocator of the vectors");
        p.act = reinterpret_cast<int64_t *>(act);
    }
    if (S->lxd_delta != delta) {
        std::vector<double> lxd(S->Lx);
        for (int64_t j = 0; j < S->n; j++) lxd[S->Lp[j]] += delta;
        HIPCHK(hipMemcpy(S->d_Lxd, lxd.data(), lxd.size() * sizeof(double), hipMemcpyHostToDevice));
        S->lxd_delta = delta;
    }
    return KVX_OK;
}

int polish_impl(kvx_admm *S, double delta, int64_t refine_iter, double *out)
{
    if (!S || !out || refine_iter < 0 || !(delta > 0.0)) { set_last_error("kvx_admm_polish: delta > 0 and refine_iter >= 0 are required"); return KVX_EINVAL; }
    int rc = need_setup(S, "kvx_admm_polish");
    if (rc || (rc = polish_buffers(S, delta))) return rc;
    PolishDev &p = S->p;
    p.a = S->d;
    p.delta = delta;
    S->polished = false;
    const int64_t ld = std::max<int64_t>(1, S->n);
    HIPCHK(hipMemsetAsync(p.xh, 0, (size_t)S->n * sizeof(double), nullptr));
    HIPCHK(hipMemsetAsync(p.yh, 0, (size_t)S->m * sizeof(double), nullptr));
    launch_polish_active(nullptr, p, S->d_ppart);
    if ((rc = kvx_atda_assemble_dev(S->plan, S->d.Ax, p.w, S->d_Lxd, S->d_Sx))) return rc;
    S->stale = true;                                                    // from here on the kept factor is not that of S
    if ((rc = kvx_chol_factorize_async_dev(S->F, S->d_Sx))) return rc;
    S->nfact++;
    for (int64_t pass = 0; pass <= refine_iter; pass++) {               // the first solve, then the refinement passes
        launch_polish_residual(nullptr, p, S->d_ppart);
        if ((rc = kvx_chol_solve_async_dev(S->F, 0, p.rhs, 1, ld))) return rc;
        launch_polish_correct(nullptr, p);
    }
    launch_polish_finish(nullptr, p, S->d_ppart, S->d_pres);
    HIPCHK(hipGetLastError());
    double res[POLISH_NRES];
    HIPCHK(hipMemcpy(res, S->d_pres, sizeof(res), hipMemcpyDeviceToHost));      // the one host synchronisation
    std::fill(out, out + 16, 0.0);
    out[1] = res[0]; out[2] = res[1];
    int64_t minor = 0;
    rc = kvx_chol_status(S->F, &minor);
    if (rc == KVX_ENOTPOSDEF) { out[0] = -1.0; return KVX_OK; }         // not an error: the caller keeps the ADMM solution
    if (rc) return rc;
    out[0] = 1.0;
    std::copy(res, res + POLISH_NRES, out + 1);
    S->polished = true;
    return KVX_OK;
}

int polish_state_impl(kvx_admm *S, double *x, double *z, double *y, int64_t *act)
{
    if (!S) return KVX_EINVAL;
    int rc = need_setup(S, "kvx_admm_polish_state");
    if (rc) return rc;
    if (!S->p.act) { set_last_error("kvx_admm_polish_state: kvx_admm_polish has not run"); return KVX_EINVAL; }
    if ((rc = fetch(x, S->p.xh, S->n)) || (rc = fetch(z, S->p.zh, S->m)) || (rc = fetch(y, S->p.yh, S->m))) return rc;
    if (act) HIPCHK(hipMemcpy(act, S->p.act, (size_t)S->m * sizeof(int64_t), hipMemcpyDeviceToHost));
    return KVX_OK;
}

int polish_accept_impl(kvx_admm *S)
{
    if (!S) return KVX_EINVAL;
    const int rc = need_setup(S, "kvx_admm_polish_accept");
    if (rc) return rc;
    if (!S->polished) { set_last_error("kvx_admm_polish_accept: no polished solution is held"); return KVX_EINVAL; }
    const size_t nb = (size_t)S->n * sizeof(double), mb = (size_t)S->m * sizeof(double);
    HIPCHK(hipMemcpyAsync(S->d.x, S->p.xh, nb, hipMemcpyDeviceToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(S->d.z, S->p.zh, mb, hipMemcpyDeviceToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(S->d.y, S->p.yh, mb, hipMemcpyDeviceToDevice, nullptr));
    HIPCHK(hipMemsetAsync(S->d.dx, 0, nb, nullptr));
    HIPCHK(hipMemsetAsync(S->d.dy, 0, mb, nullptr));
    return KVX_OK;
}

// ---- a batch on the kept factor ---------------------------------------------------------------------------------------------
int batch_end_impl(kvx_admm *S)
{
    if (!S) return KVX_EINVAL;
    for (void *p : S->bowned) {
        S->owned.erase(std::remove(S->owned.begin(), S->owned.end(), p), S->owned.end());
        (void)pool_free(p);
    }
    S->bowned.clear();
    S->b = AdmmBatchDev{};
    S->d_run = nullptr;
    S->d_bpart = S->d_bres = nullptr;
    return KVX_OK;
}

int batch_zeros(kvx_admm *S, double **dst, int64_t count)
{
    const int rc = zeros(S, dst, count);                                // on failure nothing was pushed for this pointer
    if (!rc) S->bowned.push_back(*dst);
    return rc;
}

int batch_begin_impl(kvx_admm *S, int64_t B, const double *Q, const double *L, const double *U)
{
    if (!S) return KVX_EINVAL;
    if (B < 1 || B > 65535) { set_last_error("kvx_admm_batch_begin: 1 <= B <= 65535 is required"); return KVX_EINVAL; }
    const int64_t m = S->m, n = S->n;
    // every member gives every row the rho class it has in the kept problem: one rho vector, one factor
    if (L || U)
        for (int64_t bm = 0; bm < B; bm++)
            for (int64_t i = 0; i < m; i++) {
                const double lr = L ? L[i + bm * m] : 0.0, ur = U ? U[i + bm * m] : 0.0;
                const double l = !L ? S->l[i] : (lr <= -OSQP_INFTY * MIN_SCALING ? -OSQP_INFTY : S->E[i] * lr);
                const double u = !U ? S->u[i] : (ur >= OSQP_INFTY * MIN_SCALING ? OSQP_INFTY : S->E[i] * ur);
                if (!(l <= u)) {
                    set_last_error("kvx_admm_batch_begin: l <= u does not hold in member " + std::to_string(bm) + ", row " + std::to_string(i));
                    return KVX_EINVAL;
                }
                if (rho_class(l, u) != rho_class(S->l[i], S->u[i])) {
                    set_last_error("kvx_admm_batch_begin: member " + std::to_string(bm) + ", row " + std::to_string(i) +
                                   " is not in the rho class the row has in the kept problem");
                    return KVX_EINVAL;
                }
            }
    int rc = need_setup(S, "kvx_admm_batch_begin");
    if (rc) return rc;
    AdmmBatchDev &b = S->b;
    if (b.B != B) {
        batch_end_impl(S);
        b.a = S->d;
        b.B = B;
        double *run = nullptr;                                          // B int flags in a buffer of doubles
        const int64_t nb = admm_batch_residual_blocks(b);
        if ((rc = batch_zeros(S, &b.q, n * B)) || (rc = batch_zeros(S, &b.x, n * B)) || (rc = batch_zeros(S, &b.dx, n * B)) ||
            (rc = batch_zeros(S, &b.xt, n * B)) || (rc = batch_zeros(S, &b.l, m * B)) || (rc = batch_zeros(S, &b.u, m * B)) ||
            (rc = batch_zeros(S, &b.z, m * B)) || (rc = batch_zeros(S, &b.y, m * B)) || (rc = batch_zeros(S, &b.dy, m * B)) ||
            (rc = batch_zeros(S, &S->d_bpart, B * ADMM_NRES * nb)) || (rc = batch_zeros(S, &S->d_bres, B * ADMM_NRES)) ||
            (rc = batch_zeros(S, &run, B))) {
            batch_end_impl(S);
            return rc;
        }
        S->d_run = reinterpret_cast<int *>(run);
        b.run = S->d_run;
    }
    b.a = S->d;                                                         // the kept q, l, u as they are now
    const size_t nb_ = (size_t)(n * B) * sizeof(double), mb_ = (size_t)(m * B) * sizeof(double);
    if (Q) HIPCHK(hipMemcpy(b.xt, Q, nb_, hipMemcpyHostToDevice));     // xt and dy stage the raw data
    launch_admm_batch_scale_q(nullptr, b, S->c, Q ? b.xt : nullptr);
    if (L) HIPCHK(hipMemcpy(b.dy, L, mb_, hipMemcpyHostToDevice));
    launch_admm_batch_scale_bound(nullptr, b, false, L ? b.dy : nullptr);
    if (U) HIPCHK(hipMemcpy(b.dy, U, mb_, hipMemcpyHostToDevice));
    launch_admm_batch_scale_bound(nullptr, b, true, U ? b.dy : nullptr);
    HIPCHK(hipMemsetAsync(b.x, 0, nb_, nullptr));
    HIPCHK(hipMemsetAsync(b.dx, 0, nb_, nullptr));
    HIPCHK(hipMemsetAsync(b.z, 0, mb_, nullptr));
    HIPCHK(hipMemsetAsync(b.y, 0, mb_, nullptr));
    HIPCHK(hipMemsetAsync(b.dy, 0, mb_, nullptr));
    HIPCHK(hipMemsetAsync(S->d_bres, 0, (size_t)(B * ADMM_NRES) * sizeof(double), nullptr));
    HIPCHK(hipGetLastError());
    return KVX_OK;
}

int need_batch(kvx_admm *S, const char *who)
{
    const int rc = need_setup(S, who);
    if (rc) return rc;
    if (S->b.B < 1) { set_last_error(std::string(who) + ": kvx_admm_batch_begin has not run"); return KVX_EINVAL; }
    return KVX_OK;
}

int batch_iterate_impl(kvx_admm *S, int64_t k, const int64_t *running, double *out)
{
    if (!S || k < 0 || !running || !out) return KVX_EINVAL;
    int rc = need_batch(S, "kvx_admm_batch_iterate");
    if (rc) return rc;
    const AdmmBatchDev &b = S->b;
    std::vector<int> run((size_t)b.B);
    for (int64_t bm = 0; bm < b.B; bm++) run[(size_t)bm] = running[bm] != 0;
    HIPCHK(hipMemcpy(S->d_run, run.data(), run.size() * sizeof(int), hipMemcpyHostToDevice));
    const int64_t ld = std::max<int64_t>(1, S->n);
    if (S->stale && k > 0) {                                            // a polish took the factor over: S at the current rho again
        if ((rc = refactor(S, S->rho0))) return rc;
    }
    for (int64_t it = 0; it < k; it++) {
        launch_admm_batch_rhs(nullptr, b);
        if ((rc = kvx_chol_solve_async_dev(S->F, 0, b.xt, b.B, ld))) return rc;
        launch_admm_batch_update(nullptr, b);
    }
    launch_admm_batch_residuals(nullptr, b, S->d_bpart, S->d_bres);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, S->d_bres, (size_t)(b.B * ADMM_NRES) * sizeof(double), hipMemcpyDeviceToHost));      // the one host synchronisation
    return KVX_OK;
}

int batch_state_impl(kvx_admm *S, double *x, double *z, double *y, double *dx, double *dy)
{
    if (!S) return KVX_EINVAL;
    int rc = need_batch(S, "kvx_admm_batch_state");
    if (rc) return rc;
    const AdmmBatchDev &b = S->b;
    if ((rc = fetch(x, b.x, S->n * b.B)) || (rc = fetch(z, b.z, S->m * b.B)) || (rc = fetch(y, b.y, S->m * b.B)) ||
        (rc = fetch(dx, b.dx, S->n * b.B)) || (rc = fetch(dy, b.dy, S->m * b.B)))
        return rc;
    return KVX_OK;
}

int batch_solution_impl(kvx_admm *S, const int64_t *kinds, double *X, double *Y)
{
    if (!S || !kinds || !X || !Y) return KVX_EINVAL;
    int rc = need_batch(S, "kvx_admm_batch_solution");
    if (rc) return rc;
    const AdmmBatchDev &b = S->b;
    const int64_t m = S->m, n = S->n, B = b.B;
    bool any[3] = {false, false, false};
    for (int64_t bm = 0; bm < B; bm++) {
        if (kinds[bm] < -1 || kinds[bm] > 2) { set_last_error("kvx_admm_batch_solution: a kind is -1, 0, 1 or 2"); return KVX_EINVAL; }
        if (kinds[bm] >= 0) any[kinds[bm]] = true;
    }
    std::vector<double> x, dx, y, dy, l, u;
    if (any[0]) { x.resize((size_t)(n * B)); y.resize((size_t)(m * B)); if ((rc = fetch(x.data(), b.x, n * B)) || (rc = fetch(y.data(), b.y, m * B))) return rc; }
    if (any[1]) {
        dy.resize((size_t)(m * B)); l.resize((size_t)(m * B)); u.resize((size_t)(m * B));
        if ((rc = fetch(dy.data(), b.dy, m * B)) || (rc = fetch(l.data(), b.l, m * B)) || (rc = fetch(u.data(), b.u, m * B))) return rc;
    }
    if (any[2]) { dx.resize((size_t)(n * B)); if ((rc = fetch(dx.data(), b.dx, n * B))) return rc; }
    const double cinv = 1.0 / S->c;
    for (int64_t bm = 0; bm < B; bm++) {
        const int64_t kind = kinds[bm];
        double *xo = X + bm * n, *yo = Y + bm * m;
        std::fill(xo, xo + n, 0.0);
        std::fill(yo, yo + m, 0.0);
        if (kind == 0 || kind == 2) {                                   // x = D x, or the certificate D dx
            const double *src = (kind == 0 ? x.data() : dx.data()) + bm * n;
            for (int64_t j = 0; j < n; j++) xo[j] = src[j] * S->D[j];
        }
        if (kind == 0 || kind == 1) {                                   // y = E y / c, or the certificate E dy / c
            const double *src = (kind == 0 ? y.data() : dy.data()) + bm * m;
            for (int64_t i = 0; i < m; i++) {
                double v = src[i];
                if (kind == 1) {                                        // without the parts that push against an infinite bound
                    const bool ui = u[(size_t)(i + bm * m)] >= OSQP_INFTY * MIN_SCALING, li = l[(size_t)(i + bm * m)] <= -OSQP_INFTY * MIN_SCALING;
                    v = ui && li ? 0.0 : (ui ? std::min(v, 0.0) : (li ? std::max(v, 0.0) : v));
                }
                yo[i] = S->E[i] * v * cinv;
            }
        }
    }
    return KVX_OK;
}

}  // namespace

extern "C" {

int kvx_admm_plan(int64_t m, int64_t n, const int64_t *Ap, const int64_t *Ai, const double *Ax, const int64_t *Pp, const int64_t *Pi,
                  const double *Px, const double *q, const double *l, const double *u, int64_t scaling, double *D, double *E,
                  double *c, int64_t *snz, kvx_admm **out)
{
    return guarded([&] { return plan_impl(m, n, Ap, Ai, Ax, Pp, Pi, Px, q, l, u, scaling, D, E, c, snz, out); });
}

int kvx_admm_pattern(kvx_admm *S, int64_t *snz, int64_t *Sp, int64_t *Si)
{
    if (!S) return KVX_EINVAL;
    if (snz) *snz = S->snz;
    if (Sp) std::copy(S->Sp.begin(), S->Sp.end(), Sp);
    if (Si) std::copy(S->Si.begin(), S->Si.end(), Si);
    return KVX_OK;
}

int kvx_admm_rho_vector(kvx_admm *S, double rho, double *rho_host)
{
    if (!S || !rho_host || !(rho > 0.0)) return KVX_EINVAL;
    rho_vector(S, rho, rho_host);
    return KVX_OK;
}

int kvx_admm_setup_dev(kvx_admm *S, double sigma, double rho, double alpha)
{
    return guarded([&] { return setup_impl(S, sigma, rho, alpha); });
}

int kvx_admm_iterate(kvx_admm *S, int64_t k, double *out_host)
{
    return guarded([&] { return iterate_impl(S, k, out_host); });
}

int kvx_admm_set_rho(kvx_admm *S, double rho)
{
    return guarded([&] {
        if (!S || !(rho > 0.0)) return (int)KVX_EINVAL;
        if (!have_device("kvx_admm_set_rho")) return (int)KVX_EDEVICE;
        if (!S->dev) { set_last_error("kvx_admm_set_rho: kvx_admm_setup_dev has not run"); return (int)KVX_EINVAL; }
        return refactor(S, rho);                                        // also what restores a factor a polish took over
    });
}

int kvx_admm_state(kvx_admm *S, double *x, double *z, double *y, double *dx, double *dy)
{
    if (!S) return KVX_EINVAL;
    if (!have_device("kvx_admm_state")) return KVX_EDEVICE;
    if (!S->dev) { set_last_error("kvx_admm_state: kvx_admm_setup_dev has not run"); return KVX_EINVAL; }
    int rc;
    if ((rc = fetch(x, S->d.x, S->n)) || (rc = fetch(z, S->d.z, S->m)) || (rc = fetch(y, S->d.y, S->m)) || (rc = fetch(dx, S->d.dx, S->n)) ||
        (rc = fetch(dy, S->d.dy, S->m)))
        return rc;
    return KVX_OK;
}

int kvx_admm_solution(kvx_admm *S, int kind, double *x, double *y)
{
    return guarded([&] {
        if (!S || kind < 0 || kind > 3 || (kind != 1 && !x) || (kind != 2 && !y)) return (int)KVX_EINVAL;
        if (kind == 3 && !S->polished) { set_last_error("kvx_admm_solution: no polished solution is held"); return (int)KVX_EINVAL; }
        if (!have_device("kvx_admm_solution")) return (int)KVX_EDEVICE;
        if (!S->dev) { set_last_error("kvx_admm_solution: kvx_admm_setup_dev has not run"); return (int)KVX_EINVAL; }
        int rc;
        const double cinv = 1.0 / S->c;
        if (kind != 1) {                                                // x = D x (kind 0), D xh (kind 3), the certificate D dx (kind 2)
            if ((rc = fetch(x, kind == 0 ? S->d.x : (kind == 3 ? S->p.xh : S->d.dx), S->n))) return rc;
            for (int64_t j = 0; j < S->n; j++) x[j] *= S->D[j];
        }
        if (kind != 2) {                                                // y = E y / c (kind 0), E yh / c (kind 3), the certificate E dy / c (kind 1)
            if ((rc = fetch(y, kind == 0 ? S->d.y : (kind == 3 ? S->p.yh : S->d.dy), S->m))) return rc;
            for (int64_t i = 0; i < S->m; i++) {
                double v = y[i];
                if (kind == 1) {                                        // without the parts that push against an infinite bound
                    const bool ui = S->u[i] >= OSQP_INFTY * MIN_SCALING, li = S->l[i] <= -OSQP_INFTY * MIN_SCALING;
                    v = ui && li ? 0.0 : (ui ? std::min(v, 0.0) : (li ? std::max(v, 0.0) : v));
                }
                y[i] = S->E[i] * v * cinv;
            }
        }
        return (int)KVX_OK;
    });
}

int kvx_admm_update(kvx_admm *S, const double *q, const double *l, const double *u)
{
    return guarded([&] { return update_impl(S, q, l, u); });
}

int kvx_admm_warm_start(kvx_admm *S, const double *x, const double *y)
{
    return guarded([&] { return warm_start_impl(S, x, y); });
}

int kvx_admm_cold_start(kvx_admm *S)
{
    return guarded([&] { return cold_start_impl(S); });
}

int kvx_admm_polish(kvx_admm *S, double delta, int64_t refine_iter, double *out_host)
{
    return guarded([&] { return polish_impl(S, delta, refine_iter, out_host); });
}

int kvx_admm_polish_state(kvx_admm *S, double *x, double *z, double *y, int64_t *act)
{
    return guarded([&] { return polish_state_impl(S, x, z, y, act); });
}

int kvx_admm_polish_accept(kvx_admm *S)
{
    return guarded([&] { return polish_accept_impl(S); });
}

int kvx_admm_info(kvx_admm *S, int64_t info[8])
{
    if (!S || !info) return KVX_EINVAL;
    const int64_t v[8] = {S->m, S->n, S->snz, S->nfact, S->niter, (int64_t)S->rs.size(), (int64_t)S->rl.size(), S->dev ? 1 : 0};
    std::copy(v, v + 8, info);
    return KVX_OK;
}

int kvx_admm_batch_begin(kvx_admm *S, int64_t B, const double *Q, const double *L, const double *U)
{
    return guarded([&] { return batch_begin_impl(S, B, Q, L, U); });
}

int kvx_admm_batch_iterate(kvx_admm *S, int64_t k, const int64_t *running, double *out_host)
{
    return guarded([&] { return batch_iterate_impl(S, k, running, out_host); });
}

int kvx_admm_batch_state(kvx_admm *S, double *x, double *z, double *y, double *dx, double *dy)
{
    return guarded([&] { return batch_state_impl(S, x, z, y, dx, dy); });
}

int kvx_admm_batch_solution(kvx_admm *S, const int64_t *kinds, double *X, double *Y)
{
    return guarded([&] { return batch_solution_impl(S, kinds, X, Y); });
}

int kvx_admm_batch_end(kvx_admm *S)
{
    return guarded([&] { return batch_end_impl(S); });
}

void kvx_admm_free(kvx_admm *S)
{
    if (!S) return;
    for (void *p : S->owned) (void)pool_free(p);
    if (S->F) kvx_chol_free(S->F);
    if (S->plan) kvx_atda_free(S->plan);
    delete S;
}

}  // extern "C"
