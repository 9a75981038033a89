// C-ABI entry points of the ADMM solver behind kvxopt.osqp (include/kvxhip.h, kvx_admm_*): minimise 1/2 x'Px + q'x subject to
// l <= Ax <= u by the iteration of OSQP (Stellato et al. 2020) on one kept Cholesky factor of
//
//     S = P + sigma I + A' diag(rho) A.
//
// The plan is host work (admm_plan.cpp).  Everything after it runs in HBM: kvx_admm_iterate issues
// k x {k_admm_rhs, kvx_chol_solve_async_dev, k_admm_update} back to back, then the residual kernels, and reads 24 doubles.  No CPU
// fallback: without a HIP device the device entry points return KVX_EDEVICE.
//
// A handle can be kept across solves: kvx_admm_update replaces q, l, u (rescaled with the kept D, E, c; one refactorisation only
// when a row changes its rho class), kvx_admm_warm_start / kvx_admm_cold_start set the state, and kvx_admm_polish solves the
// equality-constrained QP of the guessed active set on S_pol = P + delta I + A' diag(w) A -- the analysed pattern, the same
// kvx_chol, whose numeric factor it takes over: the handle marks the ADMM factor stale and the next iteration rebuilds it.
// A batch on the kept factor is in admm_batch_api.cpp.
#include "admm_internal.hpp"

using namespace kvx;

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

// rho vector to the device, S assembled on its pattern and factored
int refactor(kvx_admm *S, double rho)
{
    S->rho0 = std::min(std::max(rho, RHO_MIN), RHO_MAX);
    S->rho.resize((size_t)S->m);
    admm_rho_vector(S, rho, S->rho.data());
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
    if (admm_need_setup(nullptr, "kvx_admm_setup_dev")) return KVX_EDEVICE;
    if (S->dev) { set_last_error("kvx_admm_setup_dev: called twice"); return KVX_EINVAL; }
    AdmmDev &d = S->d;
    d.m = S->m; d.n = S->n; d.ns = (int64_t)S->rs.size(); d.nl = (int64_t)S->rl.size();
    d.sigma = S->sigma = sigma; d.alpha = S->alpha = alpha; d.cinv = 1.0 / S->c;
    int rc = 0;
#define UP(dst, src) if ((rc = up(S, &d.dst, S->src))) return rc
    UP(Ap, Ap); UP(Ai, Ai); UP(Ax, Ax); UP(Tp, Tp); UP(Ti, Ti); UP(Tx, Tx); UP(Fp, Fp); UP(Fi, Fi); UP(Fx, Fx); UP(rs, rs); UP(rl, rl);
    UP(q, q); UP(l, l); UP(u, u); UP(D, D); UP(Dinv, Dinv); UP(E, E); UP(Einv, Einv);
#undef UP
    std::vector<void *> &own = S->owned;
    double *rho_dev = nullptr;
    if ((rc = zeros(own, &rho_dev, S->m))) return rc;
    d.rho = rho_dev;
    if ((rc = zeros(own, &d.x, S->n)) || (rc = zeros(own, &d.z, S->m)) || (rc = zeros(own, &d.y, S->m)) || (rc = zeros(own, &d.dx, S->n)) ||
        (rc = zeros(own, &d.dy, S->m)) || (rc = zeros(own, &d.xt, S->n)) || (rc = zeros(own, &S->d_Sx, S->snz)) ||
        (rc = zeros(own, &S->d_part, ADMM_NRES * admm_residual_blocks(d))) || (rc = zeros(own, &S->d_res, ADMM_NRES)))
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
    int rc = admm_need_setup(S, "kvx_admm_iterate");
    if (rc) return rc;
    const int64_t ld = std::max<int64_t>(1, S->n);
    if (k > 0 && (rc = admm_restore_factor(S))) return rc;
    for (int64_t it = 0; it < k; it++) {
        launch_admm_rhs(nullptr, S->d);
        if ((rc = kvx_chol_solve_async_dev(S->F, 0, S->d.xt, 1, ld))) return rc;
        launch_admm_update(nullptr, S->d);
    }
    S->niter += k;
    launch_admm_residuals(nullptr, S->d, S->d_part, S->d_res);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, S->d_res, ADMM_NRES * sizeof(double), hipMemcpyDeviceToHost));
    return KVX_OK;
}

int state_impl(kvx_admm *S, double *x, double *z, double *y, double *dx, double *dy)
{
    if (!S) return KVX_EINVAL;
    int rc = admm_need_setup(S, "kvx_admm_state");
    if (rc) return rc;
    if ((rc = fetch(x, S->d.x, S->n)) || (rc = fetch(z, S->d.z, S->m)) || (rc = fetch(y, S->d.y, S->m)) || (rc = fetch(dx, S->d.dx, S->n)) ||
        (rc = fetch(dy, S->d.dy, S->m)))
        return rc;
    return KVX_OK;
}

// kind 0: x = D x, y = E y / c; 3: the same of xh, yh; 1: the certificate E dy / c; 2: the certificate D dx
int solution_impl(kvx_admm *S, int kind, double *x, double *y)
{
    if (!S || kind < 0 || kind > 3 || (kind != 1 && !x) || (kind != 2 && !y)) return KVX_EINVAL;
    if (kind == 3 && !S->polished) { set_last_error("kvx_admm_solution: no polished solution is held"); return KVX_EINVAL; }
    int rc = admm_need_setup(S, "kvx_admm_solution");
    if (rc) return rc;
    if (kind != 1) {
        if ((rc = fetch(x, kind == 0 ? S->d.x : (kind == 3 ? S->p.xh : S->d.dx), S->n))) return rc;
        admm_unscale_x(S, x, x);
    }
    if (kind != 2) {
        if ((rc = fetch(y, kind == 0 ? S->d.y : (kind == 3 ? S->p.yh : S->d.dy), S->m))) return rc;
        admm_unscale_y(S, y, kind == 1 ? S->l.data() : nullptr, S->u.data(), y);
    }
    return KVX_OK;
}

// ---- the kept problem: update, warm start, polish ---------------------------------------------------------------------------
int stage_buffer(kvx_admm *S)
{
    if (S->d_stage) return KVX_OK;
    return zeros(S->owned, &S->d_stage, S->n + 2 * S->m);
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
            if (l) ln[i] = scaled_bound(l[i], S->E[i], false);
            if (u) un[i] = scaled_bound(u[i], S->E[i], true);
            if (check_row("kvx_admm_update", ln[i], un[i])) return KVX_EINVAL;
            changed = changed || rho_class(ln[i], un[i]) != rho_class(S->l[i], S->u[i]);
        }
    }
    int rc = admm_need_setup(S, "kvx_admm_update");
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
    int rc = admm_need_setup(S, "kvx_admm_warm_start");
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
    const int rc = admm_need_setup(S, "kvx_admm_cold_start");
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
    std::vector<void *> &own = S->owned;
    int rc = 0;
    if (!p.act) {
        if ((rc = zeros(own, &p.w, S->m)) || (rc = zeros(own, &p.b, S->m)) || (rc = zeros(own, &p.xh, S->n)) || (rc = zeros(own, &p.zh, S->m)) ||
            (rc = zeros(own, &p.yh, S->m)) || (rc = zeros(own, &p.e2, S->m)) || (rc = zeros(own, &p.we2, S->m)) || (rc = zeros(own, &p.rhs, S->n)) ||
            (rc = zeros(own, &S->d_ppart, POLISH_NRES * polish_part_stride(S->d))) || (rc = zeros(own, &S->d_pres, POLISH_NRES)) ||
            (rc = zeros(own, &S->d_Lxd, (int64_t)S->Lx.size())) || (rc = zeros(own, &p.act, S->m)))
            return rc;
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
    int rc = admm_need_setup(S, "kvx_admm_polish");
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
    int rc = admm_need_setup(S, "kvx_admm_polish_state");
    if (rc) return rc;
    if (!S->p.act) { set_last_error("kvx_admm_polish_state: kvx_admm_polish has not run"); return KVX_EINVAL; }
    if ((rc = fetch(x, S->p.xh, S->n)) || (rc = fetch(z, S->p.zh, S->m)) || (rc = fetch(y, S->p.yh, S->m))) return rc;
    if (act) HIPCHK(hipMemcpy(act, S->p.act, (size_t)S->m * sizeof(int64_t), hipMemcpyDeviceToHost));
    return KVX_OK;
}

int polish_accept_impl(kvx_admm *S)
{
    if (!S) return KVX_EINVAL;
    const int rc = admm_need_setup(S, "kvx_admm_polish_accept");
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

}  // namespace

namespace kvx {
// S == nullptr: the device alone is asked for
int admm_need_setup(const kvx_admm *S, const char *who)
{
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd < 1) {
        set_last_error(std::string(who) + ": no HIP device; the ADMM iteration has no CPU fallback");
        return KVX_EDEVICE;
    }
    if (S && !S->dev) { set_last_error(std::string(who) + ": kvx_admm_setup_dev has not run"); return KVX_EINVAL; }
    return KVX_OK;
}

int admm_restore_factor(kvx_admm *S)
{
    return S->stale ? refactor(S, S->rho0) : (int)KVX_OK;
}
}  // namespace kvx

extern "C" {

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
        const int rc = admm_need_setup(S, "kvx_admm_set_rho");
        return rc ? rc : refactor(S, rho);                              // also what restores a factor a polish took over
    });
}

int kvx_admm_state(kvx_admm *S, double *x, double *z, double *y, double *dx, double *dy)
{
    return guarded([&] { return state_impl(S, x, z, y, dx, dy); });
}

int kvx_admm_solution(kvx_admm *S, int kind, double *x, double *y)
{
    return guarded([&] { return solution_impl(S, kind, x, y); });
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

void kvx_admm_free(kvx_admm *S)
{
    if (!S) return;
    (void)admm_batch_end(S);
    for (void *p : S->owned) (void)pool_free(p);
    if (S->F) kvx_chol_free(S->F);
    if (S->plan) kvx_atda_free(S->plan);
    delete S;
}

}  // extern "C"
