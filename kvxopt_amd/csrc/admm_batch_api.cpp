// kvx_admm_batch_* (include/kvxhip.h): B data sets (q_b, l_b, u_b) through the one kept factor of a kvx_admm problem
// (admm_batch.hip): buffers of its own, column-major, one triangular solve with B right-hand sides per iteration, one host read
// of B x 24 numbers per check.  The kept problem's data, state, rho and factor are not touched (a stale factor is rebuilt once,
// as kvx_admm_iterate does).
#include "admm_internal.hpp"

using namespace kvx;

namespace kvx {
int admm_batch_end(kvx_admm *S)
{
    if (!S) return KVX_EINVAL;
    for (void *p : S->bowned) (void)pool_free(p);
    S->bowned.clear();
    S->b = AdmmBatchDev{};
    S->d_bpart = S->d_bres = nullptr;
    return KVX_OK;
}
}  // namespace kvx

namespace {

int batch_begin_impl(kvx_admm *S, int64_t B, const double *Q, const double *L, const double *U)
{
    if (!S) return KVX_EINVAL;
    if (B < 1 || B > 65535) { set_last_error("kvx_admm_batch_begin: 1 <= B <= 65535 is required"); return KVX_EINVAL; }
    const int64_t m = S->m, n = S->n;
    // every member gives every row the rho class it has in the kept problem: one rho vector, one factor
    if (L || U)
        for (int64_t bm = 0; bm < B; bm++)
            for (int64_t i = 0; i < m; i++) {
                const double l = L ? scaled_bound(L[i + bm * m], S->E[i], false) : S->l[i];
                const double u = U ? scaled_bound(U[i + bm * m], S->E[i], true) : S->u[i];
                const auto where = [&] { return "member " + std::to_string(bm) + ", row " + std::to_string(i); };
                if (!(l <= u)) return check_row("kvx_admm_batch_begin", l, u, " in " + where());
                if (rho_class(l, u) != rho_class(S->l[i], S->u[i])) {
                    set_last_error("kvx_admm_batch_begin: " + where() + " is not in the rho class the row has in the kept problem");
                    return KVX_EINVAL;
                }
            }
    int rc = admm_need_setup(S, "kvx_admm_batch_begin");
    if (rc) return rc;
    AdmmBatchDev &b = S->b;
    if (b.B != B) {
        admm_batch_end(S);
        b.a = S->d;
        b.B = B;
        std::vector<void *> &own = S->bowned;
        int *run = nullptr;
        const int64_t nb = admm_residual_blocks(b.a);
        if ((rc = zeros(own, &b.q, n * B)) || (rc = zeros(own, &b.x, n * B)) || (rc = zeros(own, &b.dx, n * B)) ||
            (rc = zeros(own, &b.xt, n * B)) || (rc = zeros(own, &b.l, m * B)) || (rc = zeros(own, &b.u, m * B)) ||
            (rc = zeros(own, &b.z, m * B)) || (rc = zeros(own, &b.y, m * B)) || (rc = zeros(own, &b.dy, m * B)) ||
            (rc = zeros(own, &S->d_bpart, B * ADMM_NRES * nb)) || (rc = zeros(own, &S->d_bres, B * ADMM_NRES)) ||
            (rc = zeros(own, &run, B))) {
            admm_batch_end(S);
            return rc;
        }
        b.run = run;
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
    const int rc = admm_need_setup(S, who);
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
    HIPCHK(hipMemcpy(const_cast<int *>(b.run), run.data(), run.size() * sizeof(int), hipMemcpyHostToDevice));
    const int64_t ld = std::max<int64_t>(1, S->n);
    if (k > 0 && (rc = admm_restore_factor(S))) return rc;
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
    for (int64_t bm = 0; bm < B; bm++) {                                // per member what kvx_admm_solution gives; kind -1: zeros
        const int64_t kind = kinds[bm];
        double *xo = X + bm * n, *yo = Y + bm * m;
        std::fill(xo, xo + n, 0.0);
        std::fill(yo, yo + m, 0.0);
        if (kind == 0 || kind == 2) admm_unscale_x(S, (kind == 0 ? x.data() : dx.data()) + bm * n, xo);
        if (kind == 0) admm_unscale_y(S, y.data() + bm * m, nullptr, nullptr, yo);
        if (kind == 1) admm_unscale_y(S, dy.data() + bm * m, l.data() + bm * m, u.data() + bm * m, yo);
    }
    return KVX_OK;
}

}  // namespace

extern "C" {

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
    return guarded([&] { return admm_batch_end(S); });
}

}  // extern "C"
