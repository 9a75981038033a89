// The plan of the ADMM solver behind kvxopt.osqp (kvx_admm_plan and the entries that only read it); nothing here needs a device.
// The plan validates the data, equilibrates it (Ruiz passes on the KKT matrix [[P, A'], [A, 0]] and the cost scaling), keeps the
// scaled A by columns and by rows, the scaled P as its lower triangle (for S) and in full (for P x), builds the kvx_atda plan of
// A with the pattern tril(P) U I -- sigma has a slot in every column -- and analyses that pattern once.
#include "admm_internal.hpp"

#include <cmath>
#include <memory>

using namespace kvx;

namespace kvx {
void admm_rho_vector(const kvx_admm *S, double rho, double *out)
{
    rho = std::min(std::max(rho, RHO_MIN), RHO_MAX);
    const double by_class[3] = {RHO_MIN, RHO_EQ_OVER_RHO_INEQ * rho, rho};
    for (int64_t i = 0; i < S->m; i++) out[i] = by_class[rho_class(S->l[i], S->u[i])];
}
}  // namespace kvx

namespace {
inline double limit_scaling(double v) { return v < MIN_SCALING ? 1.0 : (v > MAX_SCALING ? MAX_SCALING : v); }

// dn[j] = the largest |entry| of column j of the symmetric matrix whose lower triangle is (Lp, Li, Lx), over what dn holds
void sym_column_norms(const kvx_admm *S, std::vector<double> &dn)
{
    for (int64_t j = 0; j < S->n; j++)
        for (int64_t e = S->Lp[j]; e < S->Lp[j + 1]; e++) {
            const double a = std::fabs(S->Lx[e]);
            dn[j] = std::max(dn[j], a);
            dn[S->Li[e]] = std::max(dn[S->Li[e]], a);
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
        if (check_row("kvx_admm_plan", l[i], u[i])) return KVX_EINVAL;
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
        sym_column_norms(S, dn);                                        // column norms of [[P, A'], [A, 0]]
        for (int64_t j = 0; j < n; j++)
            for (int64_t e = S->Ap[j]; e < S->Ap[j + 1]; e++) {
                const double a = std::fabs(S->Ax[e]);
                dn[j] = std::max(dn[j], a);
                en[S->Ai[e]] = std::max(en[S->Ai[e]], a);
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
        sym_column_norms(S, dn);
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
        S->l[i] = scaled_bound(l[i], S->E[i], false);
        S->u[i] = scaled_bound(u[i], S->E[i], true);
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
    admm_rho_vector(S, rho, rho_host);
    return KVX_OK;
}

int kvx_admm_info(kvx_admm *S, int64_t info[8])
{
    if (!S || !info) return KVX_EINVAL;
    const int64_t v[8] = {S->m, S->n, S->snz, S->nfact, S->niter, (int64_t)S->rs.size(), (int64_t)S->rl.size(), S->dev ? 1 : 0};
    std::copy(v, v + 8, info);
    return KVX_OK;
}

}  // extern "C"
