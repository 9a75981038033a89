// C-ABI entry points of the sparse LU path (include/kvxhip.h, kvx_lu_*): what the reference's src/C/klu.c binds
// from SuiteSparse KLU (klu_analyze :141, klu_factor :161, klu_solve/klu_tsolve :187-198, klu_extract :444-449,
// Udiag/Rs/Pnum/Q for the determinant :760-822).  Device-only numeric phase: no CPU fallback.
#include "lu_internal.hpp"

#include <cmath>
#include <cstdlib>
#include <new>
#include <stdexcept>

namespace {

// The values of a factorisation made from device memory: kept in M.Ax when the analysis asks for it.
int keep_values(kvx_lu_num *N, const double *values_dev)
{
    N->have_vals = values_dev == N->M.Ax;
    if (N->have_vals || !(N->sym->Y.flags & KVX_LU_FLAG_KEEP_VALUES)) return KVX_OK;
    HIPCHK(hipMemcpyAsync(N->M.Ax, values_dev, (size_t)N->nnz * sizeof(double), hipMemcpyDeviceToDevice, N->st));
    N->have_vals = true;
    return KVX_OK;
}

template <class T>
T *mdup(const std::vector<T> &v)
{
    T *p = (T *)std::malloc(std::max<size_t>(v.size(), 1) * sizeof(T));
    if (p && !v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

struct Trip { int64_t r, c; double v; };
void to_ccs(int64_t n, std::vector<Trip> &t, std::vector<int64_t> &ptr, std::vector<int64_t> &idx, std::vector<double> &val)
{
    std::sort(t.begin(), t.end(), [](const Trip &a, const Trip &b) { return a.c != b.c ? a.c < b.c : a.r < b.r; });
    ptr.assign((size_t)n + 1, 0);
    idx.resize(t.size());
    val.resize(t.size());
    for (size_t q = 0; q < t.size(); q++) { ptr[t[q].c + 1]++; idx[q] = t[q].r; val[q] = t[q].v; }
    for (int64_t j = 0; j < n; j++) ptr[j + 1] += ptr[j];
}

}  // namespace

extern "C" {

int kvx_lu_analyze(int64_t n, const int64_t *colptr, const int64_t *rowind, const double *values, kvx_lu_sym **out)
{
    return kvx_lu_analyze_opts(n, colptr, rowind, values, 0, out);
}

int kvx_lu_analyze_opts(int64_t n, const int64_t *colptr, const int64_t *rowind, const double *values, int64_t flags, kvx_lu_sym **out)
{
    if (!out || !colptr || (!rowind && n > 0 && colptr[n] > 0) || (flags & ~(int64_t)(KVX_LU_FLAG_NO_BTF | KVX_LU_FLAG_KEEP_VALUES))) return KVX_EINVAL;
    *out = nullptr;
    kvx_lu_sym *S = new (std::nothrow) kvx_lu_sym();
    if (!S) return KVX_ENOMEM;
    try {
        lu_analyze(n, colptr, rowind, values, S->Y, (flags & KVX_LU_FLAG_NO_BTF) != 0);
        S->Y.flags = flags;
    } catch (const std::bad_alloc &) {
        delete S;
        return KVX_ENOMEM;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        delete S;
        return KVX_EINVAL;
    }
    *out = S;
    return KVX_OK;
}

void kvx_lu_free_symbolic(kvx_lu_sym *S) { delete S; }

void kvx_lu_free_numeric(kvx_lu_num *N)
{
    if (!N) return;
    if (N->st) (void)hipDeviceSynchronize();       // streams and events go back to the pool idle
    for (LuGraph *g : {&N->g_pass, &N->g_solve[0], &N->g_solve[1], &N->g_refine[0], &N->g_refine[1]}) g->drop();
    free_structure(N);
    lu_free_block(N->RM);
    lu_free_block(N->RF);
    lu_free_block(N->M);
    for (const LuLevelEvents &E : N->ev)
        for (hipEvent_t e : {E.A, E.B, E.C, E.D}) pool_event_put(e, false);
    if (N->ev0) pool_event_put(N->ev0, false);
    if (N->st3) pool_stream_put(N->st3);
    if (N->st2) pool_stream_put(N->st2);
    if (N->st) pool_stream_put(N->st);
    delete N;
}

int kvx_lu_sym_info(kvx_lu_sym *S, int64_t info[8])
{
    if (!S || !info) return KVX_EINVAL;
    info[0] = S->Y.n; info[1] = S->Y.nnz; info[2] = S->Y.S.nsuper; info[3] = S->Y.nmerges;
    info[4] = S->Y.structurally_singular ? 1 : 0; info[5] = S->Y.S.lnz; info[6] = S->Y.S.nlevels; info[7] = S->Y.S.max_m;
    return KVX_OK;
}

static int kvx_lu_sym_btf_impl(kvx_lu_sym *S, int64_t *nblocks, int64_t *nlevels, int64_t *blk)
{
    if (!S || !nblocks || !nlevels) return KVX_EINVAL;
    *nblocks = S->Y.nblocks;
    *nlevels = S->Y.nblev;
    if (blk) for (int64_t j = 0; j < S->Y.n; j++) blk[j] = S->Y.blk[(size_t)j];
    return KVX_OK;
}

int kvx_lu_sym_btf(kvx_lu_sym *S, int64_t *nblocks, int64_t *nlevels, int64_t *blk)
{
    return guarded([&] { return kvx_lu_sym_btf_impl(S, nblocks, nlevels, blk); });
}

int kvx_lu_sym_matching(kvx_lu_sym *S, int64_t *rowfor)
{
    if (!S || !rowfor) return KVX_EINVAL;
    std::copy(S->Y.rowfor.begin(), S->Y.rowfor.end(), rowfor);
    return KVX_OK;
}

static int new_numeric(kvx_lu_sym *S, int64_t nnz, kvx_lu_num **out)
{
    if (!S || !out) return KVX_EINVAL;
    *out = nullptr;
    if (nnz != S->Y.nnz) { set_last_error("A does not have the analysed sparsity pattern"); return KVX_EINVAL; }
    kvx_lu_num *N = new (std::nothrow) kvx_lu_num();
    if (!N) return KVX_ENOMEM;
    N->sym = S; N->n = S->Y.n; N->nnz = S->Y.nnz;
    N->K = read_lu_knobs();
    N->graphs_on = N->K.graph;
    *out = N;
    return KVX_OK;
}

static int kvx_lu_factor_dev_impl(kvx_lu_sym *S, int64_t nnz, const double *values_dev, kvx_lu_num **out)
{
    int rc = new_numeric(S, nnz, out);
    if (rc) return rc;
    kvx_lu_num *N = *out;
    if ((rc = ensure_device(N)) || (rc = lu_wait_for_caller(N)) || (rc = keep_values(N, values_dev)) || (rc = factor_loop(N, values_dev, 0))) { kvx_lu_free_numeric(N); *out = nullptr; return rc; }
    return KVX_OK;
}

int kvx_lu_factor_dev(kvx_lu_sym *S, int64_t nnz, const double *values_dev, kvx_lu_num **out)
{
    return guarded([&] { return kvx_lu_factor_dev_impl(S, nnz, values_dev, out); });
}

static int kvx_lu_factor_impl(kvx_lu_sym *S, int64_t nnz, const double *values, kvx_lu_num **out)
{
    int rc = new_numeric(S, nnz, out);
    if (rc) return rc;
    kvx_lu_num *N = *out;
    if ((rc = ensure_device(N))) { kvx_lu_free_numeric(N); *out = nullptr; return rc; }
    if (hipMemcpy(N->M.Ax, values, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = KVX_EDEVICE;
    N->have_vals = !rc;
    if (!rc) rc = factor_loop(N, N->M.Ax, 0);
    if (rc) { kvx_lu_free_numeric(N); *out = nullptr; return rc; }
    return KVX_OK;
}

int kvx_lu_factor(kvx_lu_sym *S, int64_t nnz, const double *values, kvx_lu_num **out)
{
    return guarded([&] { return kvx_lu_factor_impl(S, nnz, values, out); });
}

static int kvx_lu_refactor_dev_impl(kvx_lu_num *N, int64_t nnz, const double *values_dev)
{
    if (!N || nnz != N->nnz) return KVX_EINVAL;
    if (int rc = lu_wait_for_caller(N)) return rc;
    if (int rc = keep_values(N, values_dev)) return rc;
    if (!N->factored) return factor_loop(N, values_dev, 0);
    return factor_loop(N, values_dev, 1);
}

int kvx_lu_refactor_dev(kvx_lu_num *N, int64_t nnz, const double *values_dev)
{
    return guarded([&] { return kvx_lu_refactor_dev_impl(N, nnz, values_dev); });
}

static int kvx_lu_refactor_impl(kvx_lu_num *N, int64_t nnz, const double *values)
{
    if (!N || nnz != N->nnz || !values) return KVX_EINVAL;
    HIPCHK(hipMemcpy(N->M.Ax, values, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
    return kvx_lu_refactor_dev(N, nnz, N->M.Ax);
}

int kvx_lu_refactor(kvx_lu_num *N, int64_t nnz, const double *values)
{
    return guarded([&] { return kvx_lu_refactor_impl(N, nnz, values); });
}

int kvx_lu_solve_dev(kvx_lu_num *N, int trans, double *B_dev, int64_t nrhs, int64_t ldB)
{
    return guarded([&] { return lu_solve_any(N, false, trans, B_dev, nrhs, ldB, 0, nullptr); });
}

int kvx_lu_solve(kvx_lu_num *N, int trans, double *B, int64_t nrhs, int64_t ldB)
{
    return guarded([&] { return lu_solve_any(N, true, trans, B, nrhs, ldB, 0, nullptr); });
}

int kvx_lu_solve_refine_dev(kvx_lu_num *N, int trans, double *B_dev, int64_t nrhs, int64_t ldB, int64_t steps, double *berr_out)
{
    return guarded([&] { return lu_solve_any(N, false, trans, B_dev, nrhs, ldB, steps, berr_out); });
}

int kvx_lu_solve_refine(kvx_lu_num *N, int trans, double *B, int64_t nrhs, int64_t ldB, int64_t steps, double *berr_out)
{
    return guarded([&] { return lu_solve_any(N, true, trans, B, nrhs, ldB, steps, berr_out); });
}

int kvx_lu_num_info(kvx_lu_num *N, int64_t info[8])
{
    if (!N || !info) return KVX_EINVAL;
    info[0] = N->P.nfront; info[1] = N->P.nlevels; info[2] = N->P.max_m; info[3] = N->P.max_k;
    info[4] = N->P.lsize; info[5] = N->P.arena; info[6] = N->attempts; info[7] = N->factored ? 1 : 0;
    return KVX_OK;
}

int kvx_lu_num_graph_replays(kvx_lu_num *N, int64_t *replays)
{
    if (!N || !replays) return KVX_EINVAL;
    *replays = N->graph_replays;
    return KVX_OK;
}

int kvx_lu_num_work(kvx_lu_num *N, double work[5])
{
    if (!N || !work) return KVX_EINVAL;
    for (int i = 0; i < 5; i++) work[i] = 0.0;
    for (const LuFrontH &f : N->P.fr) {
        const double k = f.k, m = f.m, u = m - k;
        // columns j = 0 .. k-1 of a front of order m: (m - j - 1) divisions + 2 (m - j - 1)^2 flops of the rank-1 update
        const double fl = 2.0 * (k * u * u + u * k * (k - 1.0) + (k - 1.0) * k * (2.0 * k - 1.0) / 6.0) + k * u + k * (k - 1.0) / 2.0;
        work[0] += fl;
        work[1] += 2.0 * m * k - k * k;
        work[2] += u * u;
        if (f.m > KVX_LU_LDS_M) { work[3] += 1.0; work[4] += fl; }
    }
    return KVX_OK;
}

static int kvx_lu_extract_impl(kvx_lu_num *N, int64_t *lnz, int64_t **Lp, int64_t **Li, double **Lx, int64_t *unz, int64_t **Up,
                   int64_t **Ui, double **Ux, int64_t *fnz, int64_t **Fp, int64_t **Fi, double **Fx, int64_t *P_out,
                   int64_t *Q_out, double *Rs, int64_t *nblocks, int64_t **r_out)
{
    if (!N || !lnz || !Lp || !Li || !Lx || !unz || !Up || !Ui || !Ux || !fnz || !Fp || !Fi || !Fx || !P_out || !Q_out || !Rs ||
        !nblocks || !r_out)
        return KVX_EINVAL;
    if (!N->factored) { set_last_error("singular matrix"); return KVX_ESINGULAR; }
    const LuPlan &P = N->P;
    const int64_t n = N->n;
    std::vector<double> hL((size_t)P.lsize), hU((size_t)P.lsize), rinv((size_t)n);
    std::vector<int32_t> lperm((size_t)n);
    HIPCHK(hipMemcpy(hL.data(), N->S.Lx, (size_t)P.lsize * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hU.data(), N->S.Ux, (size_t)P.lsize * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(rinv.data(), N->M.rinv, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(lperm.data(), N->S.lperm, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int64_t> finalpos((size_t)n);
    for (int64_t f = 0; f < P.nfront; f++) {
        const int32_t p0 = P.fr[f].p0, k = P.fr[f].k;
        for (int32_t t = 0; t < k; t++) {
            finalpos[p0 + lperm[p0 + t]] = p0 + t;
            P_out[p0 + t] = P.prow[p0 + lperm[p0 + t]];
        }
    }
    for (int64_t j = 0; j < n; j++) { Q_out[j] = P.qcol[j]; Rs[j] = 1.0 / rinv[P_out[j]]; }
    std::vector<Trip> tl, tu;
    tl.reserve((size_t)P.lnz_bound);
    tu.reserve((size_t)P.unz_bound);
    for (int64_t f = 0; f < P.nfront; f++) {
        const int32_t p0 = P.fr[f].p0, k = P.fr[f].k, m = P.fr[f].m;
        const int32_t *rows = P.rowidx.data() + P.rowptr[f];
        const double *lp = hL.data() + P.px[f], *upn = hU.data() + P.px[f];
        for (int32_t t = 0; t < k; t++) {
            tl.push_back({p0 + t, p0 + t, 1.0});
            for (int32_t i = t + 1; i < m; i++) {
                const double v = lp[i + (int64_t)t * m];
                if (v != 0.0) tl.push_back({i < k ? (int64_t)(p0 + i) : finalpos[rows[i]], p0 + t, v});
            }
            for (int32_t i = t; i < m; i++) {
                const double v = upn[i + (int64_t)t * m];
                if (v != 0.0 || i == t) tu.push_back({p0 + t, i < k ? (int64_t)(p0 + i) : (int64_t)rows[i], v});
            }
        }
    }
    std::vector<int64_t> lp_, li_, up_, ui_;
    std::vector<double> lx_, ux_;
    to_ccs(n, tl, lp_, li_, lx_);
    to_ccs(n, tu, up_, ui_, ux_);
    *lnz = (int64_t)li_.size();
    *unz = (int64_t)ui_.size();
    // F: the off-diagonal blocks, rows in final pivotal order (the in-front interchanges permute them with their rows)
    std::vector<Trip> tf;
    {
        std::vector<double> hF(P.fcol.size());
        if (!hF.empty()) HIPCHK(hipMemcpy(hF.data(), N->S.fval_r, hF.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t pr = 0; pr < n; pr++)
            for (int64_t e = P.fptr_r[pr]; e < P.fptr_r[pr + 1]; e++)
                if (hF[(size_t)e] != 0.0) tf.push_back({finalpos[pr], (int64_t)P.fcol[(size_t)e], hF[(size_t)e]});
    }
    std::vector<int64_t> fp_, fi_;
    std::vector<double> fx_;
    to_ccs(n, tf, fp_, fi_, fx_);
    *fnz = (int64_t)fi_.size();
    *nblocks = (int64_t)P.rblocks.size() - 1;
    *Lp = mdup(lp_); *Li = mdup(li_); *Lx = mdup(lx_);
    *Up = mdup(up_); *Ui = mdup(ui_); *Ux = mdup(ux_);
    *Fp = mdup(fp_); *Fi = mdup(fi_); *Fx = mdup(fx_);
    *r_out = mdup(P.rblocks);
    if (!*Lp || !*Li || !*Lx || !*Up || !*Ui || !*Ux || !*Fp || !*Fi || !*Fx || !*r_out) return KVX_ENOMEM;
    return KVX_OK;
}

int kvx_lu_extract(kvx_lu_num *N, int64_t *lnz, int64_t **Lp, int64_t **Li, double **Lx, int64_t *unz, int64_t **Up,
                   int64_t **Ui, double **Ux, int64_t *fnz, int64_t **Fp, int64_t **Fi, double **Fx, int64_t *P_out,
                   int64_t *Q_out, double *Rs, int64_t *nblocks, int64_t **r_out)
{
    return guarded([&] { return kvx_lu_extract_impl(N, lnz, Lp, Li, Lx, unz, Up, Ui, Ux, fnz, Fp, Fi, Fx, P_out, Q_out, Rs, nblocks, r_out); });
}

// Determinant as the reference computes it (klu.c:760-822): prod(Udiag[k] * Rs[k]) times the signs of P and Q.
static int kvx_lu_det_impl(kvx_lu_num *N, double *det)
{
    if (!N || !det) return KVX_EINVAL;
    if (!N->factored) { set_last_error("singular matrix"); return KVX_ESINGULAR; }
    const LuPlan &P = N->P;
    const int64_t n = N->n;
    int rc = ensure_rhs(N, 1);
    if (rc) return rc;
    launch_lu_udiag(N->D, (int)P.nfront, N->R.X, N->st);
    std::vector<double> ud((size_t)n), rinv((size_t)n);
    std::vector<int32_t> lperm((size_t)n);
    HIPCHK(hipMemcpyAsync(ud.data(), N->R.X, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, N->st));
    HIPCHK(hipMemcpyAsync(rinv.data(), N->M.rinv, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, N->st));
    HIPCHK(hipMemcpyAsync(lperm.data(), N->S.lperm, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, N->st));
    HIPCHK(hipStreamSynchronize(N->st));
    std::vector<int64_t> pf((size_t)n);
    for (int64_t f = 0; f < P.nfront; f++)
        for (int32_t t = 0; t < P.fr[f].k; t++) pf[P.fr[f].p0 + t] = P.prow[P.fr[f].p0 + lperm[P.fr[f].p0 + t]];
    double dd = 1.0;
    for (int64_t k = 0; k < n; k++) dd *= ud[k] / rinv[pf[k]];
    int64_t npiv = 0;
    std::vector<int64_t> w;
    for (int pass = 0; pass < 2; pass++) {
        w = pass ? P.qcol : pf;
        for (int64_t i = 0; i < n; i++)
            while (w[i] != i) { const int64_t t = w[w[i]]; w[w[i]] = w[i]; w[i] = t; npiv++; }
    }
    *det = (npiv & 1) ? -dd : dd;
    return KVX_OK;
}

int kvx_lu_det(kvx_lu_num *N, double *det)
{
    return guarded([&] { return kvx_lu_det_impl(N, det); });
}

int64_t kvx_dbg_lu_schedule(kvx_lu_sym *S, int64_t *out, int64_t cap)
{
    if (!S || cap < 0 || (cap > 0 && !out)) return -1;
    std::vector<int64_t> v;
    try {
        LuPlan P;
        lu_build_plan(S->Y, P);
        v.push_back(P.nlevels);
        for (int32_t l = 0; l < P.nlevels; l++) {
            const LuLevelSched &L = P.sched[(size_t)l];
            const int64_t b = P.levelptr[l], e = P.levelptr[l + 1];
            v.push_back(e - b);
            for (int64_t q = b; q < e; q++) { v.push_back(P.fr[P.levellist[q]].m); v.push_back(P.fr[P.levellist[q]].k); }
            v.push_back((int64_t)L.lds.size());
            for (const LuLdsLaunch &r : L.lds) v.insert(v.end(), {r.first - b, r.count, r.cls, r.side});
            v.insert(v.end(), {L.big_first - b, L.big_count, L.bm, L.bk, (int64_t)L.steps.size()});
            for (const LuBigStep &s : L.steps) v.insert(v.end(), {s.jb, s.width, s.lds_work});
        }
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
    if ((int64_t)v.size() <= cap) std::copy(v.begin(), v.end(), out);
    return (int64_t)v.size();
}

}  // extern "C"
