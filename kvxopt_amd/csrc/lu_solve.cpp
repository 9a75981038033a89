// The solves of the sparse LU path: the sweeps over the plan's stages, the refinement around them, and the one body that the four
// solve entry points (plain / refined, host / device memory) share.
#include "lu_internal.hpp"

namespace {

// The solution overwrites B, or goes to Out (B is then only read).
int enqueue_solve(kvx_lu_num *N, int trans, double *B_dev, int64_t nrhs, int64_t ldB, double *Out_dev = nullptr, int64_t ldOut = 0)
{
    if (!Out_dev) { Out_dev = B_dev; ldOut = ldB; }
    const LuPlan &P = N->P;
    const LuDev &d = N->D;
    const LuStructD &S = N->S;
    const int64_t n = N->n;
    double *X = N->R.X, *W = N->R.W;
    // A x = b:  L U (Q' x) = R P b         A' x = b:  U' L' (R^-1 P x) = Q' b
    if (!trans) launch_lu_gather(n, (int)nrhs, S.prow, N->M.rinv, B_dev, ldB, X, n, N->st);
    else launch_lu_gather(n, (int)nrhs, S.qcol, nullptr, B_dev, ldB, X, n, N->st);
    // block levels (one without BTF); inside a level the stages are the tree depths of its blocks: forward sweep leaves ->
    // roots, backward sweep roots -> leaves.  A x = b walks the block levels upwards (a block after the later blocks its rows
    // touch), A' x = b downwards; the products with the off-diagonal blocks F come first.
    auto sweep = [&](int32_t t, bool fwd, int unit) {
        const int64_t sb = P.stageptr[t], se = P.stageptr[t + 1], nb = P.stage_nbig[t];
        if (fwd) {
            launch_lu_fwd(d, S.slists + sb, (int)(se - nb - sb), P.stage_smallm[t], P.stage_smallk[t], unit, X, n, (int)nrhs, W, P.wsize, N->st);
            launch_lu_fwd_big(d, S.slists + se - nb, (int)nb, P.stage_bigm[t], P.stage_bigk[t], unit, X, n, (int)nrhs, W, P.wsize, N->st);
        } else {
            launch_lu_bwd(d, S.slists + sb, (int)(se - nb - sb), P.stage_smallm[t], P.stage_smallk[t], unit, X, n, (int)nrhs, N->st);
            launch_lu_bwd_big(d, S.slists + se - nb, (int)nb, P.stage_bigm[t], P.stage_bigk[t], unit, X, n, (int)nrhs, W, P.wsize, N->st);
        }
    };
    for (int32_t li = 0; li < P.nblev; li++) {
        const int32_t l = trans ? P.nblev - 1 - li : li;
        if (P.nblev > 1 && !P.fcol.empty()) {
            const int64_t cnt = P.flevptr[l + 1] - P.flevptr[l];
            if (!trans) launch_lu_fterm(cnt, (int)nrhs, S.flevpos + P.flevptr[l], S.fptr_r, S.fcol, S.fval_r, X, n, N->st);
            else launch_lu_fterm(cnt, (int)nrhs, S.flevpos + P.flevptr[l], S.fptr_c, S.frow, S.fval_c, X, n, N->st);
        }
        for (int32_t t = P.levstage[l + 1] - 1; t >= P.levstage[l]; t--) sweep(t, true, trans ? 0 : 1);
        for (int32_t t = P.levstage[l]; t < P.levstage[l + 1]; t++) sweep(t, false, trans ? 1 : 0);
    }
    if (!trans) launch_lu_scatter(n, (int)nrhs, S.qcol, nullptr, X, n, Out_dev, ldOut, N->st);
    else launch_lu_scatter(n, (int)nrhs, S.prow, N->M.rinv, X, n, Out_dev, ldOut, N->st);
    HIPCHK(hipGetLastError());
    return KVX_OK;
}

// x <- solve(b), then up to `steps` corrections, each kept only if it lowers the componentwise backward error of its column
// (lu_refine.hip).  b stays in B until the last launch writes the result there; nothing is read back between the steps.
int enqueue_refine(kvx_lu_num *N, int trans, double *B_dev, int64_t nrhs, int64_t ldB, int64_t steps)
{
    const int64_t n = N->n;
    const int nr = (int)nrhs;
    const LuRefineD &F = N->RF;
    const int64_t *rp = trans ? N->RM.ap : N->RM.csrp;            // the CCS is the row-wise view of A'
    const int32_t *ci = trans ? N->M.ai32 : N->RM.csrc, *src = trans ? nullptr : N->RM.csrs;
    int rc = enqueue_solve(N, trans, B_dev, nrhs, ldB, F.rx, n);
    if (rc) return rc;
    launch_lu_resid(n, nr, rp, ci, src, N->M.Ax, B_dev, ldB, F.rx, n, nullptr, 0, F.rd[0], n, F.ratio, N->st);
    launch_lu_berr(n, nr, F.ratio, F.part, F.om[0], 1, F.berr, 2, F.act[0], N->st);
    if (steps == 0)                                               // (only the backward error was asked for)
        launch_lu_accept(n, nr, F.rx, n, nullptr, 0, B_dev, ldB, F.om[0], F.act[0], nullptr, nullptr, nullptr, F.berr + 1, 2, N->st);
    for (int64_t s = 0; s < steps; s++) {
        double *d = F.rd[s & 1], *rnext = F.rd[(s + 1) & 1];
        const bool last = s == steps - 1;
        if ((rc = enqueue_solve(N, trans, d, nrhs, n))) return rc;
        launch_lu_resid(n, nr, rp, ci, src, N->M.Ax, B_dev, ldB, F.rx, n, d, n, rnext, n, F.ratio, N->st);
        launch_lu_berr(n, nr, F.ratio, F.part, F.omc, 1, nullptr, 0, nullptr, N->st);
        launch_lu_accept(n, nr, F.rx, n, d, n, last ? B_dev : F.rx, last ? ldB : n, F.om[s & 1], F.act[s & 1], F.omc, F.om[(s + 1) & 1],
                         F.act[(s + 1) & 1], last ? F.berr + 1 : nullptr, 2, N->st);
    }
    HIPCHK(hipGetLastError());
    return KVX_OK;
}

}  // namespace

int lu_solve_any(kvx_lu_num *N, bool host, int trans, double *B, int64_t nrhs, int64_t ldB, int64_t steps, double *berr_out)
{
    const bool plain = steps == 0 && !berr_out;                   // the plain solve: its own launches, its own graph key, the same bits
    // (the entry points differ in where a null B is turned away: the plain solve from device memory never looks, the plain
    // solve from host memory looks first, the refined ones look last)
    if (!N || (trans != 0 && trans != 1) || nrhs < 0 || ldB < std::max<int64_t>(1, N->n)) return KVX_EINVAL;
    if (plain ? host && !B : steps < 0 || steps >= ((int64_t)1 << 20)) return KVX_EINVAL;
    if (!N->factored) { set_last_error("singular matrix"); return KVX_ESINGULAR; }
    if (!plain) {
        if (nrhs > 65535) { set_last_error("a refined solve takes at most 65535 right-hand sides at a time"); return KVX_EINVAL; }
        if (!N->have_vals) {
            set_last_error("refined solve: this factor was made from device values and its analysis has no KVX_LU_FLAG_KEEP_VALUES");
            return KVX_EINVAL;
        }
        if (N->sym->Y.csr_ptr.empty()) { set_last_error("refined solve: more than 2^31-1 entries"); return KVX_EINVAL; }
        if (!B) return KVX_EINVAL;
    }
    if (nrhs == 0) return KVX_OK;
    int rc = ensure_rhs(N, nrhs);
    if (!rc && !plain) rc = ensure_refine(N, nrhs);
    if (!rc && !host) rc = lu_wait_for_caller(N);
    if (rc) return rc;
    const int64_t n = N->n, ld = host ? n : ldB;
    double *Bd = host ? N->R.B : B;
    const size_t col = (size_t)n * sizeof(double);
    if (host) HIPCHK(hipMemcpy2DAsync(Bd, col, B, (size_t)ldB * sizeof(double), col, (size_t)nrhs, hipMemcpyHostToDevice, N->st));
    if (plain) rc = run_graphed(N, N->g_solve[trans], {Bd, nrhs, ld}, [&] { return enqueue_solve(N, trans, Bd, nrhs, ld); });
    else rc = run_graphed(N, N->g_refine[trans], {Bd, nrhs | (steps << 32), ld}, [&] { return enqueue_refine(N, trans, Bd, nrhs, ld, steps); });
    if (rc) return rc;
    if (host) HIPCHK(hipMemcpy2DAsync(B, (size_t)ldB * sizeof(double), Bd, col, col, (size_t)nrhs, hipMemcpyDeviceToHost, N->st));
    if (berr_out) HIPCHK(hipMemcpyAsync(berr_out, N->RF.berr, (size_t)(2 * nrhs) * sizeof(double), hipMemcpyDeviceToHost, N->st));
    HIPCHK(hipStreamSynchronize(N->st));
    return KVX_OK;
}
