// The numeric factorisation of the sparse LU path: the level loop over the plan's schedule (lu_symbolic.hpp LuLevelSched), its
// launch graph, and the merge-and-retry loop around it.
#include "lu_internal.hpp"

// Run `body` (enqueues on N->st, forks to the side streams by events and joins them again) from a launch graph: replayed when
// `g` was captured under the same key, captured when the key of the previous call comes again, launch by launch otherwise.
// Whatever goes wrong with capture or instantiation turns the graphs of this factor off; the launches then go out one by one.
int run_graphed(kvx_lu_num *N, LuGraph &g, LuGraphKey key, const std::function<int()> &body)
{
    if (!N->graphs_on) return body();
    key.version = N->version;
    if (g.exec && g.key == key) {
        HIPCHK(hipGraphLaunch(g.exec, N->st));
        N->graph_replays++;
        return KVX_OK;
    }
    // A capture and an instantiation cost milliseconds: a caller that hands over another buffer at every call must not pay them
    // every time.  The launches go out one by one until the same key comes twice in a row.
    const bool again = g.seen == key && key.ptr != nullptr;
    g.seen = key;
    if (!again) return body();
    g.drop();
    if (hipStreamBeginCapture(N->st, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); N->graphs_on = false; return body(); }
    const int rc = body();
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(N->st, &graph);
    if (rc || e != hipSuccess || !graph) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        N->graphs_on = false;
        return rc ? rc : body();
    }
    const hipError_t ei = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) { (void)hipGetLastError(); g.exec = nullptr; N->graphs_on = false; return body(); }
    g.key = key;
    HIPCHK(hipGraphLaunch(g.exec, N->st));
    return KVX_OK;
}

namespace {

// One numeric pass over the current plan.
int enqueue_pass(kvx_lu_num *N, const double *Ax_dev, int reuse)
{
    const LuPlan &P = N->P;
    const LuDev &d = N->D;
    const LuStructD &S = N->S;
    launch_lu_zero(N->n, N->M.rmax, N->st);                       // (a kernel, not a memset node of the launch graph)
    launch_lu_rowmax(N->nnz, N->M.ai32, Ax_dev, N->M.rmax, N->st);
    launch_lu_rinv(N->n, N->M.rmax, N->M.rinv, N->st);
    launch_lu_fvals((int64_t)P.fcol.size(), S.fsrc_r, Ax_dev, N->M.rinv, N->M.ai32, S.fval_r, N->st);
    launch_lu_fvals((int64_t)P.fcol.size(), S.fsrc_c, Ax_dev, N->M.rinv, N->M.ai32, S.fval_c, N->st);
    HIPCHK(hipEventRecord(N->ev0, N->st));
    HIPCHK(hipStreamWaitEvent(N->st2, N->ev0, 0));
    int32_t lastA = -1, lastB = -1;                            // deepest-so-far levels with work recorded on st / st2
    for (int32_t l = P.nlevels - 1; l >= 0; l--) {
        const LuLevelSched &L = P.sched[(size_t)l];
        const LuLevelEvents &E = N->ev[(size_t)l];
        const bool hasA = !L.lds.empty(), hasB = L.big_count > 0;
        // everything of the levels below must be complete: each stream waits for the other's latest record
        if (hasA && lastB >= 0) HIPCHK(hipStreamWaitEvent(N->st, N->ev[(size_t)lastB].B, 0));
        if (hasB && lastA >= 0) HIPCHK(hipStreamWaitEvent(N->st2, N->ev[(size_t)lastA].A, 0));
        for (size_t i = 0; i < L.lds.size(); i++) {           // independent launches, each as long as its slowest front: alternate streams
            const LuLdsLaunch &r = L.lds[i];
            if (i == 1) {                                     // the first one that goes to st3: fork
                HIPCHK(hipEventRecord(E.C, N->st));
                HIPCHK(hipStreamWaitEvent(N->st3, E.C, 0));
            }
            launch_lu_fronts(d, S.lists + r.first, r.count, r.cls, lu_front_kernel(N->K, r.count, d.arena_size), 0, Ax_dev, N->tol, N->stol,
                             reuse, r.side ? N->st3 : N->st);
        }
        if (L.lds.size() > 1) {
            HIPCHK(hipEventRecord(E.D, N->st3));
            HIPCHK(hipStreamWaitEvent(N->st, E.D, 0));
        }
        if (hasB && N->K.unblocked)
            launch_lu_fronts(d, S.lists + L.big_first, L.big_count, 0, LU_FRONT_TILED, L.bk, Ax_dev, N->tol, N->stol, reuse, N->st2);
        else if (hasB) {                                      // big fronts of the level: blocked multi-launch path
            const uint8_t *sw = (reuse && (size_t)l < N->swap_steps.size() && !N->swap_steps[(size_t)l].empty()) ? N->swap_steps[(size_t)l].data() : nullptr;
            launch_lu_big_level(d, S.lists + L.big_first, L, Ax_dev, N->tol, N->stol, reuse, N->st2, sw);
            // diagnostics: the k_lub_panel launches of this level in which a front really has more than 4096 rows left
            for (const LuBigStep &s : L.steps)
                if (s.lds_work) lu_count(LU_CNT_PANEL_LDS_WORK);
        }
        if (hasA) { HIPCHK(hipEventRecord(E.A, N->st)); lastA = l; }
        if (hasB) { HIPCHK(hipEventRecord(E.B, N->st2)); lastB = l; }
    }
    if (lastB >= 0) HIPCHK(hipStreamWaitEvent(N->st, N->ev[(size_t)lastB].B, 0));
    else if (!N->ev.empty()) {                                    // st2 forked from st above: joined again whether or not it got work
        HIPCHK(hipEventRecord(N->ev[0].B, N->st2));
        HIPCHK(hipStreamWaitEvent(N->st, N->ev[0].B, 0));
    }
    HIPCHK(hipGetLastError());
    return KVX_OK;
}

// fail_host receives the per-front flags.
int numeric_pass(kvx_lu_num *N, const double *Ax_dev, int reuse, std::vector<int32_t> &fail_host)
{
    const LuPlan &P = N->P;
    // the events of the level schedule exist before anything is captured
    while ((int32_t)N->ev.size() < P.nlevels) {
        LuLevelEvents E;
        for (hipEvent_t *e : {&E.A, &E.B, &E.C, &E.D}) HIPCHK(pool_event_get(e, false));
        N->ev.push_back(E);
    }
    int rc;
    if (reuse) rc = run_graphed(N, N->g_pass, {Ax_dev, (int64_t)N->swap_version, 0}, [&] { return enqueue_pass(N, Ax_dev, reuse); });   // the steady state: replayed
    else rc = enqueue_pass(N, Ax_dev, reuse);
    if (rc) return rc;
    if (N->K.timing) fprintf(stderr, "  lu   (pass enqueued, %d levels)\n", (int)P.nlevels);
    fail_host.resize((size_t)P.nfront);
    HIPCHK(hipMemcpyAsync(fail_host.data(), N->S.fail, (size_t)P.nfront * sizeof(int32_t), hipMemcpyDeviceToHost, N->st));
    HIPCHK(hipStreamSynchronize(N->st));
    N->attempts++;
    return KVX_OK;
}

// After a factorisation that chose its pivots: which pivot blocks of the blocked fronts interchange rows at all (the blocks are
// the steps of the level's schedule, those that launch_lu_big_level runs).
int refresh_swap_steps(kvx_lu_num *N)
{
    const LuPlan &P = N->P;
    N->swap_version++;                                            // (the launches of a refactorisation depend on these flags)
    N->swap_steps.assign((size_t)P.nlevels, {});
    if (N->K.unblocked) return KVX_OK;
    if (std::none_of(P.sched.begin(), P.sched.end(), [](const LuLevelSched &L) { return L.big_count > 0; })) return KVX_OK;
    std::vector<int32_t> ipiv((size_t)N->n);
    HIPCHK(hipMemcpy(ipiv.data(), N->S.ipiv, (size_t)N->n * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int32_t l = 0; l < P.nlevels; l++) {
        const LuLevelSched &L = P.sched[(size_t)l];
        for (const LuBigStep &s : L.steps) {
            uint8_t any = 0;
            for (int64_t q = L.big_first; q < L.big_first + L.big_count && !any; q++) {
                const LuFrontH &f = P.fr[P.levellist[q]];
                for (int t = s.jb; t < std::min(s.jb + s.width, (int)f.k) && !any; t++) any = ipiv[(size_t)f.p0 + t] != 0;
            }
            N->swap_steps[(size_t)l].push_back(any);
        }
    }
    return KVX_OK;
}

}  // namespace

// Factor with the merge-and-retry loop of lu_symbolic.hpp (4).
int factor_loop(kvx_lu_num *N, const double *Ax_dev, int reuse)
{
    N->factored = false;
    if (N->sym->Y.structurally_singular) {
        set_last_error("singular matrix (structurally rank deficient)");
        return KVX_ESINGULAR;
    }
    std::vector<int32_t> fail;
    LuLap tl{N->K.timing};
    for (int iter = 0; iter < 100000; iter++) {
        int rc = numeric_pass(N, Ax_dev, reuse, fail);
        if (rc) return rc;
        tl.lap("numeric pass");
        const LuPlan &P = N->P;
        std::vector<int32_t> minimal;
        std::vector<char> below((size_t)P.nfront, 0);
        for (int64_t f = 0; f < P.nfront; f++) {
            const bool flagged = fail[f] != 0;
            if (flagged && !below[f]) minimal.push_back((int32_t)f);
            if ((flagged || below[f]) && P.fr[f].parent >= 0) below[P.fr[f].parent] = 1;
        }
        if (minimal.empty()) {
            N->factored = true;
            if (!reuse && (rc = refresh_swap_steps(N))) return rc;
            return KVX_OK;
        }
        if (reuse) { reuse = 0; continue; }                   // klu.c:296-303: a refactorisation that runs into numerical trouble becomes a full one
        if (!lu_merge_fronts(N->sym->Y, P, minimal)) {
            set_last_error("singular matrix");
            return KVX_ESINGULAR;
        }
        tl.lap("merge fronts");
        if ((rc = upload_structure(N))) return rc;
        tl.t = std::chrono::steady_clock::now();
    }
    set_last_error("singular matrix");
    return KVX_ESINGULAR;
}
