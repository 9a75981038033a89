// The triangular solves: the level sweeps, the rhs-major form for many right-hand sides, factorisation and solve as one enqueue,
// sparse right-hand sides.
#include "chol_internal.hpp"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <vector>

namespace kvx {

// Fork the independent kernel groups of one level onto the side streams; join at level end.
struct LevelStreams {
    SweepStreams S;
    hipStream_t lds, wave;
    bool fork_lds, fork_wave;
    static SweepStreams own(kvx_chol *F)
    {
        if (F->K.solve_nofork) return SweepStreams{F->stream, F->stream, F->stream, F->ev_fork, F->ev_join[0], F->ev_join[1]};
        return SweepStreams{F->stream, F->side[0], F->side[1], F->ev_fork, F->ev_join[0], F->ev_join[1]};
    }
    LevelStreams(kvx_chol *F, bool have_big, bool have_lds, bool have_wave, const SweepStreams *ss = nullptr) : S(ss ? *ss : own(F))
    {
        fork_lds = have_lds && (have_big || have_wave) && S.lds != S.main;
        fork_wave = have_wave && have_big && S.wave != S.main;
        lds = fork_lds ? S.lds : S.main;
        wave = fork_wave ? S.wave : S.main;
        if (fork_lds || fork_wave) {
            (void)hipEventRecord(S.fork, S.main);
            if (fork_lds) (void)hipStreamWaitEvent(S.lds, S.fork, 0);
            if (fork_wave) (void)hipStreamWaitEvent(S.wave, S.fork, 0);
        }
    }
    void join()
    {
        if (fork_lds) { (void)hipEventRecord(S.join0, S.lds); (void)hipStreamWaitEvent(S.main, S.join0, 0); }
        if (fork_wave) { (void)hipEventRecord(S.join1, S.wave); (void)hipStreamWaitEvent(S.main, S.join1, 0); }
    }
};

void enqueue_fwd(kvx_chol *F, double *X, int64_t ldx, int nrhs, int lfrom, int lto, const SweepStreams *ss, bool wait_levels, bool sub_tail)
{
    Symbolic &S = F->S;
    const int64_t wstride = std::max(S.wrk_size[0], S.wrk_size[1]);
    hipStream_t sm = ss ? ss->main : F->stream;
    if (lfrom < 0) lfrom = S.nlevels - 1;
    if (lfrom == S.nlevels - 1 && F->nsub > 0 && !wait_levels) {       // the leaf subtrees: one wavefront each, before any level
        ProfScope ps(F, FAM_FWD, sm);
        launch_fwd_subtree(sm, F->ds, F->d_subs, F->nsub, F->d_cd_woff, F->d_Lx, X, ldx, nrhs, F->d_W[0], F->d_W[1], wstride, F->d_depth);
    }
    if (wait_levels && sub_tail && F->nsub > 0) {
        // the part of the tree at level lto and below is factored: its subtrees (the groups are stored by ascending level) in one launch
        (void)hipStreamWaitEvent(sm, F->ev_lvl[(size_t)lto], 0);
        const int off = F->sub_lvl_off[(size_t)lto];
        launch_fwd_subtree(sm, F->ds, F->d_subs_lvl + off, F->nsub - off, F->d_cd_woff, F->d_Lx, X, ldx, nrhs, F->d_W[0], F->d_W[1], wstride, F->d_depth);
    }
    for (int l = lfrom; l >= lto; l--) {
        const LevelPlan &P = F->plan[l];
        const double *Wch = F->d_W[(l + 1) & 1];
        double *Wout = F->d_W[l & 1];
        const int64_t woff = F->sw_off[l];
        const int wcnt = F->sw_cnt[l];
        const int nlds = F->solve_merged ? 0 : P.scnt[1];
        const int nsubl = (wait_levels && !sub_tail && F->nsub > 0) ? F->sub_lvl_cnt[(size_t)l] : 0;
        if (wcnt == 0 && P.scnt[0] == 0 && nlds == 0 && nsubl == 0) continue;
        if (wait_levels) (void)hipStreamWaitEvent(sm, F->ev_lvl[(size_t)l], 0);         // level l (and every deeper one) is factored
        if (nsubl > 0)      // behind a factorisation in flight: the subtrees ROOTED at this level (their fronts are at this depth or deeper)
            launch_fwd_subtree(sm, F->ds, F->d_subs_lvl + F->sub_lvl_off[(size_t)l], nsubl, F->d_cd_woff, F->d_Lx, X, ldx, nrhs, F->d_W[0], F->d_W[1],
                               wstride, F->d_depth);
        if (wcnt == 0 && P.scnt[0] == 0 && nlds == 0) continue;
        // with subtrees: every small front of the level that is outside them goes into ONE launch of the LDS kernel;
        // without (sharded mode): the wave classes keep their own kernel and stream
        LevelStreams ls(F, P.scnt[0] > 0, F->solve_merged ? wcnt > 0 : nlds > 0, F->solve_merged ? false : wcnt > 0, ss);
        if (wcnt > 0) {
            if (F->solve_merged) {
                ProfScope ps(F, FAM_FWD, ls.lds);
                launch_fwd_lds(ls.lds, F->ds, F->d_lists_sw + woff, wcnt, F->sw_kmax[l], F->d_Lx, X, ldx, nrhs, Wch, Wout, wstride);
            } else {
                ProfScope ps(F, FAM_FWD, ls.wave);
                launch_fwd_wave(ls.wave, F->ds, F->d_lists_sw + woff, wcnt, F->sw_kmax[l], F->d_Lx, X, ldx, nrhs, Wch, Wout, wstride);
            }
        }
        if (nlds > 0) {
            ProfScope ps(F, FAM_FWD, ls.lds);
            launch_fwd_lds(ls.lds, F->ds, F->d_lists + P.soff[1], nlds, std::max(P.maxk[KVX_CLS_LDS128], P.maxk[KVX_CLS_LDS96]),
                           F->d_Lx, X, ldx, nrhs, Wch, Wout, wstride);
        }
        if (P.scnt[0] > 0) {
            ProfScope ps(F, FAM_FWD, sm);
            launch_fwd_big(sm, F->ds, F->d_lists + P.soff[0], P.scnt[0], P.smaxm[0], P.big_maxk, F->d_Lx, F->d_Linv,
                           X, F->d_X0, ldx, nrhs, F->d_WK, S.n, Wch, Wout, wstride, P.scnt[0]);
        }
        ls.join();
    }
}

void enqueue_bwd(kvx_chol *F, double *X, int64_t ldx, int nrhs, int lfrom, int lto)
{
    Symbolic &S = F->S;
    if (lto < 0) lto = S.nlevels - 1;
    for (int l = lfrom; l <= lto; l++) {
        const LevelPlan &P = F->plan[l];
        const int64_t woff = F->sw_off[l];
        const int wcnt = F->sw_cnt[l];
        const int nlds = F->solve_merged ? 0 : P.scnt[1];
        if (wcnt == 0 && P.scnt[0] == 0 && nlds == 0) continue;
        LevelStreams ls(F, P.scnt[0] > 0, F->solve_merged ? wcnt > 0 : nlds > 0, F->solve_merged ? false : wcnt > 0);
        if (wcnt > 0) {
            if (F->solve_merged) {
                ProfScope ps(F, FAM_BWD, ls.lds);
                launch_bwd_lds(ls.lds, F->ds, F->d_lists_sw + woff, wcnt, F->d_Lx, X, ldx, nrhs);
            } else {
                ProfScope ps(F, FAM_BWD, ls.wave);
                launch_bwd_wave(ls.wave, F->ds, F->d_lists_sw + woff, wcnt, F->sw_maxm[l], 32, F->d_Lx, X, ldx, nrhs);
            }
        }
        if (nlds > 0) {
            ProfScope ps(F, FAM_BWD, ls.lds);
            launch_bwd_lds(ls.lds, F->ds, F->d_lists + P.soff[1], nlds, F->d_Lx, X, ldx, nrhs);
        }
        if (P.scnt[0] > 0) {
            ProfScope ps(F, FAM_BWD);
            launch_bwd_big(F->stream, F->ds, F->d_lists + P.soff[0], P.scnt[0], P.smaxm[0], P.big_maxk, F->d_Lx, F->d_Linv,
                           X, ldx, nrhs, F->d_WK, S.n);
        }
        ls.join();
    }
    if (lto == S.nlevels - 1 && F->nsub > 0) {        // the leaf subtrees last: every ancestor is solved
        if (nrhs == 1 && F->prof_family < 0) {
            // one right-hand side: the three size groups (registers for 32 / 48 / 64 rows of a column) side by side on three streams --
            // the walks of the largest group alone fit the GPU in one round instead of two to three for all of them in its kernel
            const int cnt[3] = {F->nsub32, F->nsub48 - F->nsub32, F->nsub - F->nsub48};
            const int off[3] = {0, F->nsub32, F->nsub48};
            const int cap[3] = {32, 48, 64};
            hipStream_t ss[3] = {F->stream, F->side[0], F->side[1]};
            const bool fork = (cnt[0] > 0) + (cnt[1] > 0) + (cnt[2] > 0) > 1;
            if (fork) {
                (void)hipEventRecord(F->ev_fork, F->stream);
                for (int g = 1; g < 3; g++)
                    if (cnt[g] > 0) (void)hipStreamWaitEvent(ss[g], F->ev_fork, 0);
            }
            for (int g = 2; g >= 0; g--)               // (the longest walks first)
                launch_bwd_subtree_group(fork ? ss[g] : F->stream, cap[g], F->ds, F->d_subs + off[g], cnt[g], F->d_Lx, X, ldx);
            if (fork)
                for (int g = 1; g < 3; g++)
                    if (cnt[g] > 0) { (void)hipEventRecord(F->ev_join[g - 1], ss[g]); (void)hipStreamWaitEvent(F->stream, F->ev_join[g - 1], 0); }
        } else {
            ProfScope ps(F, FAM_BWD);
            launch_bwd_subtree(F->stream, F->ds, F->d_subs, F->nsub, F->nsub32, F->d_Lx, X, ldx, nrhs);
        }
    }
}

// the small fronts of a level: the LDS classes (k <= 64) and the wave classes (k <= 32), each with the largest pivot count it holds
static void small_lists(const LevelPlan &P, int64_t off[2], int cnt[2], int kmax[2])
{
    off[0] = P.soff[1]; cnt[0] = P.scnt[1]; kmax[0] = std::max(P.maxk[KVX_CLS_LDS128], P.maxk[KVX_CLS_LDS96]);
    off[1] = P.soff[2]; cnt[1] = P.scnt[2]; kmax[1] = 0;
    for (int c = KVX_CLS_WAVE0; c < KVX_NCLS; c++) kmax[1] = std::max(kmax[1], P.maxk[c]);
}

void enqueue_fwd_wide(kvx_chol *F, double *XT, int nchunk)
{
    Symbolic &S = F->S;
    const int64_t wstride = std::max(S.wrk_size[0], S.wrk_size[1]);
    for (int l = S.nlevels - 1; l >= 0; l--) {
        const LevelPlan &P = F->plan[l];
        const double *Wch = F->d_W[(l + 1) & 1];
        double *Wout = F->d_W[l & 1];
        int64_t off[2]; int cnt[2], kmax[2];
        small_lists(P, off, cnt, kmax);
        if (cnt[0] == 0 && cnt[1] == 0 && P.scnt[0] == 0) continue;
        LevelStreams ls(F, P.scnt[0] > 0, cnt[0] > 0, cnt[1] > 0);
        for (int g = 0; g < 2; g++)
            if (cnt[g] > 0) {
                hipStream_t sg = g == 0 ? ls.lds : ls.wave;
                ProfScope ps(F, FAM_FWD, sg);
                launch_wide_fwd_small(sg, F->ds, F->d_lists + off[g], cnt[g], kmax[g], nchunk, F->d_Lx, XT, S.n, Wch, Wout, wstride,
                                      F->d_inv_ptr, F->d_inv_src);
            }
        if (P.scnt[0] > 0) {
            ProfScope ps(F, FAM_FWD);
            launch_wide_fwd_big(F->stream, F->ds, F->d_lists + P.soff[0], P.scnt[0], P.smaxm[0], P.big_maxk, nchunk, F->d_Lx, F->d_Linv,
                                XT, S.n, Wch, Wout, wstride, F->d_inv_ptr, F->d_inv_src);
        }
        ls.join();
    }
}

void enqueue_bwd_wide(kvx_chol *F, double *XT, int nchunk)
{
    Symbolic &S = F->S;
    for (int l = 0; l < S.nlevels; l++) {
        const LevelPlan &P = F->plan[l];
        int64_t off[2]; int cnt[2], kmax[2];
        small_lists(P, off, cnt, kmax);
        if (cnt[0] == 0 && cnt[1] == 0 && P.scnt[0] == 0) continue;
        LevelStreams ls(F, P.scnt[0] > 0, cnt[0] > 0, cnt[1] > 0);
        for (int g = 0; g < 2; g++)
            if (cnt[g] > 0) {
                hipStream_t sg = g == 0 ? ls.lds : ls.wave;
                ProfScope ps(F, FAM_BWD, sg);
                launch_wide_bwd_small(sg, F->ds, F->d_lists + off[g], cnt[g], kmax[g], nchunk, F->d_Lx, XT, S.n);
            }
        if (P.scnt[0] > 0) {
            ProfScope ps(F, FAM_BWD);
            launch_wide_bwd_big(F->stream, F->ds, F->d_lists + P.soff[0], P.scnt[0], P.big_maxk, nchunk, F->d_Lx, F->d_Linv, XT, S.n);
        }
        ls.join();
    }
}

// the graph slot of a sweep sequence, made at its first call (null: this call takes no graph)
static kvx_chol::SolveGraph *solve_graph_slot(kvx_chol *F, bool allowed, int kind, int nrhs)
{
    if (!allowed || !F->K.use_graph || getenv("KVX_DBG_NO_SOLVE_GRAPH")) return nullptr;
    for (auto &g : F->g_solve)
        if (g.kind == kind && g.nrhs == nrhs) return &g;
    F->g_solve.push_back({kind, nrhs, 0, LazyExec{}});
    return &F->g_solve.back();
}

// B_dev: n x nrhs, leading dimension ldB, device memory.
int solve_dev(kvx_chol *F, int sys, double *B, int64_t nrhs, int64_t ldB, bool async)
{
    Symbolic &S = F->S;
    const int64_t n = S.n;
    if (sys < 0 || sys > 8) { set_err("invalid value for sys"); return KVX_EINVAL; }
    // A factorisation still in flight on the factor's stream (kvx_chol_factorize_async_dev): the solve is queued
    // behind it at once -- no host round trip between the two -- and its status is examined when both are done
    // (on failure B holds garbage and the call reports the singular factor, as it would have before starting).
    const bool deferred = F->pending;
    int rc = KVX_OK;
    if (!deferred) {
        rc = finish_factor(F, nullptr);
        if (rc == KVX_ESYMBOLIC) { set_err("called with symbolic factor"); return rc; }
        if (rc == KVX_ENOTPOSDEF) { set_err("singular matrix"); return KVX_ESINGULAR; }
        if (rc) return rc;
    }
    if (n == 0 || nrhs == 0) return deferred ? ((rc = finish_factor(F, nullptr)) == KVX_ENOTPOSDEF ? KVX_ESINGULAR : rc) : KVX_OK;
    if (ldB < std::max<int64_t>(1, n)) { set_err("ldB must be >= max(1,n)"); return KVX_EINVAL; }
    if (sys == 6 && F->is_ll) return KVX_OK;   // D = I for an LL' factor
    hipStream_t st = F->stream;
    const bool ldl = !F->is_ll && sys >= 2 && sys <= 6;
    if (ldl && !F->diag_valid) {
        if (!F->d_diag) HIPCHK(pool_malloc((void **)&F->d_diag, (size_t)n * sizeof(double)));
        launch_extract_diag(st, F->ds, S.nsuper, F->d_Lx, F->d_diag);
        F->diag_valid = true;
    }
    // wstride: both parity buffers are allocated with wrk_size[p]*x_cap; use a common stride
    // many right-hand sides of a plain LL' system: rhs-major blocks of 64 (kernels_wide.hip)
    const int kind0 = (sys == 0 || sys == 1) ? 0 : ((sys == 2 || sys == 4) ? 1 : ((sys == 3 || sys == 5) ? 2 : -1));
    // A block of 64 costs the same whatever it holds, the older kernels grow with every right-hand side: measured break-even
    // (scratch/wide_thresh.py, 2-D grids) at 48 right-hand sides for n = 5e4, ~22 for n = 2.5e5, ~9 for n = 1e6.
    const bool wide_by_size = nrhs >= 48 || (nrhs >= 8 && (double)nrhs * (double)n >= 6e6);
    bool wide = kind0 >= 0 && F->prof_family < 0 && (F->K.wide_from < 0 ? wide_by_size : (F->K.wide_from > 0 && nrhs >= F->K.wide_from));
    if (wide) {
        if ((rc = ensure_wide(F))) return rc;
        wide = F->wide_state == 1;
    }
    // rhs-major passes: at most 1024 right-hand sides, fewer on very large systems (the workspace is a few blocks of n x pass doubles)
    const int wide_pass = (int)std::max<int64_t>(64, std::min<int64_t>(1024, ((int64_t)(1e9 / (double)std::max<int64_t>(n, 1)) / 64) * 64));
    const int chunk_max = wide ? wide_pass : 65535;
    for (int64_t r0 = 0; r0 < nrhs; r0 += chunk_max) {
        int nr = (int)std::min<int64_t>(chunk_max, nrhs - r0);
        double *Bc = B + r0 * ldB;
        if ((rc = ensure_solve_ws(F, wide ? (int64_t)((nr + 63) / 64) * 64 : nr))) return rc;
        HIPCHK(hipEventRecord(F->ev[2], st));
        if (wide) {
            const int nchunk = (nr + 63) / 64;
            // LDL' view: D L' x = b  ->  Lc' x = diag^-1 b;  L' x = b  ->  Lc' x = diag b (on the way in);
            //            L D x = b   ->  x = diag^-1 Lc^-1 b;  L x = b   ->  x = diag Lc^-1 b (on the way out)
            const bool sc_in = ldl && (sys == 3 || sys == 5), sc_out = ldl && (sys == 2 || sys == 4);
            launch_wide_gather(st, sys == 0 ? F->d_iperm : nullptr, n, nr, Bc, ldB, F->d_X, sc_in ? F->d_diag : nullptr, sys == 3 ? 1 : 0);
            auto body = [&]() -> int {
                if (kind0 == 0 || kind0 == 1) enqueue_fwd_wide(F, F->d_X, nchunk);
                if (kind0 == 0 || kind0 == 2) enqueue_bwd_wide(F, F->d_X, nchunk);
                return hipGetLastError() == hipSuccess ? KVX_OK : KVX_EDEVICE;
            };
            kvx_chol::SolveGraph *slot = solve_graph_slot(F, true, kind0 + 8, nchunk);
            if ((rc = capture_or_replay(F, slot, F->g_solve.size() <= 16, body))) return rc;
            launch_wide_scatter(st, sys == 0 ? F->d_iperm : nullptr, n, nr, F->d_X, Bc, ldB, sc_out ? F->d_diag : nullptr, sys == 2 ? 1 : 0);
            HIPCHK(hipEventRecord(F->ev[3], st));
            HIPCHK(hipGetLastError());
            continue;
        }
        // every system is solved on the staging block d_X (n x nr, ld = n): fixed pointers, so the
        // triangular sweeps can be replayed from a captured graph
        const int kind = kind0;
        if (sys == 0 || sys == 7) launch_perm_gather(st, F->d_perm, n, nr, Bc, ldB, F->d_X, n);
        else if (sys == 8) launch_perm_scatter(st, F->d_perm, n, nr, Bc, ldB, F->d_X, n);
        else HIPCHK(hipMemcpy2DAsync(F->d_X, n * sizeof(double), Bc, ldB * sizeof(double), n * sizeof(double), nr, hipMemcpyDeviceToDevice, st));
        // LDL' view: D L' x = b  ->  Lc' x = diag^-1 b;  L' x = b  ->  Lc' x = diag b;  D x = b  ->  x = diag^-2 b
        if (ldl && (sys == 3 || sys == 5 || sys == 6)) launch_diag_scale(st, n, nr, F->d_diag, F->d_X, n, sys == 3 ? 1 : (sys == 5 ? 0 : 2));
        if (kind >= 0) {
            auto body = [&]() -> int {
                if (kind == 0 || kind == 1) {
                    // the first forward step of a big front is spread over workgroups that all read the front's
                    // pivot entries of the rhs while one of them overwrites them with y: they read this copy
                    launch_copy_d(F->stream, F->d_X0, F->d_X, n * (int64_t)nr);         // (a kernel, not a memcpy node: see factor_prologue)
                    enqueue_fwd(F, F->d_X, n, nr);
                }
                if (kind == 0 || kind == 2) enqueue_bwd(F, F->d_X, n, nr);
                return hipGetLastError() == hipSuccess ? KVX_OK : KVX_EDEVICE;
            };
            kvx_chol::SolveGraph *slot = solve_graph_slot(F, F->prof_family < 0, kind, nr);
            if ((rc = capture_or_replay(F, slot, F->g_solve.size() <= 16, body))) return rc;
        }
        // L D x = b  ->  x = diag^-1 Lc^-1 b;  L x = b  ->  x = diag Lc^-1 b
        if (ldl && (sys == 2 || sys == 4)) launch_diag_scale(st, n, nr, F->d_diag, F->d_X, n, sys == 2 ? 1 : 0);
        if (sys == 0) launch_perm_scatter(st, F->d_perm, n, nr, F->d_X, n, Bc, ldB);
        else HIPCHK(hipMemcpy2DAsync(Bc, ldB * sizeof(double), F->d_X, n * sizeof(double), n * sizeof(double), nr, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipEventRecord(F->ev[3], st));
        HIPCHK(hipGetLastError());
    }
    if (async) {
        // no host synchronisation: the caller's (null-stream) work is ordered behind the solve by an event; a factorisation
        // that was still in flight stays pending and its status is examined at the next synchronising call
        HIPCHK(hipEventRecord(F->ev_out, st));
        HIPCHK(hipStreamWaitEvent(nullptr, F->ev_out, 0));
        return KVX_OK;
    }
    HIPCHK(hipStreamSynchronize(st));
    if (deferred) {
        rc = finish_factor(F, nullptr);
        if (rc == KVX_ENOTPOSDEF) { set_err("singular matrix"); return KVX_ESINGULAR; }
        if (rc) return rc;
    }
    prof_collect(F);
    float ms = 0;
    if (hipEventElapsedTime(&ms, F->ev[2], F->ev[3]) == hipSuccess) { F->ms_solve = ms; F->have_stime = true; }
    return KVX_OK;
}

// Numeric factorisation AND the solve of A X = B (sys 0) as ONE enqueue: the right-hand sides are known before the factorisation
// starts, so the forward sweep does not have to wait for all of it -- level l of the sweep needs the fronts of level l and below
// only.  The sweep runs on the stream of the factorisation's small-front launches (side[0], idle at the top of the tree) behind one event per level of the factorisation: by the
// time the root front is factored the sweep has reached the top of the tree, and what is left of it is the root's own step
// (config 2: 0.65 ms of forward sweep hidden under the pivot chain of the top levels).  Same kernels on the same data in the
// same order per front as kvx_chol_factorize_dev + kvx_chol_solve_dev: bitwise the same factor and solution.  The whole
// sequence replays from a captured graph from the second call with the same (nrhs, B, ldB) on.
int factor_solve_dev(kvx_chol *F, const double *values_dev, double *B, int64_t nrhs, int64_t ldB, bool async)
{
    int rc = ensure_device(F);
    if (rc) return rc;
    Symbolic &S = F->S;
    const int64_t n = S.n;
    if (nrhs < 0) { set_err("nrhs out of range"); return KVX_EINVAL; }
    if (n > 0 && nrhs > 0 && ldB < n) { set_err("ldB must be >= max(1,n)"); return KVX_EINVAL; }
    // outside the pipelined form: sharded factors, LDL' views, the rhs-major path of many right-hand sides, family timing
    // ... and HIP runtimes before 7.2: under 7.0.51831 (the one inside the PyTorch wheel, which a process gets when it imports torch
    // before this library) hipGraphLaunch of the captured five-stream sequence crashes inside the runtime (the three-stream graphs
    // of the separate calls replay correctly there); without a graph the pipelined form is slower than the two replayed graphs
    static const bool old_runtime = [] {
        int v = 0;
        if (hipRuntimeGetVersion(&v) != hipSuccess) { (void)hipGetLastError(); return true; }
        const char *e = getenv("KVX_DBG_FUSED_ANY_RUNTIME");          // debugging only: reproduces the crash of DESIGN.md section 5
        return v < 70200000 && !(e && e[0] == '1');
    }();
    // (KVX_FACTOR_SUBTREES=1 keeps the pipelined form since round 4 -- the subtree launches precede the level loop on the factor's
    //  stream, so a level's completion event covers them: config 4b's first direction 1.41 -> 1.29 ms, still behind the level
    //  schedule's 1.20-1.26; KVX_SUBTREES_PLAIN=1: two enqueues as before)
    const bool plain = F->dist_nranks != 1 || !F->is_ll || nrhs == 0 || nrhs > 16 || n == 0 || F->prof_family >= 0 || (F->factor_subtrees && getenv("KVX_SUBTREES_PLAIN")) ||
                       old_runtime || !F->K.use_graph;
    if ((rc = wait_for_caller(F))) return rc;
    if (S.nnzA > 0) HIPCHK(hipMemcpyAsync(F->d_Ax, values_dev, S.nnzA * sizeof(double), hipMemcpyDeviceToDevice, F->stream));
    F->last_fused_path = plain ? 2 : 1;
    if (plain) {
        if ((rc = enqueue_factor(F))) return rc;
        rc = solve_dev(F, 0, B, nrhs, ldB, async);
        // the factorisation was enqueued by THIS call: its failure is the call's result (KVX_ENOTPOSDEF and the failing column, as
        // the one-enqueue form and kvx_chol_factorize report it), not solve_dev's "singular matrix" for a factor found unusable.
        // (Enqueue-only form: the status stays deferred to kvx_chol_status, which reports KVX_ENOTPOSDEF too.)
        if (rc == KVX_ESINGULAR && !async && F->numeric && F->minor < S.n) { set_err("matrix is not positive definite"); return KVX_ENOTPOSDEF; }
        return rc;
    }
    const int nr = (int)nrhs;
    static const bool dbg_t = getenv("KVX_DBG_T") != nullptr;
    const auto t_in = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (dbg_t) fprintf(stderr, "factor_solve_dev %s: %.0f us\n", what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_in).count());
    };
    if ((rc = ensure_solve_ws(F, nr))) return rc;
    lap("solve workspace");
    if (F->ev_lvl.empty()) {
        F->ev_lvl.assign((size_t)S.nlevels, nullptr);
        for (auto &e : F->ev_lvl) HIPCHK(pool_event_get(&e, false));
        for (int i = 0; i < 4; i++) HIPCHK(pool_event_get(&F->ev_pipe[i], false));
        if (F->nsub > 0) {
            std::vector<std::vector<SubDesc>> by((size_t)S.nlevels);
            for (const SubDesc &d : F->subs_host) by[(size_t)S.depth[(size_t)d.hi]].push_back(d);      // (fronts of a subtree are numbered in postorder: hi is the root)
            std::vector<SubDesc> flat;
            F->sub_lvl_off.assign((size_t)S.nlevels, 0);
            F->sub_lvl_cnt.assign((size_t)S.nlevels, 0);
            for (int l = 0; l < S.nlevels; l++) {
                F->sub_lvl_off[(size_t)l] = (int)flat.size();
                F->sub_lvl_cnt[(size_t)l] = (int)by[(size_t)l].size();
                flat.insert(flat.end(), by[(size_t)l].begin(), by[(size_t)l].end());
            }
            if (F->d_subs_lvl) { (void)pool_free(F->d_subs_lvl); F->d_subs_lvl = nullptr; }
            if ((rc = upload(&F->d_subs_lvl, flat))) return rc;
        }
        // the level the sweep starts at: the deepest one from which up no level holds more than KVX_PIPE_FRONTS fronts.  Default 4 --
        // on the 2-D systems the sweep then starts when the children of the root are factored and runs beside the root's own pivot
        // chain, a handful of workgroups per launch (config 2: step 5.15 -> 4.66 ms; started two levels earlier, beside launches of
        // thousands of tiles, 4.83; five levels earlier 5.2: the sweep's workgroups then delay the factorisation by what they gain)
        int lim = 4;
        if (const char *e = getenv("KVX_PIPE_FRONTS")) lim = atoi(e);
        F->pipe_from = 0;
        for (int l = 0; l < S.nlevels; l++) {
            if (S.levelptr[(size_t)l + 1] - S.levelptr[(size_t)l] > lim) break;
            F->pipe_from = l;
        }
    }
    lap("pipeline set-up");
    hipStream_t st = F->stream, s2 = F->K.pipe_own_stream ? F->side[2] : F->side[0];
    auto body = [&]() -> int {
        // the sweep's stream joins behind the values (and, in a capture, the capture): right-hand sides into the work vector first
        HIPCHK(hipEventRecord(F->ev_pipe[0], st));
        HIPCHK(hipStreamWaitEvent(s2, F->ev_pipe[0], 0));
        launch_perm_gather(s2, F->d_perm, n, nr, B, ldB, F->d_X, n);
        launch_copy_d(s2, F->d_X0, F->d_X, n * (int64_t)nr);
        F->pipe_on = true;
        F->pipe_nr = nr;
        const int rb = enqueue_factor_body(F);                     // (with the forward sweep of every level right behind that level)
        F->pipe_on = false;
        if (rb) return rb;
        HIPCHK(hipEventRecord(F->ev_pipe[0], s2));
        HIPCHK(hipStreamWaitEvent(st, F->ev_pipe[0], 0));
        enqueue_bwd(F, F->d_X, n, nr);
        launch_perm_scatter(st, F->d_perm, n, nr, F->d_X, n, B, ldB);
        return hipGetLastError() == hipSuccess ? KVX_OK : KVX_EDEVICE;
    };
    HIPCHK(hipEventRecord(F->ev[0], st));
    F->factor_calls++;
    F->diag_valid = false;
    kvx_chol::FusedGraph *slot = nullptr;
    if (F->K.use_graph && !dbg_no_factor_graph() && !getenv("KVX_FUSED_EAGER")) {
        for (auto &g : F->g_fused)
            if (g.nrhs == nr && g.B == B && g.ldB == ldB) slot = &g;
        if (!slot) {
            if (F->g_fused.size() >= 4) {                           // (right-hand sides at changing addresses: no pile of graphs)
                for (auto &g : F->g_fused) g.exec.drop();
                F->g_fused.clear();
            }
            F->g_fused.push_back({nr, B, ldB, 0, LazyExec{}});
            slot = &F->g_fused.back();
        }
    }
    if ((rc = capture_or_replay(F, slot, true, body))) return rc;
    lap("capture, graph launch or eager enqueue");
    HIPCHK(hipEventRecord(F->ev[1], st));                           // (the two parts are not separable here: last_timing reports the whole
    HIPCHK(hipGetLastError());                                      //  call as the factorisation and 0 for the solve)
    F->pending = true;
    F->have_ftime = false;
    if (async) {
        // no host synchronisation: the caller's (null-stream) work is ordered behind the call by an event; the status of the
        // factorisation is examined at the next synchronising call (kvx_chol_status)
        HIPCHK(hipEventRecord(F->ev_out, st));
        HIPCHK(hipStreamWaitEvent(nullptr, F->ev_out, 0));
        return KVX_OK;
    }
    HIPCHK(hipStreamSynchronize(st));
    rc = finish_factor(F, nullptr);
    F->ms_solve = 0.0; F->have_stime = true;
    if (rc == KVX_ENOTPOSDEF) { set_err("singular matrix"); return KVX_ENOTPOSDEF; }
    return rc;
}

// Sparse right-hand sides, forward systems (L x = b, L D x = b): only the REACH of a block of columns is swept -- the fronts
// that hold a nonzero row of the block and their ancestors in the supernodal elimination tree (the supernodal form of
// CHOLMOD's sparse-rhs solve, cholmod.c:524-587; misc.kkt_chol2 forms L^-1 P A' this way, misc.py:1483-1487).  Everything
// outside the reach is zero and is neither computed nor copied back.  Per block of up to 64 columns: host marks the reach
// (leaf subtrees are taken whole: they are one launch anyway), uploads the filtered level lists, the device sweeps them with
// the ordinary forward kernels (the update vectors of children outside the reach are cleared first -- the parents pull them),
// and only the rows of the swept fronts come back.
int spsolve_forward_reach(kvx_chol *F, int sys, int64_t ncol, const int64_t *Bp, const int64_t *Bi, const double *Bx,
                          std::vector<int64_t> &xp, std::vector<int64_t> &xi, std::vector<double> &xx)
{
    Symbolic &S = F->S;
    const int64_t n = S.n, ns = S.nsuper;
    hipStream_t st = F->stream;
    if (F->col2sn.empty()) {
        F->col2sn.resize((size_t)n);
        for (int64_t s = 0; s < ns; s++)
            for (int64_t c = S.super[s]; c < S.super[s + 1]; c++) F->col2sn[(size_t)c] = (int32_t)s;
        F->sub_of.assign((size_t)ns, -1);
        for (size_t i = 0; i < F->subs_host.size(); i++)
            for (int q = F->subs_host[i].lo; q <= F->subs_host[i].hi; q++) F->sub_of[(size_t)q] = (int32_t)i;
    }
    const bool subs_on = F->nsub > 0;
    const int64_t wstride = std::max(S.wrk_size[0], S.wrk_size[1]);
    const int64_t chunk = 64;
    std::vector<uint8_t> mark((size_t)ns, 0), submark(F->subs_host.size(), 0);
    std::vector<int32_t> touched;                            // fronts marked in this block (for the reset)
    std::vector<int64_t> pos;
    std::vector<double> val, back;
    std::vector<int32_t> lists, rows;
    std::vector<int64_t> slots;
    std::vector<SubDesc> subs;
    int rc;
    for (int64_t c0 = 0; c0 < ncol; c0 += chunk) {
        const int nc = (int)std::min<int64_t>(chunk, ncol - c0);
        touched.clear(); pos.clear(); val.clear();
        std::vector<size_t> touched_subs;
        for (int j = 0; j < nc; j++) {
            const size_t first = pos.size();
            for (int64_t p = Bp[c0 + j]; p < Bp[c0 + j + 1]; p++) {
                const int64_t r = Bi[p];
                if (r < 0 || r >= n) { set_err("row index out of range in B"); return KVX_EINVAL; }
                bool dup = false;
                for (size_t q = first; q < pos.size() && !dup; q++)       // (columns are short; duplicates are summed as the dense path does)
                    if (pos[q] == r + (int64_t)j * n) { val[q] += Bx[p]; dup = true; }
                if (!dup) { pos.push_back(r + (int64_t)j * n); val.push_back(Bx[p]); }
                for (int32_t f = F->col2sn[(size_t)r]; f >= 0 && !mark[(size_t)f]; f = S.sparent[(size_t)f]) {
                    mark[(size_t)f] = 1;
                    touched.push_back(f);
                }
            }
        }
        if (subs_on)
            for (size_t t = 0, e = touched.size(); t < e; t++) {                  // a touched subtree is swept whole
                const int32_t sb = F->sub_of[(size_t)touched[t]];
                if (sb < 0 || submark[(size_t)sb]) continue;
                submark[(size_t)sb] = 1;
                touched_subs.push_back((size_t)sb);
                for (int q = F->subs_host[(size_t)sb].lo; q <= F->subs_host[(size_t)sb].hi; q++)
                    if (!mark[(size_t)q]) { mark[(size_t)q] = 1; touched.push_back(q); }
            }
        // filtered lists: per level [big | lds (unmerged mode only) | small], the slots to clear, the subtrees, the rows to fetch
        struct Lv { int64_t big, lds, sw, zs; int nbig, nlds, nsw, nz; };
        std::vector<Lv> lv((size_t)S.nlevels);
        lists.clear(); slots.clear(); subs.clear(); rows.clear();
        for (size_t sb : touched_subs) subs.push_back(F->subs_host[sb]);
        for (int l = 0; l < S.nlevels; l++) {
            const LevelPlan &P = F->plan[l];
            Lv &v = lv[(size_t)l];
            auto take = [&](const int32_t *src, int cnt, int64_t &off, int &out) {
                off = (int64_t)lists.size();
                for (int i = 0; i < cnt; i++)
                    if (mark[(size_t)src[i]]) lists.push_back(src[i]);
                out = (int)((int64_t)lists.size() - off);
            };
            take(S.levellist.data() + P.soff[0], P.scnt[0], v.big, v.nbig);
            if (F->solve_merged) { v.lds = 0; v.nlds = 0; }
            else take(S.levellist.data() + P.soff[1], P.scnt[1], v.lds, v.nlds);
            take(F->lsw_host.data() + F->sw_off[l], F->sw_cnt[l], v.sw, v.nsw);
            v.zs = (int64_t)slots.size() / 2;
            for (int64_t q = v.big; q < (int64_t)lists.size(); q++) {
                const int32_t f = lists[(size_t)q];
                for (int64_t c = S.childptr[f]; c < S.childptr[f + 1]; c++) {
                    const int32_t ch = S.children[(size_t)c];
                    if (!mark[(size_t)ch] && S.sn_m[ch] > S.sn_k[ch]) { slots.push_back(S.wx[ch]); slots.push_back(S.sn_m[ch] - S.sn_k[ch]); }
                }
            }
            v.nz = (int)((int64_t)slots.size() / 2 - v.zs);
        }
        std::sort(touched.begin(), touched.end());
        for (int32_t f : touched)
            for (int64_t c = S.super[f]; c < S.super[f + 1]; c++) rows.push_back((int32_t)c);
        const int64_t nrow = (int64_t)rows.size();
        // device side
        if ((rc = ensure_solve_ws(F, nc))) return rc;
        int32_t *d_l = nullptr, *d_rows = nullptr;
        int64_t *d_slots = nullptr, *d_pos = nullptr;
        double *d_val = nullptr, *d_back = nullptr;
        SubDesc *d_sb = nullptr;
        auto release = [&] {
            for (void *q : {(void *)d_l, (void *)d_rows, (void *)d_slots, (void *)d_pos, (void *)d_val, (void *)d_back, (void *)d_sb})
                if (q) (void)pool_free(q);
        };
        auto up = [&](void **dst, const void *src, size_t bytes) -> int {
            HIPCHK(pool_malloc(dst, std::max<size_t>(bytes, 8)));
            if (bytes) HIPCHK(hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, st));
            return KVX_OK;
        };
        rc = up((void **)&d_l, lists.data(), lists.size() * sizeof(int32_t));
        if (!rc) rc = up((void **)&d_rows, rows.data(), rows.size() * sizeof(int32_t));
        if (!rc) rc = up((void **)&d_slots, slots.data(), slots.size() * sizeof(int64_t));
        if (!rc) rc = up((void **)&d_pos, pos.data(), pos.size() * sizeof(int64_t));
        if (!rc) rc = up((void **)&d_val, val.data(), val.size() * sizeof(double));
        if (!rc) rc = up((void **)&d_sb, subs.data(), subs.size() * sizeof(SubDesc));
        if (!rc && hipSuccess != pool_malloc((void **)&d_back, std::max<size_t>((size_t)(nrow * nc), 1) * sizeof(double))) rc = KVX_EDEVICE;
        if (rc) { release(); return rc; }
        auto body = [&]() -> int {
            HIPCHK(hipMemsetAsync(F->d_X, 0, (size_t)n * nc * sizeof(double), st));
            launch_scatter_entries(st, d_pos, d_val, (int64_t)pos.size(), F->d_X);
            HIPCHK(hipMemcpyAsync(F->d_X0, F->d_X, (size_t)n * nc * sizeof(double), hipMemcpyDeviceToDevice, st));
            if (!subs.empty())
                launch_fwd_subtree(st, F->ds, d_sb, (int)subs.size(), F->d_cd_woff, F->d_Lx, F->d_X, n, nc, F->d_W[0], F->d_W[1], wstride, F->d_depth);
            for (int l = S.nlevels - 1; l >= 0; l--) {
                const LevelPlan &P = F->plan[l];
                const Lv &v = lv[(size_t)l];
                if (v.nbig + v.nlds + v.nsw == 0) continue;
                double *Wch = F->d_W[(l + 1) & 1], *Wout = F->d_W[l & 1];
                launch_zero_slots(st, d_slots + 2 * v.zs, v.nz, nc, Wch, wstride);
                if (v.nsw > 0) {
                    if (F->solve_merged) launch_fwd_lds(st, F->ds, d_l + v.sw, v.nsw, F->sw_kmax[l], F->d_Lx, F->d_X, n, nc, Wch, Wout, wstride);
                    else launch_fwd_wave(st, F->ds, d_l + v.sw, v.nsw, F->sw_kmax[l], F->d_Lx, F->d_X, n, nc, Wch, Wout, wstride);
                }
                if (v.nlds > 0)
                    launch_fwd_lds(st, F->ds, d_l + v.lds, v.nlds, std::max(P.maxk[KVX_CLS_LDS128], P.maxk[KVX_CLS_LDS96]), F->d_Lx, F->d_X,
                                   n, nc, Wch, Wout, wstride);
                if (v.nbig > 0)
                    launch_fwd_big(st, F->ds, d_l + v.big, v.nbig, P.smaxm[0], P.big_maxk, F->d_Lx, F->d_Linv, F->d_X, F->d_X0, n, nc,
                                   F->d_WK, S.n, Wch, Wout, wstride, P.scnt[0]);
            }
            if (!F->is_ll) {                                      // LDL' view: L D x = b -> diag^-1 Lc^-1 b;  L x = b -> diag Lc^-1 b
                if (!F->diag_valid) {
                    if (!F->d_diag) HIPCHK(pool_malloc((void **)&F->d_diag, (size_t)n * sizeof(double)));
                    launch_extract_diag(st, F->ds, S.nsuper, F->d_Lx, F->d_diag);
                    F->diag_valid = true;
                }
                launch_diag_scale(st, n, nc, F->d_diag, F->d_X, n, sys == 2 ? 1 : 0);
            }
            launch_perm_gather(st, d_rows, nrow, nc, F->d_X, n, d_back, nrow);
            HIPCHK(hipGetLastError());
            back.resize((size_t)(nrow * nc));
            if (nrow * nc) HIPCHK(hipMemcpyAsync(back.data(), d_back, back.size() * sizeof(double), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            return KVX_OK;
        };
        rc = body();
        release();
        if (rc) return rc;
        for (int j = 0; j < nc; j++) {
            for (int64_t i = 0; i < nrow; i++) {
                const double v = back[(size_t)(i + (int64_t)j * nrow)];
                if (v != 0.0) { xi.push_back(rows[(size_t)i]); xx.push_back(v); }
            }
            xp[(size_t)(c0 + j + 1)] = (int64_t)xi.size();
        }
        for (int32_t f : touched) mark[(size_t)f] = 0;
        for (size_t sb : touched_subs) submark[sb] = 0;
    }
    return KVX_OK;
}
}  // namespace kvx
