// The numeric factorisation: the launch schedule of the level loop (enqueue_factor_body and its pieces, one function per schedule
// and ONE function that chooses between them), its capture / replay, its status.
#include "chol_internal.hpp"

#include <algorithm>
#include <climits>
#include <string>

namespace kvx {

// Device-pointer entry points: the caller's producers run on the legacy null stream (the kvx_nt_* /
// kvx_atda_* / kvx_spmv_* calls, torch's default stream); the factor's stream is non-blocking, so
// order it explicitly behind them.
int wait_for_caller(kvx_chol *F)
{
    HIPCHK(hipEventRecord(F->ev_in, nullptr));
    HIPCHK(hipStreamWaitEvent(F->stream, F->ev_in, 0));
    return KVX_OK;
}

namespace {

bool dbg_memset_nodes() { return getenv("KVX_DBG_MEMSET_NODES") != nullptr; }

// zero L, reset the status word, scatter A
int factor_prologue(kvx_chol *F)
{
    Symbolic &S = F->S;
    hipStream_t st = F->stream;
    // Plain kernels, not memset nodes: replayed from a captured graph under the HIP runtime that ships inside the PyTorch wheel
    // (7.0.51831, the one a process gets once torch is imported), the memset nodes of a SMALL factor were not ordered before
    // the kernels behind them -- a dense 200 x 200 K of misc.kkt_chol2 failed at column 0 in 28 of 30 replays
    // (scratch/graph_stress.py; ROCm 7.2's own runtime replays them correctly).  KVX_DBG_MEMSET_NODES=1 restores the nodes.
    const bool nodes = dbg_memset_nodes();
    if (F->d_scptr && !nodes) {
        ProfScope ps(F, FAM_SCATTER);          // zero L, reset the status word and scatter A: one pass over L
        launch_init_factor(st, F->d_Ax, F->d_ssrc, F->d_sdst, F->d_scptr, S.lsize, F->d_Lx, F->d_status);
        return KVX_OK;
    }
    if (nodes) {
        HIPCHK(hipMemsetAsync(F->d_Lx, 0, std::max<int64_t>(S.lsize, 1) * sizeof(double), st));
        HIPCHK(hipMemsetAsync(F->d_status, 0x7f, sizeof(int), st));   // 0x7f7f7f7f = "no failing column"
    } else {
        launch_clear_factor(st, F->d_Lx, S.lsize, F->d_status);
    }
    ProfScope ps(F, FAM_SCATTER);
    launch_scatter_a(st, F->d_Ax, F->d_amap, S.nnzA, F->d_Lx);
    return KVX_OK;
}

// the status word to the host: published by a kernel, or copied
int factor_epilogue(kvx_chol *F)
{
    if (F->h_status_dev && !dbg_memset_nodes()) launch_publish_status(F->stream, F->d_status, F->h_status_dev);
    else HIPCHK(hipMemcpyAsync(F->h_status, F->d_status, sizeof(int), hipMemcpyDeviceToHost, F->stream));
    return KVX_OK;
}

// (F->factor_subtrees) the leaf subtrees: one wavefront each, all depths at once, the three LDS sizes on three streams
int factor_subtree_walk(kvx_chol *F)
{
    hipStream_t st = F->stream;
    const int caps[3] = {32, 48, 64};
    hipStream_t ss[3] = {st, F->side[0], F->side[1]};
    const bool fork[3] = {false, F->nsubf[1] > 0, F->nsubf[2] > 0};
    if (fork[1] || fork[2]) {
        HIPCHK(hipEventRecord(F->ev_fork, st));
        for (int g = 1; g < 3; g++)
            if (fork[g]) HIPCHK(hipStreamWaitEvent(ss[g], F->ev_fork, 0));
    }
    // (largest images first: they hold the fewest subtrees per CU)
    const int64_t offs[3] = {0, F->nsubf[0], F->nsubf[0] + F->nsubf[1]};
    for (int g = 2; g >= 0; g--) {
        if (F->nsubf[g] == 0) continue;
        ProfScope ps(F, FAM_SMALL, ss[g]);
        launch_factor_subtree(ss[g], caps[g], F->ds, F->d_subs_f + offs[g], F->nsubf[g], F->d_depth, F->d_Lx, F->d_U[0], F->d_U[1], F->d_status);
    }
    for (int g = 1; g < 3; g++)
        if (fork[g]) { HIPCHK(hipEventRecord(F->ev_join[g - 1], ss[g])); HIPCHK(hipStreamWaitEvent(st, F->ev_join[g - 1], 0)); }
    return KVX_OK;
}

// one level of the factorisation, as its pieces see it
struct Level {
    kvx_chol *F;
    int l;
    const LevelPlan &P;
    const int32_t *lbase;       // the level lists in use (d_flists or d_lists)
    const double *Uch;          // update matrices of the children
    double *Uout;               // ... of this level's fronts
    const int32_t *list;        // the big fronts of the level: their list, their number, the largest order
    int nbig, bigm;
};

// The fronts of one level are independent.  The big-front chain keeps the main stream; the small-
// front launches (two LDS classes, three wave row capacities) are each latency-bound by their
// slowest front, so they are spread over the streams by estimated duration (longest first onto
// the least loaded stream) instead of queueing up: two side streams beside a big chain, main +
// two side streams on the levels without big fronts.  Joined at level end (join_small_fronts).
int small_fronts(const Level &L, bool side_used[2])
{
    kvx_chol *F = L.F;
    const LevelPlan &P = L.P;
    hipStream_t st = F->stream;
    const bool have_big = L.nbig > 0;
    struct Item { int c; int cnt; int64_t off; double est; int stream; int mcap; int kmax; };
    Item items[5];
    int nitems = 0;
    for (int c = KVX_CLS_LDS128; c < KVX_CLS_WAVE0; c++)
        if (P.cnt[c] > 0) {
            const double slots = c == KVX_CLS_LDS128 ? 512.0 : 1024.0;         // packed LDS image: two / four fronts per CU
            items[nitems++] = Item{c, P.cnt[c], P.off[c], (P.maxk[c] > 32 ? 80.0 : 45.0) * std::max(1.0, P.cnt[c] / slots), 0, 0, 0};
        }
    for (int c = KVX_CLS_WAVE0; c < KVX_NCLS; c += 2) {
        const int cnt = P.cnt[c] + P.cnt[c + 1];
        if (cnt == 0) continue;
        const int mcap = wave_class_mcap(c);
        const double base = mcap == 64 ? 35.0 : (mcap == 48 ? 28.0 : 18.0), slots = mcap == 64 ? 2048.0 : (mcap == 48 ? 4096.0 : 8192.0);
        items[nitems++] = Item{c, cnt, P.cnt[c] > 0 ? P.off[c] : P.off[c + 1], base * std::max(1.0, cnt / slots), 0, mcap, P.cnt[c] > 0 ? 32 : 16};
    }
    std::sort(items, items + nitems, [](const Item &x, const Item &y) { return x.est > y.est; });
    double load[3] = {have_big ? 1e30 : 0.0, 0.0, 0.0};                          // main, side[0], side[1]
    if (F->K.side_spread == 0) load[0] = have_big ? 1e30 : -1e30;               // KVX_SIDE_SPREAD=0: everything small on one stream
    side_used[0] = side_used[1] = false;
    for (int i = 0; i < nitems; i++) {
        int best = 0;
        for (int t = 1; t < 3; t++)
            if (load[t] < load[best]) best = t;
        if (F->K.side_spread == 0) best = have_big ? 1 : 0;
        load[best] += items[i].est;
        items[i].stream = best;
        if (best > 0) side_used[best - 1] = true;
    }
    if (side_used[0] || side_used[1]) {
        HIPCHK(hipEventRecord(F->ev_fork, st));
        for (int i = 0; i < 2; i++)
            if (side_used[i]) HIPCHK(hipStreamWaitEvent(F->side[i], F->ev_fork, 0));
    }
    for (int i = 0; i < nitems; i++) {
        const Item &it = items[i];
        hipStream_t sl = it.stream == 0 ? st : F->side[it.stream - 1];
        ProfScope ps(F, FAM_SMALL, sl);
        if (it.c < KVX_CLS_WAVE0)
            launch_front_small(sl, it.c == KVX_CLS_LDS128 ? 128 : 96, P.maxk[it.c] <= 32 ? 32 : 64, F->ds, L.lbase + it.off, it.cnt, F->d_Lx, L.Uch, L.Uout, F->d_status);
        else    // the k <= 32 and k <= 16 lists of one row capacity are adjacent -> one launch
            launch_front_wave(sl, it.mcap, it.kmax, F->ds, L.lbase + it.off, it.cnt, F->d_Lx, L.Uch, L.Uout, F->d_status);
    }
    return KVX_OK;
}

int join_small_fronts(kvx_chol *F, const bool side_used[2])
{
    for (int i = 0; i < 2; i++)
        if (side_used[i]) { HIPCHK(hipEventRecord(F->ev_join[i], F->side[i])); HIPCHK(hipStreamWaitEvent(F->stream, F->ev_join[i], 0)); }
    return KVX_OK;
}

// Extend-add of every big front of the level, one launch, and the first diagonal block of the chain.
// Few workgroups in the extend-add (the top of the tree, small systems): the first diagonal block is assembled and factored
// by a workgroup of the same launch (k_assemble_big_potrf) -- one launch less on the level's critical path.
// (K.asm_potrf_wgs: the largest launch, in workgroups, that takes this form)
void assemble_big(const Level &L)
{
    kvx_chol *F = L.F;
    hipStream_t st = F->stream;
    const bool fused = (int64_t)L.nbig * ((L.bigm + KVX_ASM_TC - 1) / KVX_ASM_TC) <= F->K.asm_potrf_wgs;
    {
        ProfScope ps(F, FAM_ASSEMBLE);
        if (fused) launch_assemble_big_potrf(st, F->ds, L.list, L.nbig, L.bigm, F->d_Lx, L.Uch, L.Uout, F->d_Linv, F->d_status);
        else launch_assemble_big(st, F->ds, L.list, L.nbig, L.bigm, F->d_Lx, L.Uch, L.Uout);
    }
    if (!fused) { ProfScope ps(F, FAM_POTRF); launch_potrf_blk(st, F->ds, L.list, L.nbig, 0, F->d_Lx, F->d_Linv, F->d_status); }
}

// ---- the pivot chain of the big fronts of a level: three schedules, and the choice between them --------------------------------
enum ChainKind { CHAIN_TWO_LEVEL, CHAIN_BLOCKED, CHAIN_PAIRS };
// cls: the trailing updates number their workgroups over size classes of the chain lists (launch_syrk_step); always so when blocked
struct ChainChoice { ChainKind kind; bool cls; };

// do the chain lists of level l (build_chain_lists) cover its pivot columns?
bool have_chain_lists(const kvx_chol *F, int l, const LevelPlan &P)
{
    return (size_t)l < F->chain_steps.size() && (int)F->chain_steps[(size_t)l].size() * KVX_NB >= P.chain_maxk &&
           (int)F->u_steps[(size_t)l].size() * F->K.u_block >= P.chain_maxk;
}

// The policy, and nothing else: which schedule the chain of a level takes.
ChainChoice choose_chain(const LevelPlan &P, const CholKnobs &K, bool have_lists)
{
    // two-level outer blocks: for very large fronts only, and only in the round-3 schedule (see chain_two_level)
    if (P.maxm[KVX_CLS_BIG] >= K.two_level_m && K.defer_u == 0) return ChainChoice{CHAIN_TWO_LEVEL, false};
    // Round 4: the update matrices are left out of the chain (launches limited to the pivot columns) wherever a level's
    // fronts have more than one panel, and brought up to date afterwards by rank-(<= u_block) updates with LDS-staged
    // tiles (launch_syrk_u): K = 64 per pass over C moved 16 bytes per 128 flops and bound the ~20-nnz/row systems by
    // exactly that traffic.  KVX_DEFER_U=0: the round-3 schedule; KVX_U_BLOCK: panel columns per pass (default 256).
    const bool cls = !K.syrk_direct && have_lists;
    // ... where a level's chain is bound by throughput: its flops per panel step would keep the machine busy for longer
    // than the ~30 us of latency a step has anyway (KVX_BLOCKED_GF: Gflop per step from which on, default 0.5.  21-point
    // system, one box, thresholds 0 / 0.3 / 0.7 / 1.5 / never: 23.6 / 23.8 / 23.9 / 24.4 / 26.3 ms; config 2, where no level
    // reaches 0.3: blocked everywhere 4.97 - 5.45 ms against 4.76 - 4.97)
    const int nsteps = (P.chain_maxk + KVX_NB - 1) / KVX_NB;
    const bool blocked = K.defer_u && cls && P.big_flops * 1e-9 >= K.blocked_gf * nsteps;
    return ChainChoice{blocked ? CHAIN_BLOCKED : CHAIN_PAIRS, cls};
}

// one trailing update of the chain: the fronts still in it at step jb, numbered over size classes (LDS-staged tiles),
// or the round-3 launches over (tiles of the largest front) x (all big fronts of the level)
void syrk_step(const Level &L, bool cls, int jb, int klen, int col_lim)
{
    kvx_chol *F = L.F;
    hipStream_t st = F->stream;
    ProfScope ps(F, FAM_SYRK);
    if (cls) {
        const kvx_chol::ChainList &cl = F->chain_steps[(size_t)L.l][(size_t)(jb / KVX_NB)];
        launch_syrk_step(st, F->ds, F->d_chain + cl.off, F->chain_m.data() + cl.off, F->chain_k.data() + cl.off, cl.cnt, jb, klen,
                         F->d_Lx, L.Uout, F->d_Linv, F->d_status, col_lim);
    } else if (klen == 2 * KVX_NB) {
        launch_syrk_pair(st, F->ds, L.list, L.nbig, L.bigm, jb, F->d_Lx, L.Uout, F->d_Linv, F->d_status, col_lim);
    } else if (col_lim < KVX_COLS_PIVOT) {
        launch_syrk_inner(st, F->ds, L.list, L.nbig, L.bigm, jb, col_lim, F->d_Lx, L.Uout, F->d_Linv, F->d_status);
    } else {
        launch_syrk_trailing(st, F->ds, L.list, L.nbig, L.bigm, jb, F->d_Lx, L.Uout, F->d_Linv, F->d_status, col_lim);
    }
}

void trsm_step(const Level &L, int jb)
{
    ProfScope ps(L.F, FAM_TRSM);
    launch_trsm_blk(L.F->stream, L.F->ds, L.list, L.nbig, L.bigm, jb, L.F->d_Lx, L.F->d_Linv);
}

// one panel over the whole trailing matrix, the panel solve inside the update (size classes of the chain list of step jb)
void syrk_solve_step(const Level &L, int jb)
{
    kvx_chol *F = L.F;
    ProfScope ps(F, FAM_SYRK);
    const kvx_chol::ChainList &cl = F->chain_steps[(size_t)L.l][(size_t)(jb / KVX_NB)];
    launch_syrk_solve(F->stream, F->ds, F->d_chain + cl.off, F->chain_m.data() + cl.off, F->chain_k.data() + cl.off, cl.cnt, jb,
                      F->d_Lx, L.Uout, F->d_Linv, F->d_status);
}

// the panels jb0, jb0 + 64, ... that steps of that form left unsolved, one launch over the fronts still in the chain at step jb0
// (largest first)
void trsm_panels_step(const Level &L, int jb0, int npanels)
{
    kvx_chol *F = L.F;
    ProfScope ps(F, FAM_TRSM);
    const kvx_chol::ChainList &cl = F->chain_steps[(size_t)L.l][(size_t)(jb0 / KVX_NB)];
    if (cl.cnt > 0) launch_trsm_panels(F->stream, F->ds, F->d_chain + cl.off, cl.cnt, F->chain_m[(size_t)cl.off], jb0, npanels, F->d_Lx, F->d_Linv);
}

// Outer blocks of `outer_block` (1024) columns, one rank-1024 update of the trailing matrix per block (128-tile kernel: 34 TF/s
// on a dense trailing matrix; rocBLAS dgemm at K = 256 reaches 48-59).  Measured on MI355X against the
// single-level path: dense n = 10240 14.8 vs 16.7 ms, 3-D 80^3 49.6 vs 51.0 ms, but 21-point 1000^2
// (fronts <= 5007, many per level) 29.1 vs 24.3 ms -- the outer update is an extra serial launch per
// block, so it is used for very large fronts only (look-ahead -- the outer update of block b beside the panel chain
// of block b + 1 on a second stream -- was measured slower, docs/lab.md)
void chain_two_level(const Level &L)
{
    kvx_chol *F = L.F;
    hipStream_t st = F->stream;
    const int OB = F->K.outer_block, maxk = L.P.chain_maxk;
    for (int ob = 0; ob < maxk; ob += OB) {
        for (int jb = ob; jb < std::min(ob + OB, maxk); jb += KVX_NB) {
            trsm_step(L, jb);
            { ProfScope ps(F, FAM_SYRK); launch_syrk_inner(st, F->ds, L.list, L.nbig, L.bigm, jb, ob + OB, F->d_Lx, L.Uout, F->d_Linv, F->d_status); }
        }
        { ProfScope ps(F, FAM_SYRK); launch_syrk_outer(st, F->ds, L.list, L.nbig, L.bigm, ob, OB, F->d_Lx, L.Uout, F->d_Linv, F->d_status); }
    }
}

// Round 4, the blocked schedule.  The pivot columns go in blocks of OB = u_block (256).  On the chain's stream a
// panel of block b updates only what is left of the block ("inner", at most three tile columns, K = 64); when the
// block is solved, ONE rank-OB update ("near") brings the next block's columns up to date and factors its first
// diagonal block; everything further right -- later pivot columns and the update matrix -- gets its rank-OB update
// ("far") on a stream of its own, beside the next block's chain: K = 64 per pass over C moved 16 bytes per 128
// flops and bound the ~20-nnz/row systems by exactly that traffic.  near(b + 1) and far(b) meet in the columns of
// block b + 2: near(b + 1) waits for far(b); far(b + 1) follows far(b) on its stream.
// KVX_DEFER_U=0: the round-3 schedule; KVX_U_STREAM=0: the far updates on the chain's stream.
int chain_blocked(const Level &L)
{
    kvx_chol *F = L.F;
    hipStream_t st = F->stream;
    const int OB = F->K.u_block, maxk = L.P.chain_maxk;
    const std::vector<kvx_chol::ChainList> &far = F->u_steps[(size_t)L.l];
    // (family timing sums the durations of single launches: the far updates stay behind the chain then, so that a launch's
    //  duration is its own and not that of two kernels sharing the machine)
    hipStream_t su = (F->K.u_stream && F->prof_family < 0) ? F->side[2] : st;
    bool forked = false;
    for (int ob = 0, b = 0; ob < maxk; ob += OB, b++) {
        const int bend = std::min(ob + OB, maxk);
        for (int jb = ob; jb < bend; jb += KVX_NB) {
            trsm_step(L, jb);
            if (jb + KVX_NB < bend) syrk_step(L, true, jb, KVX_NB, ob + OB);
        }
        const kvx_chol::ChainList &fl = far[(size_t)b];
        if (fl.cnt > 0) {
            if (su != st) {
                while ((int)F->ev_u.size() <= 2 * b + 1) { hipEvent_t e = nullptr; HIPCHK(pool_event_get(&e, false)); F->ev_u.push_back(e); }
                HIPCHK(hipEventRecord(F->ev_u[(size_t)(2 * b)], st));
                HIPCHK(hipStreamWaitEvent(su, F->ev_u[(size_t)(2 * b)], 0));
                forked = true;
                syrk_count(SYRK_FAR_SIDE);
            }
            {
                ProfScope ps(F, FAM_SYRK, su);
                launch_syrk_far(su, F->ds, F->d_chain + fl.off, F->chain_m.data() + fl.off, F->chain_k.data() + fl.off, fl.cnt, ob, OB,
                                ob + 2 * OB, F->d_Lx, L.Uout);
            }
            if (su != st) HIPCHK(hipEventRecord(F->ev_u[(size_t)(2 * b + 1)], su));
        }
        if (bend < maxk) {
            // near(b) touches the columns of block b + 1, which far(b - 1) has updated with block b - 1
            if (su != st && b >= 1 && far[(size_t)(b - 1)].cnt > 0) HIPCHK(hipStreamWaitEvent(st, F->ev_u[(size_t)(2 * (b - 1) + 1)], 0));
            syrk_step(L, true, ob, OB, ob + 2 * OB);
        }
    }
    if (forked) {
        if (!F->ev_ujoin) HIPCHK(pool_event_get(&F->ev_ujoin, false));
        HIPCHK(hipEventRecord(F->ev_ujoin, su));
        HIPCHK(hipStreamWaitEvent(st, F->ev_ujoin, 0));
    }
    return KVX_OK;
}

// Pair schedule where a launch holds many tiles (the levels bound by the read-modify-write of the trailing matrices): panel
// jb updates only the columns of panel jb + 64 (one tile column), panel jb + 64 is solved, and ONE pass over everything
// right of both applies the two panels together -- half the passes over the trailing matrices, the same number of
// launches.  Where a launch is a handful of tiles (the pivot chain at the top of the tree) the pass over C is not what the
// step waits for and the eight operand rounds of a K = 128 tile would lengthen the chain: one panel per launch there.
// (K.pair_tiles: from this tile count on -- an upper estimate: largest front x fronts in the launch)
// Where a launch is at most K.solve_in_update_tiles tiles (same estimate; 0 = never) the step is ONE launch: the update's
// workgroups solve the panel rows they need themselves (syrk_solve_step).  They cannot store them -- the solved rows go where
// the others still read the unsolved ones -- so the panels of such steps [owed, owed_end) are solved once more and stored by one
// launch when the chain is through (or before a step of the two-launch form, should one follow): nothing in between reads them.
void chain_pairs(const Level &L, bool cls)
{
    const int maxk = L.P.chain_maxk;
    int owed = 0, owed_end = 0;
    auto settle = [&] {
        if (owed_end > owed) trsm_panels_step(L, owed, (owed_end - owed) / KVX_NB);
        owed = owed_end = 0;
    };
    for (int jb = 0; jb < maxk;) {
        const int64_t T = (L.bigm - jb - 1 + KVX_TILE - 1) / KVX_TILE;
        const int64_t tiles = T * (T + 1) / 2 * L.nbig;
        const bool pair = jb + KVX_NB < maxk && tiles >= L.F->K.pair_tiles;
        if (solve_in_update(L.F->K, cls, pair, KVX_NB, INT_MAX, tiles)) {
            syrk_solve_step(L, jb);
            if (owed_end == owed) owed = jb;
            owed_end = jb + KVX_NB;
            jb += KVX_NB;
            continue;
        }
        settle();
        // the trailing update of panel jb also factors and inverts the diagonal block of panel jb + 64
        trsm_step(L, jb);
        if (!pair) {
            syrk_step(L, cls, jb, KVX_NB, INT_MAX);
            jb += KVX_NB;
            continue;
        }
        syrk_step(L, cls, jb, KVX_NB, jb + 2 * KVX_NB);
        trsm_step(L, jb + KVX_NB);
        syrk_step(L, cls, jb, 2 * KVX_NB, INT_MAX);
        jb += 2 * KVX_NB;
    }
    settle();
}

// kvx_chol_factorize_solve_dev: level l is complete -- its forward sweep goes onto the sweep's own streams right here, so
// that its launches sit between the factorisation's in submission order too (enqueued after the whole factorisation they
// were submitted -- eagerly and from a replayed graph alike -- only when the last front had been)
int pipe_level_hook(kvx_chol *F, int l)
{
    Symbolic &S = F->S;
    HIPCHK(hipEventRecord(F->ev_lvl[(size_t)l], F->stream));
    // The sweep goes onto side[0] -- the stream of the factorisation's small-front launches, which has nothing left to do at the
    // top of the tree -- not onto a stream of its own: a replayed graph runs its parallel branches on streams the executable
    // creates for itself, as many as the capture is wide, and a process gets four hardware queues; with a fourth / fifth
    // branch two of them share a queue and the step was 4.65 or 4.9 ms from one process to the next, depending on whether the
    // pivot chain's queue was the shared one.  KVX_PIPE_OWN_STREAM=1: side[2] (the old form, for comparison).
    hipStream_t sw = F->K.pipe_own_stream ? F->side[2] : F->side[0];
    const SweepStreams ss2{sw, sw, sw, F->ev_pipe[1], F->ev_pipe[2], F->ev_pipe[3]};
    // Below pipe_from the levels hold thousands of small fronts that fill the CUs: a sweep beside them only takes their
    // wavefront slots (measured: the factorisation lost what the sweep gained).  From pipe_from up the factorisation is a chain
    // of small launches on an idle machine: the sweep of everything below starts there in one go, then follows level by level.
    if (l == F->pipe_from) enqueue_fwd(F, F->d_X, S.n, F->pipe_nr, S.nlevels - 1, l, &ss2, true, true);
    else if (l < F->pipe_from) enqueue_fwd(F, F->d_X, S.n, F->pipe_nr, l, l, &ss2, true);
    return KVX_OK;
}

}  // namespace

// enqueue the numeric factorisation; d_Ax already holds the values
// levels lfrom, lfrom - 1, ..., lto; prologue = zero L, reset the status word, scatter A; epilogue = fetch the status
int enqueue_factor_body(kvx_chol *F, int lfrom, int lto, bool prologue, bool epilogue)
{
    Symbolic &S = F->S;
    int rc;
    if (prologue && (rc = factor_prologue(F))) return rc;
    if (lfrom < 0) lfrom = S.nlevels - 1;
    if (F->factor_subtrees && prologue && lfrom == S.nlevels - 1 && (rc = factor_subtree_walk(F))) return rc;
    const int32_t *lbase = F->fplan_on ? F->d_flists : F->d_lists;
    for (int l = lfrom; l >= lto; l--) {
        const LevelPlan &P = F->fplan_on ? F->fplan[l] : F->plan[l];
        const Level L{F, l, P, lbase, F->d_U[(l + 1) & 1], F->d_U[l & 1], lbase + P.off[KVX_CLS_BIG], P.cnt[KVX_CLS_BIG], P.maxm[KVX_CLS_BIG]};
        bool side_used[2];
        if ((rc = small_fronts(L, side_used))) return rc;
        if (L.nbig > 0) {
            assemble_big(L);
            const ChainChoice c = choose_chain(P, F->K, have_chain_lists(F, l, P));
            if (c.kind == CHAIN_TWO_LEVEL) chain_two_level(L);
            else if (c.kind == CHAIN_PAIRS) chain_pairs(L, c.cls);
            else if ((rc = chain_blocked(L))) return rc;
        }
        if ((rc = join_small_fronts(F, side_used))) return rc;
        if (F->pipe_on && (rc = pipe_level_hook(F, l))) return rc;
    }
    if (epilogue && (rc = factor_epilogue(F))) return rc;
    HIPCHK(hipGetLastError());
    return KVX_OK;
}

void dump_graph_dot(hipGraph_t graph)              // debugging: the captured graph (nodes and edges) as a .dot file
{
    const char *dot = getenv("KVX_DBG_GRAPH_DOT");
    if (!dot) return;
    static int serial = 0;
    const std::string path = std::string(dot) + "." + std::to_string(serial++) + ".dot";
    if (hipGraphDebugDotPrint(graph, path.c_str(), 0) != hipSuccess) (void)hipGetLastError();
}

int enqueue_factor(kvx_chol *F)
{
    if (F->dist_nranks > 1) { set_err("sharded factor: use kvx_chol_dist_factorize"); return KVX_EINVAL; }
    hipStream_t st = F->stream;
    HIPCHK(hipEventRecord(F->ev[0], st));
    const char *dbg_ng = dbg_no_factor_graph();
    const bool graph_ok = F->K.use_graph && F->prof_family < 0 && !(dbg_ng && (atoll(dbg_ng) == 1 || atoll(dbg_ng) == F->S.n));
    F->factor_calls++;
    F->diag_valid = false;
    // (a capture records the launches without running them: the call that takes it still runs its own launches below)
    if (graph_ok && !F->g_factor.tried && F->factor_calls >= 2)
        capture_graph(F, [&] { return enqueue_factor_body(F); }, F->g_factor);   // (sharded mode drives the body itself)
    hipGraphExec_t fexec = graph_ok ? F->g_factor.ready() : nullptr;
    if (fexec) {
        const char *e = getenv("KVX_DBG_GRAPH_SYNC");                            // debugging: 1 = synchronise before the replay, 2 = after, 3 = both
        const int sync = e ? atoi(e) : 0;
        if (sync & 1) HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGraphLaunch(fexec, st));
        if (sync & 2) HIPCHK(hipStreamSynchronize(st));
    } else {
        int rc = enqueue_factor_body(F);
        if (rc) return rc;
    }
    HIPCHK(hipEventRecord(F->ev[1], st));
    HIPCHK(hipGetLastError());
    F->pending = true;
    F->have_ftime = false;
    return KVX_OK;
}

int finish_factor(kvx_chol *F, int64_t *minor)
{
    if (F->pending) {
        HIPCHK(hipStreamSynchronize(F->stream));
        F->pending = false;
        prof_collect(F);
        float ms = 0;
        if (hipEventElapsedTime(&ms, F->ev[0], F->ev[1]) == hipSuccess) { F->ms_factor = ms; F->have_ftime = true; }
        int st = *F->h_status;
        F->numeric = true;
        F->minor = (st >= 0x7f7f7f7f) ? F->S.n : (int64_t)st;
    }
    if (minor) *minor = F->minor;
    if (!F->numeric) return KVX_ESYMBOLIC;
    return F->minor < F->S.n ? KVX_ENOTPOSDEF : KVX_OK;
}

}  // namespace kvx

// the policy of the fused chain step on the host (tests/test_solve_in_update_cpu.py): 1 = the step solves its own panel rows
extern "C" int kvx_dbg_solve_in_update(int64_t knob, int cls, int pair, int klen, int col_lim, int64_t tiles)
{
    CholKnobs K;
    K.solve_in_update_tiles = knob;
    return solve_in_update(K, cls != 0, pair != 0, klen, col_lim, tiles) ? 1 : 0;
}
