// Device set-up of a Cholesky factor: the environment knobs, the launch plan of the level lists, the leaf subtrees, the chain lists
// of the big fronts, the device tables, the solve workspace.
#include "chol_internal.hpp"

#include <algorithm>
#include <climits>
#include <vector>

namespace kvx {

bool syrk_direct() { static const bool v = [] { const char *e = getenv("KVX_SYRK_DIRECT"); return e && e[0] == '1'; }(); return v; }

CholKnobs read_chol_knobs()
{
    CholKnobs K;
    const char *e;
    auto is1 = [](const char *v) { return v && v[0] == '1'; };
    if ((e = getenv("KVX_SUB_MAXF"))) K.sub_maxf = std::max(1, std::min(atoi(e), KVX_SUB_MAXF));
    K.factor_subtrees = is1(getenv("KVX_FACTOR_SUBTREES"));
    if ((e = getenv("KVX_U_BLOCK"))) K.u_block = std::max(64, atoi(e) / 64 * 64);
    K.init_two_passes = getenv("KVX_INIT_TWO_PASSES") != nullptr;
    K.use_subtrees = !is1(getenv("KVX_NO_SUBTREES"));
    K.use_graph = !is1(getenv("KVX_NO_GRAPH"));
    if ((e = getenv("KVX_WIDE_FROM"))) K.wide_from = std::max(0, atoi(e));
    if ((e = getenv("KVX_SIDE_SPREAD"))) K.side_spread = atoi(e);
    if ((e = getenv("KVX_TWO_LEVEL_M"))) K.two_level_m = atoi(e);
    if ((e = getenv("KVX_OUTER_BLOCK")) && atoi(e) >= 64) K.outer_block = atoi(e) / 64 * 64;
    if ((e = getenv("KVX_ASM_POTRF_WGS"))) K.asm_potrf_wgs = atoll(e);
    if ((e = getenv("KVX_PAIR_TILES"))) K.pair_tiles = atoll(e);
    if ((e = getenv("KVX_SOLVE_IN_UPDATE_TILES"))) K.solve_in_update_tiles = std::max<long long>(0, atoll(e));
    if ((e = getenv("KVX_DEFER_U"))) K.defer_u = atoi(e);
    K.syrk_direct = syrk_direct();
    if ((e = getenv("KVX_BLOCKED_GF"))) K.blocked_gf = atof(e);
    if ((e = getenv("KVX_U_STREAM"))) K.u_stream = atoi(e);
    K.pipe_own_stream = is1(getenv("KVX_PIPE_OWN_STREAM"));
    K.solve_nofork = (e = getenv("KVX_SOLVE_NOFORK")) && atoi(e) != 0;
    return K;
}

// per-level launch plan of the level lists (lists / lptr: fronts grouped by level, each level sorted by kernel class)
void build_plan_from(const Symbolic &S, const std::vector<int32_t> &lists, const std::vector<int64_t> &lptr, std::vector<LevelPlan> &plan)
{
    plan.assign((size_t)S.nlevels, LevelPlan());
    for (int l = 0; l < S.nlevels; l++) {
        LevelPlan &P = plan[l];
        for (int c = 0; c < KVX_NCLS; c++) { P.off[c] = 0; P.cnt[c] = 0; P.maxm[c] = 0; P.maxk[c] = 0; }
        for (int g = 0; g < 3; g++) { P.soff[g] = 0; P.scnt[g] = 0; P.smaxm[g] = 0; }
        for (int64_t q = lptr[l]; q < lptr[l + 1]; q++) {
            int s = lists[q];
            int m = S.sn_m[s], k = S.sn_k[s];
            int c = front_class(m, k);
            if (P.cnt[c] == 0) P.off[c] = q;
            P.cnt[c]++;
            P.maxm[c] = std::max(P.maxm[c], m);
            P.maxk[c] = std::max(P.maxk[c], k);
            if (c == KVX_CLS_BIG) {
                P.big_maxk = std::max(P.big_maxk, k);
                P.chain_maxk = std::max(P.chain_maxk, k);
                P.big_flops += (double)k * k * k / 3.0 + (double)(m - k) * k * (double)m;   // potrf + panel solve + trailing update
            }
            int g = c == KVX_CLS_BIG ? 0 : (c < KVX_CLS_WAVE0 ? 1 : 2);
            if (P.scnt[g] == 0) P.soff[g] = q;
            P.scnt[g]++;
            P.smaxm[g] = std::max(P.smaxm[g], m);
        }
    }
}

// from F->lists_host / F->lptr_host (the level lists already uploaded to d_lists)
void build_plan(kvx_chol *F) { build_plan_from(F->S, F->lists_host, F->lptr_host, F->plan); }

void destroy_graphs(kvx_chol *F)
{
    F->g_factor.drop();
    for (auto &g : F->g_solve) g.exec.drop();
    F->g_solve.clear();
    for (auto &g : F->g_fused) g.exec.drop();
    F->g_fused.clear();
}

// Leaf subtrees for the solves: maximal subtrees made of wave-class fronts only, small enough for one wavefront
// (front count, pivot columns, LDS stack of update vectors).
// fronts per subtree: longer walks serialise more fronts in one wavefront, shorter ones leave more to the level loop (flat
// optimum 8..16 on the 1e6-unknown systems).  Round 4: a small system has a few hundred subtrees on an idle machine and its
// sweeps are chains of dependent launches -- a walk of 12 fronts is then the longest link (41 / 56 us of config 4b's 440 us
// solve); with 4 fronts per walk the loop of config 4b runs at 587-599 it/s against 548-575 (2: 560-598, 3: 513-601, 5: 557-588).
static int subtree_maxf(const Symbolic &S, const CholKnobs &K) { return K.sub_maxf > 0 ? K.sub_maxf : (S.n <= 150000 ? 4 : 12); }

// The choice alone, nothing written: take(lo, hi, woff) is called for every subtree [lo, hi], roots descending; woff (one buffer,
// reused) = the LDS stack offsets of its fronts.
template <class Take>
static void pick_subtrees(const Symbolic &S, int maxf, Take take)
{
    const int64_t ns = S.nsuper;
    std::vector<int32_t> cnt((size_t)ns, 1), minidx((size_t)ns);
    std::vector<uint8_t> ok((size_t)ns, 0), in_sub((size_t)ns, 0);
    std::vector<int64_t> woff;
    for (int64_t s = 0; s < ns; s++) {
        minidx[s] = (int32_t)s;
        bool good = front_class(S.sn_m[s], S.sn_k[s]) >= KVX_CLS_WAVE0;
        for (int64_t c = S.childptr[s]; c < S.childptr[s + 1]; c++) {
            const int32_t ch = S.children[c];
            good = good && ok[ch];
            cnt[s] += cnt[ch];
            minidx[s] = std::min(minidx[s], minidx[ch]);
        }
        const int64_t lo = s - cnt[s] + 1;
        good = good && cnt[s] <= maxf && minidx[s] == lo && lo >= 0 &&
               (S.super[s + 1] - S.super[lo]) <= KVX_SUB_MAXCOLS;
        ok[s] = good;
    }
    for (int64_t s = ns - 1; s >= 0; s--) {
        if (!ok[s] || in_sub[s]) continue;
        if (S.sparent[s] >= 0 && ok[S.sparent[s]]) continue;      // not maximal
        const int64_t lo = s - cnt[s] + 1;
        // LDS stack of update vectors in postorder: a front pops its children, then pushes its own
        int64_t sp = 0, top = 0;
        woff.assign((size_t)cnt[s], 0);
        bool fits = true;
        for (int64_t q = lo; q <= s; q++) {
            for (int64_t c = S.childptr[q]; c < S.childptr[q + 1]; c++) sp -= S.sn_m[S.children[c]] - S.sn_k[S.children[c]];
            woff[q - lo] = sp;
            if (q != s) sp += S.sn_m[q] - S.sn_k[q];
            top = std::max(top, sp);
            if (sp < 0) fits = false;
        }
        if (!fits || top > KVX_SUB_STACK) continue;               // stays in the level lists
        for (int64_t q = lo; q <= s; q++) in_sub[q] = 1;
        take(lo, s, woff);
    }
}

// kvx_chol_get_info: the solve subtrees of this factor and the fronts inside them.  Two stored numbers: build_subtrees sets them
// at the device set-up; a query before that computes them once, as the set-up would cut the tree with the environment of that
// first query (no device needed).
void subtree_counts(kvx_chol *F, int64_t out[2])
{
    if (!F->sub_info_set) {
        F->sub_info[0] = F->sub_info[1] = 0;
        const CholKnobs K = read_chol_knobs();
        if (K.use_subtrees && F->dist_nranks == 1 && (int64_t)F->S.rel.size() < INT32_MAX)
            pick_subtrees(F->S, subtree_maxf(F->S, K), [&](int64_t lo, int64_t hi, const std::vector<int64_t> &) {
                F->sub_info[0]++;
                F->sub_info[1] += hi - lo + 1;
            });
        F->sub_info_set = true;
    }
    out[0] = F->sub_info[0];
    out[1] = F->sub_info[1];
}

// Host analysis, once per factor: the update vector of a subtree root is written long before its parent's level runs, so it
// gets a slot of its own behind the recycled part of its parity buffer (S.wx / S.wrk_size are adjusted before anything is uploaded).
void analyze_subtrees(kvx_chol *F)
{
    Symbolic &S = F->S;
    const int64_t ns = S.nsuper;
    F->in_sub.assign((size_t)ns, 0);
    F->subs_host.clear();
    F->cd_woff_host.assign(S.children.size(), 0);
    int64_t extra[2] = {0, 0};
    const int64_t base[2] = {S.wrk_size[0], S.wrk_size[1]};
    // factorisation: every front of a subtree gets a slot of its parity buffer that no other front reuses (the level schedule
    // recycles the buffers level by level; subtrees are factored before the level loop, at all depths at once)
    int64_t uextra[2] = {0, 0};
    const int64_t ubase[2] = {S.upd_size[0], S.upd_size[1]};
    // (opt-in, KVX_FACTOR_SUBTREES=1 -- measured slower than the level schedule, see build_subtrees: the slots cost
    // sum u^2 doubles over the subtree fronts, 270 MB on config 2)
    const bool uniq = F->K.factor_subtrees;
    pick_subtrees(S, subtree_maxf(S, F->K), [&](int64_t lo, int64_t s, const std::vector<int64_t> &woff) {
        for (int64_t q = lo; q <= s; q++) {
            F->in_sub[q] = 1;
            for (int64_t c = S.childptr[q]; c < S.childptr[q + 1]; c++) F->cd_woff_host[c] = (int32_t)woff[S.children[c] - lo];
            if (uniq) {
                const int pq = S.depth[q] & 1;
                const int64_t uq = S.sn_m[q] - S.sn_k[q];
                S.ux[q] = ubase[pq] + uextra[pq];
                uextra[pq] += uq * uq;
            }
        }
        F->subs_host.push_back(SubDesc{(int32_t)lo, (int32_t)s, (int32_t)S.super[lo], (int32_t)(S.super[s + 1] - S.super[lo])});
        const int p = S.depth[s] & 1;
        S.wx[s] = base[p] + extra[p];
        extra[p] += S.sn_m[s] - S.sn_k[s];
    });
    S.wrk_size[0] = base[0] + extra[0];
    S.wrk_size[1] = base[1] + extra[1];
    S.upd_size[0] = ubase[0] + uextra[0];
    S.upd_size[1] = ubase[1] + uextra[1];
}

// per-level solve lists without the subtree fronts, and the subtree tables, on the device
// Lists for the LDS-staged trailing update (chol_internal.hpp: chain_steps / u_steps), from the plan the factorisation uses.
int build_chain_lists(kvx_chol *F)
{
    Symbolic &S = F->S;
    const std::vector<LevelPlan> &plan = F->fplan_on ? F->fplan : F->plan;
    const std::vector<int32_t> &lists = F->fplan_on ? F->flists_host : F->lists_host;
    F->chain_steps.assign((size_t)S.nlevels, {});
    F->u_steps.assign((size_t)S.nlevels, {});
    F->chain_host.clear(); F->chain_m.clear(); F->chain_k.clear();
    std::vector<int32_t> fr;
    for (int l = 0; l < S.nlevels && l < (int)plan.size(); l++) {
        const LevelPlan &P = plan[l];
        const int nbig = P.cnt[KVX_CLS_BIG];
        if (nbig == 0) continue;
        fr.assign(lists.begin() + P.off[KVX_CLS_BIG], lists.begin() + P.off[KVX_CLS_BIG] + nbig);
        auto emit = [&](std::vector<kvx_chol::ChainList> &out, int kb, bool far) {
            // far: the fronts with anything right of column kb + 2 u_block (update matrix included), by the order of that region
            auto region = [&](int32_t f) { return far ? S.sn_m[f] - std::min(kb + 2 * F->K.u_block, S.sn_k[f]) : S.sn_m[f]; };
            std::vector<int32_t> act;
            for (int32_t f : fr)
                if (S.sn_k[f] > kb && region(f) > 0) act.push_back(f);
            std::stable_sort(act.begin(), act.end(), [&](int32_t a, int32_t b) { return region(a) > region(b); });
            out.push_back(kvx_chol::ChainList{(int64_t)F->chain_host.size(), (int)act.size()});
            for (int32_t f : act) { F->chain_host.push_back(f); F->chain_m.push_back(S.sn_m[f]); F->chain_k.push_back(S.sn_k[f]); }
        };
        for (int jb = 0; jb < P.chain_maxk; jb += KVX_NB) emit(F->chain_steps[l], jb, false);
        for (int kb = 0; kb < P.chain_maxk; kb += F->K.u_block) emit(F->u_steps[l], kb, true);
    }
    if (F->d_chain) { (void)pool_free(F->d_chain); F->d_chain = nullptr; }
    if (F->chain_host.empty()) return KVX_OK;
    return upload(&F->d_chain, F->chain_host);
}

// size group of a leaf subtree: its largest front has at most 32 rows (0), at most 48 (1), more (2)
static int sub_group(const Symbolic &S, const SubDesc &d)
{
    int mm = 0;
    for (int q = d.lo; q <= d.hi; q++) mm = std::max(mm, S.sn_m[q]);
    return mm <= 32 ? 0 : (mm <= 48 ? 1 : 2);
}

int build_subtrees(kvx_chol *F)
{
    Symbolic &S = F->S;
    const bool enabled = F->K.use_subtrees && F->dist_nranks == 1 && (int64_t)S.rel.size() < INT32_MAX;
    std::vector<int32_t> lsw;
    F->sw_off.assign((size_t)S.nlevels, 0);
    F->sw_cnt.assign((size_t)S.nlevels, 0);
    F->sw_kmax.assign((size_t)S.nlevels, 0);
    F->sw_maxm.assign((size_t)S.nlevels, 0);
    for (int l = 0; l < S.nlevels; l++) {
        F->sw_off[l] = (int64_t)lsw.size();
        // the LDS-class fronts and the wave-class fronts left outside the subtrees share one launch per level and sweep
        int kmax = 0, maxm = 0;
        for (int64_t q = F->lptr_host[l]; q < F->lptr_host[l + 1]; q++) {
            const int32_t f = F->lists_host[q];
            const int c = front_class(S.sn_m[f], S.sn_k[f]);
            if (c == KVX_CLS_BIG || (c >= KVX_CLS_WAVE0 && enabled && F->in_sub[f])) continue;
            if (!enabled && c < KVX_CLS_WAVE0) continue;           // without subtrees: wave fronts only, their own launch
            lsw.push_back(f);
            kmax = std::max(kmax, (int)S.sn_k[f]);
            maxm = std::max(maxm, (int)S.sn_m[f]);
        }
        F->sw_cnt[l] = (int)((int64_t)lsw.size() - F->sw_off[l]);
        F->sw_kmax[l] = kmax;
        F->sw_maxm[l] = maxm;
    }
    if (lsw.empty()) lsw.push_back(0);
    std::vector<SubDesc> subs;
    F->nsub32 = 0;
    F->nsub48 = 0;
    for (int pass = 0; pass < 3; pass++)
        for (const SubDesc &d : F->subs_host) {
            if (sub_group(S, d) != pass) continue;
            subs.push_back(d);
            if (pass == 0) F->nsub32++;
            if (pass <= 1) F->nsub48++;
        }
    F->nsub = enabled ? (int)subs.size() : 0;
    F->sub_info[0] = F->nsub;
    F->sub_info[1] = 0;
    if (enabled)
        for (const SubDesc &d : subs) F->sub_info[1] += d.hi - d.lo + 1;
    F->sub_info_set = true;
    F->solve_merged = enabled;
    if (!enabled) { F->nsub32 = 0; F->nsub48 = 0; }
    if (subs.empty()) subs.push_back(SubDesc{0, -1, 0, 0});
    // edge records of the subtree walk: (update rows, offset of the relative indices, LDS stack offset) per tree edge
    std::vector<int32_t> cd_woff(3 * std::max<size_t>(S.children.size(), 1), 0);
    for (int64_t q = 0; q < S.nsuper; q++)
        for (int64_t c = S.childptr[q]; c < S.childptr[q + 1]; c++) {
            const int32_t ch = S.children[c];
            cd_woff[3 * c] = S.sn_m[ch] - S.sn_k[ch];
            cd_woff[3 * c + 1] = (int32_t)(S.rowptr[ch] + S.sn_k[ch]);
            cd_woff[3 * c + 2] = F->cd_woff_host[c];
        }
    int rc;
    for (void *p : {(void *)F->d_subs, (void *)F->d_cd_woff, (void *)F->d_lists_sw, (void *)F->d_depth})
        if (p) (void)pool_free(p);
    F->d_subs = nullptr; F->d_cd_woff = nullptr; F->d_lists_sw = nullptr; F->d_depth = nullptr;
    if ((rc = upload(&F->d_subs, subs))) return rc;
    if ((rc = upload(&F->d_cd_woff, cd_woff))) return rc;
    F->lsw_host = lsw;
    if ((rc = upload(&F->d_lists_sw, lsw))) return rc;
    // factorisation: the subtrees grouped by the LDS image their largest front needs (32 / 48 / 64 rows), and level lists without
    // their fronts (the fplan / d_flists pair the sharded mode uses for its own filtered lists; it keeps subtrees off)
    // Opt-in (KVX_FACTOR_SUBTREES=1).  Measured on MI355X, config 2: the two large groups of subtrees take 0.49 / 0.55 ms side by
    // side and the level loop reaches its first big front at 0.86 ms instead of 0.81; factor 3.69 -> 4.00 ms.  A front costs a
    // wavefront ~30 us under load either way (pivot sweeps are issue-bound FP64, the rest memory latency); the level schedule
    // keeps every front of a level in flight, a walk only one front per subtree.
    F->factor_subtrees = enabled && F->dist == nullptr && F->K.factor_subtrees;
    F->nsubf[0] = F->nsubf[1] = F->nsubf[2] = 0;
    if (F->factor_subtrees) {
        std::vector<SubDesc> fs;
        for (int g = 0; g < 3; g++)
            for (const SubDesc &d : F->subs_host)
                if (sub_group(S, d) == g) { fs.push_back(d); F->nsubf[g]++; }
        if (fs.empty()) fs.push_back(SubDesc{0, -1, 0, 0});
        if (F->d_subs_f) { (void)pool_free(F->d_subs_f); F->d_subs_f = nullptr; }
        if ((rc = upload(&F->d_subs_f, fs))) return rc;
        std::vector<int32_t> fl;
        std::vector<int64_t> flp((size_t)S.nlevels + 1, 0);
        for (int l = 0; l < S.nlevels; l++) {
            for (int64_t q = F->lptr_host[l]; q < F->lptr_host[l + 1]; q++)
                if (!F->in_sub[F->lists_host[q]]) fl.push_back(F->lists_host[q]);
            flp[l + 1] = (int64_t)fl.size();
        }
        if (F->d_flists) { (void)pool_free(F->d_flists); F->d_flists = nullptr; }
        if ((rc = upload(&F->d_flists, fl))) return rc;
        build_plan_from(S, fl, flp, F->fplan);
        F->fplan_on = true;
        F->flists_host = fl;
    }
    std::vector<int32_t> dep(S.depth.begin(), S.depth.end());
    if (dep.empty()) dep.push_back(0);
    if ((rc = upload(&F->d_depth, dep))) return rc;
    return build_chain_lists(F);
}

int ensure_device(kvx_chol *F)
{
    if (F->dev_ready) return KVX_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_err("no HIP device visible: the kvxhip numeric path has no CPU fallback");
        return KVX_EDEVICE;
    }
    Symbolic &S = F->S;
    F->K = read_chol_knobs();
    analyze_subtrees(F);
    HIPCHK(pool_stream_get(&F->stream));
    for (int i = 0; i < 4; i++) HIPCHK(pool_event_get(&F->ev[i], true));
    for (int i = 0; i < 3; i++) {
        HIPCHK(pool_stream_get(&F->side[i]));
        HIPCHK(pool_event_get(&F->ev_join[i], false));
    }
    HIPCHK(pool_event_get(&F->ev_fork, false));
    HIPCHK(pool_event_get(&F->ev_in, false));
    HIPCHK(pool_event_get(&F->ev_out, false));
    int rc;
    std::vector<int32_t> first((size_t)S.nsuper), perm32((size_t)S.n);
    for (int64_t s = 0; s < S.nsuper; s++) first[s] = (int32_t)S.super[s];
    for (int64_t i = 0; i < S.n; i++) perm32[i] = (int32_t)S.perm[i];
    if ((rc = upload(&F->d_k, S.sn_k))) return rc;
    if ((rc = upload(&F->d_m, S.sn_m))) return rc;
    if ((rc = upload(&F->d_first, first))) return rc;
    if ((rc = upload(&F->d_rowidx, S.rowidx))) return rc;
    if ((rc = upload(&F->d_rel, S.rel))) return rc;
    if ((rc = upload(&F->d_children, S.children))) return rc;
    if ((rc = upload(&F->d_perm, perm32))) return rc;
    if ((rc = upload(&F->d_lists, S.levellist))) return rc;
    std::vector<int64_t> px(S.px.begin(), S.px.end());
    if ((rc = upload(&F->d_px, px))) return rc;
    if ((rc = upload(&F->d_rowptr, S.rowptr))) return rc;
    if ((rc = upload(&F->d_ux, S.ux))) return rc;
    if ((rc = upload(&F->d_wx, S.wx))) return rc;
    if ((rc = upload(&F->d_childptr, S.childptr))) return rc;
    if ((rc = upload(&F->d_amap, S.amap))) return rc;
    if (S.nnzA < INT32_MAX && F->part.empty() && !F->K.init_two_passes) {
        // the scatter map once more, grouped by the chunk of the factor an entry goes to: k_init_factor zeroes L and scatters A in one
        // pass.  A counting sort ON THE DEVICE over the map just uploaded (histogram, the scan of the ~10^5 chunk counters on the host,
        // placement) -- on the host it was 12-18 ms of every first call on a new pattern with 3 M entries, more than a thousand of the
        // steps it speeds up by 0.05 ms would give back.  (Sharded factors keep the two launches: their layout is trimmed afterwards.)
        const int sh = init_factor_shift();
        const int64_t nchunk = std::max<int64_t>((S.lsize + ((int64_t)1 << sh) - 1) >> sh, 1);
        int64_t *d_cnt = nullptr;
        HIPCHK(pool_malloc((void **)&F->d_scptr, (size_t)(nchunk + 1) * sizeof(int64_t)));
        HIPCHK(pool_malloc((void **)&d_cnt, (size_t)(nchunk + 1) * sizeof(int64_t)));
        HIPCHK(pool_malloc((void **)&F->d_sdst, (size_t)std::max<int64_t>(S.nnzA, 1) * sizeof(int64_t)));
        HIPCHK(pool_malloc((void **)&F->d_ssrc, (size_t)std::max<int64_t>(S.nnzA, 1) * sizeof(int32_t)));
        HIPCHK(hipMemsetAsync(d_cnt, 0, (size_t)(nchunk + 1) * sizeof(int64_t), nullptr));
        launch_scatter_group_count(nullptr, F->d_amap, S.nnzA, sh, d_cnt);
        std::vector<int64_t> cptr((size_t)nchunk + 1);
        HIPCHK(hipMemcpy(cptr.data(), d_cnt, (size_t)(nchunk + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
        // slot q + 1 counted chunk q: the running sum turns the slots into "entries in the chunks before q", the start of chunk q
        std::vector<int64_t> start((size_t)nchunk + 1);
        int64_t run = 0;
        for (int64_t q = 0; q < nchunk; q++) { start[(size_t)q] = run; run += cptr[(size_t)q + 1]; }
        start[(size_t)nchunk] = run;
        HIPCHK(hipMemcpy(F->d_scptr, start.data(), (size_t)(nchunk + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_cnt, start.data(), (size_t)(nchunk + 1) * sizeof(int64_t), hipMemcpyHostToDevice));          // the cursors
        launch_scatter_group_place(nullptr, F->d_amap, S.nnzA, sh, d_cnt, F->d_sdst, F->d_ssrc);
        HIPCHK(hipDeviceSynchronize());
        (void)pool_free(d_cnt);
        F->scnt = run;
    }
    HIPCHK(pool_malloc((void **)&F->d_Lx, (std::max<int64_t>(S.lsize, 1) + 2) * sizeof(double)));   // + 2: k_syrk_lds reads row pairs (16-byte loads at clamped rows)
    for (int p = 0; p < 2; p++)
        HIPCHK(pool_malloc((void **)&F->d_U[p], std::max<int64_t>(S.upd_size[p], 1) * sizeof(double)));
    HIPCHK(pool_malloc((void **)&F->d_Ax, std::max<int64_t>(S.nnzA, 1) * sizeof(double)));
    HIPCHK(pool_malloc((void **)&F->d_status, sizeof(int)));
    HIPCHK(hipHostMalloc((void **)&F->h_status, sizeof(int), hipHostMallocMapped));
    *F->h_status = 0x7f7f7f7f;
    if (hipHostGetDevicePointer((void **)&F->h_status_dev, F->h_status, 0) != hipSuccess) { (void)hipGetLastError(); F->h_status_dev = nullptr; }
    std::vector<int64_t> &loff_host = F->linv_off_host;
    {
        // inverted diagonal blocks of the big fronts: ceil(k/NB) blocks of NB x NB each
        std::vector<int64_t> &loff = loff_host;
        loff.assign((size_t)S.nsuper, -1);
        int64_t tot = 0;
        for (int64_t s = 0; s < S.nsuper; s++)
            if (front_class(S.sn_m[s], S.sn_k[s]) == KVX_CLS_BIG && (F->part.empty() || F->part[s])) { loff[s] = tot; tot += (int64_t)((S.sn_k[s] + KVX_NB - 1) / KVX_NB) * KVX_NB * KVX_NB; }
        if ((rc = upload(&F->d_linv_off, loff))) return rc;
        HIPCHK(pool_malloc((void **)&F->d_Linv, std::max<int64_t>(tot, 1) * sizeof(double)));
        F->dev_bytes = (S.lsize + S.upd_size[0] + S.upd_size[1] + S.nnzA + tot) * (int64_t)sizeof(double);
    }
    {
        std::vector<FrontDesc> fd((size_t)S.nsuper);
        std::vector<ChildDesc> cd(S.children.size());
        std::vector<int32_t> tiles;
        for (int64_t s = 0; s < S.nsuper; s++) {
            FrontDesc &d = fd[s];
            d.k = S.sn_k[s]; d.m = S.sn_m[s]; d.first = (int32_t)S.super[s];
            d.nchild = (int32_t)(S.childptr[s + 1] - S.childptr[s]);
            d.px = S.px[s]; d.rowptr = S.rowptr[s]; d.ux = S.ux[s]; d.wx = S.wx[s]; d.childptr = S.childptr[s];
            d.linv = loff_host[s];
            for (int64_t c = S.childptr[s]; c < S.childptr[s + 1]; c++) {
                int32_t ch = S.children[c];
                ChildDesc &e = cd[c];
                e.kc = S.sn_k[ch]; e.uc = S.sn_m[ch] - S.sn_k[ch];
                e.rel = S.rowptr[ch] + S.sn_k[ch]; e.ux = S.ux[ch]; e.wx = S.wx[ch];
                e.tile = -1;
                if (front_class(d.m, d.k) == KVX_CLS_BIG) {
                    // tiles[x] = first update column j of the child with rel[j] >= x * KVX_ASM_TC
                    e.tile = (int64_t)tiles.size();
                    const int ntile = (d.m + KVX_ASM_TC - 1) / KVX_ASM_TC;
                    const int32_t *rl = S.rel.data() + e.rel;
                    int j = 0;
                    for (int x = 0; x <= ntile; x++) {
                        while (j < e.uc && rl[j] < x * KVX_ASM_TC) j++;
                        tiles.push_back(j);
                    }
                }
            }
        }
        if ((rc = upload(&F->d_fd, fd))) return rc;
        if ((rc = upload(&F->d_cd, cd))) return rc;
        if ((rc = upload(&F->d_tiles, tiles))) return rc;
    }
    F->ds = DevSym{F->d_k, F->d_m, F->d_first, F->d_px, F->d_rowptr, F->d_rowidx, F->d_rel,
                   F->d_ux, F->d_wx, F->d_childptr, F->d_children, F->d_linv_off, F->d_fd, F->d_cd, F->d_tiles, 0.0, 0.0};
    if (F->opts.dbound > 0.0) {
        // cholmod.options['dbound'] (cholmod.c:116-117; CHOLMOD: "entries of L_kk smaller than dbound are replaced by dbound").
        // reserved[3] = 1: replace by 1e64 instead -- the row drops out of the solves (the customary cure for normal equations
        // A D A' that lose rank numerically near the end of an interior-point run; used by lp.KKTDiagEqDev).
        F->ds.piv_floor = F->opts.dbound * F->opts.dbound;
        F->ds.piv_repl = F->opts.reserved[3] == 1 ? 1e128 : F->ds.piv_floor;
    }
    F->lists_host = S.levellist;
    F->lptr_host = S.levelptr;
    build_plan(F);
    if ((rc = build_subtrees(F))) return rc;
    F->dev_ready = true;
    return KVX_OK;
}

int ensure_solve_ws(kvx_chol *F, int64_t nrhs)
{
    if (nrhs <= F->x_cap) return KVX_OK;
    Symbolic &S = F->S;
    // room for two right-hand sides from the start: an interior-point loop solves with one at its starting point and with two
    // inside the iteration, and growing the workspace drops the captured sweeps -- which WAITS for an instantiation in flight
    // (10-20 ms inside the first iteration of a first call, measured)
    nrhs = std::max<int64_t>(nrhs, 2);
    for (auto &g : F->g_solve) g.exec.drop();
    F->g_solve.clear();                          // the captured sweeps point into the old workspace
    for (auto &g : F->g_fused) g.exec.drop();
    F->g_fused.clear();
    if (F->d_X) { (void)pool_free(F->d_X); F->d_X = nullptr; }
    if (F->d_X0) { (void)pool_free(F->d_X0); F->d_X0 = nullptr; }
    if (F->d_WK) { (void)pool_free(F->d_WK); F->d_WK = nullptr; }
    for (int p = 0; p < 2; p++)
        if (F->d_W[p]) { (void)pool_free(F->d_W[p]); F->d_W[p] = nullptr; }
    F->x_cap = 0;
    HIPCHK(pool_malloc((void **)&F->d_X, std::max<int64_t>(S.n * nrhs, 1) * sizeof(double)));
    HIPCHK(pool_malloc((void **)&F->d_X0, std::max<int64_t>(S.n * nrhs, 1) * sizeof(double)));
    HIPCHK(pool_malloc((void **)&F->d_WK, std::max<int64_t>(S.n * nrhs, 1) * sizeof(double)));
    const int64_t wmax = std::max(S.wrk_size[0], S.wrk_size[1]);   // common per-rhs stride of both parity buffers
    for (int p = 0; p < 2; p++)
        HIPCHK(pool_malloc((void **)&F->d_W[p], std::max<int64_t>(wmax * nrhs, 1) * sizeof(double)));
    F->x_cap = nrhs;
    return KVX_OK;
}

// ---- many right-hand sides: rhs-major blocks of 64 (kernels_wide.hip) ---------------------------------------------------------
// The inverse of the relative indices: for every row of every front, the rows of its children's update vectors that are added to
// it, children in list order (the order the single-rhs kernels add them in).  Host pass over the tree, once per analysis.
int ensure_wide(kvx_chol *F)
{
    if (F->wide_state != 0) return KVX_OK;
    Symbolic &S = F->S;
    F->wide_state = -1;
    if (F->dist_nranks != 1 || S.sum_m >= INT32_MAX - 1 || (int64_t)S.rel.size() >= INT32_MAX) return KVX_OK;
    if (std::max(S.wrk_size[0], S.wrk_size[1]) >= INT32_MAX) return KVX_OK;
    const int64_t nrow = S.rowptr[S.nsuper];
    std::vector<int32_t> ptr((size_t)nrow + 1, 0);
    for (int64_t s = 0; s < S.nsuper; s++)
        for (int64_t ci = S.childptr[s]; ci < S.childptr[s + 1]; ci++) {
            const int32_t c = S.children[ci];
            const int64_t kc = S.sn_k[c], uc = S.sn_m[c] - kc;
            const int32_t *rel = S.rel.data() + S.rowptr[c] + kc;
            for (int64_t i = 0; i < uc; i++) ptr[(size_t)(S.rowptr[s] + rel[i]) + 1]++;
        }
    for (int64_t r = 0; r < nrow; r++) ptr[(size_t)r + 1] += ptr[(size_t)r];
    std::vector<int32_t> src((size_t)std::max<int64_t>(ptr[(size_t)nrow], 1), 0);
    {
        std::vector<int32_t> cur(ptr.begin(), ptr.end() - 1);
        for (int64_t s = 0; s < S.nsuper; s++)
            for (int64_t ci = S.childptr[s]; ci < S.childptr[s + 1]; ci++) {
                const int32_t c = S.children[ci];
                const int64_t kc = S.sn_k[c], uc = S.sn_m[c] - kc;
                const int32_t *rel = S.rel.data() + S.rowptr[c] + kc;
                for (int64_t i = 0; i < uc; i++) src[(size_t)cur[(size_t)(S.rowptr[s] + rel[i])]++] = (int32_t)(S.wx[c] + i);
            }
    }
    int rc;
    std::vector<int32_t> ip32((size_t)S.n);
    for (int64_t j = 0; j < S.n; j++) ip32[(size_t)j] = (int32_t)S.iperm[(size_t)j];
    if ((rc = upload(&F->d_iperm, ip32))) return rc;
    if ((rc = upload(&F->d_inv_ptr, ptr))) return rc;
    if ((rc = upload(&F->d_inv_src, src))) return rc;
    F->wide_state = 1;
    return KVX_OK;
}
}  // namespace kvx
