// C-ABI entry points of the general-cone KKT assembly (include/kvxhip.h, kvx_cone_*): the plan of
//
//     S = Gs' Gs,   Gs = pack2(W^-T G)          (the reference's misc.kkt_chol, misc.py:1267-1277: scale, pack2, syrk)
//
// on a fixed sparsity pattern, for G with 'l' rows, 'q' cones and 's' blocks.  S is the sum over the blocks of their
// Gram matrices, each dense over the clique of columns that touch the block:
//   'l' rows and the plain part of the 'q' cones: G' diag(w) G with w = di^2 / 1 / beta_k^2 -- the kvx_atda plan (kkt_api.cpp)
//     of the 'l' + 'q' rows, whose P pattern is the union of the 'q' and 's' cliques, so its pattern is the whole of S;
//   'q' cone k: (4 |v_k|^2 p p' - 2 (p q' + q p')) / beta_k^2 with p = G_k' J v_k, q = G_k' v_k (W_k = beta_k (2 v_k v_k' - J));
//   's' block k: Y_k' Y_k with Y_k = pack2 of the congruence rti_k' G_k(:, j) rti_k of every clique column j (misc.py:1271-1272).
// The 'q' and 's' parts are gathered per entry of the P pattern in a fixed order (cones, then blocks, each by index) into
// the P values of the kvx_atda assembly: no floating-point atomics, the same bits on every run.
//
// kvx_cone_plan_h / kvx_cone_assemble_h_dev: S = H + Gs' Gs with a symmetric H given by its lower CCS pattern (coneqp: H = P,
// misc.py:1275-1277: K += H; symm(K)).  The P pattern is then the union of the cliques and tril(H), and the same gather adds
// the H value of an entry last (cones, then blocks, then H); an entry outside the cliques has no other source.
#include "../../include/kvxhip.h"
#include "abi_guard.hpp"
#include "cone.hpp"
#include "devpool.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace kvx;

#define HIPCHK(call)                                                             \
    do {                                                                         \
        hipError_t e_ = (call);                                                  \
        if (e_ != hipSuccess) return KVX_EDEVICE;                                \
    } while (0)

struct kvx_cone {
    int64_t ml = 0, nq = 0, ns = 0, n = 0, N = 0, mq = 0, gnz = 0;
    std::vector<int64_t> q, s;
    kvx_atda *T = nullptr;                      // 'l' + 'q' rows, with the P pattern of the cliques
    int64_t snz = 0;
    // 'l' + 'q' rows
    std::vector<int64_t> lq_idx;                // Gx positions of the entries of G_lq (its CCS order)
    std::vector<int32_t> rcone;                 // cone of every 'q' row
    // 'q' cones: (cone, clique column) pairs, cone by cone
    std::vector<int64_t> qoff;                  // nq + 1 row offsets inside the 'q' section
    int64_t npairs = 0;
    std::vector<int64_t> pr_ptr, pr_pos, pr_vrow;
    std::vector<int32_t> pr_head;
    // 's' blocks
    std::vector<int64_t> sc;                    // clique sizes c_k
    std::vector<int64_t> doff, yoff, goff, mpv, off2s;   // per block: dense, packed, Gram offsets; m(m+1)/2; offset in r / rti
    int64_t dtot = 0, ytot = 0, gtot = 0;       // dtot: doubles of ONE chunk buffer (dense columns, congruence workspace)
    std::vector<int64_t> chunk, fbase;          // per block: clique columns per chunk, index of its first (block, column) pair
    std::vector<int64_t> dsrc, ddst, dcolptr;   // densification, by (block, column): Gx position -> a m^2 + (lower-triangle row)
    std::vector<int64_t> tab;                   // per block {0, m^2, 0, m}: the one-block tables of kvx_nts_scale_dev
    std::vector<int64_t> f2, f1, fp;            // one pseudo-block per (block, column): the tables of one kvx_nts_pack_dev call
    std::vector<int32_t> tblk, ti, tj;          // Gram tiles
    // P pattern (the cliques) and its per-entry item lists
    std::vector<int64_t> Pp, Pi;
    std::vector<int64_t> qptr, qa, qb, sptr, sidx;
    std::vector<int32_t> qk;
    bool hasH = false;                          // planned with an H pattern (kvx_cone_plan_h with Hp != NULL)
    int64_t hnz = 0;                            // entries of the caller's H pattern (both triangles)
    std::vector<int64_t> hidx;                  // per entry of the P pattern: position of its H value, or -1
    // device
    bool dev = false;
    int64_t *d_lq = nullptr, *d_qoff = nullptr, *d_prptr = nullptr, *d_prpos = nullptr, *d_prvrow = nullptr;
    int32_t *d_rcone = nullptr, *d_prhead = nullptr, *d_qk = nullptr, *d_tblk = nullptr, *d_ti = nullptr, *d_tj = nullptr;
    int64_t *d_dsrc = nullptr, *d_ddst = nullptr, *d_tab = nullptr, *d_f2 = nullptr, *d_f1 = nullptr, *d_fp = nullptr;
    int64_t *d_yoff = nullptr, *d_mp = nullptr, *d_sc = nullptr, *d_goff = nullptr;
    int64_t *d_qptr = nullptr, *d_qa = nullptr, *d_qb = nullptr, *d_sptr = nullptr, *d_sidx = nullptr, *d_hidx = nullptr;
    double *d_w = nullptr, *d_glq = nullptr, *d_nv2 = nullptr, *d_p = nullptr, *d_q = nullptr, *d_D = nullptr, *d_work = nullptr,
           *d_Y = nullptr, *d_C = nullptr, *d_px = nullptr;
    std::vector<void *> owned;
};

namespace {

template <class T>
int up(kvx_cone *C, T **dst, const std::vector<T> &src)
{
    HIPCHK(pool_malloc((void **)dst, std::max<size_t>(src.size(), 1) * sizeof(T)));
    C->owned.push_back(*dst);
    if (!src.empty()) HIPCHK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return KVX_OK;
}

int scratch(kvx_cone *C, double **dst, int64_t count)
{
    HIPCHK(pool_malloc((void **)dst, (size_t)std::max<int64_t>(count, 1) * sizeof(double)));
    C->owned.push_back(*dst);
    return KVX_OK;
}

int cone_device(kvx_cone *C)
{
    if (C->dev) return KVX_OK;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return KVX_EDEVICE;
    int rc = 0;
#define UP(d, h) if ((rc = up(C, &C->d, C->h))) return rc
    UP(d_lq, lq_idx); UP(d_rcone, rcone); UP(d_qoff, qoff); UP(d_prptr, pr_ptr); UP(d_prpos, pr_pos); UP(d_prvrow, pr_vrow);
    UP(d_prhead, pr_head); UP(d_dsrc, dsrc); UP(d_ddst, ddst); UP(d_tab, tab); UP(d_f2, f2); UP(d_f1, f1); UP(d_fp, fp);
    UP(d_tblk, tblk); UP(d_ti, ti); UP(d_tj, tj); UP(d_yoff, yoff); UP(d_mp, mpv); UP(d_sc, sc); UP(d_goff, goff);
    UP(d_qptr, qptr); UP(d_qk, qk); UP(d_qa, qa); UP(d_qb, qb); UP(d_sptr, sptr); UP(d_sidx, sidx);
    if (C->hasH) UP(d_hidx, hidx);
#undef UP
    if ((rc = scratch(C, &C->d_w, C->ml + C->mq)) || (rc = scratch(C, &C->d_glq, (int64_t)C->lq_idx.size())) ||
        (rc = scratch(C, &C->d_nv2, C->nq)) || (rc = scratch(C, &C->d_p, C->npairs)) || (rc = scratch(C, &C->d_q, C->npairs)) ||
        (rc = scratch(C, &C->d_D, C->dtot)) || (rc = scratch(C, &C->d_work, C->dtot)) || (rc = scratch(C, &C->d_Y, C->ytot)) ||
        (rc = scratch(C, &C->d_C, C->gtot)) || (rc = scratch(C, &C->d_px, (int64_t)C->Pi.size())))
        return rc;
    C->dev = true;
    return KVX_OK;
}

struct Item {
    int64_t key;        // column * n + row of the entry of S
    int32_t cone;       // 'q' cone, -1 for an 's' Gram entry, -2 for an entry of H
    int64_t a, b;       // 'q': indices into p / q;  's': a = index into the Gram buffer;  H: a = position in Hx
};

}  // namespace

extern "C" {

// misc.py:1213-1277 (kkt_chol: Gs = pack2(W^-T G), K = Gs' Gs) -- the sparsity structure of that product, host only.
static int kvx_cone_plan_impl(int64_t ml, int64_t nq, const int64_t *q, int64_t ns, const int64_t *s, int64_t n, const int64_t *Gp,
                              const int64_t *Gi, const int64_t *Hp, const int64_t *Hi, kvx_cone **out)
{
    if (!out || ml < 0 || nq < 0 || ns < 0 || n < 0 || (n > 0 && !Gp) || (nq > 0 && !q) || (ns > 0 && !s)) return KVX_EINVAL;
    *out = nullptr;
    std::unique_ptr<kvx_cone> hold(new kvx_cone());
    kvx_cone *C = hold.get();
    C->ml = ml; C->nq = nq; C->ns = ns; C->n = n;
    C->q.assign(q, q + nq);
    C->s.assign(s, s + ns);
    C->qoff.assign((size_t)nq + 1, 0);
    for (int64_t k = 0; k < nq; k++) {
        if (q[k] < 1 || q[k] > ((int64_t)1 << 40)) { set_last_error("kvx_cone_plan: 'q' cones must have a positive order"); return KVX_EINVAL; }
        C->qoff[k + 1] = C->qoff[k] + q[k];
    }
    C->mq = C->qoff[nq];
    const int64_t mlq = ml + C->mq;
    C->off2s.assign((size_t)ns + 1, 0);
    for (int64_t k = 0; k < ns; k++) {
        if (s[k] < 0 || s[k] > 4096) { set_last_error("kvx_cone_plan: 's' blocks must have an order between 0 and 4096"); return KVX_EINVAL; }
        C->off2s[k + 1] = C->off2s[k] + s[k] * s[k];
    }
    const int64_t N = mlq + C->off2s[ns];
    C->N = N;
    const int64_t gnz = n ? Gp[n] : 0;
    if (n && Gp[0] != 0) return KVX_EINVAL;
    for (int64_t j = 0; j < n; j++)
        if (Gp[j + 1] < Gp[j]) return KVX_EINVAL;
    if (gnz > 0 && !Gi) return KVX_EINVAL;
    for (int64_t p = 0; p < gnz; p++)
        if (Gi[p] < 0 || Gi[p] >= N) { set_last_error("kvx_cone_plan: row index of G out of range"); return KVX_EINVAL; }
    C->gnz = gnz;
    if (Hp) {
        if (n && Hp[0] != 0) return KVX_EINVAL;
        for (int64_t j = 0; j < n; j++)
            if (Hp[j + 1] < Hp[j]) return KVX_EINVAL;
        C->hnz = n ? Hp[n] : 0;
        if (C->hnz > 0 && !Hi) return KVX_EINVAL;
        for (int64_t p = 0; p < C->hnz; p++)
            if (Hi[p] < 0 || Hi[p] >= n) { set_last_error("kvx_cone_plan_h: row index of H out of range"); return KVX_EINVAL; }
        C->hasH = true;
    }
    C->rcone.resize((size_t)C->mq);
    for (int64_t k = 0; k < nq; k++)
        for (int64_t r = C->qoff[k]; r < C->qoff[k + 1]; r++) C->rcone[r] = (int32_t)k;
    // which 's' block a row belongs to (-1: strict upper triangle or an 'l' / 'q' row)
    std::vector<int32_t> sblk;
    std::vector<int64_t> srow_local;
    auto s_of = [&](int64_t r, int64_t &lr) -> int64_t {
        if (r < mlq) return -1;
        const int64_t x = r - mlq;
        const int64_t k = std::upper_bound(C->off2s.begin(), C->off2s.end(), x) - C->off2s.begin() - 1;
        const int64_t m = s[k];
        lr = x - C->off2s[k];
        if (lr % m < lr / m) return -1;         // strict upper triangle: ignored, as scale and sgemv ignore it (misc.py:801-833)
        return k;
    };
    // ---- 'l' + 'q' rows: G_lq as a CCS of its own
    std::vector<int64_t> lqp((size_t)n + 1, 0), lqi;
    for (int64_t j = 0; j < n; j++) {
        for (int64_t p = Gp[j]; p < Gp[j + 1]; p++)
            if (Gi[p] < mlq) { C->lq_idx.push_back(p); lqi.push_back(Gi[p]); }
        lqp[j + 1] = (int64_t)lqi.size();
    }
    // ---- 'q' cliques: pairs (cone, column), cone by cone, columns ascending
    std::vector<int64_t> mark((size_t)std::max<int64_t>(nq, ns), -1), cnt((size_t)nq + 1, 0);
    for (int64_t j = 0; j < n; j++)
        for (int64_t p = Gp[j]; p < Gp[j + 1]; p++) {
            const int64_t r = Gi[p];
            if (r < ml || r >= mlq) continue;
            const int64_t k = C->rcone[r - ml];
            if (mark[k] != j) { mark[k] = j; cnt[k + 1]++; }
        }
    std::vector<int64_t> pqoff(cnt);
    for (int64_t k = 0; k < nq; k++) pqoff[k + 1] += pqoff[k];
    C->npairs = nq ? pqoff[nq] : 0;
    std::vector<int64_t> pcol((size_t)C->npairs), pcnt((size_t)C->npairs + 1, 0), cur(pqoff.begin(), pqoff.end()), last((size_t)nq, -1);
    std::fill(mark.begin(), mark.end(), -1);
    for (int64_t j = 0; j < n; j++)
        for (int64_t p = Gp[j]; p < Gp[j + 1]; p++) {
            const int64_t r = Gi[p];
            if (r < ml || r >= mlq) continue;
            const int64_t k = C->rcone[r - ml];
            if (mark[k] != j) { mark[k] = j; last[k] = cur[k]++; pcol[last[k]] = j; }
            pcnt[last[k] + 1]++;
        }
    C->pr_ptr.assign(pcnt.begin(), pcnt.end());
    for (int64_t t = 0; t < C->npairs; t++) C->pr_ptr[t + 1] += C->pr_ptr[t];
    C->pr_pos.resize((size_t)C->pr_ptr[C->npairs]);
    C->pr_vrow.resize(C->pr_pos.size());
    C->pr_head.resize(C->pr_pos.size());
    {
        std::vector<int64_t> fill(C->pr_ptr.begin(), C->pr_ptr.end() - 1);
        std::fill(mark.begin(), mark.end(), -1);
        std::vector<int64_t> cur2(pqoff.begin(), pqoff.end());
        for (int64_t j = 0; j < n; j++)
            for (int64_t p = Gp[j]; p < Gp[j + 1]; p++) {
                const int64_t r = Gi[p];
                if (r < ml || r >= mlq) continue;
                const int64_t k = C->rcone[r - ml];
                if (mark[k] != j) { mark[k] = j; last[k] = cur2[k]++; }
                const int64_t e = fill[last[k]]++;
                C->pr_pos[e] = p;
                C->pr_vrow[e] = r - ml;
                C->pr_head[e] = (r - ml == C->qoff[k]) ? 1 : 0;
            }
    }
    // ---- 's' cliques (lower triangles only) and the densification map
    std::vector<std::vector<int64_t>> scol((size_t)ns);
    std::fill(mark.begin(), mark.end(), -1);
    for (int64_t j = 0; j < n; j++)
        for (int64_t p = Gp[j]; p < Gp[j + 1]; p++) {
            int64_t lr = 0;
            const int64_t k = s_of(Gi[p], lr);
            if (k < 0) continue;
            if (mark[k] != j) { mark[k] = j; scol[k].push_back(j); }
        }
    int64_t ws = (int64_t)1 << 26;              // KVX_CONE_WS_DOUBLES overrides (tests run the chunked path on small blocks)
    if (const char *e = getenv("KVX_CONE_WS_DOUBLES")) ws = std::max<int64_t>(1, atoll(e));
    C->sc.resize((size_t)ns); C->doff.resize((size_t)ns); C->yoff.resize((size_t)ns); C->goff.resize((size_t)ns); C->mpv.resize((size_t)ns);
    for (int64_t k = 0; k < ns; k++) {
        const int64_t m = s[k], c = (int64_t)scol[k].size();
        C->sc[k] = c; C->mpv[k] = m * (m + 1) / 2;
        // the dense columns and the congruence workspace are processed in chunks of at most ws doubles each (at least one column)
        const int64_t ch = m ? std::max<int64_t>(1, std::min<int64_t>({c, 65535, ws / (m * m)})) : std::max<int64_t>(c, 1);
        C->chunk.push_back(ch);
        C->fbase.push_back((int64_t)C->f2.size());
        C->doff[k] = 0; C->yoff[k] = C->ytot; C->goff[k] = C->gtot;
        C->dtot = std::max<int64_t>(C->dtot, m * m * std::min<int64_t>(ch, c)); C->ytot += C->mpv[k] * c; C->gtot += c * c;
        C->tab.insert(C->tab.end(), {0, m * m, 0, m});
        for (int64_t a = 0; a < c; a++) {
            C->f2.push_back((a % ch) * m * m);
            C->fp.push_back(C->yoff[k] + a * C->mpv[k]);
        }
        const int64_t nt = (c + 15) / 16;
        for (int64_t x = 0; x < nt; x++)
            for (int64_t y = 0; y <= x; y++) { C->tblk.push_back((int32_t)k); C->ti.push_back((int32_t)x); C->tj.push_back((int32_t)y); }
    }
    // f1 holds cumulative orders: pseudo-block t has order f1[t + 1] - f1[t]
    {
        std::vector<int64_t> f1;
        f1.push_back(0);
        for (int64_t k = 0; k < ns; k++)
            for (int64_t a = 0; a < C->sc[k]; a++) f1.push_back(f1.back() + s[k]);
        C->f1.swap(f1);
    }
    {
        // entries grouped by (block, clique column): pair t = fbase_k + a owns [dcolptr[t], dcolptr[t + 1])
        const int64_t npair = (int64_t)C->f2.size();
        std::vector<int64_t> pos((size_t)ns, 0), cnt((size_t)npair + 1, 0), tof;
        std::vector<int64_t> lrs;
        std::fill(mark.begin(), mark.end(), -1);
        for (int64_t j = 0; j < n; j++)
            for (int64_t p = Gp[j]; p < Gp[j + 1]; p++) {
                int64_t lr = 0;
                const int64_t k = s_of(Gi[p], lr);
                if (k < 0) continue;
                if (mark[k] != j) { mark[k] = j; pos[k]++; }
                const int64_t tp = C->fbase[k] + pos[k] - 1;
                cnt[tp + 1]++;
                tof.push_back(tp); lrs.push_back((pos[k] - 1) * s[k] * s[k] + lr); C->dsrc.push_back(p);
            }
        for (int64_t x = 0; x < npair; x++) cnt[x + 1] += cnt[x];
        C->dcolptr = cnt;
        std::vector<int64_t> src(C->dsrc.size()), dst(C->dsrc.size()), fill(cnt.begin(), cnt.end() - 1);
        for (size_t e = 0; e < tof.size(); e++) { const int64_t u = fill[tof[e]]++; src[u] = C->dsrc[e]; dst[u] = lrs[e]; }
        C->dsrc.swap(src);
        C->ddst.swap(dst);
    }
    // ---- P pattern: the union of the cliques, with its item lists in a fixed order ('q' cones by index, then 's' blocks)
    std::vector<Item> items;
    for (int64_t k = 0; k < nq; k++) {
        const int64_t c = pqoff[k + 1] - pqoff[k];
        for (int64_t b = 0; b < c; b++)
            for (int64_t a = b; a < c; a++)
                items.push_back(Item{pcol[pqoff[k] + b] * n + pcol[pqoff[k] + a], (int32_t)k, pqoff[k] + a, pqoff[k] + b});
    }
    for (int64_t k = 0; k < ns; k++) {
        const int64_t c = C->sc[k];
        for (int64_t b = 0; b < c; b++)
            for (int64_t a = b; a < c; a++)
                items.push_back(Item{scol[k][b] * n + scol[k][a], -1, C->goff[k] + a + c * b, 0});
    }
    if (Hp)                                     // lower triangle of H; what lies above the diagonal is ignored (misc.py:1275-1277)
        for (int64_t j = 0; j < n; j++)
            for (int64_t p = Hp[j]; p < Hp[j + 1]; p++)
                if (Hi[p] >= j) items.push_back(Item{j * n + Hi[p], -2, p, 0});
    std::stable_sort(items.begin(), items.end(), [](const Item &x, const Item &y) { return x.key < y.key; });
    C->Pp.assign((size_t)n + 1, 0);
    C->qptr.push_back(0);
    C->sptr.push_back(0);
    for (size_t u = 0; u < items.size();) {
        const int64_t key = items[u].key;
        C->Pi.push_back(key % n);
        C->Pp[key / n + 1]++;
        int64_t hpos = -1;
        for (; u < items.size() && items[u].key == key; u++) {
            if (items[u].cone >= 0) { C->qk.push_back(items[u].cone); C->qa.push_back(items[u].a); C->qb.push_back(items[u].b); }
            else if (items[u].cone == -1) C->sidx.push_back(items[u].a);
            else if (hpos < 0) hpos = items[u].a;
            else { set_last_error("kvx_cone_plan_h: the pattern of H holds an entry twice"); return KVX_EINVAL; }
        }
        if (Hp) C->hidx.push_back(hpos);
        C->qptr.push_back((int64_t)C->qk.size());
        C->sptr.push_back((int64_t)C->sidx.size());
    }
    for (int64_t j = 0; j < n; j++) C->Pp[j + 1] += C->Pp[j];
    int rc = kvx_atda_plan(mlq, n, lqp.data(), lqi.data(), C->Pp.data(), C->Pi.data(), &C->T);
    if (rc) return rc;
    rc = kvx_atda_pattern(C->T, &C->snz, nullptr, nullptr);
    if (rc) return rc;
    *out = hold.release();
    return KVX_OK;
}

int kvx_cone_plan(int64_t ml, int64_t nq, const int64_t *q, int64_t ns, const int64_t *s, int64_t n, const int64_t *Gp,
                  const int64_t *Gi, kvx_cone **out)
{
    return guarded([&] { return kvx_cone_plan_impl(ml, nq, q, ns, s, n, Gp, Gi, nullptr, nullptr, out); });
}

int kvx_cone_plan_h(int64_t ml, int64_t nq, const int64_t *q, int64_t ns, const int64_t *s, int64_t n, const int64_t *Gp,
                    const int64_t *Gi, const int64_t *Hp, const int64_t *Hi, kvx_cone **out)
{
    return guarded([&] { return kvx_cone_plan_impl(ml, nq, q, ns, s, n, Gp, Gi, Hp, Hi, out); });
}

int kvx_cone_pattern(kvx_cone *C, int64_t *snz, int64_t *Sp, int64_t *Si)
{
    if (!C) return KVX_EINVAL;
    return kvx_atda_pattern(C->T, snz, Sp, Si);
}

static int kvx_cone_assemble_impl(kvx_cone *C, const double *Gx, const double *di, const double *v, const double *beta,
                                  const double *rti, const double *Hx, double *Sx)
{
    if (C && Hx && !C->hasH) { set_last_error("kvx_cone_assemble_h_dev: the plan has no H pattern"); return KVX_EINVAL; }
    if (C && C->hasH && C->hnz && !Hx) {
        set_last_error("kvx_cone_assemble_dev: the plan has an H pattern, its values go through kvx_cone_assemble_h_dev");
        return KVX_EINVAL;
    }
    if (!C || !Sx || (C->gnz && !Gx) || (C->ml && !di) || (C->nq && (!v || !beta)) || (C->dtot && !rti)) return KVX_EINVAL;
    int rc = cone_device(C);
    if (rc) return rc;
    const int64_t nlq = (int64_t)C->lq_idx.size();
    if (C->ml + C->mq) launch_cone_weights(nullptr, C->ml, C->mq, C->d_rcone, di, beta, C->d_w);
    launch_cone_gather(nullptr, nlq, C->d_lq, Gx, C->d_glq);
    if (C->npairs) {                                            // 'q': p, q of every (cone, column) pair, |v_k|^2
        launch_cone_vnorm(nullptr, C->nq, C->d_qoff, v, C->d_nv2);
        launch_cone_pq(nullptr, C->npairs, C->d_prptr, C->d_prpos, C->d_prvrow, C->d_prhead, Gx, v, C->d_p, C->d_q);
    }
    if (C->dtot) {                                              // 's': densify, congruence, pack2, Gram
        // column chunks of every block through one dense buffer: densify, congruence, pack2 into Y (Y and the Gram buffer are whole)
        for (int64_t k = 0; k < C->ns; k++) {
            const int64_t m = C->s[k], c = C->sc[k], ch = C->chunk[k];
            for (int64_t c0 = 0; c0 < c && m; c0 += ch) {
                const int64_t nc = std::min<int64_t>(ch, c - c0), t0 = C->fbase[k] + c0;
                const int64_t e0 = C->dcolptr[t0], e1 = C->dcolptr[t0 + nc];
                HIPCHK(hipMemsetAsync(C->d_D, 0, nc * m * m * sizeof(double), nullptr));
                launch_cone_move(nullptr, e1 - e0, C->d_dsrc + e0, Gx, C->d_ddst + e0, c0 * m * m, C->d_D);
                rc = kvx_nts_scale_dev(1, C->d_tab + 4 * k, C->d_tab + 4 * k + 2, rti + C->off2s[k], C->d_D, m * m, nc, 0, C->d_work, m * m);
                if (rc) return rc;
                if ((rc = kvx_nts_pack_dev(nc, C->d_f2 + t0, C->d_f1 + t0, C->d_fp + t0, C->d_D, C->d_Y, 2))) return rc;
            }
        }
        launch_cone_gram(nullptr, (int64_t)C->tblk.size(), C->d_tblk, C->d_ti, C->d_tj, C->d_yoff, C->d_mp, C->d_sc, C->d_goff, C->d_Y, C->d_C);
    }
    const int64_t pnz = (int64_t)C->Pi.size();
    launch_cone_pgather(nullptr, pnz, C->d_qptr, C->d_qk, C->d_qa, C->d_qb, C->d_p, C->d_q, C->d_nv2, beta, C->d_sptr, C->d_sidx, C->d_C,
                        C->hasH && C->hnz ? C->d_hidx : nullptr, Hx, C->d_px);
    HIPCHK(hipGetLastError());
    return kvx_atda_assemble_dev(C->T, C->d_glq, C->d_w, pnz ? C->d_px : nullptr, Sx);
}

int kvx_cone_assemble_dev(kvx_cone *C, const double *Gx_dev, const double *di_dev, const double *v_dev, const double *beta_dev,
                          const double *rti_dev, double *Sx_dev)
{
    return guarded([&] { return kvx_cone_assemble_impl(C, Gx_dev, di_dev, v_dev, beta_dev, rti_dev, nullptr, Sx_dev); });
}

int kvx_cone_assemble_h_dev(kvx_cone *C, const double *Gx_dev, const double *di_dev, const double *v_dev, const double *beta_dev,
                            const double *rti_dev, const double *Hx_dev, double *Sx_dev)
{
    return guarded([&] { return kvx_cone_assemble_impl(C, Gx_dev, di_dev, v_dev, beta_dev, rti_dev, Hx_dev, Sx_dev); });
}

void kvx_cone_free(kvx_cone *C)
{
    if (!C) return;
    for (void *p : C->owned) (void)pool_free(p);
    if (C->T) kvx_atda_free(C->T);
    delete C;
}

int kvx_vec_scatter_dev(int64_t n, const double *x_dev, const int64_t *idx_dev, double *y_dev)
{
    if (n < 0) return KVX_EINVAL;
    launch_cone_scatter(nullptr, n, idx_dev, x_dev, y_dev);
    HIPCHK(hipGetLastError());
    return KVX_OK;
}

int kvx_nts_colscale_dev(int64_t ns, const int64_t *off2_dev, const int64_t *off1_dev, double *x_dev, const double *w_dev)
{
    if (ns < 0) return KVX_EINVAL;
    launch_nts_colscale(nullptr, ns, off2_dev, off1_dev, x_dev, w_dev);
    HIPCHK(hipGetLastError());
    return KVX_OK;
}

}  // extern "C"
