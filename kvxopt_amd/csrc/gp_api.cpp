// C-ABI entry points of the geometric-program evaluator (include/kvxhip.h, kvx_gp_*): the plan of the log-sum-exp blocks
//
//     f_i(x) = log sum_k exp(F_i x + g_i)_k,  i = 0..m        (the reference's Fgp closure, cvxprog.py:2094-2153)
//
// and its evaluation in HBM.  The plan (host only) sorts the CCS of F by rows inside every column, so that the entries of one
// block in one column -- a "segment", one entry of Df -- lie together; it keeps
//   a CSR view of F (row pointers, columns, positions of the values in the caller's Fx) for y = F x + g,
//   the segments with the pattern of Df (row i of Df: the columns the rows of block i meet),
//   per block the dense K_i x c_i factor Fsc_i = diag(y_i)^1/2 (F_i - 1 Df_i) over its c_i columns and the c_i x c_i Gram matrix,
//   the lower pattern of H (the union of the cliques of the blocks) with, per entry, its Gram entries in block order.
// The values of F are read from the caller's buffer at every evaluation through the position maps: nothing of F is copied.
#include "../../include/kvxhip.h"
#include "abi_guard.hpp"
#include "cone.hpp"
#include "devpool.hpp"
#include "gp.hpp"

#include <algorithm>
#include <memory>
#include <vector>

using namespace kvx;

#define HIPCHK(call)                                                             \
    do {                                                                         \
        hipError_t e_ = (call);                                                  \
        if (e_ != hipSuccess) return KVX_EDEVICE;                                \
    } while (0)

struct kvx_gp {
    int64_t nblk = 0, n = 0, l = 0, nnz = 0, dnz = 0, hnz = 0, dtot = 0, gtot = 0;
    std::vector<int64_t> boff;                  // nblk + 1 row offsets of the blocks
    std::vector<int64_t> rp, ci, src;           // CSR view of F; src: position of the value in Fx
    std::vector<int64_t> pos, row;              // F sorted by (column, row): position in Fx, row
    std::vector<int64_t> seg, dfe;              // dnz + 1 segment starts in the sorted order; segment of every sorted entry
    std::vector<int64_t> Dfp, Dfi;              // CCS pattern of Df ((m + 1) x n): entry e is segment e
    std::vector<int64_t> coff, dpos;            // per block: its columns' entries of Df, columns ascending
    std::vector<int64_t> foff, goff, dd;        // dense factors, Gram matrices; place of every sorted entry in its dense factor
    std::vector<int64_t> kb, cb;                // per block K_i, c_i (the tables of launch_cone_gram)
    std::vector<int32_t> tblk, ti, tj;          // Gram tiles
    std::vector<int64_t> Hp, Hi, hptr, hidx;    // lower pattern of H and its items
    std::vector<int32_t> hblk;
    std::vector<int64_t> lst[3], glst[2];       // blocks by size class; entries of Df by segment length
    // device
    bool dev = false;
    int64_t *d_boff = nullptr, *d_rp = nullptr, *d_ci = nullptr, *d_src = nullptr, *d_pos = nullptr, *d_row = nullptr, *d_seg = nullptr,
            *d_dfe = nullptr, *d_coff = nullptr, *d_dpos = nullptr, *d_foff = nullptr, *d_goff = nullptr, *d_dd = nullptr, *d_kb = nullptr,
            *d_cb = nullptr, *d_hptr = nullptr, *d_hidx = nullptr, *d_lst[3] = {nullptr, nullptr, nullptr}, *d_glst[2] = {nullptr, nullptr};
    int32_t *d_tblk = nullptr, *d_ti = nullptr, *d_tj = nullptr, *d_hblk = nullptr;
    double *d_y = nullptr, *d_D = nullptr, *d_C = nullptr;
    std::vector<void *> owned;
};

namespace {

template <class T>
int up(kvx_gp *P, T **dst, const std::vector<T> &src)
{
    HIPCHK(pool_malloc((void **)dst, std::max<size_t>(src.size(), 1) * sizeof(T)));
    P->owned.push_back(*dst);
    if (!src.empty()) HIPCHK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return KVX_OK;
}

int scratch(kvx_gp *P, double **dst, int64_t count)
{
    HIPCHK(pool_malloc((void **)dst, (size_t)std::max<int64_t>(count, 1) * sizeof(double)));
    P->owned.push_back(*dst);
    return KVX_OK;
}

int gp_device(kvx_gp *P)
{
    if (P->dev) return KVX_OK;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) {
        set_last_error("kvx_gp_eval_dev: no HIP device; the evaluation has no CPU fallback");
        return KVX_EDEVICE;
    }
    int rc = 0;
#define UP(d, h) if ((rc = up(P, &P->d, P->h))) return rc
    UP(d_boff, boff); UP(d_rp, rp); UP(d_ci, ci); UP(d_src, src); UP(d_pos, pos); UP(d_row, row); UP(d_seg, seg); UP(d_dfe, dfe);
    UP(d_coff, coff); UP(d_dpos, dpos); UP(d_foff, foff); UP(d_goff, goff); UP(d_dd, dd); UP(d_kb, kb); UP(d_cb, cb);
    UP(d_hptr, hptr); UP(d_hidx, hidx); UP(d_hblk, hblk); UP(d_tblk, tblk); UP(d_ti, ti); UP(d_tj, tj);
    UP(d_lst[0], lst[0]); UP(d_lst[1], lst[1]); UP(d_lst[2], lst[2]); UP(d_glst[0], glst[0]); UP(d_glst[1], glst[1]);
#undef UP
    if ((rc = scratch(P, &P->d_y, P->l)) || (rc = scratch(P, &P->d_D, P->dtot)) || (rc = scratch(P, &P->d_C, P->gtot))) return rc;
    P->dev = true;
    return KVX_OK;
}

struct HItem {
    int64_t key;        // column * n + row of the entry of H
    int32_t blk;
    int64_t idx;        // its entry of the block's Gram matrix
};

int gp_plan_impl(int64_t nblk, const int64_t *K, int64_t n, const int64_t *Fp, const int64_t *Fi, kvx_gp **out)
{
    if (!out || nblk < 1 || !K || n < 0 || (n > 0 && !Fp)) return KVX_EINVAL;
    *out = nullptr;
    std::unique_ptr<kvx_gp> hold(new kvx_gp());
    kvx_gp *P = hold.get();
    P->nblk = nblk; P->n = n;
    P->boff.assign((size_t)nblk + 1, 0);
    for (int64_t b = 0; b < nblk; b++) {
        if (K[b] < 1 || K[b] > ((int64_t)1 << 40)) { set_last_error("kvx_gp_plan: 'K' must hold positive integers"); return KVX_EINVAL; }
        P->boff[b + 1] = P->boff[b] + K[b];
    }
    const int64_t l = P->boff[nblk];
    P->l = l;
    if (n && Fp[0] != 0) return KVX_EINVAL;
    for (int64_t j = 0; j < n; j++)
        if (Fp[j + 1] < Fp[j]) return KVX_EINVAL;
    const int64_t nnz = n ? Fp[n] : 0;
    if (nnz > 0 && !Fi) return KVX_EINVAL;
    for (int64_t p = 0; p < nnz; p++)
        if (Fi[p] < 0 || Fi[p] >= l) { set_last_error("kvx_gp_plan: row index of F out of range"); return KVX_EINVAL; }
    P->nnz = nnz;
    std::vector<int64_t> blk_of((size_t)l);
    for (int64_t b = 0; b < nblk; b++)
        for (int64_t r = P->boff[b]; r < P->boff[b + 1]; r++) blk_of[r] = b;
    // ---- F sorted by rows inside every column; the segments and the pattern of Df
    P->pos.resize((size_t)nnz); P->row.resize((size_t)nnz); P->dfe.resize((size_t)nnz);
    P->Dfp.assign((size_t)n + 1, 0);
    std::vector<int64_t> la;                                    // per segment: index of its column among the columns of its block
    std::vector<int64_t> cnt((size_t)nblk, 0);
    for (int64_t j = 0; j < n; j++) {
        const int64_t p0 = Fp[j], p1 = Fp[j + 1];
        for (int64_t p = p0; p < p1; p++) P->pos[p] = p;
        std::sort(P->pos.begin() + p0, P->pos.begin() + p1, [&](int64_t a, int64_t b) { return Fi[a] < Fi[b]; });
        int64_t last = -1;
        for (int64_t q = p0; q < p1; q++) {
            const int64_t r = Fi[P->pos[q]];
            if (q > p0 && r == P->row[q - 1]) { set_last_error("kvx_gp_plan: the pattern of F holds an entry twice"); return KVX_EINVAL; }
            P->row[q] = r;
            const int64_t b = blk_of[r];
            if (b != last) {
                last = b;
                P->seg.push_back(q);
                P->Dfi.push_back(b);
                la.push_back(cnt[b]++);
            }
            P->dfe[q] = (int64_t)P->seg.size() - 1;
        }
        P->Dfp[j + 1] = (int64_t)P->Dfi.size();
    }
    P->seg.push_back(nnz);
    P->dnz = (int64_t)P->Dfi.size();
    // ---- per block: its columns (ascending) as entries of Df, the dense factor and the Gram matrix
    P->coff.assign((size_t)nblk + 1, 0); P->foff.assign((size_t)nblk + 1, 0); P->goff.assign((size_t)nblk + 1, 0);
    P->kb.resize((size_t)nblk); P->cb.resize((size_t)nblk);
    for (int64_t b = 0; b < nblk; b++) {
        const int64_t c = cnt[b];
        P->kb[b] = K[b]; P->cb[b] = c;
        P->coff[b + 1] = P->coff[b] + c;
        P->foff[b + 1] = P->foff[b] + K[b] * c;
        P->goff[b + 1] = P->goff[b] + c * c;
        const int64_t nt = (c + 15) / 16;
        for (int64_t x = 0; x < nt; x++)
            for (int64_t y = 0; y <= x; y++) { P->tblk.push_back((int32_t)b); P->ti.push_back((int32_t)x); P->tj.push_back((int32_t)y); }
        P->lst[K[b] <= GP_SMALL_MAX ? 0 : (K[b] <= GP_WAVE_MAX ? 1 : 2)].push_back(b);
    }
    P->dtot = P->foff[nblk]; P->gtot = P->goff[nblk];
    P->dpos.resize((size_t)P->dnz);
    std::vector<int64_t> bcol((size_t)P->dnz);                  // column of every entry of dpos
    for (int64_t j = 0; j < n; j++)
        for (int64_t e = P->Dfp[j]; e < P->Dfp[j + 1]; e++) {
            const int64_t u = P->coff[P->Dfi[e]] + la[e];
            P->dpos[u] = e;
            bcol[u] = j;
        }
    for (int64_t e = 0; e < P->dnz; e++) P->glst[P->seg[e + 1] - P->seg[e] > GP_SEG_WAVE ? 1 : 0].push_back(e);
    P->dd.resize((size_t)nnz);
    for (int64_t q = 0; q < nnz; q++) {
        const int64_t e = P->dfe[q], b = P->Dfi[e];
        P->dd[q] = P->foff[b] + la[e] * K[b] + (P->row[q] - P->boff[b]);
    }
    // ---- CSR view (columns ascending inside every row)
    P->rp.assign((size_t)l + 1, 0);
    for (int64_t q = 0; q < nnz; q++) P->rp[P->row[q] + 1]++;
    for (int64_t r = 0; r < l; r++) P->rp[r + 1] += P->rp[r];
    P->ci.resize((size_t)nnz); P->src.resize((size_t)nnz);
    {
        std::vector<int64_t> fill(P->rp.begin(), P->rp.end() - 1);
        for (int64_t j = 0; j < n; j++)
            for (int64_t q = Fp[j]; q < Fp[j + 1]; q++) {
                const int64_t u = fill[P->row[q]]++;
                P->ci[u] = j;
                P->src[u] = P->pos[q];
            }
    }
    // ---- lower pattern of H: the union of the cliques, the items of an entry in block order
    std::vector<HItem> items;
    for (int64_t b = 0; b < nblk; b++) {
        const int64_t c = P->cb[b], o = P->coff[b];
        for (int64_t y = 0; y < c; y++)
            for (int64_t x = y; x < c; x++) items.push_back(HItem{bcol[o + y] * n + bcol[o + x], (int32_t)b, P->goff[b] + x + c * y});
    }
    std::stable_sort(items.begin(), items.end(), [](const HItem &x, const HItem &y) { return x.key < y.key; });
    P->Hp.assign((size_t)n + 1, 0);
    P->hptr.push_back(0);
    for (size_t u = 0; u < items.size();) {
        const int64_t key = items[u].key;
        P->Hi.push_back(key % n);
        P->Hp[key / n + 1]++;
        for (; u < items.size() && items[u].key == key; u++) { P->hblk.push_back(items[u].blk); P->hidx.push_back(items[u].idx); }
        P->hptr.push_back((int64_t)P->hblk.size());
    }
    for (int64_t j = 0; j < n; j++) P->Hp[j + 1] += P->Hp[j];
    P->hnz = (int64_t)P->Hi.size();
    *out = hold.release();
    return KVX_OK;
}

int gp_eval_impl(kvx_gp *P, const double *Fx, const double *g, const double *x, const double *z, double *f, double *Dfx, double *Hx)
{
    if (!P || !g || !f || (P->nnz && !Fx) || (P->n && !x) || (P->dnz && !Dfx)) return KVX_EINVAL;
    if (z && P->hnz && !Hx) { set_last_error("kvx_gp_eval_dev: z is given, Hx_dev is not"); return KVX_EINVAL; }
    int rc = gp_device(P);
    if (rc) return rc;
    for (int c = 0; c < 3; c++)
        launch_gp_lse(nullptr, c, (int64_t)P->lst[c].size(), P->d_lst[c], P->d_boff, P->d_rp, P->d_ci, P->d_src, Fx, g, x, P->d_y, f);
    for (int w = 0; w < 2; w++)
        launch_gp_grad(nullptr, w, (int64_t)P->glst[w].size(), P->d_glst[w], P->d_seg, P->d_pos, P->d_row, Fx, P->d_y, Dfx);
    if (z && P->hnz) {
        launch_gp_fsc_fill(nullptr, P->dtot, P->nblk, P->d_foff, P->d_boff, P->d_coff, P->d_dpos, Dfx, P->d_y, P->d_D);
        launch_gp_fsc_nz(nullptr, P->nnz, P->d_pos, P->d_row, P->d_dd, P->d_dfe, Fx, Dfx, P->d_y, P->d_D);
        launch_cone_gram(nullptr, (int64_t)P->tblk.size(), P->d_tblk, P->d_ti, P->d_tj, P->d_foff, P->d_kb, P->d_cb, P->d_goff, P->d_D, P->d_C);
        launch_gp_hgather(nullptr, P->hnz, P->d_hptr, P->d_hblk, P->d_hidx, z, P->d_C, Hx);
    }
    HIPCHK(hipGetLastError());
    return KVX_OK;
}

}  // namespace

extern "C" {

int kvx_gp_plan(int64_t nblk, const int64_t *K, int64_t n, const int64_t *Fp, const int64_t *Fi, kvx_gp **out)
{
    return guarded([&] { return gp_plan_impl(nblk, K, n, Fp, Fi, out); });
}

int kvx_gp_pattern(kvx_gp *P, int64_t *dnz, int64_t *Dfp, int64_t *Dfi, int64_t *hnz, int64_t *Hp, int64_t *Hi)
{
    if (!P) return KVX_EINVAL;
    if (dnz) *dnz = P->dnz;
    if (hnz) *hnz = P->hnz;
    if (Dfp) std::copy(P->Dfp.begin(), P->Dfp.end(), Dfp);
    if (Dfi) std::copy(P->Dfi.begin(), P->Dfi.end(), Dfi);
    if (Hp) std::copy(P->Hp.begin(), P->Hp.end(), Hp);
    if (Hi) std::copy(P->Hi.begin(), P->Hi.end(), Hi);
    return KVX_OK;
}

int kvx_gp_eval_dev(kvx_gp *P, const double *Fx_dev, const double *g_dev, const double *x_dev, const double *z_dev, double *f_dev,
                    double *Dfx_dev, double *Hx_dev)
{
    return guarded([&] { return gp_eval_impl(P, Fx_dev, g_dev, x_dev, z_dev, f_dev, Dfx_dev, Hx_dev); });
}

void kvx_gp_free(kvx_gp *P)
{
    if (!P) return;
    for (void *p : P->owned) (void)pool_free(p);
    delete P;
}

}  // extern "C"
