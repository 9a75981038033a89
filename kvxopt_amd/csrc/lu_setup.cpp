// Set-up of a sparse LU numeric object: the knob table, streams, the plan and its device blocks, the buffers of the solves.
#include "lu_internal.hpp"

#include <cstdlib>
#include <new>
#include <stdexcept>

LuKnobs read_lu_knobs()
{
    LuKnobs K;
    auto off = [](const char *name) { const char *e = std::getenv(name); return e && e[0] == '0'; };
    K.graph = !off("KVX_LU_GRAPH");
    K.unblocked = std::getenv("KVX_LU_UNBLOCKED") != nullptr;
    K.lds_legacy = std::getenv("KVX_LU_LDS_LEGACY") != nullptr;
    K.wp = !off("KVX_LU_WP");
    if (const char *e = std::getenv("KVX_LU_WP_MAXCNT")) K.wp_maxcnt = atoi(e);
    K.timing = std::getenv("KVX_LU_TIMING") != nullptr;
    K.dump_plan = std::getenv("KVX_LU_DUMP_PLAN") != nullptr;
    return K;
}

void free_structure(kvx_lu_num *N)
{
    lu_free_block(N->S);
    for (double *p : {N->R.W, N->R.X, N->R.B})
        if (p) (void)pool_free(p);
    N->R = {};
}

int upload_structure(kvx_lu_num *N)
{
    LuLap tl{N->K.timing};
    N->version++;                                                 // (captured launch sequences belong to the old plan)
    free_structure(N);
    tl.lap("free structure");
    try {
        lu_build_plan(N->sym->Y, N->P);
    } catch (const std::bad_alloc &) {
        return KVX_ENOMEM;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return KVX_EINVAL;
    }
    const LuPlan &P = N->P;
    if ((int64_t)P.max_k > 8000) {                              // k_lu_fwd_big_init keeps the permuted pivot part in LDS
        set_last_error("LU pivot block of " + std::to_string(P.max_k) + " columns exceeds what the solve kernels hold in LDS");
        return KVX_EINVAL;
    }
    std::vector<LuFrontD> fd((size_t)P.nfront);
    for (int64_t f = 0; f < P.nfront; f++) {
        LuFrontD &F = fd[f];
        F.k = P.fr[f].k; F.m = P.fr[f].m; F.p0 = P.fr[f].p0; F.nchild = P.fr[f].nchild;
        F.px = P.px[f]; F.rowptr = P.rowptr[f]; F.childptr = P.childptr[f]; F.aptr = P.aptr[f];
        F.upd_off = P.upd_off[f]; F.wx = P.wx[f]; F.upd_ld = P.upd_ld[f]; F.acnt = (int32_t)(P.aptr[f + 1] - P.aptr[f]);
    }
    LuStructD &S = N->S;
    Arena A;
    A.up(&S.fr, fd);
    A.up(&S.rowidx, P.rowidx);
    A.up(&S.rel, P.rel);
    A.up(&S.children, P.children);
    A.up(&S.adst, P.a_dst);
    A.up(&S.asrc, P.a_src);
    A.up(&S.prow, P.prow);
    A.up(&S.qcol, P.qcol);
    A.up(&S.lists, P.levellist);
    A.up(&S.slists, P.stagelist);
    A.up(&S.fcol, P.fcol);
    A.up(&S.frow, P.frow);
    A.up(&S.flevpos, P.flevpos);
    A.up(&S.fptr_r, P.fptr_r);
    A.up(&S.fptr_c, P.fptr_c);
    A.up(&S.fsrc_r, P.fsrc_r);
    A.up(&S.fsrc_c, P.fsrc_c);
    A.alloc(&S.fval_r, (int64_t)P.fcol.size());
    A.alloc(&S.fval_c, (int64_t)P.fcol.size());
    A.alloc(&S.ipiv, N->n);
    A.alloc(&S.lperm, N->n);
    A.alloc(&S.fail, P.nfront);
    A.alloc(&S.Lx, P.lsize);
    A.alloc(&S.Ux, P.lsize);
    A.alloc(&S.arena, P.arena);
    tl.lap("build plan");
    if (int rc = A.commit(&S.block)) return rc;
    tl.lap("upload plan");
    LuDev &d = N->D;
    d.fr = S.fr; d.rowidx = S.rowidx; d.rel = S.rel; d.children = S.children;
    d.a_src = S.asrc; d.a_dst = S.adst; d.ai32 = N->M.ai32; d.rinv = N->M.rinv;
    d.Lx = S.Lx; d.Ux = S.Ux; d.arena = S.arena; d.ipiv = S.ipiv; d.lperm = S.lperm; d.fail = S.fail;
    d.arena_size = P.arena;
    if (N->K.dump_plan) lu_dump_levels(P, stderr);
    return KVX_OK;
}

// Device-pointer entry points: the caller's producers (torch's default stream, the kvx_* kernels of the KKT layer) run on
// the legacy null stream, N->st is non-blocking: order it behind them explicitly (st2 / st3 fork from st).  Same contract
// as the Cholesky path (api.cpp wait_for_caller); documented in include/kvxhip.h.
int lu_wait_for_caller(kvx_lu_num *N)
{
    HIPCHK(hipEventRecord(N->ev0, nullptr));
    HIPCHK(hipStreamWaitEvent(N->st, N->ev0, 0));
    return KVX_OK;
}

int ensure_device(kvx_lu_num *N)
{
    if (N->dev) return KVX_OK;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) {
        set_last_error("no HIP device: the LU numeric phase has no CPU fallback");
        return KVX_EDEVICE;
    }
    LuLap tl{N->K.timing};
    HIPCHK(pool_stream_get(&N->st));
    HIPCHK(pool_stream_get(&N->st2));
    HIPCHK(pool_stream_get(&N->st3));
    HIPCHK(pool_event_get(&N->ev0, false));
    tl.lap("streams + event");
    std::vector<int32_t> ai32((size_t)N->nnz);
    for (int64_t p = 0; p < N->nnz; p++) ai32[p] = (int32_t)N->sym->Y.Ai[p];
    Arena A;
    A.up(&N->M.ai32, ai32);
    A.alloc(&N->M.rinv, N->n);
    A.alloc(&N->M.rmax, N->n);
    A.alloc(&N->M.Ax, N->nnz);
    if (int rc = A.commit(&N->M.block)) return rc;
    tl.lap("per-matrix arrays");
    N->dev = true;
    return upload_structure(N);
}

int ensure_rhs(kvx_lu_num *N, int64_t nrhs)
{
    LuRhsD &R = N->R;
    if (nrhs <= R.cap) return KVX_OK;
    for (double *p : {R.W, R.X, R.B})
        if (p) (void)pool_free(p);
    R = {};
    auto get = [](double **p, int64_t count) { return pool_malloc((void **)p, (size_t)std::max<int64_t>(count, 1) * sizeof(double)); };
    HIPCHK(get(&R.W, N->P.wsize * nrhs));
    HIPCHK(get(&R.X, N->n * nrhs));
    HIPCHK(get(&R.B, N->n * nrhs));
    R.cap = nrhs;
    N->version++;                                                 // (new work buffers)
    return KVX_OK;
}

int ensure_refine(kvx_lu_num *N, int64_t nrhs)
{
    const LuSymbolic &Y = N->sym->Y;
    if (!N->RM.block) {
        Arena A;
        A.up(&N->RM.ap, Y.Ap);
        A.up(&N->RM.csrp, Y.csr_ptr);
        A.up(&N->RM.csrc, Y.csr_col);
        A.up(&N->RM.csrs, Y.csr_src);
        if (int rc = A.commit(&N->RM.block)) return rc;
    }
    LuRefineD &F = N->RF;
    if (nrhs <= F.cap) return KVX_OK;
    lu_free_block(F);
    const int64_t n = N->n;
    Arena A;
    A.alloc(&F.rx, n * nrhs);
    A.alloc(&F.rd[0], n * nrhs);
    A.alloc(&F.rd[1], n * nrhs);
    A.alloc(&F.ratio, n * nrhs);
    A.alloc(&F.part, lu_berr_parts(n) * nrhs);
    A.alloc(&F.om[0], nrhs);
    A.alloc(&F.om[1], nrhs);
    A.alloc(&F.omc, nrhs);
    A.alloc(&F.berr, 2 * nrhs);
    A.alloc(&F.act[0], nrhs);
    A.alloc(&F.act[1], nrhs);
    if (int rc = A.commit(&F.block)) return rc;
    F.cap = nrhs;
    N->version++;                                                 // (new work buffers)
    return KVX_OK;
}
