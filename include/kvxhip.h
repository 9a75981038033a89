/*
 * kvxhip.h -- C ABI of libkvxhip.so: MI355X (gfx950) implementation of the KKT
 * factor/solve hot path of sanurielf/kvxopt.
 *
 * Every entry point is what the reference's Python/C extension layer would bind for
 * this path; the reference interface each one replaces is cited as file:line relative
 * to the reference tree.  Plain pointers and sizes only; indices are int64 (the
 * reference's int_t = Py_ssize_t, src/C/kvxopt.h:46), values are IEEE double.
 *
 * Pointer kinds: *_host = host memory, *_dev = device (HBM) memory of the current
 * HIP device.  Unless a name ends in _dev, pointers are host pointers.
 *
 * Return value: 0 = KVX_OK, otherwise one of the KVX_E* codes below.  The thin host
 * layer maps codes to the exceptions the reference raises (see each function).
 */
#ifndef KVXHIP_H
#define KVXHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KVX_OK            0
#define KVX_EINVAL        1   /* bad argument            -> ValueError / TypeError          */
#define KVX_ENOMEM        2   /* host or device OOM     -> MemoryError                      */
#define KVX_ENOTPOSDEF    3   /* factor does not exist  -> ArithmeticError(minor)           */
#define KVX_ESYMBOLIC     4   /* numeric op on a symbolic-only factor -> ValueError         */
#define KVX_ESINGULAR     5   /* solve on a failed factor -> ArithmeticError("singular")    */
#define KVX_EDEVICE       6   /* HIP runtime error / no GPU -> RuntimeError (never a CPU fallback) */
#define KVX_EPERM         7   /* p is not a valid permutation -> ValueError                 */

typedef struct kvx_chol kvx_chol;          /* opaque factor: replaces the cholmod_factor capsule (cholmod.c:287-290) */
typedef struct kvx_atda kvx_atda;          /* opaque plan for S = G' D G on a fixed pattern (misc.py:1418-1462) */

/* Options: replaces cholmod.options / set_options() (cholmod.c:87-129). */
typedef struct {
    int32_t supernodal;     /* cholmod.options['supernodal'] (spsolvers.rst:731-736).  2 (default): P A P' = L L'.  0: P A P' = L D L'.
                             * 1: LL' if flops / nnz(L) >= 40 (CHOLMOD's rule), else LDL'.  One set of kernels computes Lc with
                             * P A P' = Lc Lc'; the LDL' factor is that result seen as L = Lc diag(Lc)^-1, D = diag(Lc)^2: solve
                             * sys = 2..6, getfactor (D on the diagonal, unit diagonal of L implicit) and diag (refused) follow it */
    int32_t ordering;       /* the library's own ordering (used when p == NULL, or compared with p when reserved[4] = 1):
                             * 0 = best of nested dissection (from order reserved[6] on) and, up to order reserved[5] (default 200 000), approximate minimum degree --
                             * the one with the least fill, CHOLMOD's strategy of trying several methods (cholmod.c:65-76);
                             * 1 = natural; 2 = nested dissection only; 3 = approximate minimum degree only (the role of AMD) */
    int32_t postorder;      /* 1 (default) elimination-tree postorder on top of the ordering (cholmod.c:113-115) */
    int32_t relax_small;    /* relaxed-amalgamation: always merge if merged width <= this (default 4)    */
    double  relax_z1;       /* zero-fraction bounds for widths <=16, <=48, any (defaults .8, .1, and for any width    */
    double  relax_z2;       /* relax_z3 < 0 = by the order of the matrix: .2 up to 150 000 columns, .075 beyond;      */
    double  relax_z3;       /* 0 = no relaxation of wide supernodes)                                                   */
    double  dbound;         /* cholmod.options['dbound'] (cholmod.c:116-117); 0 = off: a pivot d <= 0 fails.  > 0: CHOLMOD's rule,
                             * L_kk < dbound is replaced by dbound; with reserved[3] = 1 by 1e64 (the row drops out of the solves) */
    int32_t reserved[8];    /* [0] nd_leaf, [1] leaf_cols, [2] leaf_rows, [3] dbound mode, [4] 1 = a given p competes with the library's own
                             * ordering(s) and the least fill wins (cholmod.options['nmethods'] = 0 or 2); 0 = p is used as given
                             * (nmethods = 1), [5] largest order for the minimum-degree candidate of ordering 0, [6] smallest order for which
                             * ordering 0 computes the dissection beside the minimum degree (default 20 000; -1 = always)                */
} kvx_chol_opts;

void kvx_chol_default_opts(kvx_chol_opts *o);

/* Library / device probes (host layer uses these to fail loudly when there is no GPU). */
const char *kvx_version(void);
int  kvx_device_count(void);            /* number of visible HIP devices (0 on a CPU-only box) */
int  kvx_current_device(void);          /* the calling thread's current HIP device, -1 without one: device objects (factors, plans,
                                         * KKT objects) live on the device that was current when they were built; the host layer's
                                         * caches key on it                                    */
int  kvx_set_device(int dev);           /* make `dev` the calling thread's current HIP device (a rank process of the sharded mode
                                         * picks its GPU with this before anything else touches HIP) */
const char *kvx_last_error(void);       /* text of the last error on this thread               */
int  kvx_graph_instantiate_failures(void); /* launch graphs whose instantiation (on a thread of the library) failed since the process
                                         * started: those handles run their launches eagerly -- correct, slower */

/* ---- sparse Cholesky: replaces kvxopt.cholmod ------------------------------------------ */

/* symbolic(A, p, uplo)  -- cholmod.c:244-291 (pack :132-181, analyze_p :274).
 * A is n x n CCS (colptr[n+1], rowind[nnz], rows sorted within a column); only the `uplo`
 * ('L' or 'U') triangle is read.  perm: NULL, or n int64 with P*A*P' = L*L',
 * (PAP')(i,j) = A(perm[i],perm[j]).  Host-only work; no GPU needed. */
int kvx_chol_analyze(int64_t n, const int64_t *colptr, const int64_t *rowind, int uplo,
                     const int64_t *perm, const kvx_chol_opts *opts, kvx_chol **out);

/* numeric(A, F) -- cholmod.c:322-398.  values[nnz] are the entries of the matrix whose
 * pattern was analysed (same order).  On KVX_ENOTPOSDEF, *minor = failing column (index in
 * the permuted matrix, as CHOLMOD's L->minor, cholmod.c:376-379). */
int kvx_chol_factorize(kvx_chol *F, const double *values, int64_t *minor);
int kvx_chol_factorize_dev(kvx_chol *F, const double *values_dev, int64_t *minor);
/* Asynchronous variant: enqueue only; status is read later by kvx_chol_status(). */
int kvx_chol_factorize_async_dev(kvx_chol *F, const double *values_dev);
int kvx_chol_status(kvx_chol *F, int64_t *minor);      /* synchronises the factor's stream */

/* solve(F, B, sys, nrhs, ldB, offsetB) -- cholmod.c:429-499; sys 0..8 = A, LDL', LD, DL', L,
 * L', D, P, P' (:437-439) with D = I for an LL' factor (spsolvers.rst:640-668).  B (n x nrhs, leading dimension ldB >= max(1,n)) is
 * overwritten.  The caller applies offsetB to the pointer.  After kvx_chol_factorize_async_dev the solve
 * is queued behind the factorisation without a host round trip; a failed factorisation is then reported by
 * the solve (KVX_ESINGULAR, B undefined), as the reference's solve does on a failed factor (cholmod.c:456).
 * With many right-hand sides (48, or 8 when nrhs * n >= 6e6; KVX_WIDE_FROM) an LL' solve works on rhs-major blocks of 64 with GEMM-shaped panel products (FP64 MFMA):
 * its columns agree with single-rhs solves to rounding, not bit for bit -- CHOLMOD's BLAS-3 solves do not either. */
int kvx_chol_solve(kvx_chol *F, int sys, double *B, int64_t nrhs, int64_t ldB);
int kvx_chol_solve_dev(kvx_chol *F, int sys, double *B_dev, int64_t nrhs, int64_t ldB);
/* Enqueue only: no host synchronisation; work the caller submits to the null stream afterwards is ordered behind the
 * solve.  Errors of a factorisation still in flight are reported by the next synchronising call (kvx_chol_status). */
int kvx_chol_solve_async_dev(kvx_chol *F, int sys, double *B_dev, int64_t nrhs, int64_t ldB);
/* numeric(A, F) followed by solve(F, B) with sys = 0 (cholmod.c:322-398 then :429-499; what linsolve does after its analysis,
 * cholmod.c:618-753) as ONE enqueue on device buffers: the forward sweep follows the factorisation level by level on streams of
 * its own, so only the backward sweep and the root's forward step are left when the last front is factored.  Same kernels, same
 * order per front: the factor and X are bitwise those of kvx_chol_factorize_dev + kvx_chol_solve_dev.  Synchronises; returns
 * KVX_ENOTPOSDEF with *minor = failing column (B_dev then holds garbage).  The factor stays usable for further solves. */
int kvx_chol_factorize_solve_dev(kvx_chol *F, const double *values_dev, double *B_dev, int64_t nrhs, int64_t ldB, int64_t *minor);
/* ... with host buffers: the numeric + solve part of linsolve(A, B) (cholmod.c:663-753) in one call. */
int kvx_chol_factorize_solve(kvx_chol *F, const double *values, double *B, int64_t nrhs, int64_t ldB, int64_t *minor);
/* ... enqueue only: the caller's later null-stream work is ordered behind it; kvx_chol_status reports the factorisation afterwards
 * (the form misc.kkt_chol2's factor + first solves take inside the interior-point loop). */
int kvx_chol_factorize_solve_async_dev(kvx_chol *F, const double *values_dev, double *B_dev, int64_t nrhs, int64_t ldB);

/* spsolve(F, B, sys) -- cholmod.c:524-587.  B is n x ncol CCS; the result is returned as a
 * newly malloc'ed CCS triple the caller frees with kvx_free() (entries that are exactly zero are dropped, as
 * cholmod_spsolve does on a supernodal factor).  The forward systems (sys 2: L D x = b, 4: L x = b) sweep only the reach
 * of each block of 64 columns in the supernodal elimination tree -- the fronts that hold a nonzero row of the block and
 * their ancestors -- and copy back only the rows of those fronts; the other codes solve dense column blocks. */
int kvx_chol_spsolve(kvx_chol *F, int sys, int64_t ncol, const int64_t *Bp, const int64_t *Bi,
                     const double *Bx, int64_t **Xp, int64_t **Xi, double **Xx);

/* diag(F) -- cholmod.c:900-945: diagonal of L in permuted order, n doubles.  An LDL' factor is refused (KVX_ESYMBOLIC,
 * "F must be a nonsingular supernodal Cholesky factor", cholmod.c:919-922): its D comes from solve(sys = 6). */
int kvx_chol_diag(kvx_chol *F, double *d);

/* getfactor(F) -- cholmod.c:948-985: L as CCS (lower, sorted). Call with Lp=Li=Lx=NULL to
 * query *lnz first. */
int kvx_chol_get_factor(kvx_chol *F, int64_t *lnz, int64_t *Lp, int64_t *Li, double *Lx);

/* Introspection used by bench/tests: the measure of SURVEY 8(d). */
typedef struct {
    int64_t n, nnz_a;        /* order, entries of the analysed triangle                      */
    int64_t lnz;             /* sum_j c_j: nnz(L) for the permutation used (simplicial count)  */
    double  flops;           /* sum_j c_j^2                                                   */
    int64_t nsuper;          /* supernodes (fronts)                                           */
    int64_t lsize;           /* doubles stored for L (dense panels, >= lnz)                   */
    int64_t nlevels;         /* elimination-tree levels = dependent launch stages             */
    int64_t max_front;       /* largest front order m                                         */
    int64_t upd_size;        /* doubles in the update-matrix workspace                        */
    int64_t is_numeric;      /* 1 after a successful factorize                                */
    int64_t minor;
    int64_t solve_rowidx;    /* sum_s m_s: index entries read per triangular sweep           */
    int64_t is_ll;           /* 1: LL' factor, 0: LDL' (options['supernodal'] = 0, or 1 on a sparse factor) */
    int64_t dev_bytes;       /* bytes of the large device buffers of this handle (panels, inverted diagonal blocks, update
                              * matrices, values); 0 before the first device use.  Sharded mode: THIS rank's share          */
    int64_t lsize_local;     /* panel doubles resident on this rank (= lsize except in sharded mode: own + shared fronts)   */
    int64_t reserved[2];     /* [0] leaf subtrees the triangular sweeps walk with one wavefront each, [1] fronts inside them: as the
                              * device set-up of this handle cut them (0 / 0 under KVX_NO_SUBTREES=1); before the first device
                              * use, as it would cut them with the environment of the first such query (KVX_SUB_MAXF,
                              * KVX_NO_SUBTREES); computed once and kept on the handle                                       */
} kvx_chol_info;
int kvx_chol_get_info(kvx_chol *F, kvx_chol_info *info);
int kvx_chol_get_perm(kvx_chol *F, int64_t *perm);     /* final permutation (ordering o postorder) */
/* Supernode layout for tests: super[nsuper+1] column starts, nrows[nsuper] front orders,
 * parent[nsuper], level[nsuper]. Any pointer may be NULL. */
int kvx_chol_get_supernodes(kvx_chol *F, int64_t *super, int64_t *nrows, int64_t *parent, int64_t *level);
/* Row structure of the fronts (CHOLMOD's L->s / L->pi of a supernodal factor, cholmod.c:927-943): rowptr (nsuper + 1) and the
 * sorted permuted row indices of every front, pivot rows first.  rowidx may be NULL (sizes only: rowptr[nsuper] entries). */
int kvx_chol_get_front_rows(kvx_chol *F, int64_t *rowptr, int64_t *rowidx);
/* Dominant-kernel timing of the last factorize/solve, measured with HIP events on the
 * factor's own stream (bench.py roofline leg). ms_factor / ms_solve may be NULL. */
int kvx_chol_last_timing(kvx_chol *F, double *ms_factor, double *ms_solve);
/* Which form the last kvx_chol_factorize_solve* call took: 1 = the one-enqueue form (forward sweep pipelined behind the
 * factorisation, one launch graph), 2 = factorisation and solve as two enqueues (sharded / LDL' factors, more than 16
 * right-hand sides, family timing, KVX_NO_GRAPH, and every process whose HIP runtime is older than 7.2 -- the runtime inside
 * the PyTorch wheel, 7.0.51831, crashes in hipGraphLaunch of the one-enqueue graph), 0 = no such call yet. */
int kvx_chol_last_fused_path(kvx_chol *F);
/* Per-kernel-family timing for the roofline leg of bench.py: HIP events are recorded around
 * every launch of ONE family on the factor's own stream while it is selected.
 * family: -1 off, 0 scatter_a, 1 front_small (LDS fronts), 2 assemble_big, 3 potrf_diag,
 * 4 trsm_panel, 5 syrk_trailing (FP64 MFMA), 6 fwd_level, 7 bwd_level.
 * prof_read returns the summed kernel time and launch count since the last select. */
int kvx_chol_prof_select(kvx_chol *F, int family);
int kvx_chol_prof_read(kvx_chol *F, double *total_ms, int64_t *launches);
/* Diagnostics of the trailing update of the big fronts' pivot chain (no device needed).
 * kvx_dbg_tile_cover: the workgroup numbering of ONE launch over the fronts (orders hm, pivot counts hk, in list order) with the
 * panel columns [kb, kb + klen) and col_lim (uonly = 1: a deferred "far" update from column col_lim on), walked on the host
 * through the decode and the tile guard the kernels run.  counts[(f * tmax + ti) * tmax + tj] (count * tmax * tmax entries) =
 * workgroups that take tile (ti, tj) of front f; info (70 entries): ncls, workgroups, tiles accepted by the guard, strays
 * (accepted outside the counts array), first[17] (info + 4), T[16] (+ 21), TC[16] (+ 37), wg[17] (+ 53).  0 = done, 1 = bad args.
 * kvx_dbg_syrk_counts: trailing-update launches enqueued by this process, per kernel / schedule (out may be NULL; reset = 1
 * zeroes them); returns the number of counters.  Order: k_syrk_trailing<64> by classes, <64> grid, <128> by classes, <128> grid,
 * k_syrk_lds (chain), k_syrk_lds far, far launches walking their tiles (KVX_FAR_WGS), k_syrk_trailing128 one panel, two-level
 * outer update, far updates on a stream of their own.  A graph replay enqueues nothing and is not counted. */
int kvx_dbg_tile_cover(int uonly, const int32_t *hm, const int32_t *hk, int count, int kb, int klen, int col_lim, int tmax,
                       int32_t *counts, int64_t *info);
int kvx_dbg_syrk_counts(int64_t *out, int reset);
/* The chain step whose trailing update solves its own panel rows (k_syrk_solve, KVX_SOLVE_IN_UPDATE_TILES).
 * kvx_dbg_syrk_solve_count: such launches enqueued by this process (reset = 1 zeroes the counter after reading it).
 * kvx_dbg_solve_in_update: the host's decision for one trailing update -- knob = KVX_SOLVE_IN_UPDATE_TILES, cls = numbered over
 * size classes, pair = a step of the pair schedule, the panel columns [jb, jb + klen), col_lim, tiles = the launch's tile count
 * (upper estimate); 1 = the fused step, 0 = panel solve and update as two launches. */
int64_t kvx_dbg_syrk_solve_count(int reset);
int kvx_dbg_solve_in_update(int64_t knob, int cls, int pair, int klen, int col_lim, int64_t tiles);
/* kvx_dbg_lu_counts: launches enqueued by the sparse LU path of this process, one counter per routing outcome (out may be NULL;
 * reset = 1 zeroes them); returns the number of counters, 30.  Order: k_lu_front_wp<T> at index T (T = 1, 2, 3, 4, 6, 7; 0 and 5
 * unused), k_lu_front_tiled<T> at 8 + T, then from 16: LDS-resident legacy kernel, unblocked big fronts, k_lub_panel_reg<32,1>,
 * <16,2>, <8,4>, k_lub_panel, k_lub_panel launches in which some front has more than 4096 rows left, k_lub_trsm, k_lub_trsm left
 * out (refactorisation, block without interchanges), k_lub_gemm, forward sweep small / big, backward sweep small / big (per
 * launcher call with fronts).  A graph replay enqueues nothing and is not counted. */
int kvx_dbg_lu_counts(int64_t *out, int reset);
/* kvx_dbg_chol_small_counts: launches of the small-front kernels of the Cholesky path (m <= 128, k <= 64) enqueued by this process,
 * one counter per routing outcome of their launchers (out may be NULL; reset = 1 zeroes them); returns the number of counters, 32.
 * Order: k_front_wave at 2 * i + j (i: LDS image 32 / 48 / 64, j: <16> / <32>), from 6 k_front_lds image 96 <32>, 96 <64>, 128 <32>,
 * 128 <64>, from 10 k_factor_subtree by LDS image 32 / 48 / 64, 13 k_fwd_wave<16>, <32>, 15 k_bwd_wave<32, 32>, <32, 48>, <32, 64>,
 * 18 k_fwd_lds<32>, <64>, 20 k_bwd_lds, 21 k_fwd_subtree, 22 k_bwd_subtree<32>, <48>, <64>, 25 k_fwd_subtree_mr, 26 k_bwd_subtree_mr<32>,
 * <64>, 28 k_wide_fwd_small<32>, <64>, 30 k_wide_bwd_small<32>, <64>.  A graph replay enqueues nothing and is not counted. */
int kvx_dbg_chol_small_counts(int64_t *out, int reset);
/* kvx_dbg_chol_big_solve_counts: launches of the triangular sweeps over the big fronts of the Cholesky path (m > 128 or k > 64)
 * enqueued by this process, one counter per launch site of launch_fwd_big, launch_bwd_big, launch_wide_fwd_big and
 * launch_wide_bwd_big (out may be NULL; reset = 1 zeroes them); returns the number of counters, 17.  Order: k_fwd_big_step<true, 64>,
 * <false, 64>, <true, 256>, <false, 256>, from 4 k_fwd_big_step_mr<true, 8, 1>, <true, 8, 2>, <false, 8, 1>, <false, 8, 2>,
 * 8 k_bwd_big_init, 9 k_bwd_big_step, 10 k_bwd_big_init_mr, 11 k_bwd_big_step_mr<8, 1>, <8, 2>, 13 k_wide_fwd_big_asm,
 * 14 k_wide_fwd_big_step, 15 k_wide_bwd_big_head, 16 k_wide_bwd_big_step.  A graph replay enqueues nothing and is not counted. */
int kvx_dbg_chol_big_solve_counts(int64_t *out, int reset);
/* kvx_dbg_lu_schedule: the factor-side launch schedule of a numeric pass over the plan that the analysis S gives in its current
 * merge state (no device needed).  Returns the number of entries of the record, -1 for bad arguments or a plan that cannot be
 * built; the record is written only if cap entries hold it (call with cap = 0 for the length).  Record: nlevels, then per level
 * (0 = roots)
 *   nfront, nfront pairs (m, k): the fronts in list order;
 *   nlaunch, nlaunch quadruples (first, count, class, side): the launches of LDS fronts in launch order -- list entries
 *     [first, first + count) of the level, LDS class 16 / 32 / 48 / 64 / 88 / 112, side 0 = the main stream, 1 = the second one;
 *   first, count, bm, bk: the blocked part (fronts of order > 112) and the largest order / pivot count in it;
 *   nstep, nstep triples (jb, width, lds_work): its pivot blocks [jb, jb + width) and whether some front has pivots from jb on
 *     and more than 4096 rows left there. */
struct kvx_lu_sym;
int64_t kvx_dbg_lu_schedule(struct kvx_lu_sym *S, int64_t *out, int64_t cap);
/* ---- sharded mode: ONE system factored and solved by nranks processes, one GPU each ----------------------------
 * (the reference is single-process: the calls this stands in for are cholmod_l_factorize / cholmod_l_solve,
 * src/C/cholmod.c:362-364, 483.)  Every rank analyses the same matrix (the analysis is deterministic) and computes the
 * same map (kvx_chol_dist_map): proportional mapping of the elimination tree gives every front a contiguous range of ranks;
 *   - a range of one rank owns the front and its whole subtree: factored and solved by that rank alone;
 *   - small fronts shared by several ranks are replicated on them (identical arithmetic, nothing exchanged inside the front);
 *   - shared fronts of order >= min_m are block-cyclic: columns dealt out in blocks of `ob` columns round-robin over the
 *     range; right-looking, the owner of a pivot block factors the panel and broadcasts it (the panel ends up on every rank
 *     of the range), every rank applies the rank-ob update to the blocks it owns -- pivot columns and update matrix alike.
 * Exchange steps, all broadcasts inside the range of the receiving front: a child's update matrix (its column blocks, from
 * their owners) before the parent assembles; each factored panel; a child's update vector per solve.  One all-reduce over
 * all ranks ends a solve (every rank contributes the entries of x it reports) and one MIN ends a factorisation (failing
 * column).  No zero padding: only lower trapezoids of the blocks travel.
 * The library is collective-agnostic: it packs a message into the caller's device buffer (kvx_chol_dist_set_xchg) and calls
 * `comm` for every collective; kvxopt_amd/dist.py runs them with torch.distributed (backend "nccl" = RCCL over xGMI on a
 * node, "gloo" in the tests), a C caller would call ncclBroadcast / ncclAllReduce on its stream.  Stream contract of the
 * callback: the message is complete in null-stream order when `comm` is entered, and the collective's result must be
 * visible in null-stream order when it returns (no host synchronisation needed).  Return nonzero to abort (KVX_ECOMM). */
#define KVX_ECOMM         8   /* a collective callback failed -> RuntimeError */
#define KVX_DIST_BCAST        1   /* buf[0..count) from global rank `root` to the ranks [lo, hi)            */
#define KVX_DIST_ALLREDUCE    2   /* element-wise SUM over the ranks [lo, hi), result on every one of them   */
#define KVX_DIST_ALLREDUCE_MIN 3  /* element-wise MIN                                                        */
typedef struct { int32_t kind, root, lo, hi; int64_t count; double *buf_dev; } kvx_dist_op;
typedef int (*kvx_dist_comm_fn)(void *ctx, const kvx_dist_op *op);
/* host-only: the map for nranks ranks.  glo/ghi/mode: nsuper entries each (mode 0 = owned or replicated, 1 = block-cyclic);
 * rank_flops / panel_flops: nranks doubles -- factorisation flops each rank executes, and the part of them that is panel
 * factorisation of block-cyclic fronts; totals[0] = flops of all fronts (sum over fronts of sum_{j<k} (m-j)^2: the work executed, amalgamation zeros
 * included), totals[1] = flops of the replicated shared fronts.
 * Any output may be NULL.  ob <= 0 / min_m <= 0: defaults (512, 6144). */
int kvx_chol_dist_map(kvx_chol *F, int nranks, int ob, int min_m, int32_t *glo, int32_t *ghi, uint8_t *mode,
                      double *rank_flops, double *panel_flops, double totals[2]);
/* info[0] = n, [1] = smallest exchange buffer (doubles), [2] = recommended, [3] = shared fronts this rank takes part in,
 * [4] = of which block-cyclic, [5] = number of distinct rank ranges (kvx_chol_dist_groups), [6] = ob, [7] = min_m */
int kvx_chol_dist_setup(kvx_chol *F, int rank, int nranks, int ob, int min_m, int64_t info[8]);
int kvx_chol_dist_groups(kvx_chol *F, int32_t *lohi /* 2 * info[5] entries: lo, hi pairs; ranges of >= 2 ranks */);
int kvx_chol_dist_set_xchg(kvx_chol *F, double *xchg_dev, int64_t count);
/* numeric factorisation of the sharded factor; values_dev identical on all ranks.  *minor as kvx_chol_factorize_dev,
 * already the minimum over the ranks (every rank returns the same status). */
int kvx_chol_dist_factorize(kvx_chol *F, const double *values_dev, kvx_dist_comm_fn comm, void *ctx, int64_t *minor);
/* A X = B in place: B_dev (n x nrhs, ld = ldB) identical on all ranks on entry, the full solution on every rank on return. */
int kvx_chol_dist_solve(kvx_chol *F, double *B_dev, int64_t nrhs, int64_t ldB, kvx_dist_comm_fn comm, void *ctx);

/* ---- RCCL bound directly: the collectives of the sharded mode without torch.distributed -------------------------------
 * One process per GPU.  librccl.so is opened with dlopen at the first of these calls (KVX_RCCL_LIB overrides the path).
 * Rank 0 makes the id (kvx_rccl_unique_id) and hands its 128 bytes to the other ranks by any channel (kvxopt_amd/rccl.py: a
 * TCP socket on MASTER_ADDR:MASTER_PORT); every rank then calls kvx_rccl_init on the device it has made current (one rank per
 * device: RCCL refuses two).  kvx_rccl_split is collective over ALL ranks and creates the communicator of one rank range of
 * the factor's map (the ranges of kvx_chol_dist_groups, same order on every rank).  kvx_rccl_comm is a kvx_dist_comm_fn whose
 * ctx is the kvx_rccl*: pass both to kvx_chol_dist_factorize / kvx_chol_dist_solve.  The *_host calls move a few doubles
 * (at most 1024) through a device scratch buffer: timing rules and barriers of a benchmark.  Nothing here has a counterpart in
 * the reference (single process, src/C/cholmod.c:85). */
typedef struct kvx_rccl kvx_rccl;
int kvx_rccl_version(int *version);                       /* ncclGetVersion of the library that was opened */
int kvx_rccl_unique_id(char id[128]);
int kvx_rccl_init(int rank, int nranks, const char id[128], kvx_rccl **out);
int kvx_rccl_split(kvx_rccl *W, int lo, int hi);
int kvx_rccl_comm(void *ctx, const kvx_dist_op *op);
int kvx_rccl_allreduce_host(kvx_rccl *W, double *vals, int n, int op /* 0 SUM, 1 MAX, 2 MIN */);
int kvx_rccl_allgather_host(kvx_rccl *W, const double *mine, int n, double *all /* n * nranks */);
int kvx_rccl_barrier(kvx_rccl *W);                        /* every rank is here and its earlier device work is complete */
int kvx_rccl_stats(kvx_rccl *W, int64_t out[2]);          /* collectives through kvx_rccl_comm, bytes they moved */
void kvx_rccl_free(kvx_rccl *W);

void kvx_chol_free(kvx_chol *F);
void kvx_free(void *p);

/* ---- normal-equations assembly: replaces base.gemm(partial)+base.syrk(partial) ---------- */

/* Plan S = G' diag(w) G (+ P) on a fixed lower-triangular CCS pattern (misc.py:1418-1426,
 * 1451-1455 -> sparse.c:1260-1283, 2176-2256).  G is ml x n CCS.  The plan computes the
 * pattern of tril(G'G) (union with the lower pattern of P when Pp != NULL) and returns it
 * through kvx_atda_pattern().  The lower triangle of P is read: an entry above the diagonal is in
 * neither the pattern nor the sum, so a full symmetric P gives what its lower triangle gives;
 * entries stored at one position are added in the order they are stored.  Every entry of S is
 * written by one lane (no floating-point atomics), and an entry of a lower triangle without
 * repeats is S_ij + P_ij in one addition. */
int kvx_atda_plan(int64_t ml, int64_t n, const int64_t *Gp, const int64_t *Gi,
                  const int64_t *Pp, const int64_t *Pi, kvx_atda **out);
int kvx_atda_pattern(kvx_atda *T, int64_t *snz, int64_t *Sp, int64_t *Si);
/* Sx[snz] = sum_k w[k] G[k,i] G[k,j] (+ P[i,j]); w = di.^2. Host and device variants. */
int kvx_atda_assemble(kvx_atda *T, const double *Gx, const double *w, const double *Px, double *Sx);
int kvx_atda_assemble_dev(kvx_atda *T, const double *Gx_dev, const double *w_dev,
                          const double *Px_dev, double *Sx_dev);
/* the same with the square roots of the weights: S = G' diag(di)^2 G (+ P), what misc.kkt_chol2 forms (misc.py:1418-1426: W^-1
 * applied to G, then syrk) -- the square is taken while G is scaled, same roundings as ssqr followed by assemble */
int kvx_atda_assemble_sq_dev(kvx_atda *T, const double *Gx_dev, const double *di_dev, const double *Px_dev, double *Sx_dev);
void kvx_atda_free(kvx_atda *T);

/* ---- Nesterov-Todd scaling, orthant ('l') cone: replaces kvxopt.misc / misc_solvers ------ */
/* All vectors are device pointers of length ml (x: ml x ncols with leading dimension ldx). */

/* compute_scaling 'l' block (misc.py:284-287): d = sqrt(s./z), di = 1./d, lmbda = sqrt(s.*z) */
int kvx_nt_compute_scaling_dev(int64_t ml, const double *s, const double *z,
                               double *d, double *di, double *lmbda);
/* update_scaling 'l' block (misc.py:444-464), in place: s:=sqrt(s), z:=sqrt(z),
 * d:=d.*s./z, di:=1./d, lmbda:=s.*z */
int kvx_nt_update_scaling_dev(int64_t ml, double *s, double *z, double *d, double *di, double *lmbda);
/* scale 'l' block (misc_solvers.c:132-141): x := w .* x for each of ncols columns */
int kvx_nt_scale_dev(int64_t ml, int64_t ncols, int64_t ldx, double *x, const double *w);
/* scale2 (misc_solvers.c:287-298): inverse=0: x := x./lmbda ; inverse=1: x := x.*lmbda */
int kvx_nt_scale2_dev(int64_t ml, const double *lmbda, double *x, int inverse);
/* sprod (misc_solvers.c:662-669) x := x.*y ; sinv (:793-800) x := x./y ; ssqr (misc.py:951-952) x := y.*y */
int kvx_nt_sprod_dev(int64_t ml, double *x, const double *y);
int kvx_nt_sinv_dev(int64_t ml, double *x, const double *y);
int kvx_nt_ssqr_dev(int64_t ml, double *x, const double *y);
/* sdot (misc_solvers.c:1018) and max_step (misc_solvers.c:1065-1071: max_i -x_i) */
int kvx_nt_sdot_dev(int64_t ml, const double *x, const double *y, double *result_host);
int kvx_nt_max_step_dev(int64_t ml, const double *x, double *result_host);
/* Fused 'l'-cone steps of one interior-point iteration (each replaces a fixed run of the reference's BLAS-1 /
 * misc calls, same operations per element; the loop is bound by launches, not by bytes):
 *   newton_rhs: ds := -(lmbdasq (+ ws3 - shift)) ./ lmbda,  dz := -(scale*rz + d.*ds)      coneprog.py:1250-1298, 1146-1157
 *               (ws3 may be NULL: predictor);
 *   step_post : dz += dtau*z1, ds -= dz, [ws3 := ds.*dz], ds ./= lmbda, dz ./= lmbda        coneprog.py:1186-1191, 1303-1316
 *   update    : ds := (step*ds + 1).*lmbda (same for dz), misc.update_scaling (misc.py:444-464), s := W'lmbda,
 *               z := W^-1 lmbda                                                             coneprog.py:1343-1432  */
int kvx_lp_newton_rhs_dev(int64_t ml, const double *lmbdasq, const double *ws3, double shift, double scale, const double *rz,
                          const double *lmbda, const double *d, double *ds, double *dz);
int kvx_lp_step_post_dev(int64_t ml, double dtau, const double *z1, const double *lmbda, double *ds, double *dz, double *ws3);
int kvx_lp_update_dev(int64_t ml, double step, double *ds, double *dz, double *d, double *di, double *lmbda, double *s, double *z);
/* (newton_rhs: lmbdasq may be NULL -- lmbda o lmbda is then formed in the kernel, rounded as misc.ssqr rounds it.)
 * The remaining short launches of an iteration, fused (round 3; a launch of a few microseconds costs 4-5 us on its stream, ~85 of them
 * were a fifth of an iteration).  Same arithmetic per element, same roundings: an interior-point run is bit for bit the unfused one.
 *   update_x  : kvx_lp_update_dev and x += step*dx (coneprog.py:1339) in one launch;
 *   residuals : hrx := -G'z, rx := hrx - tau*c, hrz := G*x + s, rz := hrz - tau*h (coneprog.py:861-896, p = 0) in one launch; G by its
 *               CCS arrays and by those of its transpose (device pointers, int64 indices, as for kvx_spmv_dev);
 *   kkt_solve_pre / _post: misc.kkt_chol2's solve (misc.py:1489-1563, p = 0) around the triangular solves, for one or two right-hand
 *               sides:  x2(:,k) := xscale*xin + G'(di.*(zin.*di))   [z := W^-1 z, x += Gs'z]   and, after S^-1 on x2,
 *               xout := xoscale*x2(:,k),  zout := zoscale*(di.*(G*x2(:,k)) - zin.*di)           [z := Gs*x - z].
 *   max_col_nnz / max_row_nnz: the largest number of entries in a column / row of G (0 = not known): with at most four (eight), a
 *               column or row is summed by 4 (8) lanes instead of 16 -- the same association, the same bits. */
typedef struct kvx_kkt_side {
    const double *xin;  double xscale;  const double *zin;     /* pre */
    double *xout;       double xoscale; double *zout; double zoscale;   /* post (zin is read again) */
} kvx_kkt_side;
int kvx_lp_update_x_dev(int64_t ml, int64_t n, double step, double *ds, double *dz, double *d, double *di, double *lmbda, double *s,
                        double *z, const double *dx, double *x);
int kvx_lp_residuals_dev(int64_t ml, int64_t n, const int64_t *Gp, const int64_t *Gi, const double *Gx, int64_t max_col_nnz,
                         const int64_t *GTp, const int64_t *GTi, const double *GTx, int64_t max_row_nnz, const double *x, const double *z, const double *s,
                         const double *c, const double *h, double tau, double *hrx, double *rx, double *hrz, double *rz);
int kvx_kkt_solve_pre_dev(int64_t ml, int64_t n, const int64_t *Gp, const int64_t *Gi, const double *Gx, int64_t max_col_nnz,
                          const double *di, int nrhs, const kvx_kkt_side *sides, double *x2, int64_t ldx2);
int kvx_kkt_solve_post_dev(int64_t ml, int64_t n, const int64_t *GTp, const int64_t *GTi, const double *GTx, int64_t max_row_nnz,
                           const double *di, int nrhs, const kvx_kkt_side *sides, const double *x2, int64_t ldx2);
/* count <= 32 reductions with one host synchronisation: kind[i] = 0 sdot(x_i, y_i), 1 max_step(x_i) -- bitwise the
 * values of the single calls (the per-iteration residual norms / objectives of coneprog.py:861-896 in one go). */
/* second half of f6_no_ir + step bounds (coneprog.py:1162-1195, 1303-1321) in one host round trip: dtau is formed on the
 * device from c'dx + b'dy + th'dz (and z1'z1 when z1z1 < 0) and consumed there by dx += dtau x1, dy += dtau y1,
 * dz += dtau z1, ds -= dz, [ws3 = ds.*dz], ds ./= lmbda, dz ./= lmbda.  out_host = {dtau, z1'z1, max(-ds), max(-dz)}. */
int kvx_lp_second_half_dev(int64_t ml, int64_t n, int64_t p, const double *c, const double *b, const double *th, const double *x1,
                           const double *y1, const double *z1, const double *lmbda, double *dx, double *dy, double *dz, double *ds,
                           double *ws3, double dgi, double dtau0, double z1z1, double out_host[4]);
int kvx_nt_reduce_multi_dev(int count, const int32_t *kind, const int64_t *n, const double *const *x,
                            const double *const *y, double *out_host);
/* One interior-point iteration of conelp on the orthant without equality constraints (coneprog.py:859-1436, p = 0) in FOUR calls
 * instead of fifteen (round 4): the same kernels in the same order as the calls above -- bit for bit the same iterates -- but
 * the launches between two host synchronisations are issued from C back to back (a Python -> ctypes hop costs 10-15 us, and
 * the GPU waited for them after every synchronisation: ~250 us of a 1.9 ms iteration, rocprofv3 timeline).  All pointers are
 * device pointers; plan / F / Sx / x2 are the KKT object's (S = G' W^-2 G on its fixed pattern, its factor, two columns of work).
 *   residuals : kvx_lp_residuals_dev + the reductions of coneprog.py:861-896 -> out[10] = hrx'hrx, rx'rx, 0, 0, hrz'hrz, rz'rz,
 *               c'x, 0, h'z, lmbda'lmbda (the order lp.py reads them in);
 *   predictor : kvx_lp_newton_rhs_dev (predictor), assembly of S, kvx_kkt_solve_pre_dev, factorisation + two-column solve as one
 *               enqueue, kvx_kkt_solve_post_dev [x1 := dgi S^-1(-c ..), z1; dx, dz], th := h .* di, kvx_lp_second_half_dev
 *               -> out[4] = dtau, z1'z1, max(-ds), max(-dz); the factorisation's status stays deferred (kvx_chol_status);
 *   corrector : kvx_lp_newton_rhs_dev (shift = sigma mu, scale = 1 - sigma, ws3), KKT solve with the factor, second half;
 *   update    : kvx_lp_update_x_dev(step), then `residuals` of the next iteration with tau_next. */
typedef struct kvx_lp_ctx {
    int64_t ml, n;
    const int64_t *Gp, *Gi; const double *Gx; int64_t max_col;
    const int64_t *GTp, *GTi; const double *GTx; int64_t max_row;
    kvx_atda *plan; kvx_chol *F; double *Sx, *x2;
    double *x, *s, *z, *c, *h, *hrx, *rx, *hrz, *rz, *lmbda, *d, *di, *ds, *dz, *dx, *x1, *z1, *th, *ws3;
} kvx_lp_ctx;
int kvx_lp_iter_residuals(const kvx_lp_ctx *L, double tau, double out[10]);
int kvx_lp_iter_predictor(const kvx_lp_ctx *L, double dgi, double dtau0, double out[4]);
int kvx_lp_iter_corrector(const kvx_lp_ctx *L, double shift, double scale, double dgi, double dtau0, double z1z1, double out[4]);
int kvx_lp_iter_update(const kvx_lp_ctx *L, double step, double tau_next, double out[10]);

/* ---- BLAS-1 glue on device vectors: replaces the blas.axpy / scal / copy calls and elementwise
 * products the interior-point loop makes between KKT solves (coneprog.py:1126-1433). ------------- */
int kvx_vec_axpy_dev(int64_t n, double alpha, const double *x, double *y);
/* z := a x + b y in one pass (blas.copy + blas.axpy / blas.scal pairs of coneprog.py:861-896, 1295-1298); b == 0: z := a x */
int kvx_vec_lincomb_dev(int64_t n, double a, const double *x_dev, double b, const double *y_dev, double *z_dev);     /* y += alpha x        */
int kvx_vec_scal_dev(int64_t n, double alpha, double *x);                       /* x *= alpha          */
int kvx_vec_addc_dev(int64_t n, double c, double *x);                           /* x += c              */
int kvx_vec_fill_dev(int64_t n, double c, double *x);                           /* x := c              */
int kvx_vec_copy_dev(int64_t n, const double *x, double *y);                    /* y := x              */
int kvx_vec_copy_strided_dev(int64_t n, const double *x, int64_t incx, double *y);   /* y[i] := x[i * incx] (e.g. a dense diagonal) */
int kvx_vec_xmy_dev(int64_t n, double a, const double *x, const double *y, double b, double *z); /* z := a x.*y + b z */

/* ---- sparse mat-vec: replaces base.gemv on spmatrix (sparse.c:1073-1104) ----------------- */
/* y := alpha*op(A)*x + beta*y, A m x n CCS with int64 indices on the device. trans 'N'/'T'. */
int kvx_spmv_dev(int trans, int64_t m, int64_t n, const int64_t *Ap_dev, const int64_t *Ai_dev,
                 const double *Ax_dev, double alpha, const double *x_dev, double beta, double *y_dev);

/* ---- second-order-cone ('q') blocks of the Nesterov-Todd scaling: the 'q' parts of
 * misc.compute_scaling / update_scaling (misc.py:290-352, 467-580), misc_solvers.scale / scale2 / sprod / sinv
 * (misc_solvers.c:144-186, 301-341, 671-700, 803-835), misc.ssqr (misc.py:951-959), max_step (misc_solvers.c:1073-1085).
 * off_dev: nq + 1 cone boundaries [0, q0, q0 + q1, ...]; every vector pointer addresses the START of the 'q' section of its
 * vector (i.e. the caller adds mnl + dims['l']); one workgroup per cone, all cones of a call in one launch (null stream). */
int kvx_ntq_compute_scaling_dev(int64_t nq, const int64_t *off_dev, const double *s_dev, const double *z_dev, double *v_dev,
                                double *beta_dev /* nq */, double *lmbda_dev);
/* in place: s, z leave as st / a, zt / b (misc.py:517-523); v, beta, lmbda are updated */
int kvx_ntq_update_scaling_dev(int64_t nq, const int64_t *off_dev, double *s_dev, double *z_dev, double *v_dev, double *beta_dev,
                               double *lmbda_dev);
/* x_k := beta_k (2 v_k v_k' - J) x_k for every column of x (leading dimension ldx), or the inverse scaling */
int kvx_ntq_scale_dev(int64_t nq, const int64_t *off_dev, const double *v_dev, const double *beta_dev, double *x_dev, int64_t ldx,
                      int64_t ncols, int inverse);
int kvx_ntq_scale2_dev(int64_t nq, const int64_t *off_dev, const double *lmbda_dev, double *x_dev, int inverse);
/* op 0: x := y o x (sprod);  1: x := y o\ x (sinv);  2: x := y o y (ssqr) */
int kvx_ntq_prod_dev(int64_t nq, const int64_t *off_dev, double *x_dev, const double *y_dev, int op);
/* out_dev[k] = |x_k1| - x_k0 (the caller takes the maximum) */
int kvx_ntq_max_step_dev(int64_t nq, const int64_t *off_dev, const double *x_dev, double *out_dev);

/* ---- semidefinite ('s') blocks of the Nesterov-Todd scaling: the 's' parts of misc.compute_scaling /
 * update_scaling (misc.py:354-419, 582-634), misc_solvers.scale / scale2 / sprod / sinv / sdot / max_step
 * (misc_solvers.c:188-240, 343-397, 700-770, 845-882, 1029-1046, 1086-1160) and pack / unpack / symm / trisc / triusc
 * (misc_solvers.c:412-632, 887-988).  Block k has order m_k; off2_dev: ns + 1 offsets of the blocks in the 's' section of a
 * vector [0, m0^2, m0^2 + m1^2, ...]; off1_dev: ns + 1 offsets of their diagonals / eigenvalues [0, m0, m0 + m1, ...].  Vector
 * pointers address the START of the 's' section (r, rti: the blocks W['r'][k], W['rti'][k] back to back; lmbda: its 's' part).
 * One workgroup per block, all blocks of a call in one launch (null stream).  work_dev: scratch, sizes given per entry. */
/* r_k' z_k r_k = r_k^-1 s_k r_k^-T = diag(lmbda_k), rti_k = r_k^-T; lmbda_k descending as lapack.gesvd returns it.
 * work: 4 sum m_k^2 doubles.  status_dev: int, preset to INT_MAX; a block that is not positive definite stores its failing
 * column with atomicMin (the reference's lapack.potrf raises ArithmeticError). */
int kvx_nts_compute_scaling_dev(int64_t ns, const int64_t *off2_dev, const int64_t *off1_dev, const double *s_dev,
                                const double *z_dev, double *r_dev, double *rti_dev, double *lmbda_dev, double *work_dev,
                                int *status_dev);
/* in place (misc.py:582-634): on entry s_k, z_k hold the factors Ls, Lz of the new iterates in the current scaling, on return
 * the singular vectors U and V' of Lz' Ls; r, rti, lmbda are updated.  work: 4 sum m_k^2 doubles */
int kvx_nts_update_scaling_dev(int64_t ns, const int64_t *off2_dev, const int64_t *off1_dev, double *s_dev, double *z_dev,
                               double *r_dev, double *rti_dev, double *lmbda_dev, double *work_dev);
/* x_k := R_k' X_k R_k (form 0) or R_k X_k R_k' (form 1) for every column of x (leading dimension ldx); X_k is the symmetric
 * matrix stored in the lower triangle of x_k and only that triangle is written.  R = r or rti as the reference chooses by
 * (trans, inverse).  work: ncols * wstride doubles, wstride >= sum m_k^2 */
int kvx_nts_scale_dev(int64_t ns, const int64_t *off2_dev, const int64_t *off1_dev, const double *R_dev, double *x_dev,
                      int64_t ldx, int64_t ncols, int form, double *work_dev, int64_t wstride);
/* x_k(i, j) := x_k(i, j) / (sqrt(l_i) sqrt(l_j)) (inverse 0) or times it (inverse 1), all entries of the block */
int kvx_nts_scale2_dev(int64_t ns, const int64_t *off2_dev, const int64_t *off1_dev, const double *lmbda_dev, double *x_dev,
                       int inverse);
/* op 0: x := y o x with full 's' blocks in y (the upper triangles of y are filled by mirroring, as the reference does;
 * work: sum m_k^2);  op 1 / 2: sprod / sinv with DIAGONAL 's' blocks -- y_dev then addresses the diagonals (off1 layout) */
int kvx_nts_prod_dev(int64_t ns, const int64_t *off2_dev, const int64_t *off1_dev, double *x_dev, double *y_dev, int op,
                     double *work_dev);
/* out_dev[k] = trace inner product of the symmetric matrices stored in the lower triangles of x_k, y_k (the caller adds) */
int kvx_nts_dot_dev(int64_t ns, const int64_t *off2_dev, const int64_t *off1_dev, const double *x_dev, const double *y_dev,
                    double *out_dev);
/* out_dev[k] = -(smallest eigenvalue of x_k); with sigma_dev != NULL the eigenvalues (ascending) are stored there and the
 * eigenvectors replace x_k (misc_solvers.c:1128-1133), otherwise x is not modified.  work: 3 sum m_k^2 + 2 sum m_k */
int kvx_nts_max_step_dev(int64_t ns, const int64_t *off2_dev, const int64_t *off1_dev, double *x_dev, double *sigma_dev,
                         double *out_dev, double *work_dev);
/* mode 0 symm (upper := mirror of lower), 1 trisc (upper := 0, strict lower *= 2), 2 triusc (strict lower *= 0.5) */
int kvx_nts_tri_dev(int64_t ns, const int64_t *off2_dev, const int64_t *off1_dev, double *x_dev, int mode);
/* dir 0 pack: packed (offp_dev: ns offsets [0, m0 (m0 + 1) / 2, ...]) := lower triangles of the blocks by columns, off-diagonal
 * entries times sqrt(2) (dir 2: pack2's form, which copies the diagonal instead of dividing and multiplying it by sqrt(2));
 * dir 1 unpack: the reverse into the lower triangles (the strict upper triangles are not touched) */
int kvx_nts_pack_dev(int64_t ns, const int64_t *off2_dev, const int64_t *off1_dev, const int64_t *offp_dev, double *full_dev,
                     double *packed_dev, int dir);

/* ---- general cones: the KKT system of misc.kkt_chol (misc.py:1213-1349) for 'l' rows, 'q' cones and 's' blocks ----------
 * S = Gs' Gs with Gs = pack2(W^-T G) (misc.py:1267-1277: scale(Gs, W, 'T', 'I'), pack2, syrk), n x n, on a fixed pattern: the
 * union of the cliques of columns that touch each 'l' row, 'q' cone and 's' block (lower triangles of the 's' block rows of G
 * only: the strict upper triangle is ignored as scale and sgemv ignore it, misc.py:801-833).  G: N x n CCS, N = ml + sum q_k +
 * sum m_k^2, rows in the reference's order ('l', then the 'q' cones, then the 's' blocks stored by columns).  Host only. */
typedef struct kvx_cone kvx_cone;
int kvx_cone_plan(int64_t ml, int64_t nq, const int64_t *q, int64_t ns, const int64_t *s, int64_t n, const int64_t *Gp,
                  const int64_t *Gi, kvx_cone **out);
/* lower CCS pattern of S (Sp: n + 1, Si: snz; either may be NULL to query snz) */
int kvx_cone_pattern(kvx_cone *C, int64_t *snz, int64_t *Sp, int64_t *Si);
/* Sx_dev[snz] := S for the scaling W: di (ml, the 'l' block of W['di']), v (the 'q' vectors W['v'] back to back), beta (nq),
 * rti (the 's' blocks W['rti'] back to back, m_k^2 each).  'l' rows: di^2 g g'; 'q' cones: (G'G + 4|v|^2 p p' - 2 (p q' + q p'))
 * / beta^2 with p = G' J v, q = G' v; 's' blocks: the Gram matrix of pack2(rti' G(:, j) rti) over the clique columns j (FP64
 * MFMA).  Every entry is summed in a fixed order (no floating-point atomics).  Null stream, enqueue only. */
int kvx_cone_assemble_dev(kvx_cone *C, const double *Gx_dev, const double *di_dev, const double *v_dev, const double *beta_dev,
                          const double *rti_dev, double *Sx_dev);
/* The same with a symmetric n x n matrix H added: S = H + Gs' Gs (coneqp with H = P, misc.py:1275-1277: K += H).  Hp, Hi: CCS
 * pattern of H; its lower triangle is used and entries above the diagonal are ignored.  The pattern of S (kvx_cone_pattern) is
 * the union of the cliques and tril(H).  Hp == NULL: exactly kvx_cone_plan.  An entry stored twice is KVX_EINVAL.  Host only. */
int kvx_cone_plan_h(int64_t ml, int64_t nq, const int64_t *q, int64_t ns, const int64_t *s, int64_t n, const int64_t *Gp,
                    const int64_t *Gi, const int64_t *Hp, const int64_t *Hi, kvx_cone **out);
/* Sx_dev[snz] := H + Gs' Gs on a plan of kvx_cone_plan_h; Hx_dev: the values on (Hp, Hi), all of them (those above the diagonal
 * are not read).  H is added inside the gather of the 'q' and 's' parts, last: cones, then blocks, then H; no floating-point
 * atomics.  Hx_dev == NULL on a plan without H: exactly kvx_cone_assemble_dev.  A plan made with a non-empty H pattern is
 * assembled through this entry only: kvx_cone_assemble_dev on it, or Hx_dev == NULL here, is KVX_EINVAL.  Null stream,
 * enqueue only. */
int kvx_cone_assemble_h_dev(kvx_cone *C, const double *Gx_dev, const double *di_dev, const double *v_dev, const double *beta_dev,
                            const double *rti_dev, const double *Hx_dev, double *Sx_dev);
void kvx_cone_free(kvx_cone *C);
/* helpers of the general-cone driver (coneprog.py:1273-1280, 1379-1431): y[idx[i]] := x[i] (an 's' diagonal placed into its
 * block), and x_k(i, j) *= sqrt(w_j) for every 's' block (w in the off1 layout of the kvx_nts_* entries) */
int kvx_vec_scatter_dev(int64_t n, const double *x_dev, const int64_t *idx_dev, double *y_dev);
int kvx_nts_colscale_dev(int64_t ns, const int64_t *off2_dev, const int64_t *off1_dev, double *x_dev, const double *w_dev);

/* ---- geometric programs: the log-sum-exp blocks of solvers.gp (cvxprog.py:2094-2153, the Fgp closure) --------------------
 * f_i(x) = log sum_k exp(F_i x + g_i)_k for the nblk = m + 1 blocks of K[i] rows each of F (sum K rows, n columns, CCS; rows
 * inside a column in any order).  The plan reorders F by blocks (a CSR view for F x + g, the entries of a block in a column as
 * one segment) and fixes two patterns: Df ((m + 1) x n, CCS): row i holds the columns met by the rows of block i; H (n x n,
 * lower CCS): the union over the blocks -- block 0, the objective, included: it enters H through z[0] (cvxprog.py:2148-2150) --
 * of the cliques on those column sets.  An entry of F stored twice is KVX_EINVAL.  Host only. */
typedef struct kvx_gp kvx_gp;
int kvx_gp_plan(int64_t nblk, const int64_t *K, int64_t n, const int64_t *Fp, const int64_t *Fi, kvx_gp **out);
/* the two patterns (Dfp, Hp: n + 1; Dfi: dnz; Hi: hnz; every pointer may be NULL, e.g. to query dnz and hnz first) */
int kvx_gp_pattern(kvx_gp *P, int64_t *dnz, int64_t *Dfp, int64_t *Dfi, int64_t *hnz, int64_t *Hp, int64_t *Hi);
/* cvxprog.py:2106-2153: y = F x + g (Fx_dev: the values on the planned (Fp, Fi)); per block the maximum, exp(y - max), the sum,
 * f_dev[i] = max + log(sum), y normalised; Dfx_dev[dnz] := the values of Df = [y_i' F_i] on the plan's pattern.  With z_dev
 * (m + 1 weights) Hx_dev[hnz] := sum_i z_i F_i' (diag(y_i) - y_i y_i') F_i on the plan's lower pattern, formed as the reference
 * forms it from the centred factors diag(y_i)^1/2 (F_i - 1 Df_i) (FP64 MFMA Gram tiles), the blocks of an entry summed in
 * order.  z_dev == NULL (the line-search form F(x)): Hx_dev is not touched.  A block of one term gives y = 1, Df_i = F_i and
 * a zero Hessian term exactly.  No floating-point atomics: a second call on the same inputs gives the same bytes.  KVX_EDEVICE
 * without a GPU (no CPU fallback).  Null stream, enqueue only. */
int kvx_gp_eval_dev(kvx_gp *P, const double *Fx_dev, const double *g_dev, const double *x_dev, const double *z_dev, double *f_dev,
                    double *Dfx_dev, double *Hx_dev);
void kvx_gp_free(kvx_gp *P);

/* ---- ADMM for quadratic programs on one kept Cholesky factor: what kvxopt.osqp (src/C/osqp.c:192-368) gets from the external
 * OSQP library (osqp_setup / osqp_solve), as the published algorithm (Stellato et al., "OSQP: an operator splitting solver for
 * quadratic programs", 2020).  minimise 1/2 x'Px + q'x subject to l <= Ax <= u; A is m x n CCS, P n x n CCS of which the lower
 * triangle is read (Pp == NULL: P = 0); |bound| >= 1e26 is infinite.
 * kvx_admm_plan (host only): `scaling` Ruiz passes on [[P, A'], [A, 0]] (column infinity norms, below 1e-4 -> 1, above 1e4 ->
 * 1e4, delta = 1 / sqrt(norm)) each followed by the cost scaling gamma = 1 / max(mean column norm of P, |q|_inf) with the same
 * limits; returns D (n), E (m), c and nnz of the lower pattern of S = P + sigma I + A' diag(rho) A = tril(P) U I U tril(A'A),
 * which is analysed once.  The scaled data are c D P D, c D q, E A D, E l, E u; the state below is the scaled one.
 * kvx_admm_setup_dev(sigma, rho, alpha): uploads, builds the rho vector (1e3 rho on rows with u - l < 1e-4, 1e-6 on rows without
 * a finite bound, rho elsewhere; rho clipped to [1e-6, 1e6]), assembles S (kvx_atda_assemble_dev) and factors it;
 * KVX_ENOTPOSDEF: S is not positive definite, the problem is not convex.  x = z = y = 0.
 * kvx_admm_iterate(k, out): k iterations
 *     xt = S^-1 (sigma x - q + A'(rho o z - y)),  x+ = alpha xt + (1 - alpha) x,  v = alpha A xt + (1 - alpha) z,
 *     z+ = clip(v + y / rho, l, u),  y+ = y + rho o (v - z+),  dx = x+ - x,  dy = y+ - y
 * issued back to back without a host synchronisation, then the residuals of the state in one host read, out[24]:
 *     [0] |Ax - z|  [1] |Ax|  [2] |z|  [3] |Px + q + A'y|  [4] |Px|  [5] |A'y|  [6] |q|      infinity norms, scaled problem
 *     [7] .. [13]   the same seven of the unscaled problem (x = D x, z = E^-1 z, y = E y / c)
 *     [14] |dy|  [15] u'(dy)+ + l'(dy)-  [16] |A'dy|       unscaled, dy without the parts that push against an infinite bound
 *     [17] |dx|  [18] q'dx  [19] |P dx|  [20] max (A dx)_i over rows with finite u  [21] max -(A dx)_i over rows with finite l
 *     [22] x'Px  [23] q'x  (scaled; the objective is ([22] / 2 + [23]) / c).  A maximum over no rows is -DBL_MAX.
 * kvx_admm_set_rho: new rho vector, S reassembled on the same pattern and refactored (no new analysis).
 * kvx_admm_state: the scaled x (n), z, y (m), dx (n), dy (m) to the host; any pointer may be NULL.
 * kvx_admm_solution: kind 0: x = D x, y = E y / c;  1: y = the certificate of primal infeasibility ([14]-[16]'s dy), x not
 * written;  2: x = D dx, the certificate of dual infeasibility, y not written;  3: the polished x = D xh, y = E yh / c
 * (KVX_EINVAL unless the last kvx_admm_polish factored and no kvx_admm_update came after it).
 * kvx_admm_info: m, n, nnz(S), factorisations, iterations, rows summed by 16 lanes, rows summed by a wavefront, set up (0/1).
 * Fixed summation order, no floating-point atomics: two runs give the same bytes.  Device entry points return KVX_EDEVICE
 * without a GPU (no CPU fallback).  Null stream. */
typedef struct kvx_admm kvx_admm;
int kvx_admm_plan(int64_t m, int64_t n, const int64_t *Ap, const int64_t *Ai, const double *Ax, const int64_t *Pp, const int64_t *Pi,
                  const double *Px, const double *q, const double *l, const double *u, int64_t scaling, double *D, double *E,
                  double *c, int64_t *snz, kvx_admm **out);
int kvx_admm_pattern(kvx_admm *S, int64_t *snz, int64_t *Sp, int64_t *Si);      /* lower CCS pattern of S; pointers may be NULL */
int kvx_admm_rho_vector(kvx_admm *S, double rho, double *rho_host);             /* host only: the m entries for this rho */
int kvx_admm_setup_dev(kvx_admm *S, double sigma, double rho, double alpha);
int kvx_admm_iterate(kvx_admm *S, int64_t k, double *out_host);
int kvx_admm_set_rho(kvx_admm *S, double rho);
int kvx_admm_state(kvx_admm *S, double *x, double *z, double *y, double *dx, double *dy);
int kvx_admm_solution(kvx_admm *S, int kind, double *x, double *y);
int kvx_admm_info(kvx_admm *S, int64_t info[8]);
void kvx_admm_free(kvx_admm *S);

/* ---- a problem kept on the device across solves: same pattern, same analysis, same factor.  All after kvx_admm_setup_dev.
 * kvx_admm_update(q, l, u): host pointers to unscaled data, any of them NULL (kept).  Rescaled on the device with the plan's
 * D, E, c, which are not recomputed: q := (c D) o q, l := E o l, u := E o u; l <= -1e26 stays -1e30 and u >= 1e26 stays 1e30.  The
 * rho classes of the rows (equality, free, other) are derived again: if none changed nothing is assembled or factored, else
 * the rho vector at the current rho is issued, S reassembled on its pattern and factored once (counted by kvx_admm_info).
 * l_i > u_i: KVX_EINVAL, nothing changed (checked before a device is asked for).  The values of P and A cannot be replaced.
 * kvx_admm_warm_start(x, y): unscaled host vectors, either NULL (kept): x := D^-1 x and z := A x;  y := (c E^-1) o y;  dx = dy = 0.
 * kvx_admm_cold_start: x = z = y = dx = dy = 0; rho and the factor are kept.
 * kvx_admm_polish(delta, refine_iter, out): OSQP's polish in the scaled problem, in the eliminated form of its regularised
 * system [[P + delta I, A_act'], [A_act, -delta I]]; enqueued without a host synchronisation until the one read of out.
 *     active set from the state: lower z_i - l_i < -y_i, upper u_i - z_i < y_i;  w_i = 1 / delta on active rows, 0 elsewhere;
 *     b_i = l_i or u_i;  S_pol = P + delta I + A' diag(w) A assembled on the kept pattern and factored (no analysis);
 *     first solve   xh = S_pol^-1 (-q + A'(w o b)),  yh = w o (A xh - b);
 *     refine_iter x e1 = -q - (P xh + A' yh),  e2 = b - A xh on active rows and 0 elsewhere,
 *                   dx = S_pol^-1 (e1 + A'(w o e2)),  dy = w o (A dx - e2),  xh += dx,  yh += dy;
 *     zh = clip(A xh, l, u).
 *   out[16]:  [0] 1: factored, -1: S_pol is not positive definite (the call still returns 0; only [1], [2] are then set)
 *     [1] rows active at l  [2] rows active at u  [3] |A xh - zh|  [4] |P xh + q + A' yh|  (scaled, as [0], [3] of kvx_admm_iterate)
 *     [5] [6] the same two of the unscaled problem (as [7], [10] there)  [7] xh'P xh  [8] q'xh  (scaled; objective ([7] / 2 + [8]) / c)
 *     [9] |e1|  [10] |e2| of the last pass before its correction (refine_iter = 0: of the first solve, |q| and |b|)  [11]-[15] 0.
 *   The polished vectors live in buffers of their own: the ADMM state is not touched.  The kept numeric factor is now that of
 *   S_pol and the handle marks the ADMM factor stale: the next kvx_admm_iterate with k > 0 rebuilds it at the current rho first
 *   (one counted numeric factorisation, no analysis); kvx_admm_set_rho and a class-changing kvx_admm_update rebuild it anyway.
 *   The polish's own factorisation is counted too.
 * kvx_admm_polish_state: the scaled xh (n), zh, yh (m) and the flags -1 (at l) / 0 / +1 (at u) to the host; any pointer may be NULL.
 * kvx_admm_polish_accept: x, z, y := xh, zh, yh and dx = dy = 0, so that the next warm start begins at the polished point.
 * Whether to accept is the caller's decision.  Fixed summation order, no floating-point atomics; KVX_EDEVICE without a GPU. */
int kvx_admm_update(kvx_admm *S, const double *q, const double *l, const double *u);
int kvx_admm_warm_start(kvx_admm *S, const double *x, const double *y);
int kvx_admm_cold_start(kvx_admm *S);
int kvx_admm_polish(kvx_admm *S, double delta, int64_t refine_iter, double *out_host);
int kvx_admm_polish_state(kvx_admm *S, double *x, double *z, double *y, int64_t *act);
int kvx_admm_polish_accept(kvx_admm *S);

/* ---- a batch on the kept factor: B data sets (q_b, l_b, u_b) through the one factor of the kept problem, at its current rho.
 * All after kvx_admm_setup_dev.  Matrices are column-major, member b in column b: n x B (ld = n) or m x B (ld = m).  The batch
 * has buffers of its own: the kept problem's q, l, u, state, rho and factor are not touched.
 * kvx_admm_batch_begin(B, Q, L, U): host pointers to unscaled data, any of them NULL (the kept problem's vector in every
 *   column).  1 <= B <= 65535.  Rescaled on the device with the plan's D, E, c by the rule of kvx_admm_update; x = z = y = dx =
 *   dy = 0 for every member.  Every member must give every row the rho class (equality, free, other) it has in the kept problem
 *   and l <= u: otherwise KVX_EINVAL, the message names member and row, nothing is changed.  Device memory: 4 n B + 5 m B doubles
 *   and the B x 24 x (workgroups) partial results.
 * kvx_admm_batch_iterate(k, running, out): running[b] != 0: member b is iterated; a member with running[b] == 0 is frozen --
 *   its state and its 24 numbers are not written.  k x {right-hand sides, one triangular solve with B right-hand sides, update},
 *   then the residual kernels and one copy: out[b * 24 + i] is entry [i] of kvx_admm_iterate for member b.  A factor a polish
 *   left stale is rebuilt first at the current rho (k > 0; one counted factorisation), as kvx_admm_iterate does.  No rho ever
 *   changes inside a batch.
 * kvx_admm_batch_state: the scaled x (n x B), z, y (m x B), dx, dy to the host; any pointer may be NULL.
 * kvx_admm_batch_solution(kinds, X, Y): per member the unscaled result of kvx_admm_solution for kind 0, 1, 2 (the part a kind
 *   does not give is zero), kind -1: zeros.
 * kvx_admm_batch_end: frees the batch buffers (kvx_admm_free frees them too); a later begin allocates again.
 * Fixed summation order, no floating-point atomics; KVX_EDEVICE without a GPU, KVX_EINVAL before setup or before begin. */
int kvx_admm_batch_begin(kvx_admm *S, int64_t B, const double *Q, const double *L, const double *U);
int kvx_admm_batch_iterate(kvx_admm *S, int64_t k, const int64_t *running, double *out_host);
int kvx_admm_batch_state(kvx_admm *S, double *x, double *z, double *y, double *dx, double *dy);
int kvx_admm_batch_solution(kvx_admm *S, const int64_t *kinds, double *X, double *Y);
int kvx_admm_batch_end(kvx_admm *S);

/* ---- B small dense QPs, each with its own matrices: replaces a loop of solvers.qp calls (coneprog.py:1762-2547 on the
 * orthant: the starting point :2044-2105, the residuals and the stopping test :2167-2234, the scaling and the two directions
 * :2243-2456, the step and the scaling update :2459-2547 with misc.py:444-464; the Newton systems of misc.kkt_chol2,
 * misc.py:1436-1563, with dense Cholesky factors of S = P + G' W^-2 G and, for p > 0, of K = X'X, X = L^-1 A').
 *     minimize (1/2) x'P_b x + q_b'x   subject to   G_b x <= h_b,  A_b x = b_b,      b = 0..B-1,
 * in ONE launch, one workgroup per member from its starting point to its status (csrc/qp_batch.hip); refinement 0, no
 * initial values.  1 <= n <= 64, 1 <= ml <= 512, 0 <= p <= n, 1 <= B <= 2^31 - 1.
 * Matrices are dense and column-major per member: P n x n (only its lower triangle is read), G ml x n, A p x n (A, b, y may be
 * NULL when p = 0).  Every datum comes with its member stride in doubles: member b starts at stride * b; 0 means one for all
 * members, anything else must be at least the datum's size.
 * Options as coneprog.py:1768-1801: maxiters >= 1, feastol > 0, abstol or reltol > 0, use_correction 0 / 1.
 * Results, member b in column b: x (n x B), y (p x B), s, z (ml x B); stats (8 x B): gap, relative gap (NaN where the
 * reference returns None), primal objective, dual objective, primal infeasibility, dual infeasibility, primal slack, dual
 * slack; iterations and exitcode (B each).  exitcode 0: optimal; 1: maxiters reached; 2: singular KKT matrix after the first
 * iteration (coneprog.py:2256-2275: the iterates of that iteration are returned); 3: the factorisation with W = I or the first
 * one failed (coneprog.py:2259 raises ValueError("Rank(A) < p or Rank([P; A; G]) < n")): x, y, s, z are zero, iterations 0
 * and the stats NaN.  A factorisation fails on a pivot that is <= 0 or not finite, in S or in K.  A member never disturbs
 * another: its bytes depend on its own data alone, not on B or its place.  Fixed summation order, no floating-point atomics.
 * kvx_qp_batch_solve: host pointers; uploads, launches, downloads.  kvx_qp_batch_solve_dev: device pointers, results complete
 * on return.  KVX_EINVAL for bad sizes, limits, strides, options or NULL pointers on any box, before a device is asked for;
 * KVX_EDEVICE without a GPU (never a CPU fallback). */
int kvx_qp_batch_solve(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *q, int64_t sq,
                       const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb,
                       int64_t maxiters, double abstol, double reltol, double feastol, int use_correction, double *x, double *y, double *s,
                       double *z, double *stats, int64_t *iterations, int64_t *exitcode);
int kvx_qp_batch_solve_dev(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *q, int64_t sq,
                           const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b,
                           int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol, int use_correction, double *x,
                           double *y, double *s, double *z, double *stats, int64_t *iterations, int64_t *exitcode);

/* ---- derivatives of a solved batch of kvx_qp_batch_solve (no reference counterpart; the mathematics of Amos & Kolter,
 * "OptNet", 2017, section 3).  At the returned x, y, s, z of member b the differentiated KKT conditions are a linear system
 * with the matrix
 *     K = [P A' G'; A 0 0; G 0 -diag(s / z)],
 * the Newton matrix of the solver in the scaling di = sqrt(z / s): csrc/qp_batch_diff.hip assembles and factors it per member
 * as kvx_qp_batch_solve does (S = P + G' diag(z / s) G, X = L^-1 A', K = X'X), one workgroup per member, ONE launch, and solves
 * with `refinement` (0 to 3) steps of iterative refinement on the full system in float64 (the shape of f4, coneprog.py:2288-2316).
 * B, n, ml, p, P, G, A, their strides and their limits are those of kvx_qp_batch_solve; q, h, b do not enter.  x (n x B),
 * y (p x B), s, z (ml x B) and exitcode (B) are what kvx_qp_batch_solve returned.  The derivative is that of the solution handed
 * in, a point of the central path: for derivatives of the exact QP solve with tolerances near 1e-8 to 1e-9.
 * kvx_qp_batch_vjp (reverse mode): the cotangent gx (n x B); K [ux; uy; uz] = [-gx; 0; 0].  Results ux (n x B), uy (p x B),
 * uz (ml x B) -- the gradients of q, h, b are ux, -uz, -uy -- and for each of gP, gG, gA that is not NULL the gradient of that
 * matrix, (ux x' + x ux') / 2, uz x' + z ux', uy x' + y ux', column-major: per member, one after the other (B n^2, B ml n,
 * B p n doubles), where the matrix has a member stride, and the sum over the members as one matrix where its stride is 0
 * (csrc/qp_batch_diff.hip, k_batch_outer_sum: a second launch, fixed order, no atomics).  gP is symmetric to the last bit.
 * kvx_qp_batch_jvp (forward mode): perturbations dP (symmetric, its lower triangle read), dq, dG, dh, dA, db, each NULL (zero)
 * or with its member stride in doubles (0: one for all, otherwise at least its size);
 * K [dx; dy; dz] = [-(dP x + dq + dG'z + dA'y); db - dA x; dh - dG x] and ds = -(s / z) dz.  Results dx, dy, dz, ds.
 * gexit (B): 0 done; 1 skipped, the member's exitcode is not 0; 2 a pivot of S or K failed (<= 0 or not finite) or an entry of
 * s or z is not positive and finite.  A member with 1 or 2 has zeros in every result and adds nothing to a sum.  A member's
 * bytes depend on its own data alone, not on B or its place; two identical calls return identical bytes.  A, y, uy / dy, gA,
 * dA, db may be NULL when p = 0.
 * kvx_qp_batch_vjp, kvx_qp_batch_jvp: host pointers; upload, launch, download.  The _dev entries: device pointers, no
 * workspace, results complete on return -- what an autograd function binds.  KVX_EINVAL for bad sizes, limits, strides, a
 * refinement outside 0 to 3 or NULL required pointers on any box, before a device is asked for; KVX_EDEVICE without a GPU
 * (never a CPU fallback).  kvx_qp_batch_diff_lds_bytes: the LDS of one workgroup of the derivative in bytes, -1 outside the
 * limits; *forward (may be NULL): that of kvx_qp_batch_solve, which is never smaller. */
int kvx_qp_batch_vjp(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *G, int64_t sG,
                     const double *A, int64_t sA, const double *x, const double *y, const double *s, const double *z,
                     const int64_t *exitcode, int64_t refinement, const double *gx, double *ux, double *uy, double *uz, double *gP,
                     double *gG, double *gA, int64_t *gexit);
int kvx_qp_batch_vjp_dev(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *G, int64_t sG,
                         const double *A, int64_t sA, const double *x, const double *y, const double *s, const double *z,
                         const int64_t *exitcode, int64_t refinement, const double *gx, double *ux, double *uy, double *uz, double *gP,
                         double *gG, double *gA, int64_t *gexit);
int kvx_qp_batch_jvp(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *G, int64_t sG,
                     const double *A, int64_t sA, const double *x, const double *y, const double *s, const double *z,
                     const int64_t *exitcode, int64_t refinement, const double *dP, int64_t sdP, const double *dq, int64_t sdq,
                     const double *dG, int64_t sdG, const double *dh, int64_t sdh, const double *dA, int64_t sdA, const double *db,
                     int64_t sdb, double *dx, double *dy, double *dz, double *ds, int64_t *gexit);
int kvx_qp_batch_jvp_dev(int64_t B, int64_t n, int64_t ml, int64_t p, const double *P, int64_t sP, const double *G, int64_t sG,
                         const double *A, int64_t sA, const double *x, const double *y, const double *s, const double *z,
                         const int64_t *exitcode, int64_t refinement, const double *dP, int64_t sdP, const double *dq, int64_t sdq,
                         const double *dG, int64_t sdG, const double *dh, int64_t sdh, const double *dA, int64_t sdA, const double *db,
                         int64_t sdb, double *dx, double *dy, double *dz, double *ds, int64_t *gexit);
int64_t kvx_qp_batch_diff_lds_bytes(int64_t n, int64_t ml, int64_t p, int64_t *forward);

/* ---- B small dense LPs, each with its own matrices: replaces a loop of solvers.lp calls (coneprog.py:662-1436 on the orthant:
 * the starting point with W = I, both pushes and the optimal-at-iteration-0 return :662-842, the residuals and the three
 * stopping tests with their scalings :861-1024, the scaling, the constant system and f6_no_ir :1031-1195, the two directions
 * :1248-1333, the step and the scaling update :1336-1436 with misc.py:444-464; the Newton systems of misc.kkt_chol2,
 * misc.py:1395-1563, with dense Cholesky factors of S = G' W^-2 G and, for p > 0, of K = X'X, X = L^-1 A', and its
 * F['singular'] repair S + A'A, misc.py:1433-1458, 1526-1527, when the first factor of S fails and p > 0).
 *     minimize c_b'x   subject to   G_b x + s = h_b,  s >= 0,  A_b x = b_b,      b = 0..B-1,
 * in ONE launch, one workgroup per member from its starting point to its status or certificate (csrc/lp_batch.hip);
 * refinement 0, no starting points.  1 <= n <= 64, 1 <= ml <= 512, 0 <= p <= n, p + ml >= n, 1 <= B <= 2^31 - 1.
 * Matrices are dense and column-major per member: G ml x n, A p x n (A, b, y may be NULL when p = 0).  Every datum comes
 * with its member stride in doubles: member b starts at stride * b; 0 means one for all members, anything else must be at
 * least the datum's size.  Options as coneprog.py:425-455: maxiters >= 1, feastol > 0, abstol or reltol > 0.
 * Results, member b in column b: x (n x B), y (p x B), s, z (ml x B); stats (10 x B): gap, relative gap, primal objective,
 * dual objective, primal infeasibility, dual infeasibility, primal slack, dual slack, residual as primal infeasibility
 * certificate, residual as dual infeasibility certificate -- NaN where the reference returns None; iterations and exitcode
 * (B each).  exitcode 0: optimal; 1: maxiters reached; 2: singular KKT matrix after the first iteration (coneprog.py:1078-1109:
 * the iterates scaled by 1 / tau are returned); 3: the factorisation with W = I or the first one failed, the repair included
 * (solvers.lp raises ValueError("Rank(A) < p or Rank([G; A]) < n")): x, y, s, z are zero, iterations 0 and the stats NaN;
 * 4: primal infeasible, y and z are the certificate scaled to h'z + b'y = -1, x and s are NaN (coneprog.py:976-999);
 * 5: dual infeasible, x and s are the certificate scaled to c'x = -1, y and z are NaN (coneprog.py:1000-1024).
 * A factorisation fails on a pivot that is <= 0 or not finite, in S or in K.  A member never disturbs another: its bytes depend
 * on its own data alone, not on B or its place.  Fixed summation order, no floating-point atomics.
 * kvx_lp_batch_solve: host pointers; uploads, launches, downloads.  kvx_lp_batch_solve_dev: device pointers, results complete
 * on return.  KVX_EINVAL for bad sizes, limits, strides, options or NULL pointers on any box, before a device is asked for;
 * KVX_EDEVICE without a GPU (never a CPU fallback). */
int kvx_lp_batch_solve(int64_t B, int64_t n, int64_t ml, int64_t p, const double *c, int64_t sc, const double *G, int64_t sG,
                       const double *h, int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb, int64_t maxiters,
                       double abstol, double reltol, double feastol, double *x, double *y, double *s, double *z, double *stats,
                       int64_t *iterations, int64_t *exitcode);
int kvx_lp_batch_solve_dev(int64_t B, int64_t n, int64_t ml, int64_t p, const double *c, int64_t sc, const double *G, int64_t sG,
                           const double *h, int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb, int64_t maxiters,
                           double abstol, double reltol, double feastol, double *x, double *y, double *s, double *z, double *stats,
                           int64_t *iterations, int64_t *exitcode);

/* ---- B small dense second-order-cone programs, each with its own matrices: replaces a loop of solvers.socp calls
 * (coneprog.socp -> coneprog.conelp, coneprog.py:662-1436, with the 'q' blocks of misc.compute_scaling / update_scaling,
 * misc.py:290-352, 467-580, of misc_solvers.scale, scale2, sprod, sinv, misc_solvers.c:144-186, 301-341, 671-700, 803-835, and
 * of max_step, misc_solvers.c:1073-1085; the Newton systems of misc.kkt_chol2, misc.py:1395-1563, on Gs = W^-T G, with its
 * F['singular'] repair).
 *     minimize c_b'x   subject to   G_b x + s = h_b,  s in R^ml_+ x Q^{q[0]} x ... x Q^{q[nq-1]},  A_b x = b_b,      b = 0..B-1,
 * in ONE launch, one workgroup per member from its starting point to its status or certificate (csrc/socp_batch.hip);
 * refinement 0 (solvers.socp defaults to 1), no starting points.  The cone is the same for every member: q is a HOST array of
 * nq cone orders for both entries (it travels with the kernel's arguments), rows stacked as in conelp, the ml 'l' rows first.
 * 1 <= n <= 64, ml >= 0, 0 <= nq <= 128, every q[k] >= 1, 1 <= N = ml + sum q <= 512, 0 <= p <= n, p + N >= n,
 * 1 <= B <= 2^31 - 1.  Matrices, strides, options, results, stats, exit codes and the independence of the members are those of
 * kvx_lp_batch_solve with N rows in G, h, s and z; primal and dual slack are -max_step over the whole cone.
 * kvx_socp_batch_solve: host pointers; uploads, launches, downloads.  kvx_socp_batch_solve_dev: device pointers (q excepted),
 * no workspace, results complete on return.  KVX_EINVAL for bad sizes, limits, strides, options, NULL pointers or cone orders
 * on any box, before a device is asked for; KVX_EDEVICE without a GPU (never a CPU fallback). */
int kvx_socp_batch_solve(int64_t B, int64_t n, int64_t ml, int64_t nq, const int64_t *q, int64_t p, const double *c, int64_t sc,
                         const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b,
                         int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol, double *x, double *y, double *s,
                         double *z, double *stats, int64_t *iterations, int64_t *exitcode);
int kvx_socp_batch_solve_dev(int64_t B, int64_t n, int64_t ml, int64_t nq, const int64_t *q, int64_t p, const double *c, int64_t sc,
                             const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b,
                             int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol, double *x, double *y,
                             double *s, double *z, double *stats, int64_t *iterations, int64_t *exitcode);

/* ---- B small dense semidefinite programs, each with its own matrices: replaces a loop of solvers.sdp / solvers.conelp calls
 * (coneprog.sdp -> coneprog.conelp, coneprog.py:662-1436, with the 's' blocks of misc.compute_scaling / update_scaling,
 * misc.py:354-419, 582-634, of misc_solvers.scale, scale2, sprod, sinv, sdot and max_step, misc_solvers.c:188-240, 343-397,
 * 700-770, 845-882, 1029-1046, 1086-1160; the Newton systems of misc.kkt_chol2, misc.py:1395-1563, on Gs = W^-T G, with its
 * F['singular'] repair).
 *     minimize c_b'x   subject to   G_b x + s = h_b,  s in R^ml_+ x S^{m[0]}_+ x ... x S^{m[ns-1]}_+,  A_b x = b_b,      b = 0..B-1,
 * in ONE launch, one workgroup per member from its starting point to its status or certificate (csrc/sdp_batch.hip);
 * refinement 0 (solvers.sdp defaults to 1), no starting points.  The cone is the same for every member: m is a HOST array of ns
 * block orders for both entries (it travels with the kernel's arguments), rows stacked as in conelp, the ml 'l' rows first,
 * then every block as its m[k] x m[k] matrix in column-major order, of which only the lower triangle is read in G and h.
 * 1 <= n <= 64, ml >= 0, 0 <= ns <= 32, 1 <= m[k] <= 16, 1 <= N = ml + sum m^2 <= 384, 0 <= p <= n,
 * p + ml + sum m (m + 1) / 2 >= n, 1 <= B <= 2^31 - 1.  Matrices, strides, options, results, stats, exit codes and the
 * independence of the members are those of kvx_lp_batch_solve with N rows in G, h, s and z; the 's' blocks of s and z are
 * returned as full symmetric matrices; primal and dual slack are -max_step over the whole cone.
 * kvx_sdp_batch_solve: host pointers; uploads, launches, downloads.  kvx_sdp_batch_solve_dev: device pointers (m excepted),
 * no workspace, results complete on return.  KVX_EINVAL for bad sizes, limits, strides, options, NULL pointers or block orders
 * on any box, before a device is asked for; KVX_EDEVICE without a GPU (never a CPU fallback). */
int kvx_sdp_batch_solve(int64_t B, int64_t n, int64_t ml, int64_t ns, const int64_t *m, int64_t p, const double *c, int64_t sc,
                        const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b,
                        int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol, double *x, double *y, double *s,
                        double *z, double *stats, int64_t *iterations, int64_t *exitcode);
int kvx_sdp_batch_solve_dev(int64_t B, int64_t n, int64_t ml, int64_t ns, const int64_t *m, int64_t p, const double *c, int64_t sc,
                            const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA, const double *b,
                            int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol, double *x, double *y,
                            double *s, double *z, double *stats, int64_t *iterations, int64_t *exitcode);

/* ---- B small dense cone programs over all three kinds of cone, each with its own matrices: replaces a loop of solvers.conelp
 * calls (coneprog.conelp, coneprog.py:662-1436, with the 'q' and 's' blocks of misc.compute_scaling / update_scaling,
 * misc.py:290-419, 467-634, of misc_solvers.scale, scale2, sprod, sinv, sdot and max_step, misc_solvers.c:144-240, 301-397,
 * 671-770, 803-882, 1029-1160; the Newton systems of misc.kkt_chol2, misc.py:1395-1563, on Gs = W^-T G, with its F['singular']
 * repair).
 *     minimize c_b'x   subject to   G_b x + s = h_b,  s in R^ml_+ x Q^{q[0]} x ... x S^{m[0]}_+ x ...,  A_b x = b_b,      b = 0..B-1,
 * in ONE launch, one workgroup per member from its starting point to its status or certificate (csrc/conelp_batch.hip);
 * refinement 0 (solvers.conelp defaults to 1 with 'q' or 's' rows), no starting points.  The cone is the same for every
 * member: q and m are HOST arrays of nq cone orders and ns block orders for both entries (they travel with the kernel's
 * arguments), rows stacked as in conelp, the ml 'l' rows first, then the cones, then every block as its m[k] x m[k] matrix in
 * column-major order, of which only the lower triangle is read in G and h.
 * 1 <= n <= 64, ml >= 0, 0 <= nq <= 128, q[k] >= 1, 0 <= ns <= 32, 1 <= m[k] <= 16, 1 <= N = ml + sum q + sum m^2 <= 384,
 * 0 <= p <= n, p + ml + sum q + sum m (m + 1) / 2 >= n, 1 <= B <= 2^31 - 1.  Matrices, strides, options, results, stats, exit
 * codes and the independence of the members are those of kvx_lp_batch_solve with N rows in G, h, s and z; the 's' blocks of s
 * and z are returned as full symmetric matrices; primal and dual slack are -max_step over the whole cone.  The kernel is the
 * same whichever kinds are present; kvx_lp_batch_solve, kvx_socp_batch_solve and kvx_sdp_batch_solve are the faster entries
 * for their cones.
 * kvx_conelp_batch_solve: host pointers; uploads, launches, downloads.  kvx_conelp_batch_solve_dev: device pointers (q and m
 * excepted), no workspace, results complete on return.  KVX_EINVAL for bad sizes, limits, strides, options, NULL pointers,
 * cone orders or block orders on any box, before a device is asked for; KVX_EDEVICE without a GPU (never a CPU fallback). */
int kvx_conelp_batch_solve(int64_t B, int64_t n, int64_t ml, int64_t nq, const int64_t *q, int64_t ns, const int64_t *m, int64_t p,
                           const double *c, int64_t sc, const double *G, int64_t sG, const double *h, int64_t sh, const double *A,
                           int64_t sA, const double *b, int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol,
                           double *x, double *y, double *s, double *z, double *stats, int64_t *iterations, int64_t *exitcode);
int kvx_conelp_batch_solve_dev(int64_t B, int64_t n, int64_t ml, int64_t nq, const int64_t *q, int64_t ns, const int64_t *m, int64_t p,
                               const double *c, int64_t sc, const double *G, int64_t sG, const double *h, int64_t sh, const double *A,
                               int64_t sA, const double *b, int64_t sb, int64_t maxiters, double abstol, double reltol,
                               double feastol, double *x, double *y, double *s, double *z, double *stats, int64_t *iterations,
                               int64_t *exitcode);

/* ---- B small dense cone QPs over all three kinds of cone, each with its own matrices: replaces a loop of solvers.coneqp calls
 * (coneprog.coneqp, coneprog.py:1440-2547, with the 'q' and 's' blocks of misc.compute_scaling / update_scaling,
 * misc.py:290-419, 467-634, of misc_solvers.scale, scale2, sprod, sinv, sdot and max_step, misc_solvers.c:144-240, 301-397,
 * 671-770, 803-882, 1029-1160; the Newton systems of misc.kkt_chol with H = P, misc.py:1395-1563, on S = P + Gs'Gs,
 * Gs = W^-T G, without an A'A repair).
 *     minimize (1/2) x'P_b x + q_b'x   subject to   G_b x + s = h_b,  s in R^ml_+ x Q^{qdims[0]} x ... x S^{m[0]}_+ x ...,
 *     A_b x = b_b,      b = 0..B-1,
 * in ONE launch, one workgroup per member from its starting point to its status (csrc/coneqp_batch.hip); refinement 0
 * (solvers.coneqp defaults to 1 with 'q' or 's' rows), no initvals.  The cone, its HOST arrays qdims and m, the rows, the
 * matrices, strides and options are those of kvx_conelp_batch_solve, and so are the limits except that there is no rank
 * condition on the packed dimension: P (n x n per member, column-major, member stride sP or 0, its lower triangle read) may
 * supply the rank, and a member whose first factorisation fails ends with exit 3.  use_correction: the Mehrotra correction
 * (coneprog.py:2376-2392).  Results, stats (8 x B: gap, relative gap or NaN, primal and dual objective, primal and dual
 * infeasibility, primal and dual slack as -max_step over the whole cone), exit codes 0-3 and the independence of the members
 * are those of kvx_qp_batch_solve with N = ml + sum qdims + sum m^2 rows in G, h, s and z; the 's' blocks of s and z are
 * returned as full symmetric matrices.
 * kvx_coneqp_batch_solve: host pointers; uploads, launches, downloads.  kvx_coneqp_batch_solve_dev: device pointers (qdims
 * and m excepted), no workspace, results complete on return.  KVX_EINVAL for bad sizes, limits, strides, options, NULL
 * pointers, cone orders or block orders on any box, before a device is asked for; KVX_EDEVICE without a GPU (never a CPU
 * fallback). */
int kvx_coneqp_batch_solve(int64_t B, int64_t n, int64_t ml, int64_t nq, const int64_t *qdims, int64_t ns, const int64_t *m, int64_t p,
                           const double *P, int64_t sP, const double *q, int64_t sq, const double *G, int64_t sG, const double *h,
                           int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb, int64_t maxiters, double abstol,
                           double reltol, double feastol, int use_correction, double *x, double *y, double *s, double *z, double *stats,
                           int64_t *iterations, int64_t *exitcode);
int kvx_coneqp_batch_solve_dev(int64_t B, int64_t n, int64_t ml, int64_t nq, const int64_t *qdims, int64_t ns, const int64_t *m,
                               int64_t p, const double *P, int64_t sP, const double *q, int64_t sq, const double *G, int64_t sG,
                               const double *h, int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb, int64_t maxiters,
                               double abstol, double reltol, double feastol, int use_correction, double *x, double *y, double *s,
                               double *z, double *stats, int64_t *iterations, int64_t *exitcode);

/* ---- derivatives of a solved batch of kvx_coneqp_batch_solve (no reference counterpart).  The differentiated KKT conditions
 * of member b are a linear system with the matrix
 *     K = [P A' G'; A 0 0; G 0 -W'W],   W the Nesterov-Todd scaling of (s, z),
 * the Newton matrix of the solver.  On the 'q' and 's' rows W'W linearises the complementarity condition exactly only on the
 * central path (lmbda o lmbda = mu e), where the returned point is not.  So csrc/coneqp_batch_diff.hip, one workgroup per
 * member, ONE launch, first takes at most `centering` (0 to 16) centring steps from x, y, s, z -- a Newton step of the solver
 * with sigma = 1, no Mehrotra term, mu = s'z / degree of the point handed in, step length min(1, 0.99 / t) -- until
 * |lmbda o lmbda - mu e|_2 <= centol mu (centol > 0), and then solves with K at the centred point and `refinement` (0 to 3)
 * steps of iterative refinement on the full system in float64.  centering = 0 takes the point as it is.
 * B .. sb: the problem as kvx_coneqp_batch_solve takes it, with its limits.  x (n x B), y (p x B), s, z (N x B, 's' blocks as
 * full symmetric matrices) and exitcode (B) are what kvx_coneqp_batch_solve returned; they are not written.
 * kvx_coneqp_batch_vjp (reverse mode): the cotangent gx (n x B); K [ux; uy; uz] = [-gx; 0; 0].  Results ux (n x B), uy (p x B),
 * uz (N x B, 's' blocks full symmetric) -- the gradients of q, h, b are ux, -uz, -uy -- and for each of gP, gG, gA that is not
 * NULL the gradient of that matrix at the centred x, y, z, (ux x' + x ux') / 2, uz x' + z ux', uy x' + y ux', column-major: per
 * member, one after the other (B n^2, B N n, B p n doubles), where the matrix has a member stride, and the sum over the done
 * members as one matrix where its stride is 0 (k_batch_outer_sum of csrc/qp_batch_diff.hip: a second launch, fixed order, no
 * atomics).  Rows (i, j) and (j, i) of an 's' block of gG and of uz evaluate one expression: the gradient with respect to a
 * symmetric argument, as gP is; who holds only the lower triangle as free parameters adds the two.
 * kvx_coneqp_batch_jvp (forward mode): perturbations dP, dq, dG, dh, dA, db, each NULL (zero) or with its member stride in
 * doubles (0: one for all, otherwise at least its size); of dP and of every 's' block of dG and dh the lower triangle is read.
 * K [dx; dy; dz] = [-(dP x + dq + dG'z + dA'y); db - dA x; dh - dG x] and ds = -W'W dz.  Results dx, dy, dz, ds.
 * centrality (B): the final |lmbda o lmbda - mu e|_2 / mu, NaN for a member with gexit 1 or 2; steps (B): the centring steps
 * taken.  gexit (B): 0 done; 1 skipped, the member's exitcode is not 0; 2 the scaling or a pivot failed or a value is not
 * finite; 3 not centred within `centering` steps.  A member with 1, 2 or 3 has zeros in every derivative and adds nothing to a
 * sum.  A member's bytes depend on its own data alone, not on B or its place; two identical calls return identical bytes.
 * A, b, y, uy / dy, gA, dA, db may be NULL when p = 0.
 * kvx_coneqp_batch_vjp, kvx_coneqp_batch_jvp: host pointers; upload, launch, download.  The _dev entries: device pointers
 * (qdims and m excepted), no workspace, results complete on return.  KVX_EINVAL for bad sizes, limits, strides, options or
 * NULL required pointers on any box, before a device is asked for; KVX_EDEVICE without a GPU (never a CPU fallback).
 * kvx_coneqp_batch_diff_lds_bytes: the LDS of one workgroup of the derivative in bytes, -1 outside the limits; *forward (may
 * be NULL): that of kvx_coneqp_batch_solve, which is 8 (n + p) bytes smaller, rounded up to 16 each. */
int kvx_coneqp_batch_vjp(int64_t B, int64_t n, int64_t ml, int64_t nq, const int64_t *qdims, int64_t ns, const int64_t *m, int64_t p,
                         const double *P, int64_t sP, const double *q, int64_t sq, const double *G, int64_t sG, const double *h,
                         int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb, const double *x, const double *y,
                         const double *s, const double *z, const int64_t *exitcode, int64_t refinement, int64_t centering,
                         double centol, const double *gx, double *ux, double *uy, double *uz, double *gP, double *gG, double *gA,
                         double *centrality, int64_t *steps, int64_t *gexit);
int kvx_coneqp_batch_vjp_dev(int64_t B, int64_t n, int64_t ml, int64_t nq, const int64_t *qdims, int64_t ns, const int64_t *m, int64_t p,
                             const double *P, int64_t sP, const double *q, int64_t sq, const double *G, int64_t sG, const double *h,
                             int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb, const double *x, const double *y,
                             const double *s, const double *z, const int64_t *exitcode, int64_t refinement, int64_t centering,
                             double centol, const double *gx, double *ux, double *uy, double *uz, double *gP, double *gG, double *gA,
                             double *centrality, int64_t *steps, int64_t *gexit);
int kvx_coneqp_batch_jvp(int64_t B, int64_t n, int64_t ml, int64_t nq, const int64_t *qdims, int64_t ns, const int64_t *m, int64_t p,
                         const double *P, int64_t sP, const double *q, int64_t sq, const double *G, int64_t sG, const double *h,
                         int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb, const double *x, const double *y,
                         const double *s, const double *z, const int64_t *exitcode, int64_t refinement, int64_t centering,
                         double centol, const double *dP, int64_t sdP, const double *dq, int64_t sdq, const double *dG, int64_t sdG,
                         const double *dh, int64_t sdh, const double *dA, int64_t sdA, const double *db, int64_t sdb, double *dx,
                         double *dy, double *dz, double *ds, double *centrality, int64_t *steps, int64_t *gexit);
int kvx_coneqp_batch_jvp_dev(int64_t B, int64_t n, int64_t ml, int64_t nq, const int64_t *qdims, int64_t ns, const int64_t *m, int64_t p,
                             const double *P, int64_t sP, const double *q, int64_t sq, const double *G, int64_t sG, const double *h,
                             int64_t sh, const double *A, int64_t sA, const double *b, int64_t sb, const double *x, const double *y,
                             const double *s, const double *z, const int64_t *exitcode, int64_t refinement, int64_t centering,
                             double centol, const double *dP, int64_t sdP, const double *dq, int64_t sdq, const double *dG,
                             int64_t sdG, const double *dh, int64_t sdh, const double *dA, int64_t sdA, const double *db, int64_t sdb,
                             double *dx, double *dy, double *dz, double *ds, double *centrality, int64_t *steps, int64_t *gexit);
int64_t kvx_coneqp_batch_diff_lds_bytes(int64_t n, int64_t ml, int64_t nq, const int64_t *qdims, int64_t ns, const int64_t *m, int64_t p,
                                        int64_t *forward);

/* ---- many small dense geometric programs at once: B members of cvxprog.gp (cvxprog.py:1967-2155: the evaluator :2094-2153,
 * cp's epigraph form :1746-1964, cpl's iteration with its relaxed and backtracking line search :556-1356; the Newton systems
 * of misc.kkt_chol2, misc.py:1395-1563, on S = H + J' diag(di^2) J without an A'A repair)
 *     minimize log sum exp(F0_b x + g0_b)   subject to   log sum exp(Fi_b x + gi_b) <= 0 (i = 1..mnl),  G_b x <= h_b,
 *     A_b x = b_b,      b = 0..B-1,
 * in ONE launch, one workgroup per member from x = 0, t = 0, s = z = 1 to its status (csrc/gp_batch.hip); refinement 0
 * (solvers.gp defaults to 1).  K: a HOST array of mnl + 1 positive block sizes for both entries, block 0 the objective;
 * l = sum K.  F (l x n), G (ml x n), A (p x n): dense, column-major per member; g (l), h (ml), b (p); every datum with its
 * member stride in doubles (0: shared; otherwise at least its size).  Limits: 1 <= n <= 63, N = mnl + 1 + ml <= 192,
 * l <= 768, 0 <= p <= n, ml >= 0 (G, h may be NULL when ml = 0; A, b, y when p = 0).  Results: x (n x B), y (p x B), s, z
 * (N x B: the objective row of the epigraph form first, then the mnl constraint rows, then the ml rows of G), stats (8 x B:
 * gap, relative gap or NaN, primal and dual objective, primal and dual infeasibility, primal and dual slack), iterations and
 * exitcode (B each): 0 optimal, 1 maxiters, 2 singular KKT matrix after iteration 0, 3 the first factorisation failed (the
 * reference raises ValueError("Rank(A) < p or Rank([H(x); A; Df(x); G]) < n")): zeros, 0 iterations, NaN stats, 4 a line
 * search did not end within 64 halvings of its step (the reference has no bound): the last accepted iterate.  A member's bytes
 * do not depend on B, on its place or on the other members.
 * kvx_gp_batch_solve: host pointers; uploads, allocates the workspace, launches, downloads.  kvx_gp_batch_solve_dev: device
 * pointers (K excepted), results complete on return; scratch: B * kvx_gp_batch_scratch_doubles(n, mnl, ml, p) doubles of
 * device memory, contents arbitrary (a member's A with a zero column for t, and the saved state of its line search).
 * KVX_EINVAL for bad sizes, limits, strides, options, NULL pointers or a non-positive K[i] on any box, before a device is asked
 * for; KVX_EDEVICE without a GPU (never a CPU fallback).  kvx_gp_batch_scratch_doubles: -1 outside the limits. */
int64_t kvx_gp_batch_scratch_doubles(int64_t n, int64_t mnl, int64_t ml, int64_t p);
int kvx_gp_batch_solve(int64_t B, int64_t n, int64_t mnl, const int64_t *K, int64_t ml, int64_t p, const double *F, int64_t sF,
                       const double *g, int64_t sg, const double *G, int64_t sG, const double *h, int64_t sh, const double *A, int64_t sA,
                       const double *b, int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol, double *x, double *y,
                       double *s, double *z, double *stats, int64_t *iterations, int64_t *exitcode);
int kvx_gp_batch_solve_dev(int64_t B, int64_t n, int64_t mnl, const int64_t *K, int64_t ml, int64_t p, const double *F, int64_t sF,
                           const double *g, int64_t sg, const double *G, int64_t sG, const double *h, int64_t sh, const double *A,
                           int64_t sA, const double *b, int64_t sb, int64_t maxiters, double abstol, double reltol, double feastol,
                           double *x, double *y, double *s, double *z, double *stats, int64_t *iterations, int64_t *exitcode,
                           double *scratch);

/* ---- derivatives of a solved batch of geometric programs (csrc/gp_batch_diff.hip).  With zeta_0 = 1,
 * zeta_i = z_i (i = 1..mnl), y_i = softmax(F_i x + g_i) and Df_i = y_i'F_i per block, the optimality conditions of member b
 * differentiated at its returned x, y, s, z are a linear system in x-space (order n; the epigraph row is gone) with the matrix
 *     K = [ H  A'  J' ;  A  0  0 ;  J  0  -diag(s / z) ],   H = sum_i zeta_i F_i'(diag y_i - y_i y_i')F_i,   J = [Df_1..Df_mnl; G],
 * whose reduced matrix H + J' diag(z / s) J is assembled from the staged rows of k_gp_batch and factored once per member, one
 * workgroup each, in ONE launch, with `refinement` (0..3) steps of iterative refinement on the full system.
 * The problem arguments B .. sA are those of kvx_gp_batch_solve (K a HOST array for all entries); g enters (for y), h and b
 * do not.  x (n x B), y (p x B), exitcode (B) and s, z (N x B, N = mnl + 1 + ml, the objective row first) are what
 * kvx_gp_batch_solve[_dev] wrote; row 0 of s and z is not read.  uz, dz, ds have N rows too and row 0 is written as 0.
 * kvx_gp_batch_vjp (reverse mode): the cotangent gx (n x B); K [ux; uy; uz] = [-gx; 0; 0].  Results ux, uy (p x B), uz,
 *   gg (l x B) = dl/dg with gg_k = y_k (zeta_i (F_k - Df_i) ux + uz_i) (uz_0 = 0), and where the pointer is not NULL
 *   gF = a ux' + gg x' (l x n; a_k = zeta_i y_k), gG = uzl x' + zl ux' (ml x n), gA = uy x' + y ux' (p x n), column-major:
 *   one per member after the other for a matrix with a member stride, ONE matrix, the sum over the done members in an order
 *   fixed at compile time, for a shared one (stride 0).  dl/dh = -uzl and dl/db = -uy are left to the caller.
 *   The _dev entry takes `work`: l x B doubles of device memory that receive a, needed (not NULL) when gF is asked for and F
 *   is shared -- a workspace and not a result, since a is no derivative and a host caller has no use for l x B more doubles
 *   coming down; the host entry takes it from the pool.
 * kvx_gp_batch_jvp (forward mode): perturbations dF (l x n), dg (l), dG (ml x n), dh (ml), dA (p x n), db (p), each NULL (zero),
 *   shared (stride 0) or per member; with v = dF x + dg,
 *   K [dx; dy; dz] = [-(sum_i zeta_i (dF_i'y_i + F_i'(y_i o v_i - y_i (y_i'v_i))) + dG'zl + dA'y); db - dA x; (-y_i'v_i; dh - dG x)]
 *   and ds = -(s / z) dz.  Results dx, dy, dz, ds.
 * gexit (B): 0 done; 1 skipped since exitcode[b] != 0; 2 a failed pivot or an s_k, z_k (k >= 1) that is not positive and
 * finite.  1 and 2 leave zeros in every per-member output and add nothing to a shared sum.  A member's bytes do not depend on
 * B, on its place or on the other members.
 * Host entries: host pointers; upload, launch, download.  The _dev entries: device pointers (K excepted), results complete on
 * return.  KVX_EINVAL for bad sizes, limits, strides, refinement, NULL pointers or a non-positive K[i] on any box, before a
 * device is asked for; KVX_EDEVICE without a GPU (never a CPU fallback).  kvx_gp_batch_diff_lds_bytes: the LDS of one
 * workgroup of the derivative in bytes, -1 outside the limits; forward (may be NULL) receives that of k_gp_batch. */
int kvx_gp_batch_vjp(int64_t B, int64_t n, int64_t mnl, const int64_t *K, int64_t ml, int64_t p, const double *F, int64_t sF,
                     const double *g, int64_t sg, const double *G, int64_t sG, const double *A, int64_t sA, const double *x,
                     const double *y, const double *s, const double *z, const int64_t *exitcode, int64_t refinement, const double *gx,
                     double *ux, double *uy, double *uz, double *gg, double *gF, double *gG, double *gA, int64_t *gexit);
int kvx_gp_batch_vjp_dev(int64_t B, int64_t n, int64_t mnl, const int64_t *K, int64_t ml, int64_t p, const double *F, int64_t sF,
                         const double *g, int64_t sg, const double *G, int64_t sG, const double *A, int64_t sA, const double *x,
                         const double *y, const double *s, const double *z, const int64_t *exitcode, int64_t refinement,
                         const double *gx, double *ux, double *uy, double *uz, double *gg, double *gF, double *gG, double *gA,
                         double *work, int64_t *gexit);
int kvx_gp_batch_jvp(int64_t B, int64_t n, int64_t mnl, const int64_t *K, int64_t ml, int64_t p, const double *F, int64_t sF,
                     const double *g, int64_t sg, const double *G, int64_t sG, const double *A, int64_t sA, const double *x,
                     const double *y, const double *s, const double *z, const int64_t *exitcode, int64_t refinement, const double *dF,
                     int64_t sdF, const double *dg, int64_t sdg, const double *dG, int64_t sdG, const double *dh, int64_t sdh,
                     const double *dA, int64_t sdA, const double *db, int64_t sdb, double *dx, double *dy, double *dz, double *ds,
                     int64_t *gexit);
int kvx_gp_batch_jvp_dev(int64_t B, int64_t n, int64_t mnl, const int64_t *K, int64_t ml, int64_t p, const double *F, int64_t sF,
                         const double *g, int64_t sg, const double *G, int64_t sG, const double *A, int64_t sA, const double *x,
                         const double *y, const double *s, const double *z, const int64_t *exitcode, int64_t refinement,
                         const double *dF, int64_t sdF, const double *dg, int64_t sdg, const double *dG, int64_t sdG, const double *dh,
                         int64_t sdh, const double *dA, int64_t sdA, const double *db, int64_t sdb, double *dx, double *dy, double *dz,
                         double *ds, int64_t *gexit);
int64_t kvx_gp_batch_diff_lds_bytes(int64_t n, int64_t mnl, const int64_t *K, int64_t ml, int64_t p, int64_t *forward);

/* ---- dense helpers of the equality-constrained KKT solve with a general S (misc.py:1476-1487, 1545): K = A S^-1 A' formed
 * as a dense p x p matrix from X = S^-1 A' (kvx_chol_solve_dev with nrhs = p) when p is moderate ------------------------- */
/* Y(j, c) = sum_i A(i, j) X(i, c) for the CCS matrix A with n columns and every column c < ncols of the dense X */
int kvx_spmm_t_dev(int64_t n, int64_t ncols, const int64_t *Ap_dev, const int64_t *Ai_dev, const double *Ax_dev,
                   const double *X_dev, int64_t ldx, double *Y_dev, int64_t ldy);
/* D (m x n dense, leading dimension ld) := the CCS matrix */
int kvx_dense_from_ccs_dev(int64_t m, int64_t n, const int64_t *Ap_dev, const int64_t *Ai_dev, const double *Ax_dev,
                           double *D_dev, int64_t ld);
/* out := lower triangle of the dense p x p matrix K, column by column (the value array of a dense lower CCS pattern) */
int kvx_pack_lower_dev(int64_t p, const double *K_dev, int64_t ld, double *out_dev);
/* y := alpha A x + beta y, A dense column-major m x n (ld = lda), nrhs columns of x (ldx) and y (ldy): with X = S^-1 A' at hand,
 * S^-1 (b - A' uy) = S^-1 b - X uy is a product instead of a second solve with S (the role of misc.py:1545-1553) */
int kvx_dense_gemv_dev(int64_t m, int64_t n, int64_t nrhs, double alpha, const double *A_dev, int64_t lda, const double *x_dev, int64_t ldx,
                       double beta, double *y_dev, int64_t ldy);

/* ---- device memory plumbing for hosts without their own allocator ------------------------ */
int kvx_dev_malloc(void **p, int64_t bytes);
int kvx_dev_free(void *p);
int kvx_dev_upload(void *dst_dev, const void *src_host, int64_t bytes);
int kvx_dev_download(void *dst_host, const void *src_dev, int64_t bytes);
int kvx_dev_sync(void);
/* Device buffers, streams and events released by the library are kept in a caching pool (up to KVX_POOL_MAX_MB, default 8192)
 * and handed out again; kvx_dev_trim() gives everything cached back to the driver (e.g. before another framework needs the
 * memory).  No reference counterpart. */
int kvx_dev_trim(void);
int kvx_dev_mem_info(int64_t *free_bytes, int64_t *total_bytes);   /* hipMemGetInfo of the current device */

/* ---------------------------------------------------------------------------------------------------------
 * Sparse LU (the kvxopt.klu API, src/C/klu.c; SURVEY 8(f)1, BASELINE configs[2]).  Real 'd' matrices, square,
 * CCS with int64 indices.  Static-structure multifrontal LU with threshold partial pivoting inside the pivot
 * block of each front; fronts without an acceptable pivot are merged into their parents and the factorisation
 * repeats (kvxopt_amd/csrc/lu_symbolic.hpp).  Factorisation:  R P A Q = L U + F  as in KLU: P, Q bring A to block upper
 * triangular form (strongly connected components after the matching), L U are the factors of the diagonal blocks, F the
 * off-diagonal blocks (never eliminated), L unit lower, R = diag(1 / Rs).  (Chains of more than 64 dependent block levels
 * are factored as one block instead: they would serialise the solves.)
 * --------------------------------------------------------------------------------------------------------- */
typedef struct kvx_lu_sym kvx_lu_sym;      /* replaces the "KLU SYM D FACTOR" capsule (klu.c:36,276-279)   */
typedef struct kvx_lu_num kvx_lu_num;      /* replaces the "KLU NUM D FACTOR" capsule (klu.c:38,336-339)   */

/* symbolic(A) -- klu.c:242-291 (klu_analyze :264).  values may be NULL (pattern only: plain maximum
 * transversal); with values the matching maximises the product of the scaled diagonal.  A structurally
 * singular pattern is accepted here and reported by the numeric phase (KVX_ESINGULAR), as KLU does.
 * KVX_EINVAL: n < 1, malformed colptr/rowind. */
int kvx_lu_analyze(int64_t n, const int64_t *colptr, const int64_t *rowind, const double *values, kvx_lu_sym **out);
/* symbolic(A) of the general LU without block form -- replaces umfpack.c:240-290 (umfpack_*_symbolic): UMFPACK returns
 * P R A Q = L U with no off-diagonal part, so the choice belongs to ONE analysis, never to the process.  flags:
 *   KVX_LU_FLAG_NO_BTF       one block, an empty F and one block level, whatever the matrix and the environment say;
 *   KVX_LU_FLAG_KEEP_VALUES  numeric objects of this analysis refresh their own copy of A's values in kvx_lu_factor_dev /
 *                            kvx_lu_refactor_dev as well (the host entry points always have it): kvx_lu_solve_refine needs A.
 * kvx_lu_analyze is flags = 0 (and still honours the process-wide KVX_LU_NO_BTF=1).  KVX_EINVAL also for unknown flag bits. */
#define KVX_LU_FLAG_NO_BTF 1
#define KVX_LU_FLAG_KEEP_VALUES 2
int kvx_lu_analyze_opts(int64_t n, const int64_t *colptr, const int64_t *rowind, const double *values, int64_t flags, kvx_lu_sym **out);
void kvx_lu_free_symbolic(kvx_lu_sym *S);
/* info: n, nnz, base supernodes, merges learned so far, structurally singular (0/1), nnz(L) bound of the
 * symmetrised pattern, levels, largest base front */
int kvx_lu_sym_info(kvx_lu_sym *S, int64_t info[8]);
int kvx_lu_sym_matching(kvx_lu_sym *S, int64_t *rowfor /* n: row on the diagonal of column j */);
/* block triangular form (KLU's BTF): number of diagonal blocks, number of block levels of the back substitution, and (blk
 * may be NULL) the block of every column j -- row rowfor[j] is in the same block; entries satisfy blk[row] <= blk[col] */
int kvx_lu_sym_btf(kvx_lu_sym *S, int64_t *nblocks, int64_t *nlevels, int64_t *blk);

/* numeric(A, Fs) -- klu.c:310-379 (klu_factor :336).  nnz must equal the analysed pattern's.  The symbolic
 * object is updated when fronts are merged (it must outlive the numeric object).
 * KVX_ESINGULAR -> ArithmeticError("singular matrix") (klu.c:370-371); KVX_EDEVICE: no GPU (never a CPU fallback). */
/* Stream contract of every *_dev entry point of this header (Cholesky, LU, KKT): the library works on its own non-blocking
 * streams; on entry it orders them behind whatever the caller has already submitted to the legacy null stream (torch's
 * default stream, the kvx_nt_* / kvx_atda_* / kvx_spmv_* kernels), so a buffer written by a kernel immediately before the
 * call is read after that kernel.  Synchronous entry points return with their results complete; the *_async_* ones order
 * the null stream behind their own work instead. */
int kvx_lu_factor(kvx_lu_sym *S, int64_t nnz, const double *values, kvx_lu_num **out);
int kvx_lu_factor_dev(kvx_lu_sym *S, int64_t nnz, const double *values_dev, kvx_lu_num **out);
/* numeric with a previous factorisation (doc/source/spsolvers.rst:377-388: "a refactorization is performed"):
 * same pivot sequence, no search; falls back to a full factorisation when a reused pivot is unacceptable. */
int kvx_lu_refactor(kvx_lu_num *N, int64_t nnz, const double *values);
int kvx_lu_refactor_dev(kvx_lu_num *N, int64_t nnz, const double *values_dev);
void kvx_lu_free_numeric(kvx_lu_num *N);
/* info: fronts, levels, largest front order, largest pivot block, panel doubles, arena doubles, numeric passes, factored */
int kvx_lu_num_info(kvx_lu_num *N, int64_t info[8]);
/* Work of one numeric factorisation of the plan (bench.py roofline of the LU path): work[0] = flops (2 per multiply-add: pivot
 * block, the two panels and the rank-k update of every front), [1] = sum over fronts of the L and U panel entries 2 m k - k^2,
 * [2] = sum over fronts of u^2 (update matrices written once and read once by the parent), [3] = fronts with m > the
 * one-workgroup limit (blocked path), [4] = their share of the flops.  Algorithmic bytes of a factorisation:
 * 8 (work[1] + 2 work[2]) + 12 nnz(A). */
int kvx_lu_num_work(kvx_lu_num *N, double work[5]);
/* Launch graphs of the steady state (klu.c:296-308 refactorisation on the recorded pivot sequence, klu.c:651-665 solves on the same
 * buffers): how many times a captured sequence of launches has been replayed by this factor (0: every pass went out launch by
 * launch -- first factorisations always do, and so does a call whose buffers differ from the previous call's: a sequence is
 * captured when the same buffers come twice in a row; KVX_LU_GRAPH=0 turns the graphs off). */
int kvx_lu_num_graph_replays(kvx_lu_num *N, int64_t *replays);

/* solve(A, Fs, Fn, B, trans) -- klu.c:593-690 (klu_solve / klu_tsolve :651-665).  trans: 0 = 'N', 1 = 'T'.
 * B is n x nrhs column-major with leading dimension ldB >= max(1, n), overwritten by the solution. */
int kvx_lu_solve(kvx_lu_num *N, int trans, double *B, int64_t nrhs, int64_t ldB);
int kvx_lu_solve_dev(kvx_lu_num *N, int trans, double *B_dev, int64_t nrhs, int64_t ldB);
/* solve with iterative refinement -- what umfpack.c:582-668 gets from umfpack_*_solve (UMFPACK_IRSTEP = 2).  Per column, with
 * op(A) = A or A':  x = solve(b);  r = b - op(A) x;  omega = max_i |r_i| / (|op(A)| |x| + |b|)_i  (0 / 0 = 0);  then up to `steps`
 * times  d = solve(r), x' = x + d, r', omega':  x' is kept ONLY IF omega' < omega, otherwise x stays and the column stops changing.
 * The residual uses the caller's unscaled values (the factor's own device copy).  All of it runs on the device without a host
 * read between the steps; no floating-point atomics: two calls give the same bytes.  steps >= 0; steps = 0 with berr_out = NULL
 * is kvx_lu_solve itself (the same launches, the same bits).  berr_out: NULL or 2 nrhs doubles in HOST memory (both entry points):
 * berr_out[2 j] = omega of column j before refinement, berr_out[2 j + 1] = omega of the returned column.  nrhs <= 65535. */
int kvx_lu_solve_refine(kvx_lu_num *N, int trans, double *B, int64_t nrhs, int64_t ldB, int64_t steps, double *berr_out);
int kvx_lu_solve_refine_dev(kvx_lu_num *N, int trans, double *B_dev, int64_t nrhs, int64_t ldB, int64_t steps, double *berr_out);

/* get_numeric(A, Fs, Fn) -- klu.c:392-566 (klu_extract :444).  L, U, F come back as malloc'ed CCS triples
 * (free with kvx_free), sorted rows, no explicit zeros; P[k] = row of A that is pivot row k, Q[k] = column of A
 * that is pivot column k, Rs[k] = scale factor of pivot row k (the reference inverts it, klu.c:503-509),
 * r = block boundaries (nblocks + 1 entries). */
int kvx_lu_extract(kvx_lu_num *N, int64_t *lnz, int64_t **Lp, int64_t **Li, double **Lx, int64_t *unz, int64_t **Up,
                   int64_t **Ui, double **Ux, int64_t *fnz, int64_t **Fp, int64_t **Fi, double **Fx, int64_t *P,
                   int64_t *Q, double *Rs, int64_t *nblocks, int64_t **r);

/* get_det(A, Fs, Fn) -- klu.c:707-828: prod(Udiag[k] * Rs[k]) * sign(P) * sign(Q). */
int kvx_lu_det(kvx_lu_num *N, double *det);

#ifdef __cplusplus
}
#endif
#endif
