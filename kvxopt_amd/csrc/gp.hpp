// Launchers of gp.hip: the log-sum-exp blocks of a geometric program (gp_api.cpp), f_i(x) = log sum_k exp(F_i x + g_i)_k with
// its gradients and the dense centred factors of its Hessians (cvxprog.py:2102-2153).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace kvx {
// Size classes of the blocks (by their number of terms K): a 16-lane group, a wavefront or a 256-thread workgroup per block.
enum { GP_SMALL_MAX = 16, GP_WAVE_MAX = 256 };
// Segments (the entries of one block in one column of F) longer than this are summed by a wavefront, shorter ones by a thread.
enum { GP_SEG_WAVE = 64 };

// For every block b of list (nb of them): y = F x + g on its rows (rows in CSR form: rp, ci, src = position of the value in Fx),
// m = max y, y := exp(y - m), s = sum y, f[b] = m + log s, y := y / s.  cls 0: 16 lanes, 1: a wavefront, 2: a workgroup per block.
void launch_gp_lse(hipStream_t st, int cls, int64_t nb, const int64_t *list, const int64_t *boff, const int64_t *rp, const int64_t *ci,
                   const int64_t *src, const double *Fx, const double *g, const double *x, double *y, double *f);
// Dfx[e] = sum over segment e of Fx[pos[p]] * y[row[p]], p in [seg[e], seg[e + 1]) in order; list: the entries of this class
// (wave = 0: a thread per entry, 1: a wavefront per entry)
void launch_gp_grad(hipStream_t st, int wave, int64_t ne, const int64_t *list, const int64_t *seg, const int64_t *pos, const int64_t *row,
                    const double *Fx, const double *y, double *Dfx);
// D (the dense K_b x c_b factors, column-major at foff[b]) := -Df(b, a) sqrt(y_r) for every element ...
void launch_gp_fsc_fill(hipStream_t st, int64_t dtot, int64_t nblk, const int64_t *foff, const int64_t *boff, const int64_t *coff,
                        const int64_t *dpos, const double *Dfx, const double *y, double *D);
// ... and := (F(r, j) - Df(b, a)) sqrt(y_r) where F has an entry: dd[p] its place in D, dfe[p] the entry of Df of its segment
void launch_gp_fsc_nz(hipStream_t st, int64_t nnz, const int64_t *pos, const int64_t *row, const int64_t *dd, const int64_t *dfe,
                      const double *Fx, const double *Dfx, const double *y, double *D);
// Hx[e] = sum over the items u of entry e, in order, of z[hblk[u]] * C[hidx[u]]
void launch_gp_hgather(hipStream_t st, int64_t hnz, const int64_t *hptr, const int32_t *hblk, const int64_t *hidx, const double *z,
                       const double *C, double *Hx);
}  // namespace kvx
