// Launchers of kkt_cone.hip: assembly of S = Gs' Gs for 'l', 'q' and 's' blocks (cone_api.cpp) and the small vector helpers
// of the general-cone interior-point driver.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace kvx {
// dst[i] = src[idx[i]]
void launch_cone_gather(hipStream_t st, int64_t n, const int64_t *idx, const double *src, double *dst);
// dst[idx[i]] = src[i]   (destinations distinct)
void launch_cone_scatter(hipStream_t st, int64_t n, const int64_t *idx, const double *src, double *dst);
// dst[didx[i] - doff] = src[sidx[i]]   (destinations distinct)
void launch_cone_move(hipStream_t st, int64_t n, const int64_t *sidx, const double *src, const int64_t *didx, int64_t doff, double *dst);
// row weights of the 'l' and 'q' rows: w[r] = di[r]^2 (r < ml), 1 / beta_k^2 for the rows of cone k (rcone[r - ml] = k)
void launch_cone_weights(hipStream_t st, int64_t ml, int64_t mq, const int32_t *rcone, const double *di, const double *beta, double *w);
// per cone k: nv2[k] = v_k' v_k (in order)
void launch_cone_vnorm(hipStream_t st, int64_t nq, const int64_t *qoff, const double *v, double *nv2);
// per (cone, clique column) pair t: p[t] = sum G(r, j) (J v)_r, q[t] = sum G(r, j) v_r over the cone's rows of column j
void launch_cone_pq(hipStream_t st, int64_t npairs, const int64_t *ptr, const int64_t *pos, const int64_t *vrow, const int32_t *vhead,
                    const double *Gx, const double *v, double *p, double *q);
// lower triangle of C_b = Y_b' Y_b for every 's' block b, 16 x 16 tiles (FP64 MFMA), one wave per tile
void launch_cone_gram(hipStream_t st, int64_t ntiles, const int32_t *tblk, const int32_t *ti, const int32_t *tj, const int64_t *yoff,
                      const int64_t *mp, const int64_t *ncol, const int64_t *goff, const double *Y, double *C);
// Px[e] = sum over the 'q' items of entry e of (4 |v_k|^2 p_a p_b - 2 (p_a q_b + q_a p_b)) / beta_k^2 + sum of its 's' Gram entries
// (+ Hx[hidx[e]] last when hidx is given and hidx[e] >= 0; hidx == NULL: no H, the operations of the plain assembly)
void launch_cone_pgather(hipStream_t st, int64_t pnz, const int64_t *qptr, const int32_t *qk, const int64_t *qa, const int64_t *qb,
                         const double *p, const double *q, const double *nv2, const double *beta, const int64_t *sptr,
                         const int64_t *sidx, const double *C, const int64_t *hidx, const double *Hx, double *Px);
// x_k(i, j) *= sqrt(w_j) for every 's' block (lower and upper triangle)
void launch_nts_colscale(hipStream_t st, int64_t ns, const int64_t *off2, const int64_t *off1, double *x, const double *w);
}  // namespace kvx
