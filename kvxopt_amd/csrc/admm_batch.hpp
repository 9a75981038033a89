// Launchers of admm_batch.hip: the ADMM iteration of admm.hip for B data sets (q_b, l_b, u_b) on one scaled A, P, rho and one
// kept factor (kvx_admm_batch_*, admm_batch_api.cpp; DESIGN section 11, "A batch on the kept factor").
#pragma once
#include "admm.hpp"

namespace kvx {
// Members a group carries through one pass over the (index, value) stream of a row or column: the iteration kernels, the
// residual kernel (which holds four sums per member and column).
enum { ADMM_STRIP = 8, ADMM_RSTRIP = 4 };

// Device view of a batch: the state and the data are column-major, n x B (q, x, dx, xt; ld = n) or m x B (l, u, z, y, dy;
// ld = m), member b in column b.  run[b] != 0: member b is iterated; a member whose flag is 0 is frozen -- no kernel writes
// its x, z, y, dx, dy or its residual numbers.  A, P, rho, the scaling and the constants are those of the kept problem `a`.
struct AdmmBatchDev {
    AdmmDev a;
    int64_t B;
    double *q, *l, *u, *x, *z, *y, *dx, *dy, *xt;
    const int *run;
};

// q_b := (c D) o raw_b;  l_b, u_b := E o raw_b, +-INFTY where |raw| >= 1e26.  raw == nullptr: the kept problem's scaled
// vector in every column.
void launch_admm_batch_scale_q(hipStream_t st, const AdmmBatchDev &b, double c, const double *raw);
void launch_admm_batch_scale_bound(hipStream_t st, const AdmmBatchDev &b, bool upper, const double *raw);
// the three steps of admm.hpp for every running member; the right-hand side of a frozen member is zero
void launch_admm_batch_rhs(hipStream_t st, const AdmmBatchDev &b);
void launch_admm_batch_update(hipStream_t st, const AdmmBatchDev &b);
// part: B * ADMM_NRES * admm_residual_blocks(b.a) doubles; res: B x ADMM_NRES, member b in res[b * ADMM_NRES ...]
void launch_admm_batch_residuals(hipStream_t st, const AdmmBatchDev &b, double *part, double *res);
}  // namespace kvx
