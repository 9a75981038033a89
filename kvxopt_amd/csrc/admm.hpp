// Launchers of admm.hip: the ADMM iteration of kvxopt.osqp (admm_api.cpp) on the scaled problem
//     minimise 1/2 x'Px + q'x  subject to  l <= Ax <= u,      S = P + sigma I + A' diag(rho) A  factored once.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace kvx {
// Rows of A with fewer entries than this are summed by a 16-lane group, the others (a full wavefront's worth) by a wavefront.
enum { ADMM_ROW_WAVE = 64 };
// Entries of the result vector of launch_admm_residuals (include/kvxhip.h, kvx_admm_iterate).
enum { ADMM_NRES = 24 };

// Device view of one problem: every pointer is a device pointer.  A by columns (Ap, Ai, Ax) and by rows (Tp, Ti, Tx: the CCS
// arrays of A'); the full symmetric P by columns (Fp, Fi, Fx); rs / rl: the rows of the two length classes.
struct AdmmDev {
    int64_t m, n, ns, nl;
    const int64_t *Ap, *Ai; const double *Ax;
    const int64_t *Tp, *Ti; const double *Tx;
    const int64_t *Fp, *Fi; const double *Fx;
    const int64_t *rs, *rl;
    const double *q, *l, *u, *D, *Dinv, *E, *Einv, *rho;
    double *x, *z, *y, *dx, *dy, *xt;
    double sigma, alpha, cinv;
};

// xt_j := sigma x_j - q_j + sum_i A_ij (rho_i z_i - y_i)
void launch_admm_rhs(hipStream_t st, const AdmmDev &a);
// with xt = S^-1 rhs: zt = A xt, v = alpha zt + (1 - alpha) z, z+ = clip(v + y / rho, l, u), y+ = y + rho (v - z+), dy = y+ - y;
// x+ = alpha xt + (1 - alpha) x, dx = x+ - x -- one launch
void launch_admm_update(hipStream_t st, const AdmmDev &a);
// part: ADMM_NRES * admm_residual_blocks(a) doubles; res: ADMM_NRES doubles (two launches: per-workgroup results, then one
// wavefront per entry of res)
int64_t admm_residual_blocks(const AdmmDev &a);
void launch_admm_residuals(hipStream_t st, const AdmmDev &a, double *part, double *res);
}  // namespace kvx
