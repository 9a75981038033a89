// Launchers of admm_polish.hip: what a kept kvx_admm problem needs beyond the iteration (admm.hpp) -- new q, l, u rescaled on the
// device, a warm start, and the polish step of OSQP (Stellato et al. 2020, section 5.2) in its eliminated form on
//     S_pol = P + delta I + A' diag(w) A,   w_i = 1 / delta on the active rows and 0 elsewhere,
// which has the pattern of S and is factored by the same kvx_chol.
#pragma once
#include "admm.hpp"

namespace kvx {
// Entries of the device result of a polish (out[1 + k] of kvx_admm_polish, include/kvxhip.h).
enum { POLISH_NRES = 10 };

// Device view of the polish: the problem (a), the active set and the polished vectors, all in buffers of their own.
struct PolishDev {
    AdmmDev a;
    double *w, *b;          // m: 1 / delta or 0; the bound an active row sits at (0 elsewhere)
    int64_t *act;           // m: -1 lower, +1 upper, 0 inactive
    double *xh, *zh, *yh;   // the polished x (n), z, y (m)
    double *e2, *we2;       // m: e2 and w o e2 of the current pass
    double *rhs;            // n: e1 + A'(w o e2), overwritten by the solve with the correction of x
    double delta;
};

// the number of per-workgroup slots every entry of the result needs in `part` (POLISH_NRES * polish_part_stride doubles)
int64_t polish_part_stride(const AdmmDev &a);

// act, w, b from the ADMM state z, y; the two counts into part
void launch_polish_active(hipStream_t st, const PolishDev &p, double *part);
// one pass of  e2 = b - A xh on active rows;  e1 = -q - (P xh + A' yh);  rhs = e1 + A'(w o e2)   (two launches: e1 needs all of e2)
void launch_polish_residual(hipStream_t st, const PolishDev &p, double *part);
// with rhs = S_pol^-1 rhs:  yh += w o (A rhs - e2),  xh += rhs   (one launch)
void launch_polish_correct(hipStream_t st, const PolishDev &p);
// zh = clip(A xh, l, u), the residuals and objective terms of (xh, zh, yh); then every entry of part reduced into res
void launch_polish_finish(hipStream_t st, const PolishDev &p, double *part, double *res);

// q := (c D) o raw (n entries; c = 1 / a.cinv as given in `c`)
void launch_admm_scale_q(hipStream_t st, const AdmmDev &a, double c, const double *raw, double *q);
// l := E o raw, -1e30 where raw <= -1e26 (upper = false);  u := E o raw, 1e30 where raw >= 1e26 (upper = true)
void launch_admm_scale_bound(hipStream_t st, const AdmmDev &a, bool upper, const double *raw, double *out);
// x := D^-1 raw, then z := A x by rows
void launch_admm_warm_x(hipStream_t st, const AdmmDev &a, const double *raw);
// y := (c E^-1) o raw
void launch_admm_warm_y(hipStream_t st, const AdmmDev &a, double c, const double *raw);
}  // namespace kvx
