// The handle behind kvx_admm_* and what its three host files share: admm_plan.cpp (the host-only plan), admm_api.cpp (set-up,
// iteration, the kept problem, the polish) and admm_batch_api.cpp (a batch on the kept factor).
#pragma once
#include "../../include/kvxhip.h"
#include "abi_guard.hpp"
#include "admm.hpp"
#include "admm_batch.hpp"
#include "admm_polish.hpp"
#include "devpool.hpp"

#include <algorithm>
#include <string>
#include <vector>

#define HIPCHK(call)                                                             \
    do {                                                                         \
        hipError_t e_ = (call);                                                  \
        if (e_ != hipSuccess) return KVX_EDEVICE;                                \
    } while (0)

struct kvx_admm {
    int64_t m = 0, n = 0, snz = 0, nfact = 0, niter = 0;
    std::vector<int64_t> Ap, Ai, Tp, Ti, Lp, Li, Fp, Fi, rs, rl, Sp, Si;
    std::vector<double> Ax, Tx, Lx, Fx, q, l, u, D, Dinv, E, Einv, rho;
    double c = 1.0, sigma = 0.0, alpha = 0.0, rho0 = 0.0;
    kvx_atda *plan = nullptr;
    kvx_chol *F = nullptr;
    bool dev = false;
    kvx::AdmmDev d{};
    double *d_Lxs = nullptr, *d_Sx = nullptr, *d_part = nullptr, *d_res = nullptr;
    std::vector<void *> owned;
    // the kept problem (admm_polish.hip): staging for raw q | x (n), l | y (m), u (m); the polish buffers, allocated at first use
    bool stale = false;                 // the kept numeric factor is that of S_pol, not of S
    bool polished = false;              // xh, zh, yh hold the result of a polish that factored
    kvx::PolishDev p{};
    double *d_stage = nullptr, *d_ppart = nullptr, *d_pres = nullptr, *d_Lxd = nullptr;
    double lxd_delta = 0.0;
    // a batch on the kept factor (admm_batch.hip): B members, every buffer from kvx_admm_batch_begin is in `bowned` alone
    kvx::AdmmBatchDev b{};
    std::vector<void *> bowned;
    double *d_bpart = nullptr, *d_bres = nullptr;
};

namespace kvx {
constexpr double OSQP_INFTY = 1e30, MIN_SCALING = 1e-4, MAX_SCALING = 1e4;
constexpr double RHO_MIN = 1e-6, RHO_MAX = 1e6, RHO_TOL = 1e-4, RHO_EQ_OVER_RHO_INEQ = 1e3;

// l or u of the scaled problem from the raw bound v and the row scaling E
inline double scaled_bound(double v, double E, bool upper)
{
    if (upper) return v >= OSQP_INFTY * MIN_SCALING ? OSQP_INFTY : E * v;
    return v <= -OSQP_INFTY * MIN_SCALING ? -OSQP_INFTY : E * v;
}

// "<who>: l <= u does not hold<where>" unless it holds
inline int check_row(const char *who, double l, double u, const std::string &where = std::string())
{
    if (l <= u) return KVX_OK;
    set_last_error(std::string(who) + ": l <= u does not hold" + where);
    return KVX_EINVAL;
}

// the three classes of the rho vector on scaled bounds: 0 without a finite bound, 1 equality, 2 the others
inline int rho_class(double l, double u)
{
    if (l <= -OSQP_INFTY * MIN_SCALING && u >= OSQP_INFTY * MIN_SCALING) return 0;
    return u - l < RHO_TOL ? 1 : 2;
}

// rho_i = 1e-6 in class 0, 1e3 rho in class 1, rho in class 2 (admm_plan.cpp)
void admm_rho_vector(const kvx_admm *S, double rho, double *out);

// count (at least one) zeroed T on the device, owned by `owner`
template <class T>
int zeros(std::vector<void *> &owner, T **dst, int64_t count)
{
    const size_t bytes = (size_t)std::max<int64_t>(count, 1) * sizeof(T);
    HIPCHK(pool_malloc((void **)dst, bytes));
    owner.push_back(*dst);
    HIPCHK(hipMemset(*dst, 0, bytes));
    return KVX_OK;
}

inline int fetch(double *dst, const double *src_dev, int64_t count)
{
    if (dst && count > 0) HIPCHK(hipMemcpy(dst, src_dev, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
    return KVX_OK;
}

// admm_api.cpp: KVX_OK when a HIP device is there and kvx_admm_setup_dev has run, with the message of `who` otherwise
int admm_need_setup(const kvx_admm *S, const char *who);
// admm_api.cpp: S at the current rho again when a polish took the factor over
int admm_restore_factor(kvx_admm *S);
// admm_batch_api.cpp: frees the buffers of a batch
int admm_batch_end(kvx_admm *S);

// x = D o src (n entries);  y = E o v / c (m entries), v = src, or with the scaled bounds l, u given the part of src that does
// not push against an infinite bound (the certificate of primal infeasibility).  In place is fine.
inline void admm_unscale_x(const kvx_admm *S, const double *src, double *x)
{
    for (int64_t j = 0; j < S->n; j++) x[j] = src[j] * S->D[j];
}

inline void admm_unscale_y(const kvx_admm *S, const double *src, const double *l, const double *u, double *y)
{
    const double cinv = 1.0 / S->c;
    for (int64_t i = 0; i < S->m; i++) {
        double v = src[i];
        if (l) {
            const bool ui = u[i] >= OSQP_INFTY * MIN_SCALING, li = l[i] <= -OSQP_INFTY * MIN_SCALING;
            v = ui && li ? 0.0 : (ui ? std::min(v, 0.0) : (li ? std::max(v, 0.0) : v));
        }
        y[i] = S->E[i] * v * cinv;
    }
}
}  // namespace kvx
