"""`kvxopt.osqp` on the GPU (src/C/osqp.c): quadratic programs by ADMM on one kept Cholesky factor.

    solve(q, A, l, u, P=None, options=None) -> (status, x, y)        minimise 1/2 x'Px + q'x  s.t.  l <= Ax <= u    osqp.c:374-432
    qp(q, G, h, A=None, b=None, P=None, options=None) -> (status, x, z, y)         ... s.t. Gx <= h, Ax = b        osqp.c:442-572
    options                                                          the module-level dict of the reference
    Problem(q, A, l, u, P=None, options=None)                        the same problem kept on the device (not in the reference):
        .update(q, l, u)  .warm_start(x, y)  .solve() -> (status, x, y)  .info  .close()
        .solve_batch(Q, L=None, U=None, chunk=1024) -> (statuses, X, Y)  .batch_info     B data sets on the kept factor

The reference binds the external OSQP library; here the published algorithm (Stellato et al. 2020) runs in HBM through the
kvx_admm_* entry points of include/kvxhip.h: the plan equilibrates the data on the host, S = P + sigma I + A' diag(rho) A is
assembled on a fixed pattern and factored once (again only when rho adapts), and an iteration is two short kernels around one
triangular solve; a termination check reads 24 doubles.  DESIGN section 11 fixes every rule (scaling, rho classes, termination,
certificates, adaptive rho).  The answers follow the algorithm, not libosqp bit for bit.

A, G, P are sparse 'd' matrices (ours or kvxopt's), q, l, u, h, b dense 'd' vectors; of P the lower triangle is read.  Results are
numpy arrays, as everywhere in this package.  For a status other than solved / infeasible, x and y are zero vectors, as the
reference's freshly allocated matrices are.  In solve and qp 'linsys_solver', 'time_limit', 'delta', 'polish_refine_iter',
'adaptive_rho_fraction' and 'warm_start' are accepted without effect (every call starts from zero) and 'polish' raises.

A Problem plans, analyses and factors once and stays in HBM: update() replaces q, l, u (rescaled with the kept scaling; one
numeric refactorisation only when a row changes its rho class), every solve() continues from the state the last one left
(warm_start = 0: from zero), rho persists, and 'polish', 'delta', 'polish_refine_iter' take effect: after 'solved' the active
set is guessed, one equality-constrained QP is solved on the analysed pattern and refined, and the result is taken when its
residuals are smaller ("A kept problem").

solve_batch() runs B data sets (q_b, l_b, u_b), the columns of Q, L, U, through the kept factor at the problem's current rho: every
member starts from zero, one triangular solve with B right-hand sides per iteration, one host read per termination check for the
whole batch, a member stops at its own check.  No rho adapts, nothing is polished, the kept problem is left as it was (DESIGN
section 11, "A batch on the kept factor").
"""
import ctypes
import math
import warnings

import numpy as np

from . import _lib
from . import base as _base
from ._lib import pd, pi

options = {}

INFTY = 1e30
_NEG_MAX = -1.7976931348623157e308

_INT_OPTS = ("scaling", "adaptive_rho", "adaptive_rho_interval", "max_iter", "linsys_solver", "polish", "polish_refine_iter", "verbose",
             "scaled_termination", "check_termination", "warm_start")
_FLOAT_OPTS = ("adaptive_rho_tolerance", "adaptive_rho_fraction", "rho", "sigma", "eps_abs", "eps_rel", "eps_prim_inf", "eps_dual_inf",
               "alpha", "delta", "time_limit")
_DEFAULTS = {"scaling": 10, "adaptive_rho": 1, "adaptive_rho_interval": 0, "adaptive_rho_tolerance": 5.0, "adaptive_rho_fraction": 0.4,
             "rho": 0.1, "sigma": 1e-6, "max_iter": 4000, "eps_abs": 1e-3, "eps_rel": 1e-3, "eps_prim_inf": 1e-4, "eps_dual_inf": 1e-4,
             "alpha": 1.6, "delta": 1e-6, "linsys_solver": 0, "polish": 0, "polish_refine_iter": 3, "verbose": 1, "scaled_termination": 0,
             "check_termination": 25, "warm_start": 1, "time_limit": 0.0}


def _read_options(opts, stacklevel):
    """The defaults overridden by `opts` (osqp.c:225-269); a warning for an unknown key is attributed `stacklevel` frames up."""
    if not isinstance(opts, dict):
        opts = options
    if not isinstance(opts, dict):
        raise AttributeError("missing osqp.options dictionary")
    o = dict(_DEFAULTS)
    for key, value in opts.items():
        if not isinstance(key, str):
            continue
        if key in _INT_OPTS:
            o[key] = int(value)
        elif key in _FLOAT_OPTS:
            o[key] = float(value)
        else:
            warnings.warn("Invalid parameter name: " + key, RuntimeWarning, stacklevel=stacklevel)
    return o


def _settings(opts):
    """The settings of one call of solve / qp: these return the ADMM iterates as they are."""
    o = _read_options(opts, 5)
    if o["polish"]:
        raise NotImplementedError("kvxopt_amd.osqp: 'polish' is not built into solve and qp (the ADMM iterates are returned as they are); "
                                  "osqp.Problem polishes")
    return o


def _is_sparse_d(A):
    if isinstance(A, _base.spmatrix):
        return A.typecode == "d"
    return hasattr(A, "CCS") and getattr(A, "typecode", None) == "d"


def _dense(v, name, ndims, rows, cols):
    """The entries of a dense 'd' matrix, or of a float64 array with ndim in `ndims`, of `rows` x `cols` entries (cols None: any)
    as a flat column-major float64 array, and its size (the checks of osqp.c:393-409)."""
    if isinstance(v, _base.matrix) or (hasattr(v, "typecode") and hasattr(v, "size") and not hasattr(v, "CCS")):
        if v.typecode != "d":
            raise TypeError("%s must be a matrix with typecode 'd'" % name)
        size = tuple(v.size)
    elif isinstance(v, np.ndarray) and v.dtype == np.float64 and v.ndim in ndims:
        size = (v.shape[0], 1 if v.ndim == 1 else v.shape[1])
    else:
        raise TypeError("%s must be a matrix with typecode 'd'" % name)
    if size[0] != rows or (cols is not None and size[1] != cols):
        raise ValueError("incompatible dimensions")
    return _base.flat(v).copy(), size


def _vector(v, name, rows):
    """A dense 'd' vector of `rows` entries as a float64 array."""
    return _dense(v, name, (1, 2), rows, 1)[0]


def _matrix2(v, name, rows, cols=None):
    """A dense 'd' matrix of `rows` x `cols` entries (cols None: any) as a column-major float64 array, with the checks and texts
    of _vector."""
    flat, size = _dense(v, name, (2,), rows, cols)
    return flat.reshape((int(size[0]), int(size[1])), order="F")


def _rho_classes(lb, ub):
    """On scaled bounds: 0 without a finite bound, 1 equality (u - l < 1e-4), 2 the others (the rho vector)."""
    free = (lb <= -INFTY * 1e-4) & (ub >= INFTY * 1e-4)
    return np.where(free, 0, np.where(ub - lb < 1e-4, 1, 2))


def _check_batch(Q, L, U, n, m, E, l, u):
    """The arguments of Problem.solve_batch on the host: (Q, L, U) as column-major float64 arrays n x B, m x B (None stays None).
    E: the row scaling of the kept problem, l, u: its current unscaled bounds.  Every member must have l <= u and give every
    row the rho class it has in the kept problem; ValueError names the first (member, row)."""
    Q = _matrix2(Q, "Q", n)
    B = Q.shape[1]
    if B < 1:
        raise ValueError("incompatible dimensions")
    L = None if L is None else _matrix2(L, "L", m, B)
    U = None if U is None else _matrix2(U, "U", m, B)
    if L is None and U is None:
        return Q, L, U
    E = np.asarray(E, dtype=np.float64)
    scale = lambda raw, sign: np.where(sign * raw >= INFTY * 1e-4, sign * INFTY, (E * raw.T).T)
    kl, ku = scale(np.asarray(l, dtype=np.float64), -1.0), scale(np.asarray(u, dtype=np.float64), 1.0)
    lb = kl[:, None] if L is None else scale(L, -1.0)
    ub = ku[:, None] if U is None else scale(U, 1.0)
    lb, ub = np.broadcast_to(lb, (m, B)), np.broadcast_to(ub, (m, B))
    bad = ~(lb <= ub)
    if bad.any():
        b, i = min(zip(*np.nonzero(bad.T)))
        raise ValueError("l <= u does not hold in member %d, row %d" % (b, i))
    moved = _rho_classes(lb, ub) != _rho_classes(kl, ku)[:, None]
    if moved.any():
        b, i = min(zip(*np.nonzero(moved.T)))
        raise ValueError("member %d, row %d is not in the rho class (equality, free, other) the row has in the kept problem; "
                         "update() the problem to bounds of that shape first" % (b, i))
    return Q, L, U


class _Solver:
    """One problem on the device: the handle of kvx_admm_plan / kvx_admm_setup_dev.  D, E, c are the plan's scaling."""

    def __init__(self, q, Acc, l, u, Pcc=None, scaling=10):
        m, n, Ap, Ai, Ax = Acc
        self.m, self.n = int(m), int(n)
        self._h = None
        L = _lib.lib()
        q, l, u = _lib.as_f64(q), _lib.as_f64(l), _lib.as_f64(u)
        Ap, Ai, Ax = _lib.as_i64(Ap), _lib.as_i64(Ai), _lib.as_f64(Ax)
        self.D, self.E = np.empty(self.n), np.empty(self.m)
        c, snz, h = ctypes.c_double(), ctypes.c_int64(), ctypes.c_void_p()
        if Pcc is None:
            Pa = (None, None, None)
        else:
            keep = [_lib.as_i64(Pcc[0]), _lib.as_i64(Pcc[1]), _lib.as_f64(Pcc[2])]
            Pa = (pi(keep[0]), pi(keep[1]), pd(keep[2]))
        _lib.raise_for(L.kvx_admm_plan(self.m, self.n, pi(Ap), pi(Ai), pd(Ax), Pa[0], Pa[1], Pa[2], pd(q), pd(l), pd(u), int(scaling),
                                       pd(self.D), pd(self.E), ctypes.byref(c), ctypes.byref(snz), ctypes.byref(h)), "kvx_admm_plan")
        self._h, self.c, self.snz = h, c.value, snz.value
        self.rho = None
        self.last_res = None
        self._B = 0                                                     # members of the batch that has begun

    def pattern(self):
        Sp, Si = np.empty(self.n + 1, dtype=np.int64), np.empty(self.snz, dtype=np.int64)
        _lib.raise_for(_lib.lib().kvx_admm_pattern(self._h, None, pi(Sp), pi(Si)))
        return Sp, Si

    def rho_vector(self, rho):
        out = np.empty(self.m)
        _lib.raise_for(_lib.lib().kvx_admm_rho_vector(self._h, float(rho), pd(out)))
        return out

    def setup(self, sigma=1e-6, rho=0.1, alpha=1.6):
        rc = _lib.lib().kvx_admm_setup_dev(self._h, float(sigma), float(rho), float(alpha))
        if rc == _lib.KVX_ENOTPOSDEF:
            raise ArithmeticError(_lib.last_error() or "the problem is not convex")
        _lib.raise_for(rc, "kvx_admm_setup_dev")
        self.rho = min(max(float(rho), 1e-6), 1e6)
        return self

    def iterate(self, k):
        """k iterations without a host synchronisation, then the 24 residual numbers of kvx_admm_iterate."""
        out = np.empty(24)
        _lib.raise_for(_lib.lib().kvx_admm_iterate(self._h, int(k), pd(out)), "kvx_admm_iterate")
        self.last_res = out
        return out

    def set_rho(self, rho):
        _lib.raise_for(_lib.lib().kvx_admm_set_rho(self._h, float(rho)), "kvx_admm_set_rho")
        self.rho = min(max(float(rho), 1e-6), 1e6)

    def state(self):
        """The scaled x, z, y, dx, dy."""
        x, z, y, dx, dy = np.empty(self.n), np.empty(self.m), np.empty(self.m), np.empty(self.n), np.empty(self.m)
        _lib.raise_for(_lib.lib().kvx_admm_state(self._h, pd(x), pd(z), pd(y), pd(dx), pd(dy)), "kvx_admm_state")
        return x, z, y, dx, dy

    def update(self, q=None, l=None, u=None):
        """New unscaled q, l, u (None: kept), rescaled on the device with the kept D, E, c."""
        keep = [None if v is None else _lib.as_f64(v) for v in (q, l, u)]
        rc = _lib.lib().kvx_admm_update(self._h, *(None if v is None else pd(v) for v in keep))
        if rc == _lib.KVX_ENOTPOSDEF:
            raise ArithmeticError(_lib.last_error() or "the problem is not convex")
        _lib.raise_for(rc, "kvx_admm_update")

    def warm_start(self, x=None, y=None):
        """The state from unscaled x (then z = Ax) and y (None: kept); dx = dy = 0."""
        keep = [None if v is None else _lib.as_f64(v) for v in (x, y)]
        _lib.raise_for(_lib.lib().kvx_admm_warm_start(self._h, *(None if v is None else pd(v) for v in keep)), "kvx_admm_warm_start")

    def cold_start(self):
        _lib.raise_for(_lib.lib().kvx_admm_cold_start(self._h), "kvx_admm_cold_start")

    def polish(self, delta=1e-6, refine_iter=3):
        """The 16 numbers of kvx_admm_polish; out[0] = -1: S_pol did not factor."""
        out = np.empty(16)
        _lib.raise_for(_lib.lib().kvx_admm_polish(self._h, float(delta), int(refine_iter), pd(out)), "kvx_admm_polish")
        return out

    def polish_state(self):
        """The scaled polished x, z, y and the flags -1 (active at l) / 0 / +1 (active at u)."""
        x, z, y, act = np.empty(self.n), np.empty(self.m), np.empty(self.m), np.empty(self.m, dtype=np.int64)
        _lib.raise_for(_lib.lib().kvx_admm_polish_state(self._h, pd(x), pd(z), pd(y), pi(act)), "kvx_admm_polish_state")
        return x, z, y, act

    def polish_accept(self):
        _lib.raise_for(_lib.lib().kvx_admm_polish_accept(self._h), "kvx_admm_polish_accept")

    def solution(self, kind=0):
        """kind 0: the unscaled (x, y); 1: the certificate of primal infeasibility as y; 2: of dual infeasibility as x; 3: the
        polished (x, y)."""
        x, y = np.zeros(self.n), np.zeros(self.m)
        _lib.raise_for(_lib.lib().kvx_admm_solution(self._h, int(kind), pd(x) if kind != 1 else None, pd(y) if kind != 2 else None),
                       "kvx_admm_solution")
        return x, y

    # ---- a batch on the kept factor: column-major n x B, m x B ---------------------------------------------------------------
    def batch_begin(self, Q, L=None, U=None):
        """B = Q.shape[1] members from unscaled Q, L, U (None: the kept vector in every column), every state zero."""
        keep = [None if v is None else np.asfortranarray(v, dtype=np.float64) for v in (Q, L, U)]
        self._B = int(keep[0].shape[1])
        _lib.raise_for(_lib.lib().kvx_admm_batch_begin(self._h, self._B, *(None if v is None else pd(v) for v in keep)), "kvx_admm_batch_begin")

    def batch_iterate(self, k, running):
        """k iterations of the members with running[b] != 0, then the B x 24 residual numbers (frozen members: their last)."""
        run = np.ascontiguousarray(running, dtype=np.int64)
        out = np.empty((self._B, 24))
        _lib.raise_for(_lib.lib().kvx_admm_batch_iterate(self._h, int(k), pi(run), pd(out)), "kvx_admm_batch_iterate")
        return out

    def batch_state(self):
        """The scaled x (n x B), z, y (m x B), dx, dy."""
        B = self._B
        out = [np.empty((r, B), order="F") for r in (self.n, self.m, self.m, self.n, self.m)]
        _lib.raise_for(_lib.lib().kvx_admm_batch_state(self._h, *(pd(v) for v in out)), "kvx_admm_batch_state")
        return tuple(out)

    def batch_solution(self, kinds):
        """Per member the unscaled (x, y) of solution(kind); kind -1: zeros."""
        kinds = np.ascontiguousarray(kinds, dtype=np.int64)
        X, Y = np.empty((self.n, self._B), order="F"), np.empty((self.m, self._B), order="F")
        _lib.raise_for(_lib.lib().kvx_admm_batch_solution(self._h, pi(kinds), pd(X), pd(Y)), "kvx_admm_batch_solution")
        return X, Y

    def batch_end(self):
        _lib.raise_for(_lib.lib().kvx_admm_batch_end(self._h), "kvx_admm_batch_end")

    def info(self):
        out = np.zeros(8, dtype=np.int64)
        _lib.raise_for(_lib.lib().kvx_admm_info(self._h, pi(out)))
        return dict(zip(("m", "n", "snz", "factorisations", "iterations", "short_rows", "long_rows", "on_device"), (int(v) for v in out)))

    def close(self):
        if self._h is not None:
            _lib.lib().kvx_admm_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _measure(o):
    """Where the seven residual numbers of the measure 'scaled_termination' selects begin in the 24 (or B x 24) numbers."""
    return 0 if o["scaled_termination"] else 7


def _pri_dua(res, o):
    """The primal and the dual residual of `res` (24 numbers, or B x 24: then per member)."""
    return res.T[_measure(o)], res.T[_measure(o) + 3]


def _objective(res, c):
    """The unscaled objective of `res` (24 numbers, or B x 24: then per member); c: the plan's cost scaling."""
    return (0.5 * res.T[22] + res.T[23]) / c


def _kind(status):
    """What _Solver.solution returns for `status`: 0 the solution, 1 / 2 the certificate of primal / dual infeasibility, None zeros."""
    for kind, text in enumerate(("solved", "primal infeasible", "dual infeasible")):
        if status.startswith(text):
            return kind
    return None


def _judge(res, o, mult):
    """The status the residual vector `res` gives at tolerances times `mult`, or None (termination, certificates)."""
    ea, er, epi, edi = o["eps_abs"] * mult, o["eps_rel"] * mult, o["eps_prim_inf"] * mult, o["eps_dual_inf"] * mult
    b = _measure(o)
    prim = res[b] <= ea + er * max(res[b + 1], res[b + 2])
    dual = res[b + 3] <= ea + er * max(res[b + 4], res[b + 5], res[b + 6])
    if prim and dual:
        return "solved"
    ndy, ndx = res[14], res[17]
    if not prim and ndy > epi and res[15] < -epi * ndy and res[16] < epi * ndy:
        return "primal infeasible"
    if not dual and ndx > edi and res[18] < -edi * ndx and res[19] < edi * ndx and res[20] <= edi * ndx and res[21] <= edi * ndx:
        return "dual infeasible"
    return None


def _new_rho(res, rho):
    """The rho the scaled residuals ask for (adaptive rho)."""
    pr = res[0] / (max(res[1], res[2]) + 1e-10)
    du = res[3] / (max(res[4], res[5], res[6]) + 1e-10)
    return min(max(rho * math.sqrt(pr / (du + 1e-10)), 1e-6), 1e6)


def _next_stop(it, o, interval):
    """The iteration count of the host read after `it`: the next multiple of 'check_termination' or of `interval` (each when
    not 0), 'max_iter' at the latest."""
    nxt, check = o["max_iter"], o["check_termination"]
    if check > 0:
        nxt = min(nxt, (it // check + 1) * check)
    if interval:
        nxt = min(nxt, (it // interval + 1) * interval)
    return nxt


def _verdict(res, o, checked, it):
    """The status `res` gives after `it` iterations, or None to go on.  checked: `it` is a termination check; at 'max_iter' the
    tolerances times 10 decide between '... inaccurate' and 'maximum iterations reached'."""
    status = _judge(res, o, 1.0) if checked else None
    if status is None and it >= o["max_iter"]:
        status = _judge(res, o, 10.0)
        status = status + " inaccurate" if status else "maximum iterations reached"
    return status


def _run(S, o):
    """The ADMM loop on a solver that is set up: (status, iterations).  One host read per check."""
    check = o["check_termination"]
    adaptive = bool(o["adaptive_rho"])
    interval = (o["adaptive_rho_interval"] or 100) if adaptive else 0
    it = 0
    if o["verbose"]:
        print("iter   objective    pri res    dua res    rho")
    while True:
        nxt = _next_stop(it, o, interval)
        res = S.iterate(max(nxt - it, 0))
        it = max(nxt, it)
        checked = check > 0 and it % check == 0
        if checked or it >= o["max_iter"]:
            if o["verbose"]:
                print("%4d %12.4e  %9.2e  %9.2e  %8.2e" % ((it, _objective(res, S.c)) + _pri_dua(res, o) + (S.rho,)))
            status = _verdict(res, o, checked, it)
            if status is not None:
                return status, it
        if adaptive and it % interval == 0:
            rho = _new_rho(res, S.rho)
            if rho > o["adaptive_rho_tolerance"] * S.rho or rho < S.rho / o["adaptive_rho_tolerance"]:
                S.set_rho(rho)


def _run_batch(S, o, B):
    """The loop of _run without adaptive rho on a batch that has begun: (statuses, iterations, the B x 24 numbers of every
    member's last check).  A member that gets a status is frozen; the loop ends when no member runs."""
    check = o["check_termination"]
    running = np.ones(B, dtype=np.int64)
    statuses, its, last = [None] * B, np.zeros(B, dtype=np.int64), np.empty((B, 24))
    it = 0
    while running.any():
        nxt = _next_stop(it, o, 0)
        res = S.batch_iterate(max(nxt - it, 0), running)
        it = max(nxt, it)
        checked = check > 0 and it % check == 0
        for b in np.nonzero(running)[0]:
            status = _verdict(res[b], o, checked, it)
            if status is not None:
                statuses[b], its[b], last[b], running[b] = status, it, res[b], 0
    return statuses, its, last


def _solve(q, Acc, l, u, Pcc, opts, stats=None):
    o = _settings(opts)
    _lib.require_device()
    S = _Solver(q, Acc, l, u, Pcc, o["scaling"])
    try:
        S.setup(o["sigma"], o["rho"], o["alpha"])
        status, it = _run(S, o)
        kind = _kind(status)
        x, y = S.solution(kind) if kind is not None else (np.zeros(S.n), np.zeros(S.m))
        if stats is not None:
            stats.update(S.info())
            stats["rho"] = S.rho
        if o["verbose"]:
            print("status: %s, %d iterations, %d factorisations" % (status, it, S.info()["factorisations"]))
        return status, x, y
    finally:
        S.close()


def _sparse_arg(M, name, exc):
    if not _is_sparse_d(M):
        raise exc("%s must be a sparse 'd' matrix" % name)
    return _base.ccs(M)


def _lower(P, n, text):
    Pm, Pn, Pp, Pi, Px = _sparse_arg(P, "P", ValueError)
    if Pm != n or Pn != n:
        raise ValueError(text)
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(Pp))
    keep = Pi >= cols
    lp_ = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols[keep], minlength=n), out=lp_[1:])
    return lp_, Pi[keep].copy(), Px[keep].copy()


def _problem_args(q, A, l, u, P):
    """The arguments of solve() and Problem() checked in the order of osqp.c:374-432: (q, Acc, l, u, Pcc)."""
    Acc = _sparse_arg(A, "A", TypeError)
    m, n = Acc[0], Acc[1]
    if m <= 0:
        raise ValueError("m must be a positive integer")
    if n <= 0:
        raise ValueError("n must be a positive integer")
    q = _vector(q, "q", n)
    u = _vector(u, "u", m)
    l = _vector(l, "l", m)
    Pcc = _lower(P, n, "incompatible dimensions") if P is not None else None
    return q, Acc, l, u, Pcc


def solve(q, A, l, u, P=None, options=None, _stats=None):
    """minimize 0.5 x' P x + q' x  subject to  l <= A x <= u  (osqp.c:374-432): (status, x, y)."""
    q, Acc, l, u, Pcc = _problem_args(q, A, l, u, P)
    return _solve(q, Acc, l, u, Pcc, options, _stats)


def _polish_accepted(rp, rd, hp, hd):
    """(rp, rd): the loop's last residuals, (hp, hd): the polished ones (a kept problem)."""
    return (hp < rp and hd < rd) or (hp < rp and rd < 1e-10) or (hd < rd and rp < 1e-10)


class Problem:
    """minimize 0.5 x' P x + q' x  subject to  l <= A x <= u, kept on the device: planned, analysed and factored once.

    The arguments, their checks and the option keys are those of solve(); here 'polish', 'delta', 'polish_refine_iter' and
    'warm_start' take effect.  After every solve() `info` holds: status, iterations (of this solve), factorisations (so far),
    rho, status_polish (1 accepted, -1 rejected or not factorable, 0 not run), pri_res / dua_res (the loop's last residuals in the
    measure 'scaled_termination' selects), pri_res_polish / dua_res_polish (None when no polish factored), obj_val and
    active_lower / active_upper (None when no polish ran)."""

    def __init__(self, q, A, l, u, P=None, options=None):
        q, Acc, l, u, Pcc = _problem_args(q, A, l, u, P)
        self._o = _read_options(options, 3)
        self.info = None
        self.batch_info = None
        self._S = None
        self._l, self._u = l, u                                         # the current unscaled bounds: solve_batch checks against them
        _lib.require_device()
        S = _Solver(q, Acc, l, u, Pcc, self._o["scaling"])
        try:
            S.setup(self._o["sigma"], self._o["rho"], self._o["alpha"])
        except Exception:
            S.close()
            raise
        self._S = S

    def _solver(self):
        if self._S is None:
            raise ValueError("the problem is closed")
        return self._S

    def update(self, q=None, l=None, u=None):
        """Replace q, l, u (None: kept).  The scaling is kept; a row that changes between equality, free and the other rows
        costs one numeric refactorisation."""
        S = self._solver()
        l, u = None if l is None else _vector(l, "l", S.m), None if u is None else _vector(u, "u", S.m)
        S.update(None if q is None else _vector(q, "q", S.n), l, u)
        self._l, self._u = self._l if l is None else l, self._u if u is None else u

    def warm_start(self, x=None, y=None):
        """The state the next solve() continues from: x (with z = Ax) and y (None: kept).  With 'warm_start' = 0 every solve()
        starts from zero and this has no effect."""
        S = self._solver()
        S.warm_start(None if x is None else _vector(x, "x", S.n), None if y is None else _vector(y, "y", S.m))

    def solve(self):
        """(status, x, y) with the conventions of solve()."""
        S, o = self._solver(), self._o
        if not o["warm_start"]:
            S.cold_start()
        status, it = _run(S, o)
        res = S.last_res
        rp, rd = _pri_dua(res, o)
        info = {"status": status, "iterations": it, "status_polish": 0, "pri_res": float(rp), "dua_res": float(rd),
                "pri_res_polish": None, "dua_res_polish": None, "obj_val": _objective(res, S.c), "active_lower": None,
                "active_upper": None}
        kind = _kind(status)
        if o["polish"] and status == "solved":
            out = S.polish(o["delta"], o["polish_refine_iter"])
            info["active_lower"], info["active_upper"], info["status_polish"] = int(out[1]), int(out[2]), -1
            if out[0] > 0:
                hp, hd = (out[3], out[4]) if o["scaled_termination"] else (out[5], out[6])
                info["pri_res_polish"], info["dua_res_polish"] = float(hp), float(hd)
                if _polish_accepted(rp, rd, hp, hd):
                    S.polish_accept()
                    info["status_polish"], info["obj_val"], kind = 1, (0.5 * out[7] + out[8]) / S.c, 3
        x, y = S.solution(kind) if kind is not None else (np.zeros(S.n), np.zeros(S.m))
        info["factorisations"], info["rho"] = S.info()["factorisations"], S.rho
        self.info = info
        if o["verbose"]:
            print("status: %s, %d iterations, %d factorisations, polish: %s" % (status, it, info["factorisations"],
                                                                              {1: "accepted", -1: "rejected", 0: "not run"}[info["status_polish"]]))
        return status, x, y

    def solve_batch(self, Q, L=None, U=None, chunk=1024):
        """B data sets on the kept factor: (statuses, X, Y).  Q is n x B, L and U are m x B (None: the problem's current l / u for
        every member), dense 'd' matrices or 2-D float64 arrays.  Member b is what update(q_b, l_b, u_b), a start from
        x = z = y = 0 and the loop of solve() with adaptive_rho = 0 at the problem's current rho give: statuses[b] in the wording
        of solve(), columns b of X (n x B) and Y (m x B) the solution, the certificate or zeros as solve() returns them.

        One rho, one factor: nothing adapts and nothing is factored (a factor a polish left stale is rebuilt once); settle rho
        with a solve() first.  Every member must have l <= u and give every row the rho class (equality, free, other) it has in
        the problem now, otherwise ValueError names the first (member, row) and nothing is changed.  'sigma', 'alpha', 'eps_*',
        'check_termination', 'max_iter' and 'scaled_termination' act as in solve(); 'polish', 'warm_start' and 'adaptive_rho*'
        are ignored.  A member stops at its own termination check and is frozen from then on; one host read per check serves
        the whole batch.  More than `chunk` members run in passes of at most `chunk` (device memory of a pass: about ten
        vectors of (n + m) x chunk doubles).  The problem itself -- q, l, u, state, rho, factor -- is left as it was.

        `batch_info` holds per member `iterations`, `pri_res`, `dua_res`, `obj_val` (arrays of length B), and `rho`,
        `factorisations`."""
        S, o = self._solver(), self._o
        chunk = int(chunk)
        if not 1 <= chunk <= 65535:
            raise ValueError("chunk must be between 1 and 65535")
        Q, L, U = _check_batch(Q, L, U, S.n, S.m, S.E, self._l, self._u)
        B = Q.shape[1]
        statuses = [None] * B
        X, Y = np.empty((S.n, B), order="F"), np.empty((S.m, B), order="F")
        its, res = np.zeros(B, dtype=np.int64), np.empty((B, 24))
        try:
            for b0 in range(0, B, chunk):
                b1 = min(B, b0 + chunk)
                S.batch_begin(Q[:, b0:b1], None if L is None else L[:, b0:b1], None if U is None else U[:, b0:b1])
                st, its[b0:b1], res[b0:b1] = _run_batch(S, o, b1 - b0)
                statuses[b0:b1] = st
                X[:, b0:b1], Y[:, b0:b1] = S.batch_solution([-1 if _kind(t) is None else _kind(t) for t in st])
        finally:
            S.batch_end()
        rp, rd = _pri_dua(res, o)
        self.batch_info = {"iterations": its, "pri_res": rp.copy(), "dua_res": rd.copy(), "obj_val": _objective(res, S.c), "rho": S.rho,
                           "factorisations": S.info()["factorisations"]}
        if o["verbose"]:
            print("batch of %d: %d solved, %d to %d iterations, rho %.2e" % (B, sum(t == "solved" for t in statuses), its.min(), its.max(), S.rho))
        return statuses, X, Y

    def close(self):
        if self._S is not None:
            self._S.close()
            self._S = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def resize_problem(G, h, A, b):
    """[G; A] with l = (-INFTY, b), u = (h, b) as CCS arrays and vectors (osqp.c:104-190): ((m + p, n, colptr, rowind, values), l, u)."""
    m, n, Gp, Gi, Gx = G
    if A is None:
        return G, np.full(m, -INFTY), h.copy()
    p, _, Ap, Ai, Ax = A
    colptr = Gp + Ap
    rowind, values = np.empty(colptr[-1], dtype=np.int64), np.empty(colptr[-1])
    gc, ac = np.diff(Gp), np.diff(Ap)
    gpos = np.repeat(colptr[:-1] - Gp[:-1], gc) + np.arange(Gp[-1])                    # column j: G's entries, then A's
    apos = np.repeat(colptr[:-1] + gc - Ap[:-1], ac) + np.arange(Ap[-1])
    rowind[gpos], values[gpos] = Gi, Gx
    rowind[apos], values[apos] = Ai + m, Ax
    return (m + p, n, colptr, rowind, values), np.concatenate([np.full(m, -INFTY), b]), np.concatenate([h, b])


def qp(q, G, h, A=None, b=None, P=None, options=None, _stats=None):
    """minimize (1/2) x'Px + q'x  subject to  Gx <= h, Ax = b  (osqp.c:442-572): (status, x, z, y)."""
    Gcc = _sparse_arg(G, "G", TypeError)
    m, n = Gcc[0], Gcc[1]
    if m <= 0:
        raise ValueError("m must be a positive integer")
    if n <= 0:
        raise ValueError("n must be a positive integer")
    h = _vector(h, "h", m)
    q = _vector(q, "q", n)
    Acc, p = None, 0
    if A is not None:
        Acc = _sparse_arg(A, "A", ValueError)
        p = Acc[0]
        if Acc[1] != n:
            raise ValueError("incompatible dimensions")
    if b is not None:
        b = _vector(b, "b", p)
    elif p:
        raise ValueError("incompatible dimensions")
    Pcc = _lower(P, n, "P must be square matrix of n x n") if P is not None else None
    if p == 0:
        Acc = None
    Anew, l, u = resize_problem(Gcc, h, Acc, b)
    status, x, w = _solve(q, Anew, l, u, Pcc, options, _stats)
    return status, x, w[:m].copy(), w[m:].copy()
