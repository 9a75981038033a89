"""Dense numpy restatement of the ADMM iteration behind kvxopt_amd.osqp (OSQP, Stellato et al. 2020): the
contract the device code is tested against.  Nothing here is shared with the package: same rules, written again.

    minimise 1/2 x'Px + q'x  subject to  l <= Ax <= u          (of P the lower triangle is read; |bound| >= 1e26 is infinite)

`Admm(P, q, A, l, u, ...)` takes dense arrays.  The equilibration always runs in float64 (it defines the scaled problem); the
iteration runs in `dtype`: numpy.float64 (LAPACK Cholesky, A kept sparse for speed) or numpy.longdouble (its own Cholesky: the
yardstick of the parity tests, tiny cases only).
"""
import math

import numpy as np

INFTY = 1e30
INF_FROM = INFTY * 1e-4
NEG_MAX = -1.7976931348623157e308

DEFAULTS = {"scaling": 10, "adaptive_rho": 1, "adaptive_rho_interval": 0, "adaptive_rho_tolerance": 5.0, "rho": 0.1, "sigma": 1e-6,
            "max_iter": 4000, "eps_abs": 1e-3, "eps_rel": 1e-3, "eps_prim_inf": 1e-4, "eps_dual_inf": 1e-4, "alpha": 1.6,
            "scaled_termination": 0, "check_termination": 25}


def _limit(v):
    return np.where(v < 1e-4, 1.0, np.where(v > 1e4, 1e4, v))


def ruiz(P, q, A, passes):
    """(D, E, c, Pbar, qbar, Abar): `passes` Ruiz passes on [[P, A'], [A, 0]], each followed by the cost scaling.  P symmetric."""
    n, m = q.size, A.shape[0]
    L = np.tril(P).astype(np.float64)                   # the lower triangle carries P: (d_i L_ij) d_j, mirrored afterwards
    A, q = A.astype(np.float64).copy(), q.astype(np.float64).copy()
    D, E, c = np.ones(n), np.ones(m), 1.0
    for _ in range(passes):
        F = np.abs(L)
        F = np.maximum(F, F.T)
        dn = np.maximum(F.max(axis=0), np.abs(A).max(axis=0))
        en = np.abs(A).max(axis=1)
        dn, en = 1.0 / np.sqrt(_limit(dn)), 1.0 / np.sqrt(_limit(en))
        L = (dn[:, None] * L) * dn[None, :]
        A = (en[:, None] * A) * dn[None, :]
        q = q * dn
        D, E = D * dn, E * en
        F = np.abs(L)
        pn = np.maximum(F, F.T).max(axis=0)
        s = 0.0
        for v in pn:
            s += float(v)
        g = 1.0 / float(_limit(max(s / n, float(_limit(np.abs(q).max())))))
        L, q, c = L * g, q * g, c * g
    return D, E, c, L + np.tril(L, -1).T, q, A


def rho_vector(lb, ub, rho):
    rho = min(max(rho, 1e-6), 1e6)
    free = (lb <= -INF_FROM) & (ub >= INF_FROM)
    return np.where(free, 1e-6, np.where(ub - lb < 1e-4, 1e3 * rho, rho))


def _chol(S):
    L = np.tril(S).copy()
    n = L.shape[0]
    for j in range(n):
        d = L[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise ArithmeticError("not positive definite")
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (L[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _chol_solve(L, b):
    n = b.size
    y = b.copy()
    for j in range(n):
        y[j] = (y[j] - L[j, :j] @ y[:j]) / L[j, j]
    for j in range(n - 1, -1, -1):
        y[j] = (y[j] - L[j + 1:, j] @ y[j + 1:]) / L[j, j]
    return y


def cut(dy, lb, ub):
    """dy without the parts that push against an infinite bound."""
    ui, li = ub >= INF_FROM, lb <= -INF_FROM
    return np.where(ui & li, 0.0, np.where(ui, np.minimum(dy, 0.0), np.where(li, np.maximum(dy, 0.0), dy)))


class Admm:
    def __init__(self, P, q, A, l, u, scaling=10, sigma=1e-6, rho=0.1, alpha=1.6, dtype=np.float64):
        q, A = np.asarray(q, dtype=np.float64), np.asarray(A, dtype=np.float64)
        l, u = np.asarray(l, dtype=np.float64), np.asarray(u, dtype=np.float64)
        self.m, self.n = A.shape
        P = np.zeros((self.n, self.n)) if P is None else np.asarray(P, dtype=np.float64)
        P = np.tril(P) + np.tril(P, -1).T
        self.D, self.E, self.c, Pb, qb, Ab = ruiz(P, q, A, scaling)
        lb = np.where(l <= -INF_FROM, -INFTY, self.E * l)
        ub = np.where(u >= INF_FROM, INFTY, self.E * u)
        self.lb64, self.ub64 = lb, ub
        self.dtype = dtype
        t = lambda v: np.asarray(v, dtype=dtype)
        self.Pb, self.qb, self.Ab, self.lb, self.ub = t(Pb), t(qb), t(Ab), t(lb), t(ub)
        self.Dv, self.Ev, self.cinv = t(self.D), t(self.E), dtype(1.0) / dtype(self.c)
        self.Dinv, self.Einv = dtype(1.0) / self.Dv, dtype(1.0) / self.Ev
        self.sigma, self.alpha = dtype(sigma), dtype(alpha)
        self.fast = dtype is np.float64
        if self.fast:
            import scipy.sparse
            self.As, self.Ps = scipy.sparse.csr_matrix(Ab), scipy.sparse.csr_matrix(Pb)
            self.Ats = scipy.sparse.csr_matrix(Ab.T)
        z = lambda k: np.zeros(k, dtype=dtype)
        self.x, self.z, self.y, self.dx, self.dy = z(self.n), z(self.m), z(self.m), z(self.n), z(self.m)
        self.nfact, self.niter = 0, 0
        self.set_rho(rho)

    # products (sparse in the float64 mode, dense otherwise)
    def A_(self, v): return self.As @ v if self.fast else self.Ab @ v
    def At_(self, v): return self.Ats @ v if self.fast else self.Ab.T @ v
    def P_(self, v): return self.Ps @ v if self.fast else self.Pb @ v

    def set_rho(self, rho):
        self.rho = min(max(float(rho), 1e-6), 1e6)
        self.rv = np.asarray(rho_vector(self.lb64, self.ub64, rho), dtype=self.dtype)
        S = self.Pb + self.sigma * np.eye(self.n, dtype=self.dtype) + self.Ab.T @ (self.rv[:, None] * self.Ab)
        if self.fast:
            import scipy.linalg
            try:
                self.L = scipy.linalg.cho_factor(S, lower=True)
            except np.linalg.LinAlgError as e:
                raise ArithmeticError(str(e))
        else:
            self.L = _chol(S)
        self.nfact += 1

    def _solve(self, b):
        if self.fast:
            import scipy.linalg
            return scipy.linalg.cho_solve(self.L, b)
        return _chol_solve(self.L, b)

    def iterate(self, k):
        a = self.alpha
        for _ in range(k):
            rhs = self.sigma * self.x - self.qb + self.At_(self.rv * self.z - self.y)
            xt = self._solve(rhs)
            zt = self.A_(xt)
            xn = a * xt + (1 - a) * self.x
            v = a * zt + (1 - a) * self.z
            zn = np.minimum(np.maximum(v + self.y / self.rv, self.lb), self.ub)
            yn = self.y + self.rv * (v - zn)
            self.dx, self.dy = xn - self.x, yn - self.y
            self.x, self.z, self.y = xn, zn, yn
        self.niter += k
        return self.residuals()

    def residuals(self):
        """The 24 numbers of kvx_admm_iterate (include/kvxhip.h)."""
        r = np.zeros(24, dtype=self.dtype)
        x, z, y, ci = self.x, self.z, self.y, self.cinv
        nrm = lambda v: np.abs(v).max() if v.size else NEG_MAX
        ax, px, aty = self.A_(x), self.P_(x), self.At_(y)
        rd = px + self.qb + aty
        r[0], r[1], r[2] = nrm(ax - z), nrm(ax), nrm(z)
        r[3], r[4], r[5], r[6] = nrm(rd), nrm(px), nrm(aty), nrm(self.qb)
        r[7], r[8], r[9] = nrm(self.Einv * (ax - z)), nrm(self.Einv * ax), nrm(self.Einv * z)
        s = self.Dinv * ci
        r[10], r[11], r[12], r[13] = nrm(rd * s), nrm(px * s), nrm(aty * s), nrm(self.qb * s)
        d = cut(self.dy, self.lb, self.ub)
        fu, fl = self.ub < INF_FROM, self.lb > -INF_FROM
        r[14] = nrm(self.Ev * d * ci)
        r[15] = (np.where(fu, self.ub * np.maximum(d, 0), 0).sum() + np.where(fl, self.lb * np.minimum(d, 0), 0).sum()) * ci
        r[16] = nrm(self.At_(d) * s)
        r[17] = nrm(self.Dv * self.dx)
        r[18] = (self.qb @ self.dx) * ci
        r[19] = nrm(self.P_(self.dx) * s)
        adx = self.Einv * self.A_(self.dx)
        r[20] = adx[fu].max() if fu.any() else NEG_MAX
        r[21] = (-adx[fl]).max() if fl.any() else NEG_MAX
        r[22], r[23] = x @ px, self.qb @ x
        return r

    def sum_scales(self):
        """For the four entries of residuals() that are sums (15, 18, 22, 23): the sum of the absolute values of their terms."""
        d = cut(self.dy, self.lb, self.ub)
        fu, fl = self.ub < INF_FROM, self.lb > -INF_FROM
        ab = np.abs
        s15 = (np.where(fu, ab(self.ub) * np.maximum(d, 0), 0).sum() + np.where(fl, ab(self.lb) * ab(np.minimum(d, 0)), 0).sum()) * self.cinv
        return {15: s15, 18: (ab(self.qb) @ ab(self.dx)) * self.cinv, 22: ab(self.x) @ (ab(self.Pb) @ ab(self.x)), 23: ab(self.qb) @ ab(self.x)}

    def state(self):
        return self.x, self.z, self.y, self.dx, self.dy

    def solution(self, kind=0):
        if kind == 0:
            return self.Dv * self.x, self.Ev * self.y * self.cinv
        if kind == 1:
            return np.zeros(self.n), self.Ev * cut(self.dy, self.lb, self.ub) * self.cinv
        return self.Dv * self.dx, np.zeros(self.m)


def judge(res, o, mult=1.0, margins=None):
    """Status at tolerances times `mult`, or None.  margins (a list): relative distances of the two residual tests from their
    thresholds are appended."""
    ea, er, epi, edi = o["eps_abs"] * mult, o["eps_rel"] * mult, o["eps_prim_inf"] * mult, o["eps_dual_inf"] * mult
    b = 0 if o["scaled_termination"] else 7
    tp = ea + er * max(res[b + 1], res[b + 2])
    td = ea + er * max(res[b + 4], res[b + 5], res[b + 6])
    if margins is not None:
        margins += [abs(float(res[b] - tp)) / float(tp), abs(float(res[b + 3] - td)) / float(td)]
    prim, dual = res[b] <= tp, res[b + 3] <= td
    if prim and dual:
        return "solved"
    ndy, ndx = res[14], res[17]
    if not prim and ndy > epi and res[15] < -epi * ndy and res[16] < epi * ndy:
        return "primal infeasible"
    if not dual and ndx > edi and res[18] < -edi * ndx and res[19] < edi * ndx and res[20] <= edi * ndx and res[21] <= edi * ndx:
        return "dual infeasible"
    return None


def new_rho(res, rho):
    pr = float(res[0]) / (float(max(res[1], res[2])) + 1e-10)
    du = float(res[3]) / (float(max(res[4], res[5], res[6])) + 1e-10)
    return min(max(rho * math.sqrt(pr / (du + 1e-10)), 1e-6), 1e6)


def run(S, o, margins=None):
    """The loop of kvxopt_amd.osqp on a restatement object: (status, iterations).  margins: see judge; those of every check, and
    the relative distance of every adaptive-rho decision from its two thresholds."""
    check, max_iter = o["check_termination"], o["max_iter"]
    adaptive = bool(o["adaptive_rho"])
    interval = (o["adaptive_rho_interval"] or 100) if adaptive else 0
    it = 0
    while True:
        nxt = max_iter
        if check > 0:
            nxt = min(nxt, (it // check + 1) * check)
        if adaptive:
            nxt = min(nxt, (it // interval + 1) * interval)
        res = S.iterate(max(nxt - it, 0))
        it = max(nxt, it)
        checked = check > 0 and it % check == 0
        if checked or it >= max_iter:
            status = judge(res, o, 1.0, margins) if checked else None
            if status is None and it >= max_iter:
                status = judge(res, o, 10.0)
                status = status + " inaccurate" if status else "maximum iterations reached"
            if status is not None:
                return status, it
        if adaptive and it % interval == 0:
            rho = new_rho(res, S.rho)
            tol = o["adaptive_rho_tolerance"]
            if margins is not None:
                margins += [abs(rho - tol * S.rho) / (tol * S.rho), abs(rho - S.rho / tol) / (S.rho / tol)]
            if rho > tol * S.rho or rho < S.rho / tol:
                S.set_rho(rho)


def solve(P, q, A, l, u, opts=None, dtype=np.float64, margins=None):
    """(status, x, y, iterations, factorisations) of the restatement."""
    o = dict(DEFAULTS)
    o.update({k: v for k, v in (opts or {}).items() if k in DEFAULTS})
    S = Admm(P, q, A, l, u, int(o["scaling"]), o["sigma"], o["rho"], o["alpha"], dtype)
    status, it = run(S, o, margins)
    kind = 0 if status.startswith("solved") else 1 if status.startswith("primal") else 2 if status.startswith("dual") else None
    x, y = S.solution(kind) if kind is not None else (np.zeros(S.n), np.zeros(S.m))
    return status, np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), it, S.nfact


def dense(m, n, cp, ri, vx):
    M = np.zeros((m, n))
    M[ri, np.repeat(np.arange(n), np.diff(cp))] = vx
    return M


def stack_qp(G, h, A=None, b=None):
    """[G; A], l = (-INFTY, b), u = (h, b): the numpy stacking resize_problem is compared with."""
    if A is None or A.shape[0] == 0:
        return G, np.full(G.shape[0], -INFTY), np.asarray(h, dtype=np.float64)
    return np.vstack([G, A]), np.concatenate([np.full(G.shape[0], -INFTY), b]), np.concatenate([h, b])


# ---- the problems of the tests, as dense data: {"P": n x n or None, "q", "A": m x n, "l", "u"} ------------------------------
def golden():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_osqp_cases.json")) as f:
        return json.load(f)


def from_qp(P, q, G, h, A=None, b=None):
    As, l, u = stack_qp(np.asarray(G, dtype=np.float64), np.asarray(h, dtype=np.float64),
                        None if A is None else np.asarray(A, dtype=np.float64), None if b is None else np.asarray(b, dtype=np.float64))
    return {"P": None if P is None else np.asarray(P, dtype=np.float64), "q": np.asarray(q, dtype=np.float64), "A": As, "l": l, "u": u}


def case_basic():
    g = golden()["basic"]
    return {"P": np.array(g["P"]), "q": np.array(g["q"]), "A": np.array(g["A"]), "l": np.array(g["l"]), "u": np.array(g["u"])}


def _sym(n, cp, ri, vx):
    L = dense(n, n, cp, ri, vx)
    return L + np.tril(L, -1).T


def case_qp_grid(gx, gy):
    from kvxopt_amd import workloads
    W = workloads.qp_grid(gx, gy)
    return from_qp(_sym(W["n"], W["Pp"], W["Pi"], W["Px"]), W["q"], dense(W["ml"], W["n"], W["Gp"], W["Gi"], W["Gx"]), W["h"])


def case_lp_grid(gx, gy):
    from kvxopt_amd import workloads
    W = workloads.lp_grid(gx, gy)
    return from_qp(None, W["c"], dense(W["ml"], W["n"], W["Gp"], W["Gi"], W["Gx"]), W["h"])


def case_lp_grid_std(gx, gy):
    from kvxopt_amd import workloads
    W = workloads.lp_grid_std(gx, gy)
    return from_qp(None, W["c"], dense(W["ml"], W["n"], W["Gp"], W["Gi"], W["Gx"]), W["h"],
                   dense(W["p"], W["n"], W["Ap"], W["Ai"], W["Ax"]), W["b"])


def case_lp_grid_eq(gx, gy, p):
    from kvxopt_amd import workloads
    W = workloads.lp_grid_eq(gx, gy, p)
    return from_qp(None, W["c"], dense(W["ml"], W["n"], W["Gp"], W["Gi"], W["Gx"]), W["h"],
                   dense(W["p"], W["n"], W["Ap"], W["Ai"], W["Ax"]), W["b"])


def case_generated(with_p):
    """n = 65, m = 257: more than one wavefront of columns and more than one workgroup of rows.  Row 0 of A and column 7 are
    empty, row 5 holds every other column (64 entries: the most that an empty column leaves, summed by a wavefront), rows 10-19
    are equalities, 20-39 two-sided, 40-49 without a finite bound, the others one-sided.  P: empty, or diagonal + two off-diagonals."""
    n, m = 65, 257
    rng = np.random.default_rng(25)
    A = np.zeros((m, n))
    for i in range(m):
        A[i, rng.choice(n, 4, replace=False)] = rng.standard_normal(4)
    A[5, :] = rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
    A[0, :] = 0.0
    A[:, 7] = 0.0
    x0 = rng.standard_normal(n)
    ax = A @ x0
    l, u = np.full(m, -INFTY), ax + rng.uniform(0.5, 1.5, m)
    l[10:20] = u[10:20] = ax[10:20]
    l[20:40] = ax[20:40] - rng.uniform(0.5, 1.5, 20)
    l[40:50], u[40:50] = -INFTY, INFTY
    l[50:60], u[50:60] = ax[50:60] - 1.0, INFTY
    P = None
    if with_p:
        P = np.diag(rng.uniform(0.5, 2.0, n))
        for k in (1, 9):
            v = 0.2 * rng.standard_normal(n - k)
            P += np.diag(v, -k) + np.diag(v, k)
    return {"P": P, "q": rng.standard_normal(n), "A": A, "l": l, "u": u}


def to_ccs(M):
    """(m, n, colptr, rowind, values) of the nonzeros of a dense matrix."""
    m, n = M.shape
    ri, ci = np.nonzero(M.T)[1], np.nonzero(M.T)[0]
    cp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ci, minlength=n), out=cp[1:])
    return m, n, cp, ri.astype(np.int64), M[ri, ci].astype(np.float64)
