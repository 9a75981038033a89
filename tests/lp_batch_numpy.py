"""The restatement kvxopt_amd.lpbatch is tested against: tests/test_lp_loop_cpu.py's NumpyEngine extended by y, ry, hry, dy and
equality constraints, run through _ipm.conelp_start and _ipm.conelp_loop on one member at a time, in float64 or numpy.longdouble.
The KKT solve is misc.py:1395-1563 on dense matrices: S = G' di^2 G = L L', X = L^-1 A', K = X'X, with the explicit column
Cholesky of tests/qp_batch_numpy.py that raises ArithmeticError on a pivot <= 0 (or not finite), and kkt_chol2's F['singular']
repair: when the first factor of S fails and p > 0, S := S + A'A from then on and every solve adds A'by to bx.  `linsolve=True`
takes both triangular factors from numpy.linalg.qr (of W^-1 G and of X, never forming S or K) and substitutes by numpy.linalg.solve
(float64 only), which moves every rounding and so shows whether an iteration count sits on a rounding edge.  (numpy.linalg.solve
on S and K themselves, as tests/qp_batch_numpy.py does it, loses the primal residual of an LP near its solution, where S has no
P to keep it well conditioned.)  Also the seeded generators of feasible, primal
infeasible, dual infeasible and free-variable members the tests use, and the cache of their restated results."""
import functools
import types

import numpy as np

import qp_batch_numpy as Q
from kvxopt_amd import _ipm, workloads

QUIET = {"show_progress": False}
EXITS = {"optimal": 0, "primal infeasible": 4, "dual infeasible": 5}


class Vec:
    """What _ipm.conelp_start asks of a vector, on a numpy array `a`."""

    def __init__(self, a):
        self.a = a
        self.n = len(a)

    def fill(self, v):
        self.a[:] = v
        return self

    def copy_from(self, u):
        self.a[:] = u.a
        return self

    def set(self, values):
        self.a[:] = values
        return self

    def scal(self, alpha):
        self.a *= alpha
        return self

    def axpy(self, u, alpha=1.0):
        self.a += alpha * u.a
        return self

    def dot(self, u):
        return float(self.a @ u.a)

    def nrm2(self):
        return float(np.sqrt(self.a @ self.a))


class LpEngine:
    """The engine protocols of _ipm.conelp_start and _ipm.conelp_loop in numpy with p >= 0 equality constraints."""
    rank_msg = "Rank(A) < p or Rank([G; A]) < n"

    def __init__(self, c, G, h, A=None, b=None, dtype=np.float64, linsolve=False):
        self.t = t = dtype
        n, ml = len(c), len(h)
        self.c, self.G, self.h = (np.asarray(a, dtype=t) for a in (c, G, h))
        self.A = np.zeros((0, n), dtype=t) if A is None else np.asarray(A, dtype=t)
        self.b = np.zeros(0, dtype=t) if b is None else np.asarray(b, dtype=t)
        self.p, self.linsolve, self.singular, self.first = len(self.A), linsolve, False, True
        self.d = self.di = np.ones(ml, dtype=t)
        zn, zp, zm = (lambda k=k: Vec(np.zeros(k, dtype=t)) for k in (n, self.p, ml))
        self.x, self.dx, self.rx = zn(), zn(), zn()
        self.y, self.dy, self.ry = zp(), zp(), zp()
        self.s, self.z, self.rz, self.lmbda = zm(), zm(), zm(), zm()
        self.cv, self.bv, self.hv = Vec(self.c), Vec(self.b), Vec(self.h)

    # ---- the KKT system (misc.py:1395-1563)
    def factor(self):
        first, self.first = self.first, False
        Gs = self.di[:, None] * self.G
        try:
            self.L = self.lower(np.vstack([Gs, self.A]) if self.singular else Gs)
        except ArithmeticError:
            if not first or self.p == 0:
                raise
            self.singular = True                             # F['singular'] (misc.py:1433-1447)
            self.L = self.lower(np.vstack([Gs, self.A]))
        if self.p:
            self.X = self.fwd(self.L, self.A.T)
            self.Lk = self.lower(self.X)

    def lower(self, F):
        """A lower triangular L with L L' = F'F: the column Cholesky of F'F, or for `linsolve` R' of numpy.linalg.qr(F), which never forms
        F'F and so moves every rounding; its diagonal may be negative, and an exact zero on it is the failed pivot."""
        if not self.linsolve:
            return Q.cholesky(F.T @ F)
        if not np.all(np.isfinite(F)) or F.shape[0] < F.shape[1]:
            raise ArithmeticError("F'F is singular")
        R = np.linalg.qr(F, mode="r")
        if not np.all(np.diag(R) != 0.0):
            raise ArithmeticError("zero pivot")
        return np.ascontiguousarray(R.T)

    def fwd(self, L, B):
        return np.linalg.solve(L, B) if self.linsolve else Q.forward(L, B)

    def bwd(self, L, B):
        return np.linalg.solve(L.T, B) if self.linsolve else Q.backward(L, B)

    def ksolve(self, x, y, z):
        z = self.di * z
        x = x + self.G.T @ (self.di * z)
        if self.singular:
            x = x + self.A.T @ y
        x = self.fwd(self.L, x)
        if self.p:
            y = self.bwd(self.Lk, self.fwd(self.Lk, self.X.T @ x - y))
            x = x - self.X @ y
        x = self.bwd(self.L, x)
        return x, y, self.di * (self.G @ x) - z

    # ---- what _ipm.conelp_start asks for
    def factor_identity(self, needed):
        self.factor()

    def start_solve(self, x, y, z):
        x.a[:], y.a[:], z.a[:] = self.ksolve(x.a, y.a, z.a)

    def max_step(self, v):
        return float(max(-v.a))

    def nrm2(self, v):
        return v.nrm2()

    def dot(self, u, v):
        return u.dot(v)

    def add_e(self, v, a):
        v.a += a
        return v

    def symm(self, v):
        pass

    def Gf(self, u, v, trans="N", alpha=1.0, beta=0.0):
        v.a[:] = alpha * ((self.G.T if trans == "T" else self.G) @ u.a) + beta * v.a

    def Af(self, u, v, trans="N", alpha=1.0, beta=0.0):
        v.a[:] = alpha * ((self.A.T if trans == "T" else self.A) @ u.a) + beta * v.a

    # ---- what _ipm.conelp_loop asks for
    def stats(self, tau):
        c, G, h, A, b = self.c, self.G, self.h, self.A, self.b
        x, y, s, z = self.x.a, self.y.a, self.s.a, self.z.a
        hrx = -(A.T @ y) - G.T @ z
        hry = A @ x
        hrz = G @ x + s
        self.rx.a, self.ry.a, self.rz.a = hrx - tau * c, hry - tau * b, hrz - tau * h
        lm = self.lmbda.a
        return tuple(float(v) for v in (hrx @ hrx, self.rx.a @ self.rx.a, hry @ hry, self.ry.a @ self.ry.a, hrz @ hrz,
                                        self.rz.a @ self.rz.a, c @ x, b @ y, h @ z, lm @ lm))

    def scaling(self):
        self.d = np.sqrt(self.s.a / self.z.a)
        self.di = 1.0 / self.d
        self.lmbda.a = np.sqrt(self.s.a * self.z.a)
        return float(self.lmbda.a @ self.lmbda.a)

    def direction(self, i, sigma, mu, rt, dg, dgi, lmbda_g, wkappa3):
        lm = self.lmbda.a
        if i == 0:
            self.factor()                                    # ArithmeticError: conelp_loop ends the member
            self.x1, self.y1, self.z1 = (dgi * v for v in self.ksolve(-self.c, self.b, self.h))
        ds = lm ** 2
        dkappa = lmbda_g ** 2
        if i == 1:
            ds = ds + self.ws3 - sigma * mu
            dkappa += wkappa3 - sigma * mu
        ds = -ds / lm
        # f6_no_ir (coneprog.py:1130-1195): f3(bx, -by, -(bz + W'ds)), then the combination with (x1, y1, z1)
        dx, dy, dz = self.ksolve((1.0 - sigma) * self.rx.a, -((1.0 - sigma) * self.ry.a), -((1.0 - sigma) * self.rz.a + self.d * ds))
        dkappa = -dkappa / lmbda_g
        dtau = float(dgi * ((1.0 - sigma) * rt + dkappa / dgi + self.c @ dx + self.b @ dy + (self.di * self.h) @ dz)
                     / (1.0 + self.z1 @ self.z1))
        self.dx.a, self.dy.a, dz = dx + dtau * self.x1, dy + dtau * self.y1, dz + dtau * self.z1
        ds = ds - dz
        if i == 0:
            self.ws3 = ds * dz
        self.dtau, self.dkappa, self.ds, self.dz = dtau, dkappa - dtau, ds / lm, dz / lm

    def bounds(self, i):
        return self.dtau, self.dkappa, float(max(-self.ds)), float(max(-self.dz))

    def update(self, step, tau):
        lm = self.lmbda.a
        self.x.a = self.x.a + step * self.dx.a
        self.y.a = self.y.a + step * self.dy.a
        rs, rz = (np.sqrt((1.0 + step * v) * lm) for v in (self.ds, self.dz))       # misc.py:444-464
        self.d = self.d * rs / rz
        self.di = 1.0 / self.d
        self.lmbda.a = rs * rz
        self.s.a, self.z.a = self.d * self.lmbda.a, self.di * self.lmbda.a

    def scale(self, primal, dual):
        if primal is not None:
            self.x.a, self.s.a = primal * self.x.a, primal * self.s.a
        if dual is not None:
            self.y.a, self.z.a = dual * self.y.a, dual * self.z.a


def solve_member(c, G, h, A=None, b=None, options=None, dtype=np.float64, linsolve=False):
    """One member through _ipm.conelp_start and _ipm.conelp_loop: a namespace with status, exit (the codes of kvxopt_amd.lpbatch),
    iterations, x, y, s, z (NaN for the half a certificate comes without), singular (the A'A repair was taken) and the statistics
    gap, relgap, pcost, dcost, pres, dres, primal slack, dual slack, pinfres, dinfres (NaN for None)."""
    opt = _ipm.options(dict(QUIET, **(options or {})), {})
    n, ml, p = len(c), len(h), 0 if A is None else len(A)
    e = LpEngine(c, G, h, A, b, dtype, linsolve)
    res0 = tuple(max(1.0, v.nrm2()) for v in (e.cv, e.bv, e.hv))
    failed = False
    try:
        out = _ipm.conelp_start(e, opt, None, None, res0)
        if not isinstance(out, _ipm.Outcome):
            out = _ipm.conelp_loop(e, opt, ml, out, res0)
        failed = out.msg == _ipm.SINGULAR_MSG and out.iterations == 0                    # the first factorisation of the loop
    except (ValueError, np.linalg.LinAlgError):                                           # solvers.lp: ValueError("Rank(A) < p or ...")
        failed = True
    if failed:
        z = np.zeros
        return types.SimpleNamespace(status="unknown", exit=3, iterations=0, x=z(n), y=z(p), s=z(ml), z=z(ml), stats=(np.nan,) * 10,
                                     singular=e.singular)
    code = EXITS.get(out.status, 1 if out.msg == _ipm.MAXITERS_MSG else 2)
    xs, zs = out.status != "primal infeasible", out.status != "dual infeasible"
    nan = lambda v: np.full(len(v.a), np.nan)                                            # noqa: E731
    slacks = (float(min(e.s.a)) if xs else None, float(min(e.z.a)) if zs else None)
    stats = tuple(np.nan if v is None else float(v) for v in out.stats[:6] + slacks + out.stats[6:])
    return types.SimpleNamespace(status=out.status, exit=code, iterations=out.iterations, x=e.x.a if xs else nan(e.x),
                                 y=e.y.a if zs else nan(e.y), s=e.s.a if xs else nan(e.s), z=e.z.a if zs else nan(e.z), stats=stats,
                                 singular=e.singular)


FEASIBLE, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE = "feasible", "primal infeasible", "dual infeasible"


def members(n, ml, p, B, seed, kinds=(FEASIBLE,), free=0):
    """B members with per-member G (B, ml, n), A (B, p, n) and c (n x B), h (ml x B), b (p x B), member k of kind kinds[k % len(kinds)],
    on the feasible construction of qp_batch_numpy.members (h = G x0 + U(0.1, 1), b = A x0):
      feasible           c = -G'z0 - A'y0 with z0 ~ U(0.5, 1.5): strictly feasible on both sides, so bounded
      primal infeasible  a feasible member with rows 0 and 1 replaced by g'x <= -1 and -g'x <= -1
      dual infeasible    d in the null space of A, every row of G signed so that G d <= 0, h = G x1 + U(0.1, 1) with A x1 = b, and
                         c = -d + 0.1 w with w orthogonal to d, so c'd = -d'd < 0: feasible and unbounded along d
    free: the last `free` <= p columns of G are exactly zero (A has full rank on them), so S = G' W^-2 G is structurally singular;
    h = G x1 + U(0.1, 1) with A x1 = b then, since x0 is no longer feasible for the G that lost its columns."""
    M = Q.members(n, ml, p, B, seed)
    rng = np.random.default_rng(seed + 1000003)
    G, h = M.G.copy(), np.array(M.h)
    A = M.A if p else np.zeros((B, 0, n))
    b = np.array(M.b) if p else np.zeros((0, B))
    assert free <= p
    c = np.zeros((n, B))
    kind = [kinds[k % len(kinds)] for k in range(B)]
    for k in range(B):
        if free:                                            # h again, at a point of A x = b, for the G that lost its columns
            G[k, :, n - free:] = 0.0
            h[:, k] = G[k] @ np.linalg.lstsq(A[k], b[:, k], rcond=None)[0] + rng.uniform(0.1, 1.0, ml)
        z0, y0 = rng.uniform(0.5, 1.5, ml), rng.standard_normal(p)
        c[:, k] = -G[k].T @ z0 - A[k].T @ y0
        if kind[k] == PRIMAL_INFEASIBLE:
            g = rng.standard_normal(n)
            g[n - free:] = 0.0
            G[k, 0], G[k, 1] = g, -g
            h[0, k] = h[1, k] = -1.0
        elif kind[k] == DUAL_INFEASIBLE:
            null = np.linalg.svd(A[k])[2][p:].T if p else np.eye(n)                    # columns: a basis of the null space of A
            d = null @ rng.standard_normal(null.shape[1])
            sign = np.where(G[k] @ d > 0.0, -1.0, 1.0)
            G[k] *= sign[:, None]
            x1 = np.linalg.lstsq(A[k], b[:, k], rcond=None)[0] if p else np.zeros(n)
            h[:, k] = G[k] @ x1 + rng.uniform(0.1, 1.0, ml)
            w = rng.standard_normal(n)
            w -= d * (w @ d) / (d @ d)
            c[:, k] = -d + 0.1 * w
    return types.SimpleNamespace(n=n, ml=ml, p=p, B=B, c=np.asfortranarray(c), G=G, h=np.asfortranarray(h), A=A if p else None,
                                 b=np.asfortranarray(b) if p else None, kind=kind)


def member(M, k):
    """(c, G, h, A, b) of member k."""
    return M.c[:, k], M.G[k], M.h[:, k], None if M.A is None else M.A[k], None if M.b is None else M.b[:, k]


def dense(m, n, cp, ri, v):
    D = np.zeros((m, n))
    D[ri, np.repeat(np.arange(n), np.diff(cp))] = v
    return D


def grid_dense(p=0):
    """The data of the reference's runs G4 grid6x5 (p = 0) and G8 eq6x5p4 (p = 4) as dense arrays c, G, h, A, b."""
    L = workloads.lp_grid_eq(6, 5, p) if p else workloads.lp_grid(6, 5)
    n = L["n"]
    A, b = (dense(p, n, L["Ap"], L["Ai"], L["Ax"]), L["b"]) if p else (None, None)
    return L["c"], dense(L["ml"], n, L["Gp"], L["Gi"], L["Gx"]), L["h"], A, b


DOC_LP = ([-4., -5.], [[2., 1.], [1., 2.], [-1., 0.], [0., -1.]], [3., 3., 0., 0.])       # examples/doc/chap8/lp.py
TINY = {"doc_lp": DOC_LP + ("optimal", 4, "x"),                                          # the cases of tests/test_lp_loop_cpu.py
        "primal_infeasible": ([1.0], [[-1.0], [1.0]], [-1.0, 0.0], "primal infeasible", 4, "z"),
        "dual_infeasible": ([-1.0, 0.5], [[-1.0, 0.0], [0.0, -1.0]], [0.0, 0.0], "dual infeasible", 4, "x")}


def restate(M, options=None, dtype=np.float64, linsolve=False, which=None):
    """solve_member on every member (or those of `which`) of a batch from members()."""
    return [solve_member(*member(M, k), options, dtype, linsolve) for k in (range(M.B) if which is None else which)]


# ---- the batches of tests/test_lp_batch_gpu.py; tests/test_lp_batch_cpu.py checks that none of their counts sits on a rounding edge
SHAPES = [(1, 1, 0), (8, 17, 3), (33, 65, 5), (63, 255, 0), (64, 256, 1), (64, 257, 16), (64, 512, 64), (31, 300, 0)]
SHAPE_B = 12
THIRDS = (FEASIBLE, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE)
# Seeds at which float64, longdouble and float64 with numpy.linalg.solve agree in every status and count and the mixed batch ends
# with every exit it is to show (tests/test_lp_batch_cpu.py).  At (1, 1, 0) G is square, so the starting
# point is the vertex h / g itself and s = h - g x is a rounding error whose sign decides between "optimal at iteration 0" and
# four iterations: seed 9 is the first of 1, 2, ... at which s >= 0 for all twelve members in all three arithmetics.
SEEDS = dict(zip(SHAPES, (9, 201, 202, 203, 204, 305, 206, 207)))
# name -> (shape, B, seed, kinds, free)
BATCHES = {"shape-%d-%d-%d" % s: (s, SHAPE_B, SEEDS[s], (FEASIBLE,), 0) for s in SHAPES}
BATCHES.update({
    "certificates-8-17-3": ((8, 17, 3), 12, 331, THIRDS, 0),
    "certificates-33-65-5": ((33, 65, 5), 12, 132, THIRDS, 0),
    "free-8-17-3": ((8, 17, 3), 12, 41, (FEASIBLE,), 2),
    "free-64-256-16": ((64, 256, 16), 6, 42, (FEASIBLE,), 5),
    "independence": ((16, 33, 2), 300, 8, (FEASIBLE,), 0),
    "mixed": ((8, 17, 3), 12, 651, (FEASIBLE, FEASIBLE, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE), 0),
})
MIXED_CHANGED = (4, 8)       # the members of "mixed" the GPU test spoils: a variable nothing holds, a NaN in c (both are feasible ones)
SMALL_BATCHES = sorted(k for k in BATCHES if k != "independence")


@functools.lru_cache(maxsize=None)
def batch(name):
    (n, ml, p), B, seed, kinds, free = BATCHES[name]
    return members(n, ml, p, B, seed, kinds, free)


@functools.lru_cache(maxsize=None)
def restated(name, precision="longdouble", linsolve=False):
    """The restated results of batch(name), computed once per process and left unchanged."""
    return restate(batch(name), None, getattr(np, precision), linsolve)
