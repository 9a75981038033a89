"""The restatement kvxopt_amd.qpbatch is tested against: tests/test_qp_loop_cpu.py's NumpyQpEngine extended by equality
constraints, run through _ipm.coneqp_loop on one member at a time, in float64 or numpy.longdouble.  The KKT solve is
misc.py:1489-1563 on dense matrices: S = P + G' di^2 G = L L', X = L^-1 A', K = X'X, with an explicit column Cholesky that raises
ArithmeticError on a pivot <= 0 (or not finite); `linsolve=True` replaces both factors by numpy.linalg.solve (float64 only),
which moves every rounding and so shows whether an iteration count sits on a rounding edge.  Also the seeded generator of
feasible members the tests use, and the cache of their restated results."""
import functools
import types

import numpy as np

from kvxopt_amd import _ipm, workloads

QUIET = {"show_progress": False}


def cholesky(S):
    L = np.tril(S)
    for j in range(len(L)):
        piv = L[j, j]
        if not (piv > 0 and np.isfinite(piv)):
            raise ArithmeticError("pivot %d" % j)
        L[j, j] = np.sqrt(piv)
        L[j + 1:, j] /= L[j, j]
        L[j + 1:, j + 1:] -= np.tril(np.outer(L[j + 1:, j], L[j + 1:, j]))
    return L


def forward(L, B):
    """L^-1 B, B a vector or a matrix of right-hand sides."""
    B = B.copy()
    for j in range(len(L)):
        B[j] = B[j] / L[j, j]
        B[j + 1:] -= np.multiply.outer(L[j + 1:, j], B[j])
    return B


def backward(L, B):
    """L'^-1 B for the lower triangular L."""
    B = B.copy()
    for j in range(len(L) - 1, -1, -1):
        B[j] = B[j] / L[j, j]
        B[:j] -= np.multiply.outer(L[j, :j], B[j])
    return B


class QpEngine:
    """_ipm.coneqp_loop's engine protocol in numpy with p >= 0 equality constraints."""

    def __init__(self, P, q, G, h, A=None, b=None, dtype=np.float64, linsolve=False):
        self.t = dtype
        n = len(q)
        P = np.asarray(P, dtype=dtype)
        self.P = np.tril(P) + np.tril(P, -1).T                      # only the lower triangle is read
        self.q, self.G, self.h = (np.asarray(a, dtype=dtype) for a in (q, G, h))
        self.A = np.zeros((0, n), dtype=dtype) if A is None else np.asarray(A, dtype=dtype)
        self.b = np.zeros(0, dtype=dtype) if b is None else np.asarray(b, dtype=dtype)
        self.p, self.linsolve = len(self.A), linsolve
        self.d = self.di = np.ones(len(self.h), dtype=dtype)
        # starting point (coneprog.py:2044-2105): W = I, right-hand side (-q, b, h), s = -z, both pushed into the cone
        self.factor()
        self.x, self.y, z = self.ksolve(-self.q, self.b, self.h)
        self.s, self.z = (v + (1.0 + max(-v)) if max(-v) >= -1e-8 * max(float(np.sqrt(v @ v)), 1.0) else v for v in (-z, z))

    def factor(self):
        self.S = self.P + self.G.T @ ((self.di ** 2)[:, None] * self.G)
        if self.linsolve:
            if not np.all(np.isfinite(self.S)):
                raise ArithmeticError("S is not finite")
            self.K = self.A @ np.linalg.solve(self.S, self.A.T)
            return
        self.L = cholesky(self.S)
        if self.p:
            self.X = forward(self.L, self.A.T)
            self.Lk = cholesky(self.X.T @ self.X)

    def ksolve(self, x, y, z):
        z = self.di * z
        x = x + self.G.T @ (self.di * z)
        if self.linsolve:
            u = np.linalg.solve(self.S, x)
            y = np.linalg.solve(self.K, self.A @ u - y) if self.p else y
            x = np.linalg.solve(self.S, x - self.A.T @ y)
        else:
            x = forward(self.L, x)
            if self.p:
                y = backward(self.Lk, forward(self.Lk, self.X.T @ x - y))
                x = x - self.X @ y
            x = backward(self.L, x)
        return x, y, self.di * (self.G @ x) - z

    def stats(self):
        Pxq = self.P @ self.x + self.q
        self.rx = Pxq + self.A.T @ self.y + self.G.T @ self.z
        self.ry = self.A @ self.x - self.b
        self.rz = self.s + self.G @ self.x - self.h
        return tuple(float(v) for v in (self.x @ Pxq, self.x @ self.q, self.rx @ self.rx, self.ry @ self.ry, self.rz @ self.rz,
                                        self.y @ self.ry, self.z @ self.rz))

    def scaling(self):
        self.d = np.sqrt(self.s / self.z)
        self.di = 1.0 / self.d
        self.lmbda = np.sqrt(self.s * self.z)

    def direction(self, i, sigma_mu, eta, correction):
        ds = -self.lmbda ** 2 + sigma_mu                 # right-hand side (coneprog.py:2367-2390), then f4_no_ir (:2283-2313)
        if correction and i == 1:
            ds = ds - self.ws3
        ds = ds / self.lmbda
        self.dx, self.dy, dz = self.ksolve((-1.0 + eta) * self.rx, (-1.0 + eta) * self.ry, (-1.0 + eta) * self.rz - self.d * ds)
        ds = ds - dz
        dsdz = ds @ dz
        if correction and i == 0:
            self.ws3 = ds * dz
        self.ds, self.dz = ds / self.lmbda, dz / self.lmbda
        return float(dsdz), float(max(-self.ds)), float(max(-self.dz))

    def update(self, step):
        self.x = self.x + step * self.dx
        self.y = self.y + step * self.dy
        rs, rz = (np.sqrt((1.0 + step * v) * self.lmbda) for v in (self.ds, self.dz))       # misc.py:444-464
        self.d = self.d * rs / rz
        self.di = 1.0 / self.d
        self.lmbda = rs * rz
        self.s, self.z = self.d * self.lmbda, self.di * self.lmbda
        return float(self.lmbda @ self.lmbda)


def solve_member(P, q, G, h, A=None, b=None, options=None, dtype=np.float64, linsolve=False):
    """One member through the start and _ipm.coneqp_loop: a namespace with status, exit (the codes of kvxopt_amd.qpbatch),
    iterations, x, y, s, z and the statistics gap, relgap, pcost, dcost, pres, dres."""
    opt = _ipm.options(dict(QUIET, **(options or {})), {}, qp=True)
    ml = len(h)
    nrm = lambda v: float(np.sqrt(np.asarray(v, dtype=dtype) @ np.asarray(v, dtype=dtype)))     # noqa: E731
    try:
        e = QpEngine(P, q, G, h, A, b, dtype, linsolve)
        res0 = (max(1.0, nrm(q)), max(1.0, nrm(e.b)), max(1.0, nrm(h)))
        out = _ipm.coneqp_loop(e, opt, ml, float(e.s @ e.z), res0)
    except (ArithmeticError, ValueError, np.linalg.LinAlgError):                      # solvers.qp: ValueError("Rank(A) < p or ...")
        z = np.zeros
        return types.SimpleNamespace(status="unknown", exit=3, iterations=0, x=z(len(q)), y=z(0 if A is None else len(A)), s=z(ml),
                                     z=z(ml), stats=(np.nan,) * 6)
    code = 0 if out.status == "optimal" else (1 if out.msg == _ipm.MAXITERS_MSG else 2)
    stats = tuple(np.nan if v is None else float(v) for v in out.stats)
    return types.SimpleNamespace(status=out.status, exit=code, iterations=out.iterations, x=e.x, y=e.y, s=e.s, z=e.z, stats=stats)


def members(n, ml, p, B, seed):
    """B feasible members with per-member P (B, n, n), G (B, ml, n), A (B, p, n) and q (n x B), h (ml x B), b (p x B):
    P = F F' + 1e-2 I, h = G x0 + U(0.1, 1), b = A x0."""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((B, n, n))
    P = F @ F.transpose(0, 2, 1) + 1e-2 * np.eye(n)
    G = rng.standard_normal((B, ml, n))
    A = rng.standard_normal((B, p, n))
    x0 = rng.standard_normal((B, n, 1))
    h = (G @ x0)[:, :, 0] + rng.uniform(0.1, 1.0, (B, ml))
    b = (A @ x0)[:, :, 0]
    q = rng.standard_normal((B, n))
    return types.SimpleNamespace(n=n, ml=ml, p=p, B=B, P=P, q=np.asfortranarray(q.T), G=G, h=np.asfortranarray(h.T),
                                 A=A if p else None, b=np.asfortranarray(b.T) if p else None)


def grid_dense(p=0):
    """The data of the reference's runs G5 qp6x5 (p = 0) and G9 qpeq6x5p4 (p = 4) as dense arrays P, q, G, h, A, b."""
    Q = workloads.qp_grid(6, 5)
    n = Q["n"]

    def dense(m, cp, ri, v):
        D = np.zeros((m, n))
        D[ri, np.repeat(np.arange(n), np.diff(cp))] = v
        return D
    A = b = None
    if p:
        L = workloads.lp_grid_eq(6, 5, p)
        A, b = dense(p, L["Ap"], L["Ai"], L["Ax"]), L["b"]
    return dense(n, Q["Pp"], Q["Pi"], Q["Px"]), Q["q"], dense(Q["ml"], Q["Gp"], Q["Gi"], Q["Gx"]), Q["h"], A, b


def restate(M, options=None, dtype=np.float64, linsolve=False, which=None):
    """solve_member on every member (or those of `which`) of a batch from members()."""
    return [solve_member(M.P[k], M.q[:, k], M.G[k], M.h[:, k], None if M.A is None else M.A[k], None if M.b is None else M.b[:, k],
                         options, dtype, linsolve) for k in (range(M.B) if which is None else which)]


# ---- the batches of tests/test_qp_batch_gpu.py; tests/test_qp_batch_cpu.py checks that none of their counts sits on a rounding edge
SHAPES = [(1, 1, 0), (8, 17, 3), (33, 65, 5), (63, 255, 0), (64, 256, 1), (64, 257, 16), (64, 512, 64), (31, 300, 0)]
SHAPE_B = 12
SEEDS = {shape: 100 + k for k, shape in enumerate(SHAPES)}
INDEPENDENCE = ((16, 33, 2), 300, 7)                    # shape, B, seed
MIXED = ((8, 17, 3), 12, 14)


@functools.lru_cache(maxsize=None)
def batch(shape, B=SHAPE_B, seed=None):
    return members(*shape, B, SEEDS[shape] if seed is None else seed)


@functools.lru_cache(maxsize=None)
def restated(shape, B=SHAPE_B, seed=None, precision="longdouble", linsolve=False, correction=True):
    """The restated results of batch(shape, B, seed), computed once per process and left unchanged."""
    return restate(batch(shape, B, seed), {"use_correction": correction}, getattr(np, precision), linsolve)
