"""The restatement kvxopt_amd.conelpbatch is tested against: the engine of tests/lp_batch_numpy.py on the cone
K = R^ml_+ x Q^{q_0} x ... x S^{m_0}_+ x ... with the 'q' operations of tests/socp_batch_numpy.py and the 's' operations of
tests/sdp_batch_numpy.py, imported from there and strung together as kvxopt_amd.cone._ConeEngine strings them (coneprog.py:1308-1431),
and run through _ipm.conelp_start and _ipm.conelp_loop on one member at a time with refinement 0, in float64 or numpy.longdouble.

A vector of the cone has the 'l' rows, then the cones, then every 's' block as its full symmetric m x m matrix in column-major order;
G and h are symmetrised from their lower triangles once.  lmbda has Nd = ml + sum q_k + sum m_k entries: the 'l' and 'q' rows as they
are, then the diagonal of every block.  Every operation treats a kind of row by the expression its own restatement has for it, so
with dims['s'] = [] the engine is SocpEngine to the bit, with dims['q'] = [] SdpEngine, and with both empty LpEngine.  The KKT solve
is the one of lp_batch_numpy with Gs = W^-T G in place of diag(di) G.  Also the seeded generators of feasible, primal infeasible,
dual infeasible and free-variable members the tests use, and the cache of their restated results."""
import functools
import types

import numpy as np

import lp_batch_numpy as LPN
import sdp_batch_numpy as SDN
import socp_batch_numpy as SON
from kvxopt_amd import _ipm

QUIET = LPN.QUIET
EXITS = LPN.EXITS
Vec = LPN.Vec
mat, vec = SDN.mat, SDN.vec


class ConelpEngine(LPN.LpEngine):
    """LpEngine on R^ml_+ x Q^{q_0} x ... x S^{m_0}_+ x ...: d, di on the 'l' rows, v_k and beta_k per cone, r_k and rti_k per block,
    lmbda of length ml + sum q_k + sum m_k."""

    def __init__(self, c, G, h, dims, A=None, b=None, dtype=np.float64):
        super().__init__(c, G, h, A, b, dtype, False)
        t = dtype
        self.ml, self.q, self.sd = int(dims["l"]), [int(k) for k in dims["q"]], [int(k) for k in dims["s"]]
        self.off = SON.offsets(self.ml, self.q)
        self.Ms = self.off[-1]                               # the first 's' row
        self.blk = SDN.blocks(self.Ms, self.sd)
        self.N, self.Nd = self.Ms + sum(m * m for m in self.sd), self.Ms + sum(self.sd)
        assert self.N == len(self.h)
        if self.blk:                                         # only the lower triangles are read
            self.G, self.h = self.G.copy(), self.h.copy()
            for _, o, _, m in self.blk:
                self.h[o:o + m * m] = vec(SDN.symm(mat(self.h, o, m)))
                for j in range(self.G.shape[1]):
                    self.G[o:o + m * m, j] = vec(SDN.symm(mat(self.G[:, j], o, m)))
            self.hv = Vec(self.h)
        self.d = self.di = np.ones(self.ml, dtype=t)
        self.v = [np.concatenate([np.ones(1, dtype=t), np.zeros(m - 1, dtype=t)]) for m in self.q]
        self.beta = [t(1.0) for _ in self.q]
        self.r = [np.eye(m, dtype=t) for m in self.sd]
        self.rti = [np.eye(m, dtype=t) for m in self.sd]
        self.lmbda = Vec(np.zeros(self.Nd, dtype=t))

    def cones(self):
        return [(k, self.off[k], self.off[k + 1]) for k in range(len(self.q))]

    # ---- W, the Jordan algebra of the cone, and the KKT system
    def W(self, U, inverse=False, trans=False):
        """W U, W'U, W^-1 U or W^-T U for a vector or the columns of a matrix (W is symmetric on the 'l' and 'q' rows)."""
        d = self.di if inverse else self.d
        out = U.copy()
        out[:self.ml] = (d[:, None] if U.ndim == 2 else d) * U[:self.ml]
        for k, o, e in self.cones():
            out[o:e] = SON.scale_q(U[o:e], self.v[k], self.beta[k], inverse)
        for k, o, _, m in self.blk:
            R = self.rti[k] if inverse else self.r[k]
            out[o:o + m * m] = vec(SDN.congruence(R, mat(U, o, m), 1 if inverse != trans else 0))
        return out

    def blockwise(self, fl, fq, fs, x, *more):
        """fl on the 'l' rows, fq(k, ...) on every cone, fs(k, ...) on every block as a matrix; `more` in the layout of x."""
        out = x.copy()
        ml = self.ml
        out[:ml] = fl(x[:ml], *(u[:ml] for u in more))
        for k, o, e in self.cones():
            out[o:e] = fq(k, x[o:e], *(u[o:e] for u in more))
        for k, o, _, m in self.blk:
            out[o:o + m * m] = vec(fs(k, mat(x, o, m), *(mat(u, o, m) for u in more)))
        return out

    def lam(self, k):
        _, _, ol, m = self.blk[k]
        return self.lmbda.a[ol:ol + m]

    def expand(self, u):
        """The vector of the cone with u's 'l' and 'q' entries and diag(u_k) in every block, u of the length of lmbda."""
        out = np.zeros(self.N, dtype=self.t)
        out[:self.Ms] = u[:self.Ms]
        for _, o, ol, m in self.blk:
            out[o:o + m * m:m + 1] = u[ol:ol + m]
        return out

    def e(self, a):
        out = np.zeros(self.N, dtype=self.t)
        out[:self.ml] = a
        out[self.off[:-1]] = a
        for _, o, _, m in self.blk:
            out[o:o + m * m:m + 1] = a
        return out

    def sprod(self, x, y):
        return self.blockwise(lambda a, b: a * b, lambda k, a, b: SON.sprod_q(a, b), lambda k, X, Y: SDN.symm((Y @ X + X @ Y) / 2), x, y)

    def lam_sq(self):
        """lmbda o lmbda (sprod on the 'l' and 'q' rows, the squared diagonal on the blocks)."""
        lm = self.lmbda.a
        out = self.expand(lm * lm)
        for _, o, e in self.cones():
            out[o:e] = SON.sprod_q(lm[o:e], lm[o:e])
        return out

    def sinv(self, x):
        """lmbda o\\ x (misc_solvers.c:803-882)."""
        lm = self.lmbda.a
        return self.blockwise(lambda a: a / lm[:self.ml], lambda k, a: SON.sinv_q(a, lm[self.off[k]:self.off[k + 1]]),
                              lambda k, X: X / (np.add.outer(self.lam(k), self.lam(k)) / 2), x)

    def scale2(self, x, inverse=False):
        lm = self.lmbda.a

        def fs(k, X):
            c = np.multiply.outer(np.sqrt(self.lam(k)), np.sqrt(self.lam(k)))
            return X * c if inverse else X / c
        return self.blockwise(lambda a: a * lm[:self.ml] if inverse else a / lm[:self.ml],
                              lambda k, a: SON.scale2_q(lm[self.off[k]:self.off[k + 1]], a, inverse), fs, x)

    def factor(self):
        first, self.first = self.first, False
        Gs = self.W(self.G, True, True)
        try:
            self.L = self.lower(np.vstack([Gs, self.A]) if self.singular else Gs)
        except ArithmeticError:
            if not first or self.p == 0:
                raise
            self.singular = True
            self.L = self.lower(np.vstack([Gs, self.A]))
        if self.p:
            self.X = self.fwd(self.L, self.A.T)
            self.Lk = self.lower(self.X)

    def ksolve(self, x, y, z):
        z = self.W(z, True, True)
        x = x + self.G.T @ self.W(z, True)
        if self.singular:
            x = x + self.A.T @ y
        x = self.fwd(self.L, x)
        if self.p:
            y = self.bwd(self.Lk, self.fwd(self.Lk, self.X.T @ x - y))
            x = x - self.X @ y
        x = self.bwd(self.L, x)
        return x, y, self.W(self.G @ x, True, True) - z

    def eig(self, v):
        """Eigenvalues and eigenvectors of every block of v."""
        return [SDN.eigh(mat(v, o, m)) for _, o, _, m in self.blk]

    def max_step(self, v, eig=None):
        a = v.a if isinstance(v, Vec) else v
        t = [max(-a[:self.ml])] if self.ml else []
        t += [SON.max_step_q(a[o:e]) for _, o, e in self.cones()]
        return float(max(t + [-sig[0] for sig, _ in (self.eig(a) if eig is None else eig)]))

    def add_e(self, v, a):
        v.a += self.e(a)
        return v

    def scaling(self):
        ml, s, z, lm = self.ml, self.s.a, self.z.a, np.empty(self.Nd, dtype=self.t)
        self.d = np.sqrt(s[:ml] / z[:ml])
        self.di = 1.0 / self.d
        lm[:ml] = np.sqrt(s[:ml] * z[:ml])
        for k, o, e in self.cones():
            self.v[k], self.beta[k], lm[o:e] = SON.compute_scaling_q(s[o:e].copy(), z[o:e].copy())
        for k, o, ol, m in self.blk:
            self.r[k], self.rti[k], lm[ol:ol + m] = SDN.compute_scaling_s(mat(s, o, m), mat(z, o, m))
        self.lmbda.a = lm
        return float(lm @ lm)

    def direction(self, i, sigma, mu, rt, dg, dgi, lmbda_g, wkappa3):
        if i == 0:
            self.factor()
            self.x1, self.y1, self.z1 = (dgi * v for v in self.ksolve(-self.c, self.b, self.h))
            self.th = self.W(self.h, True, True)
        ds = self.lam_sq()
        dkappa = lmbda_g ** 2
        if i == 1:
            ds = ds + self.ws3 - self.e(sigma * mu)
            dkappa += wkappa3 - sigma * mu
        ds = -self.sinv(ds)
        dx, dy, dz = self.ksolve((1.0 - sigma) * self.rx.a, -((1.0 - sigma) * self.ry.a),
                                 -((1.0 - sigma) * self.rz.a + self.W(ds, False, True)))
        dkappa = -dkappa / lmbda_g
        dtau = float(dgi * ((1.0 - sigma) * rt + dkappa / dgi + self.c @ dx + self.b @ dy + self.th @ dz) / (1.0 + self.z1 @ self.z1))
        self.dx.a, self.dy.a, dz = dx + dtau * self.x1, dy + dtau * self.y1, dz + dtau * self.z1
        ds = ds - dz
        if i == 0:
            self.ws3 = self.sprod(ds, dz)
        self.dtau, self.dkappa, self.ds, self.dz = dtau, dkappa - dtau, self.scale2(ds), self.scale2(dz)
        self.eigs, self.eigz = self.eig(self.ds), self.eig(self.dz)          # the update consumes them (coneprog.py:1308-1321)

    def bounds(self, i):
        return self.dtau, self.dkappa, self.max_step(self.ds, self.eigs), self.max_step(self.dz, self.eigz)

    def update(self, step, tau):
        ml, lm = self.ml, self.lmbda.a
        self.x.a = self.x.a + step * self.dx.a
        self.y.a = self.y.a + step * self.dy.a
        # the 'l' and 'q' rows of the new iterates in the current scaling: scale2 with inverse 'I' of e + step ds (coneprog.py:1336-1354)
        s, z = (self.scale2(self.e(1.0) + step * v, True) for v in (self.ds, self.dz))
        new = np.empty_like(lm)
        rs, rz = np.sqrt(s[:ml]), np.sqrt(z[:ml])                                   # misc.py:444-464
        self.d = self.d * rs / rz
        self.di = 1.0 / self.d
        new[:ml] = rs * rz
        for k, o, e in self.cones():                                               # misc.py:467-580
            _, _, self.v[k], self.beta[k], new[o:e] = SON.update_scaling_q(self.v[k], self.beta[k], s[o:e], z[o:e])
        for k, o, ol, m in self.blk:                                               # coneprog.py:1356-1395
            lk = self.lam(k)
            c = np.multiply.outer(np.sqrt(lk), np.sqrt(lk))
            Ls, Lz = ((Qm * c) * np.sqrt((1.0 + step * sig) / lk) for sig, Qm in (self.eigs[k], self.eigz[k]))
            self.r[k], self.rti[k], new[ol:ol + m] = SDN.update_scaling_s(self.r[k], self.rti[k], Ls, Lz)
        self.lmbda.a = new
        self.s.a, self.z.a = self.W(self.expand(new), False, True), self.W(self.expand(new), True)


def solve_member(c, G, h, dims, A=None, b=None, options=None, dtype=np.float64):
    """One member through _ipm.conelp_start and _ipm.conelp_loop with refinement 0: the namespace of lp_batch_numpy.solve_member,
    'primal slack' and 'dual slack' as -max_step over the whole cone.  A Cholesky factor of s_k or z_k that fails in the scaling of
    the first iteration ends the member as a failed first factorisation does."""
    opt = _ipm.options(dict(QUIET, refinement=0, **(options or {})), dims)
    n, N, p = len(c), len(h), 0 if A is None else len(A)
    e = ConelpEngine(c, G, h, dims, A, b, dtype)
    res0 = tuple(max(1.0, v.nrm2()) for v in (e.cv, e.bv, e.hv))
    failed = False
    try:
        out = _ipm.conelp_start(e, opt, None, None, res0)
        if not isinstance(out, _ipm.Outcome):
            out = _ipm.conelp_loop(e, opt, e.Nd, out, res0)       # coneprog.py:1248: mu = (|lmbda|^2 + lmbda_g^2) / (1 + cdim_diag)
        failed = out.msg == _ipm.SINGULAR_MSG and out.iterations == 0
    except (ValueError, ArithmeticError, np.linalg.LinAlgError):
        failed = True
    if failed:
        z = np.zeros
        return types.SimpleNamespace(status="unknown", exit=3, iterations=0, x=z(n), y=z(p), s=z(N), z=z(N), stats=(np.nan,) * 10,
                                     singular=e.singular)
    code = EXITS.get(out.status, 1 if out.msg == _ipm.MAXITERS_MSG else 2)
    xs, zs = out.status != "primal infeasible", out.status != "dual infeasible"
    nan = lambda v: np.full(len(v.a), np.nan)                                            # noqa: E731
    slacks = (-e.max_step(e.s) if xs else None, -e.max_step(e.z) if zs else None)
    stats = tuple(np.nan if v is None else float(v) for v in out.stats[:6] + slacks + out.stats[6:])
    return types.SimpleNamespace(status=out.status, exit=code, iterations=out.iterations, x=e.x.a if xs else nan(e.x),
                                 y=e.y.a if zs else nan(e.y), s=e.s.a if xs else nan(e.s), z=e.z.a if zs else nan(e.z), stats=stats,
                                 singular=e.singular)


FEASIBLE, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE = LPN.FEASIBLE, LPN.PRIMAL_INFEASIBLE, LPN.DUAL_INFEASIBLE


def interior(ml, q, s, rng):
    """A point of the interior of K, as _interior of tests/golden/make_goldens_cones.py draws it: the 'l' rows and the cones as
    socp_batch_numpy.interior draws them, then the blocks as sdp_batch_numpy.interior does."""
    parts = [SON.interior(ml, q, rng)]
    for m in s:
        M = rng.standard_normal((m, m))
        parts.append(vec(M @ M.T / m + (0.5 + rng.random()) * np.eye(m)))
    return np.concatenate(parts)


def members(n, ml, q, s, p, B, seed, kinds=(FEASIBLE,), free=0):
    """B members with per-member G (B, N, n), A (B, p, n) and c (n x B), h (N x B), b (p x B), member k of kind kinds[k % len(kinds)],
    on the feasible construction of _feasible in tests/golden/make_goldens_cones.py (dense G with symmetric 's' blocks and 1 added to
    its diagonal, h = G x0 + s0, b = A x0, c = -G'z0 - A'y0 with s0, z0 interior to the whole cone):
      primal infeasible  with ml >= 2, rows 0 and 1 replaced by g'x <= -1 and -g'x <= -1; otherwise row ml, the head of the first cone
                         or the (0, 0) entry of the first block, becomes 0'x + s = -1, which no s of that cone or block meets
      dual infeasible    d in the null space of A, G := G + (u - G d) d'/d'd with -u interior to K so that -G d is in K,
                         h = G x1 + s0 with A x1 = b, and c = -d + 0.1 w with w orthogonal to d: feasible and unbounded along d
    free: the last `free` <= p columns of G are exactly zero, and h = G x1 + s0 with A x1 = b.
    With q or s empty the draws are those of sdp_batch_numpy.members or socp_batch_numpy.members at the same seed."""
    rng = np.random.default_rng(seed)
    q, s = list(q), list(s)
    Ms = ml + sum(q)
    N = Ms + sum(m * m for m in s)
    assert free <= p
    G = rng.standard_normal((B, N, n))
    k = np.arange(min(N, n))
    G[:, k, k] += 1.0
    for k in range(B):
        SDN.symmetrise(G[k], Ms, s)
    A = rng.standard_normal((B, p, n))
    c, h, b = np.zeros((n, B)), np.zeros((N, B)), np.zeros((p, B))
    kind = [kinds[k % len(kinds)] for k in range(B)]
    for k in range(B):
        x0, y0 = rng.standard_normal(n), rng.standard_normal(p)
        s0, z0 = interior(ml, q, s, rng), interior(ml, q, s, rng)
        b[:, k] = A[k] @ x0
        if free:
            G[k, :, n - free:] = 0.0
            x0 = np.linalg.lstsq(A[k], b[:, k], rcond=None)[0]
        h[:, k] = G[k] @ x0 + s0
        c[:, k] = -G[k].T @ z0 - A[k].T @ y0                 # full symmetric blocks: sgemv's G'z
        if kind[k] == PRIMAL_INFEASIBLE:
            if ml >= 2:
                g = rng.standard_normal(n)
                g[n - free:] = 0.0
                G[k, 0], G[k, 1] = g, -g
                h[0, k] = h[1, k] = -1.0
            else:
                G[k, ml] = 0.0
                h[ml, k] = -1.0
        elif kind[k] == DUAL_INFEASIBLE:
            null = np.linalg.svd(A[k])[2][p:].T if p else np.eye(n)
            d = null @ rng.standard_normal(null.shape[1])
            u = -interior(ml, q, s, rng)
            G[k] += np.outer(u - G[k] @ d, d) / (d @ d)
            x1 = np.linalg.lstsq(A[k], b[:, k], rcond=None)[0] if p else np.zeros(n)
            h[:, k] = G[k] @ x1 + s0
            w = rng.standard_normal(n)
            w -= d * (w @ d) / (d @ d)
            c[:, k] = -d + 0.1 * w
    return types.SimpleNamespace(n=n, ml=ml, q=q, s=s, dims={"l": ml, "q": q, "s": s}, Ms=Ms, N=N, Nd=Ms + sum(s), p=p, B=B,
                                 c=np.asfortranarray(c), G=G, h=np.asfortranarray(h), A=A if p else None,
                                 b=np.asfortranarray(b) if p else None, kind=kind)


def member(M, k):
    """(c, G, h, dims, A, b) of member k."""
    return M.c[:, k], M.G[k], M.h[:, k], M.dims, None if M.A is None else M.A[k], None if M.b is None else M.b[:, k]


def restate(M, options=None, dtype=np.float64, which=None):
    """solve_member on every member (or those of `which`) of a batch from members()."""
    return [solve_member(*member(M, k), options, dtype) for k in (range(M.B) if which is None else which)]


# ---- the batches of tests/test_conelp_batch_gpu.py; tests/test_conelp_batch_cpu.py checks that float64 and longdouble agree on each.
# A shape is (n, ml, q, s, p).  CORNER: n = p = 64 with an order-16 block and a cone of 100 rows, 148368 bytes of LDS, 4272 below
# the largest member of the box.
CORNER = (64, 28, (100,), (16,), 64)
SHAPES = [(2, 0, (1,), (1,), 0), (8, 0, (3, 4), (2, 3), 2), (16, 30, (5,), (3,), 2), (12, 3, (2,) * 6, (1, 2, 3), 2),
          (20, 3, (65,), (16,), 3), (24, 0, (2,) * 64, (3,) * 16, 4), CORNER]
SHAPE_B = 12
THIRDS = (FEASIBLE, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE)
EDGE = (8, 3, (4,), (3,), 2)
NO_QS, NO_S, NO_Q = (8, 17, (), (), 3), (8, 5, (1, 2, 7), (), 3), (6, 2, (), (1, 2, 3), 2)


def _part(tag, v):
    return tag + ("%dx%d" % (len(v), v[0]) if len(v) > 1 and len(set(v)) == 1 else "_".join(map(str, v)))


def shape_name(shape):
    n, ml, q, s, p = shape
    return "shape-%d-%d-%s-%s-%d" % (n, ml, _part("q", q), _part("s", s), p)


# At (2, 0, [1], [1], 0) G is square, so the starting point is the vertex G^-1 h itself and s = h - G x is a rounding error whose sign
# decides between "optimal at iteration 0" and four iterations, in every arithmetic for itself.  float64 and longdouble agree on that
# for all twelve members at 96 of the seeds 1 .. 99999, and the kernel, whose fused multiply-adds make it a third arithmetic, agrees
# with both at ten of those (its counts for all these seeds were recorded once and intersected with the two restatements):
# 7457 is the first; eight of its members take the loop and four end at iteration 0.
# Two more seeds were changed, never a bound: "independence" (761 -> 777: at 761 member 146 differs by 2.5e-2 of the bound between
# float64 and longdouble and member 260 ends with a singular KKT matrix after 8 iterations in float64) and "mixed" (771 -> 835, the
# first seed at which the unspoiled members end with every exit at the median count and both precisions agree on the cut-off runs).
SEEDS = dict(zip(SHAPES, (7457, 702, 703, 704, 705, 706, 707)))
# name -> (shape, B, seed, kinds, free)
BATCHES = {shape_name(s): (s, SHAPE_B, SEEDS[s], (FEASIBLE,), 0) for s in SHAPES}
BATCHES.update({
    "absent-qs": (NO_QS, 12, 721, (FEASIBLE,), 0),
    "absent-s": (NO_S, 12, 722, (FEASIBLE,), 0),
    "absent-q": (NO_Q, 12, 723, (FEASIBLE,), 0),
    "certificates": (EDGE, 12, 731, THIRDS, 0),
    "free": (EDGE, 12, 751, (FEASIBLE,), 2),
    "independence": (EDGE, 300, 777, (FEASIBLE,), 0),
    "mixed": (EDGE, 12, 835, (FEASIBLE, FEASIBLE, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE), 0),
})
MIXED_CHANGED = (0, 4, 8)    # the members of "mixed" the GPU test spoils (feasible ones): an 's' block of h whose Frobenius norm
#                              overflows, a variable nothing holds, a NaN in c
SMALL_BATCHES = sorted(k for k in BATCHES if k != "independence")


@functools.lru_cache(maxsize=None)
def batch(name):
    (n, ml, q, s, p), B, seed, kinds, free = BATCHES[name]
    return members(n, ml, q, s, p, B, seed, kinds, free)


@functools.lru_cache(maxsize=None)
def restated(name, precision="longdouble"):
    """The restated results of batch(name), computed once per process and left unchanged."""
    return restate(batch(name), None, getattr(np, precision))
