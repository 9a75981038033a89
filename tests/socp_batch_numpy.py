"""The restatement kvxopt_amd.socpbatch is tested against: the engine of tests/lp_batch_numpy.py extended by the 'q' operations of the
Nesterov-Todd scaling -- misc.compute_scaling / update_scaling (misc.py:290-352, 467-580), misc_solvers.scale, scale2, sprod, sinv
(misc_solvers.c:144-186, 301-341, 671-700, 803-835) and max_step (misc_solvers.c:1073-1085) -- strung together as
kvxopt_amd.cone._ConeEngine strings them, and run through _ipm.conelp_start and _ipm.conelp_loop on one member at a time with
refinement 0, in float64 or numpy.longdouble.  The KKT solve is the one of lp_batch_numpy with Gs = W^-T G in place of diag(di) G:
S = Gs'Gs = L L', X = L^-1 A', K = X'X, and kkt_chol2's F['singular'] repair.  Also the seeded generators of feasible, primal
infeasible, dual infeasible and free-variable members the tests use, and the cache of their restated results."""
import functools
import types

import numpy as np

import lp_batch_numpy as LPN
from kvxopt_amd import _ipm

QUIET = LPN.QUIET
EXITS = LPN.EXITS
Vec = LPN.Vec


def offsets(ml, q):
    """The first row of every cone and, last, N."""
    return [ml + int(sum(q[:k])) for k in range(len(q) + 1)]


# ---- the 'q' operations on one cone; U may be a vector or a matrix whose columns are vectors of the cone
def jnrm2(x):
    a = np.sqrt(x[1:] @ x[1:])
    return np.sqrt(x[0] - a) * np.sqrt(x[0] + a)


def scale_q(U, v, beta, inverse=False):
    """beta (2 v v' - J) U, or its inverse (1 / beta) (2 J v v' J - J) U (misc_solvers.c:144-186); W is symmetric."""
    U = U.copy()
    if inverse:
        U[0] *= -1.0
    w = v @ U
    U[0] *= -1.0
    U += 2.0 * np.multiply.outer(v, w)
    if inverse:
        U[0] *= -1.0
        return U / beta
    return U * beta


def sprod_q(x, y):
    out = y[0] * x + x[0] * y
    out[0] = x @ y
    return out


def sinv_q(x, y):
    """y o\\ x (misc_solvers.c:803-835)."""
    a = np.sqrt(y[1:] @ y[1:])
    a = (y[0] + a) * (y[0] - a)
    c, d = x[0], x[1:] @ y[1:]
    out = x.copy()
    out[0] = c * y[0] - d
    out[1:] *= a / y[0]
    out[1:] += (d / y[0] - c) * y[1:]
    return out * (1.0 / a)


def scale2_q(lm, x, inverse=False):
    a = np.sqrt(lm[1:] @ lm[1:])
    a = np.sqrt(lm[0] + a) * np.sqrt(lm[0] - a)
    lx = (lm @ x if inverse else lm[0] * x[0] - lm[1:] @ x[1:]) / a
    out = x.copy()
    out[0] = lx
    b = (x[0] + lx) / (lm[0] / a + 1.0) / a
    out[1:] += (b if inverse else -b) * lm[1:]
    return out * (a if inverse else 1.0 / a)


def max_step_q(x):
    return np.sqrt(x[1:] @ x[1:]) - x[0]


def compute_scaling_q(s, z):
    aa, bb = jnrm2(s), jnrm2(z)
    cc = np.sqrt((s @ z / aa / bb + 1.0) / 2.0)
    v = -z / bb
    v[0] *= -1.0
    v += s / aa
    v *= 1.0 / 2.0 / cc
    v[0] += 1.0
    v *= 1.0 / np.sqrt(2.0 * v[0])
    lm = np.empty_like(s)
    lm[0] = cc
    dd = 2 * cc + s[0] / aa + z[0] / bb
    lm[1:] = (cc + z[0] / bb) / dd / aa * s[1:] + (cc + s[0] / aa) / dd / bb * z[1:]
    lm *= np.sqrt(aa * bb)
    return v, np.sqrt(aa / bb), lm


def update_scaling_q(v, beta, s, z):
    aa, bb = jnrm2(s), jnrm2(z)
    s = s * (1.0 / aa)
    z = z * (1.0 / bb)
    cc = np.sqrt((1.0 + s @ z) / 2.0)
    vs = v @ s
    vz = v[0] * z[0] - v[1:] @ z[1:]
    vq = (vs + vz) / 2.0 / cc
    vu = vs - vz
    wk0 = 2 * v[0] * vq - (s[0] + z[0]) / 2.0 / cc
    dd = (v[0] * vu - s[0] / 2.0 + z[0] / 2.0) / (wk0 + 1.0)
    lm = np.empty_like(s)
    lm[0] = cc
    lm[1:] = v[1:] * (2.0 * (-dd * vq + 0.5 * vu)) + (0.5 * (1.0 - dd / cc)) * s[1:] + (0.5 * (1.0 + dd / cc)) * z[1:]
    lm *= np.sqrt(aa * bb)
    w = v * (2.0 * vq)
    w[0] -= s[0] / 2.0 / cc
    w[1:] += (0.5 / cc) * s[1:]
    w += (-0.5 / cc) * z
    w[0] += 1.0
    w *= 1.0 / np.sqrt(2.0 * w[0])
    return s, z, w, beta * np.sqrt(aa / bb), lm


class SocpEngine(LPN.LpEngine):
    """LpEngine on R^ml_+ x Q^{q_0} x ...: d, di on the 'l' rows, v_k and beta_k per cone."""

    def __init__(self, c, G, h, dims, A=None, b=None, dtype=np.float64):
        super().__init__(c, G, h, A, b, dtype, False)
        t = dtype
        self.ml, self.q = int(dims["l"]), [int(k) for k in dims["q"]]
        self.off = offsets(self.ml, self.q)
        assert self.off[-1] == len(self.h)
        self.d = self.di = np.ones(self.ml, dtype=t)
        self.v = [np.concatenate([np.ones(1, dtype=t), np.zeros(m - 1, dtype=t)]) for m in self.q]
        self.beta = [t(1.0) for _ in self.q]

    def cones(self):
        return [(k, self.off[k], self.off[k + 1]) for k in range(len(self.q))]

    # ---- W, the Jordan algebra of the cone, and the KKT system
    def W(self, U, inverse=False):
        """W U or W^-1 U (W is symmetric on 'l' and 'q' rows)."""
        d = self.di if inverse else self.d
        out = U.copy()
        out[:self.ml] = (d[:, None] if U.ndim == 2 else d) * U[:self.ml]
        for k, o, e in self.cones():
            out[o:e] = scale_q(U[o:e], self.v[k], self.beta[k], inverse)
        return out

    def blockwise(self, fl, fq, x, *more):
        out = x.copy()
        ml = self.ml
        out[:ml] = fl(x[:ml], *(u[:ml] for u in more))
        for k, o, e in self.cones():
            out[o:e] = fq(x[o:e], *(u[o:e] for u in more))
        return out

    def sprod(self, x, y):
        return self.blockwise(lambda a, b: a * b, sprod_q, x, y)

    def sinv(self, x, y):
        return self.blockwise(lambda a, b: a / b, sinv_q, x, y)

    def scale2(self, lm, x, inverse=False):
        return self.blockwise(lambda a, l: a * l if inverse else a / l, lambda a, l: scale2_q(l, a, inverse), x, lm)

    def e(self, a):
        out = np.zeros(self.off[-1], dtype=self.t)
        out[:self.ml] = a
        out[self.off[:-1]] = a
        return out

    def factor(self):
        first, self.first = self.first, False
        Gs = self.W(self.G, True)
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
        z = self.W(z, True)
        x = x + self.G.T @ self.W(z, True)
        if self.singular:
            x = x + self.A.T @ y
        x = self.fwd(self.L, x)
        if self.p:
            y = self.bwd(self.Lk, self.fwd(self.Lk, self.X.T @ x - y))
            x = x - self.X @ y
        x = self.bwd(self.L, x)
        return x, y, self.W(self.G @ x, True) - z

    def max_step(self, v):
        a = v.a if isinstance(v, Vec) else v
        t = [max(-a[:self.ml])] if self.ml else []
        return float(max(t + [max_step_q(a[o:e]) for _, o, e in self.cones()]))

    def add_e(self, v, a):
        v.a += self.e(a)
        return v

    def scaling(self):
        ml, s, z, lm = self.ml, self.s.a, self.z.a, np.empty_like(self.s.a)
        self.d = np.sqrt(s[:ml] / z[:ml])
        self.di = 1.0 / self.d
        lm[:ml] = np.sqrt(s[:ml] * z[:ml])
        for k, o, e in self.cones():
            self.v[k], self.beta[k], lm[o:e] = compute_scaling_q(s[o:e].copy(), z[o:e].copy())
        self.lmbda.a = lm
        return float(lm @ lm)

    def direction(self, i, sigma, mu, rt, dg, dgi, lmbda_g, wkappa3):
        lm = self.lmbda.a
        if i == 0:
            self.factor()
            self.x1, self.y1, self.z1 = (dgi * v for v in self.ksolve(-self.c, self.b, self.h))
            self.th = self.W(self.h, True)
        ds = self.sprod(lm, lm)
        dkappa = lmbda_g ** 2
        if i == 1:
            ds = ds + self.ws3 - self.e(sigma * mu)
            dkappa += wkappa3 - sigma * mu
        ds = -self.sinv(ds, lm)
        dx, dy, dz = self.ksolve((1.0 - sigma) * self.rx.a, -((1.0 - sigma) * self.ry.a), -((1.0 - sigma) * self.rz.a + self.W(ds)))
        dkappa = -dkappa / lmbda_g
        dtau = float(dgi * ((1.0 - sigma) * rt + dkappa / dgi + self.c @ dx + self.b @ dy + self.th @ dz) / (1.0 + self.z1 @ self.z1))
        self.dx.a, self.dy.a, dz = dx + dtau * self.x1, dy + dtau * self.y1, dz + dtau * self.z1
        ds = ds - dz
        if i == 0:
            self.ws3 = self.sprod(ds, dz)
        self.dtau, self.dkappa, self.ds, self.dz = dtau, dkappa - dtau, self.scale2(lm, ds), self.scale2(lm, dz)

    def bounds(self, i):
        return self.dtau, self.dkappa, self.max_step(self.ds), self.max_step(self.dz)

    def update(self, step, tau):
        ml, lm = self.ml, self.lmbda.a
        self.x.a = self.x.a + step * self.dx.a
        self.y.a = self.y.a + step * self.dy.a
        s, z = (self.scale2(lm, self.e(1.0) + step * v, True) for v in (self.ds, self.dz))
        new = np.empty_like(lm)
        rs, rz = np.sqrt(s[:ml]), np.sqrt(z[:ml])                                   # misc.py:444-464
        self.d = self.d * rs / rz
        self.di = 1.0 / self.d
        new[:ml] = rs * rz
        for k, o, e in self.cones():
            _, _, self.v[k], self.beta[k], new[o:e] = update_scaling_q(self.v[k], self.beta[k], s[o:e], z[o:e])
        self.lmbda.a = new
        self.s.a, self.z.a = self.W(new), self.W(new, True)


def solve_member(c, G, h, dims, A=None, b=None, options=None, dtype=np.float64):
    """One member through _ipm.conelp_start and _ipm.conelp_loop with refinement 0: the namespace of lp_batch_numpy.solve_member,
    'primal slack' and 'dual slack' as -max_step over the whole cone."""
    opt = _ipm.options(dict(QUIET, refinement=0, **(options or {})), dims)
    n, N, p = len(c), len(h), 0 if A is None else len(A)
    e = SocpEngine(c, G, h, dims, A, b, dtype)
    res0 = tuple(max(1.0, v.nrm2()) for v in (e.cv, e.bv, e.hv))
    failed = False
    try:
        out = _ipm.conelp_start(e, opt, None, None, res0)
        if not isinstance(out, _ipm.Outcome):
            out = _ipm.conelp_loop(e, opt, N, out, res0)          # coneprog.py:1248: mu = |lmbda|^2 / (1 + cdim_diag)
        failed = out.msg == _ipm.SINGULAR_MSG and out.iterations == 0
    except (ValueError, np.linalg.LinAlgError):
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


def interior(ml, q, rng):
    """A point of the interior of K, as _interior of tests/golden/make_goldens_cones.py draws it."""
    parts = [rng.uniform(0.5, 1.5, ml)]
    for m in q:
        u = rng.standard_normal(m - 1)
        parts.append(np.concatenate([[np.linalg.norm(u) + 0.5 + rng.random()], u]))
    return np.concatenate(parts)


def members(n, ml, q, p, B, seed, kinds=(FEASIBLE,), free=0):
    """B members with per-member G (B, N, n), A (B, p, n) and c (n x B), h (N x B), b (p x B), member k of kind kinds[k % len(kinds)],
    on the feasible construction of _feasible in tests/golden/make_goldens_cones.py (dense G with 1 added to its diagonal,
    h = G x0 + s0, b = A x0, c = -G'z0 - A'y0 with s0, z0 interior to K):
      primal infeasible  with ml >= 2, rows 0 and 1 replaced by g'x <= -1 and -g'x <= -1; otherwise the head row of the first cone
                         becomes 0'x + s = -1, which no s of that cone meets
      dual infeasible    d in the null space of A, G := G + (u - G d) d'/d'd with -u interior to K so that -G d is in K,
                         h = G x1 + s0 with A x1 = b, and c = -d + 0.1 w with w orthogonal to d: feasible and unbounded along d
    free: the last `free` <= p columns of G are exactly zero, and h = G x1 + s0 with A x1 = b."""
    rng = np.random.default_rng(seed)
    q = list(q)
    N = ml + sum(q)
    assert free <= p
    G = rng.standard_normal((B, N, n))
    k = np.arange(min(N, n))
    G[:, k, k] += 1.0
    A = rng.standard_normal((B, p, n))
    c, h, b = np.zeros((n, B)), np.zeros((N, B)), np.zeros((p, B))
    kind = [kinds[k % len(kinds)] for k in range(B)]
    for k in range(B):
        x0, y0 = rng.standard_normal(n), rng.standard_normal(p)
        s0, z0 = interior(ml, q, rng), interior(ml, q, rng)
        b[:, k] = A[k] @ x0
        if free:
            G[k, :, n - free:] = 0.0
            x0 = np.linalg.lstsq(A[k], b[:, k], rcond=None)[0]
        h[:, k] = G[k] @ x0 + s0
        c[:, k] = -G[k].T @ z0 - A[k].T @ y0
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
            u = -interior(ml, q, rng)
            G[k] += np.outer(u - G[k] @ d, d) / (d @ d)
            x1 = np.linalg.lstsq(A[k], b[:, k], rcond=None)[0] if p else np.zeros(n)
            h[:, k] = G[k] @ x1 + s0
            w = rng.standard_normal(n)
            w -= d * (w @ d) / (d @ d)
            c[:, k] = -d + 0.1 * w
    return types.SimpleNamespace(n=n, ml=ml, q=q, dims={"l": ml, "q": q, "s": []}, N=N, p=p, B=B, c=np.asfortranarray(c), G=G,
                                 h=np.asfortranarray(h), A=A if p else None, b=np.asfortranarray(b) if p else None, kind=kind)


def member(M, k):
    """(c, G, h, dims, A, b) of member k."""
    return M.c[:, k], M.G[k], M.h[:, k], M.dims, None if M.A is None else M.A[k], None if M.b is None else M.b[:, k]


def restate(M, options=None, dtype=np.float64, which=None):
    """solve_member on every member (or those of `which`) of a batch from members()."""
    return [solve_member(*member(M, k), options, dtype) for k in (range(M.B) if which is None else which)]


# ---- the batches of tests/test_socp_batch_gpu.py; tests/test_socp_batch_cpu.py checks that float64 and longdouble agree on each
SHAPES = [(1, 0, (1,), 0), (2, 0, (2,), 0), (3, 0, (3, 4), 0), (8, 5, (1, 2, 7), 3), (16, 31, (3,), 2), (16, 0, (33,), 0),
          (16, 0, (65,), 1), (33, 30, (64, 64), 5), (64, 0, (512,), 0), (64, 0, (4,) * 128, 16), (64, 256, (128, 128), 64)]
SHAPE_B = 12
THIRDS = (FEASIBLE, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE)
EDGE = (8, 5, (1, 2, 7), 3)


def shape_name(s):
    n, ml, q, p = s
    return "shape-%d-%d-%s-%d" % (n, ml, "q%dx%d" % (len(q), q[0]) if len(set(q)) == 1 else "q" + "_".join(map(str, q)), p)


SEEDS = dict(zip(SHAPES, (6, 8115, 303, 304, 305, 306, 307, 308, 309, 412, 311)))
# At (1, 0, [1], 0) and (2, 0, [2], 0) G is square, so the starting point is the vertex G^-1 h itself and s = h - G x is a rounding
# error; whether it lies in the cone decides between "optimal at iteration 0" and four iterations, in every arithmetic for itself.
# 6 is the first seed of 1, 2, ... at which float64 and longdouble agree on that for all twelve members of (1, 0, [1], 0); the
# kernel, whose fused multiply-adds make it a third arithmetic, agrees there too.  At (2, 0, [2], 0) float64 and longdouble first
# agree at 814, but the kernel rounds seven of those members the other way; 8115 is the first seed at which all three agree
# (the kernel's counts for the seeds 1 .. 44000 were recorded once and intersected with the two restatements).
# name -> (shape, B, seed, kinds, free)
BATCHES = {shape_name(s): (s, SHAPE_B, SEEDS[s], (FEASIBLE,), 0) for s in SHAPES}
BATCHES.update({
    "certificates-8": (EDGE, 12, 331, THIRDS, 0),
    "certificates-16": ((16, 0, (33,), 0), 12, 332, THIRDS, 0),
    "orthant": ((8, 17, (), 3), 12, 341, (FEASIBLE,), 0),
    "free": (EDGE, 12, 351, (FEASIBLE,), 2),
    "independence": (EDGE, 300, 361, (FEASIBLE,), 0),
    "mixed": (EDGE, 12, 386, (FEASIBLE, FEASIBLE, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE), 0),
})
MIXED_CHANGED = (4, 8)       # the members of "mixed" the GPU test spoils: a variable nothing holds, a NaN in c (both are feasible ones)
SMALL_BATCHES = sorted(k for k in BATCHES if k != "independence")


@functools.lru_cache(maxsize=None)
def batch(name):
    (n, ml, q, p), B, seed, kinds, free = BATCHES[name]
    return members(n, ml, q, p, B, seed, kinds, free)


@functools.lru_cache(maxsize=None)
def restated(name, precision="longdouble"):
    """The restated results of batch(name), computed once per process and left unchanged."""
    return restate(batch(name), None, getattr(np, precision))
