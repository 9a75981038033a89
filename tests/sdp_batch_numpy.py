"""The restatement kvxopt_amd.sdpbatch is tested against: the engine of tests/lp_batch_numpy.py extended by the 's' operations of the
Nesterov-Todd scaling -- misc.compute_scaling / update_scaling (misc.py:354-419, 582-634), misc_solvers.scale, scale2, sprod, sinv,
sdot and max_step (misc_solvers.c:188-240, 343-397, 700-770, 845-882, 1029-1046, 1086-1160) -- strung together as
kvxopt_amd.cone._ConeEngine strings them (coneprog.py:1308-1431), and run through _ipm.conelp_start and _ipm.conelp_loop on one
member at a time with refinement 0, in float64 or numpy.longdouble.  numpy.linalg carries no longdouble, so the Cholesky factor is the
explicit one of tests/qp_batch_numpy.py and the singular values and symmetric eigenvalues come from the one-sided Jacobi below, in
the round-robin order of csrc/kkt_s.hip, written in the working dtype.

Vectors of the cone hold every 's' block as its full symmetric m x m matrix in column-major order; G and h are symmetrised from their
lower triangles once, so G'z is misc.sgemv's product and the cone's inner product is the plain one.  The KKT solve is the one of
lp_batch_numpy with Gs = W^-T G in place of diag(di) G.  Also the seeded generators of feasible, primal infeasible, dual infeasible
and free-variable members the tests use, and the cache of their restated results."""
import functools
import types

import numpy as np

import lp_batch_numpy as LPN
import qp_batch_numpy as Q
from kvxopt_amd import _ipm

QUIET = LPN.QUIET
EXITS = LPN.EXITS
Vec = LPN.Vec
SWEEPS = 60


def blocks(ml, s):
    """(k, first row of block k in a vector of the cone, first entry of lmbda_k, m_k) for every 's' block."""
    out, o, ol = [], ml, ml
    for k, m in enumerate(s):
        out.append((k, o, ol, m))
        o += m * m
        ol += m
    return out


def mat(x, o, m):
    """Block at o of the vector (or of every column of the matrix) x as m x m [x columns]."""
    return x[o:o + m * m].reshape((m, m) + x.shape[1:], order="F")


def vec(X):
    return X.reshape((-1,) + X.shape[2:], order="F")


def symm(X):
    """The symmetric matrix of the lower triangle of X."""
    return np.tril(X) + np.tril(X, -1).T


# ---- one-sided Jacobi (Hestenes) in the round-robin order of csrc/kkt_s.hip: on return A V with mutually orthogonal columns, and V
def jacobi(A):
    A = A.copy()
    m = len(A)
    t = A.dtype.type
    V = np.eye(m, dtype=A.dtype)
    if m < 2:
        return A, V
    n = m + (m & 1)
    tol = np.finfo(A.dtype).eps * np.sqrt(t(m))
    for _ in range(SWEEPS):
        rotated = False
        for r in range(n - 1):
            for pk in range(n // 2):
                p, q = (n - 1, r) if pk == 0 else ((r + pk) % (n - 1), (r - pk + n - 1) % (n - 1))
                if p > q:
                    p, q = q, p
                if q >= m:
                    continue
                x, y = A[:, p].copy(), A[:, q].copy()
                al, be, ga = x @ x, y @ y, x @ y
                if abs(ga) <= tol * np.sqrt(al * be) or ga == 0 or not np.isfinite(ga):
                    continue
                zeta = (be - al) / (2 * ga)
                tn = (t(1) if zeta >= 0 else t(-1)) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
                c = 1 / np.sqrt(1 + tn * tn)
                s = c * tn
                A[:, p], A[:, q] = c * x - s * y, s * x + c * y
                x, y = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * x - s * y, s * x + c * y
                rotated = True
        if not rotated:
            break
    return A, V


def _ranks(nrm, descending):
    key = -nrm if descending else nrm
    return np.argsort(key, kind="stable")


def svd(W):
    """U, sigma (descending, as gesvd delivers them), V with W = U diag(sigma) V'."""
    A, V = jacobi(W)
    nrm = np.sqrt(np.sum(A * A, axis=0))
    order = _ranks(nrm, True)
    sig = nrm[order]
    inv = np.where(sig > 0, 1 / np.where(sig > 0, sig, 1), 0)
    return A[:, order] * inv, sig, V[:, order]


def eigh(X):
    """Eigenvalues (ascending) and eigenvectors of the symmetric X by the shift of csrc/kkt_s.hip: Jacobi on X + 1.5 |X|_F I."""
    fro = np.sqrt(np.sum(X * X))
    if not np.isfinite(fro):
        return np.full(len(X), np.nan, dtype=X.dtype), np.full_like(X, np.nan)
    c = 1.5 * fro if fro > 0 else X.dtype.type(1)
    A, _ = jacobi(X + c * np.eye(len(X), dtype=X.dtype))
    nrm = np.sqrt(np.sum(A * A, axis=0))
    order = _ranks(nrm, False)
    sig = nrm[order]
    return sig - c, A[:, order] / sig


# ---- the 's' operations on one block (matrices)
def congruence(R, X, form):
    """R'X R (form 0) or R X R' (form 1) for X an m x m [x columns] array of symmetric matrices (misc_solvers.c:188-240)."""
    if X.ndim == 3:
        return np.stack([congruence(R, X[:, :, j], form) for j in range(X.shape[2])], axis=2)
    return symm(R @ X @ R.T if form else R.T @ X @ R)


def compute_scaling_s(S, Z):
    Ls, Lz = Q.cholesky(S.copy()), Q.cholesky(Z.copy())
    U, lam, _ = svd(Lz.T @ Ls)
    a = np.sqrt(lam)
    return Q.backward(Lz, U) * a, (Lz @ U) / a, lam


def update_scaling_s(r, rti, Ls, Lz):
    r, rti = r @ Ls, rti @ Lz
    U, lam, V = svd(Lz.T @ Ls)
    a = 1 / np.sqrt(lam)
    return (r @ V) * a, (rti @ U) * a, lam


class SdpEngine(LPN.LpEngine):
    """LpEngine on R^ml_+ x S^{m_0} x ...: d, di on the 'l' rows, r_k, rti_k per block, lmbda of length ml + sum m_k."""

    def __init__(self, c, G, h, dims, A=None, b=None, dtype=np.float64):
        super().__init__(c, G, h, A, b, dtype, False)
        t = dtype
        self.ml, self.sd = int(dims["l"]), [int(k) for k in dims["s"]]
        self.blk = blocks(self.ml, self.sd)
        self.N, self.Nd = self.ml + sum(m * m for m in self.sd), self.ml + sum(self.sd)
        assert self.N == len(self.h)
        if self.blk:                                         # only the lower triangles are read
            self.G, self.h = self.G.copy(), self.h.copy()
            for _, o, _, m in self.blk:
                self.h[o:o + m * m] = vec(symm(mat(self.h, o, m)))
                for j in range(self.G.shape[1]):
                    self.G[o:o + m * m, j] = vec(symm(mat(self.G[:, j], o, m)))
            self.hv = Vec(self.h)
        self.d = self.di = np.ones(self.ml, dtype=t)
        self.r = [np.eye(m, dtype=t) for m in self.sd]
        self.rti = [np.eye(m, dtype=t) for m in self.sd]
        self.lmbda = Vec(np.zeros(self.Nd, dtype=t))

    # ---- W, the Jordan algebra of the cone, and the KKT system
    def W(self, U, inverse=False, trans=False):
        """W U, W'U, W^-1 U or W^-T U for a vector or the columns of a matrix."""
        d = self.di if inverse else self.d
        out = U.copy()
        out[:self.ml] = (d[:, None] if U.ndim == 2 else d) * U[:self.ml]
        for k, o, _, m in self.blk:
            R = self.rti[k] if inverse else self.r[k]
            out[o:o + m * m] = vec(congruence(R, mat(U, o, m), 1 if inverse != trans else 0))
        return out

    def blockwise(self, fl, fs, x, *more):
        """fl on the 'l' rows, fs(k, block of x, ...) on every 's' block; `more` in the layout of x."""
        out = x.copy()
        ml = self.ml
        out[:ml] = fl(x[:ml], *(u[:ml] for u in more))
        for k, o, _, m in self.blk:
            out[o:o + m * m] = vec(fs(k, mat(x, o, m), *(mat(u, o, m) for u in more)))
        return out

    def lam(self, k):
        _, _, ol, m = self.blk[k]
        return self.lmbda.a[ol:ol + m]

    def sprod(self, x, y):
        return self.blockwise(lambda a, b: a * b, lambda k, X, Y: symm((Y @ X + X @ Y) / 2), x, y)

    def sinv_diag(self, x):
        """lmbda o\\ x (misc_solvers.c:845-882)."""
        lm = self.lmbda.a
        out = self.blockwise(lambda a: a / lm[:self.ml], lambda k, X: X / (np.add.outer(self.lam(k), self.lam(k)) / 2), x)
        return out

    def scale2(self, x, inverse=False):
        lm = self.lmbda.a[:self.ml]

        def fs(k, X):
            c = np.multiply.outer(np.sqrt(self.lam(k)), np.sqrt(self.lam(k)))
            return X * c if inverse else X / c
        return self.blockwise(lambda a: a * lm if inverse else a / lm, fs, x)

    def diag(self, u):
        """The vector of the cone with u's 'l' entries and diag(u_k) in every block."""
        out = np.zeros(self.N, dtype=self.t)
        out[:self.ml] = u[:self.ml]
        for _, o, ol, m in self.blk:
            out[o:o + m * m:m + 1] = u[ol:ol + m]
        return out

    def e(self, a):
        return self.diag(np.full(self.Nd, a, dtype=self.t))

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
        return [eigh(mat(v, o, m)) for _, o, _, m in self.blk]

    def max_step(self, v, eig=None):
        a = v.a if isinstance(v, Vec) else v
        t = [max(-a[:self.ml])] if self.ml else []
        return float(max(t + [-sig[0] for sig, _ in (eig or self.eig(a))]))

    def add_e(self, v, a):
        v.a += self.e(a)
        return v

    def scaling(self):
        ml, s, z, lm = self.ml, self.s.a, self.z.a, np.empty(self.Nd, dtype=self.t)
        self.d = np.sqrt(s[:ml] / z[:ml])
        self.di = 1.0 / self.d
        lm[:ml] = np.sqrt(s[:ml] * z[:ml])
        for k, o, ol, m in self.blk:
            self.r[k], self.rti[k], lm[ol:ol + m] = compute_scaling_s(mat(s, o, m), mat(z, o, m))
        self.lmbda.a = lm
        return float(lm @ lm)

    def direction(self, i, sigma, mu, rt, dg, dgi, lmbda_g, wkappa3):
        lm = self.lmbda.a
        if i == 0:
            self.factor()
            self.x1, self.y1, self.z1 = (dgi * v for v in self.ksolve(-self.c, self.b, self.h))
            self.th = self.W(self.h, True, True)
        ds = self.diag(lm * lm)
        dkappa = lmbda_g ** 2
        if i == 1:
            ds = ds + self.ws3 - self.e(sigma * mu)
            dkappa += wkappa3 - sigma * mu
        ds = -self.sinv_diag(ds)
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
        new = np.empty_like(lm)
        s, z = ((1.0 + step * v[:ml]) * lm[:ml] for v in (self.ds, self.dz))
        rs, rz = np.sqrt(s), np.sqrt(z)                                             # misc.py:444-464
        self.d = self.d * rs / rz
        self.di = 1.0 / self.d
        new[:ml] = rs * rz
        for k, o, ol, m in self.blk:                                               # coneprog.py:1356-1395
            lk = self.lam(k)
            c = np.multiply.outer(np.sqrt(lk), np.sqrt(lk))
            Ls, Lz = ((Qm * c) * np.sqrt((1.0 + step * sig) / lk) for sig, Qm in (self.eigs[k], self.eigz[k]))
            self.r[k], self.rti[k], new[ol:ol + m] = update_scaling_s(self.r[k], self.rti[k], Ls, Lz)
        self.lmbda.a = new
        self.s.a, self.z.a = self.W(self.diag(new), False, True), self.W(self.diag(new), True)


def solve_member(c, G, h, dims, A=None, b=None, options=None, dtype=np.float64):
    """One member through _ipm.conelp_start and _ipm.conelp_loop with refinement 0: the namespace of lp_batch_numpy.solve_member,
    'primal slack' and 'dual slack' as -max_step over the whole cone.  A Cholesky factor of s_k or z_k that fails in the scaling of
    the first iteration ends the member as a failed first factorisation does."""
    opt = _ipm.options(dict(QUIET, refinement=0, **(options or {})), dims)
    n, N, p = len(c), len(h), 0 if A is None else len(A)
    e = SdpEngine(c, G, h, dims, A, b, dtype)
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


def interior(ml, s, rng):
    """A point of the interior of K, as _interior of tests/golden/make_goldens_cones.py draws it: 's' blocks M M'/m + U(0.5, 1.5) I."""
    parts = [rng.uniform(0.5, 1.5, ml)]
    for m in s:
        M = rng.standard_normal((m, m))
        parts.append(vec(M @ M.T / m + (0.5 + rng.random()) * np.eye(m)))
    return np.concatenate(parts)


def symmetrise(U, ml, s):
    """Every 's' block of the vector (or of the columns of the matrix) U as the symmetric matrix of its lower triangle, in place."""
    for _, o, _, m in blocks(ml, s):
        X = mat(U, o, m)
        iu = np.triu_indices(m, 1)
        X[iu] = X[iu[::-1]]
        U[o:o + m * m] = vec(X)
    return U


def members(n, ml, s, p, B, seed, kinds=(FEASIBLE,), free=0):
    """B members with per-member G (B, N, n), A (B, p, n) and c (n x B), h (N x B), b (p x B), member k of kind kinds[k % len(kinds)],
    on the feasible construction of _feasible in tests/golden/make_goldens_cones.py (dense G with symmetric 's' blocks and 1 added to
    its diagonal, h = G x0 + s0, b = A x0, c = -G'z0 - A'y0 with s0, z0 positive definite on the blocks):
      primal infeasible  with ml >= 2, rows 0 and 1 replaced by g'x <= -1 and -g'x <= -1; otherwise the (0, 0) entry row of the first
                         block becomes 0'x + s = -1, which no s of that block meets
      dual infeasible    d in the null space of A, G := G + (u - G d) d'/d'd with -u interior to K so that -G d is in K,
                         h = G x1 + s0 with A x1 = b, and c = -d + 0.1 w with w orthogonal to d: feasible and unbounded along d
    free: the last `free` <= p columns of G are exactly zero, and h = G x1 + s0 with A x1 = b."""
    rng = np.random.default_rng(seed)
    s = list(s)
    N = ml + sum(m * m for m in s)
    assert free <= p
    G = rng.standard_normal((B, N, n))
    k = np.arange(min(N, n))
    G[:, k, k] += 1.0
    for k in range(B):
        symmetrise(G[k], ml, s)
    A = rng.standard_normal((B, p, n))
    c, h, b = np.zeros((n, B)), np.zeros((N, B)), np.zeros((p, B))
    kind = [kinds[k % len(kinds)] for k in range(B)]
    dot = lambda Gk, z: Gk.T @ z                                                       # noqa: E731  (full symmetric blocks: sgemv's G'z)
    for k in range(B):
        x0, y0 = rng.standard_normal(n), rng.standard_normal(p)
        s0, z0 = interior(ml, s, rng), interior(ml, s, rng)
        b[:, k] = A[k] @ x0
        if free:
            G[k, :, n - free:] = 0.0
            x0 = np.linalg.lstsq(A[k], b[:, k], rcond=None)[0]
        h[:, k] = G[k] @ x0 + s0
        c[:, k] = -dot(G[k], z0) - A[k].T @ y0
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
            u = -interior(ml, s, rng)
            G[k] += np.outer(u - G[k] @ d, d) / (d @ d)
            x1 = np.linalg.lstsq(A[k], b[:, k], rcond=None)[0] if p else np.zeros(n)
            h[:, k] = G[k] @ x1 + s0
            w = rng.standard_normal(n)
            w -= d * (w @ d) / (d @ d)
            c[:, k] = -d + 0.1 * w
    return types.SimpleNamespace(n=n, ml=ml, s=s, dims={"l": ml, "q": [], "s": s}, N=N, Nd=ml + sum(s), p=p, B=B, c=np.asfortranarray(c),
                                 G=G, h=np.asfortranarray(h), A=A if p else None, b=np.asfortranarray(b) if p else None, kind=kind)


def member(M, k):
    """(c, G, h, dims, A, b) of member k."""
    return M.c[:, k], M.G[k], M.h[:, k], M.dims, None if M.A is None else M.A[k], None if M.b is None else M.b[:, k]


def restate(M, options=None, dtype=np.float64, which=None):
    """solve_member on every member (or those of `which`) of a batch from members()."""
    return [solve_member(*member(M, k), options, dtype) for k in (range(M.B) if which is None else which)]


# ---- the batches of tests/test_sdp_batch_gpu.py; tests/test_sdp_batch_cpu.py checks that float64 and longdouble agree on each
CORNER = (64, 7, (16, 11), 64)
SHAPES = [(1, 0, (1,), 0), (2, 0, (2,), 0), (3, 0, (3,), 0), (6, 2, (1, 2, 3), 2), (10, 0, (9,), 0), (12, 31, (5,), 2),
          (20, 0, (16,), 3), (24, 0, (3,) * 32, 4), (33, 30, (11, 11), 5), CORNER]
SHAPE_B = 12
THIRDS = (FEASIBLE, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE)
EDGE = (6, 2, (1, 2, 3), 2)


def shape_name(shape):
    n, ml, s, p = shape
    return "shape-%d-%d-%s-%d" % (n, ml, "s%dx%d" % (len(s), s[0]) if len(s) > 1 and len(set(s)) == 1 else "s" + "_".join(map(str, s)), p)


# At (1, 0, [1], 0) G is square, so the starting point is the vertex G^-1 h itself and s = h - G x is a rounding error whose sign
# decides between "optimal at iteration 0" and four iterations, in every arithmetic for itself.  float64 and longdouble first agree on
# all twelve members at the seeds 5, 6 and 7, and the kernel, whose fused multiply-adds make it a third arithmetic, agrees at all
# three; 7 is the first of them at which one member takes the loop and eleven end at iteration 0.
SEEDS = dict(zip(SHAPES, (7, 402, 403, 404, 405, 406, 412, 408, 409, 410)))
# name -> (shape, B, seed, kinds, free)
BATCHES = {shape_name(s): (s, SHAPE_B, SEEDS[s], (FEASIBLE,), 0) for s in SHAPES}
BATCHES.update({
    "certificates-6": (EDGE, 12, 431, THIRDS, 0),
    "certificates-10": ((10, 0, (9,), 0), 12, 432, THIRDS, 0),
    "orthant": ((8, 17, (), 3), 12, 441, (FEASIBLE,), 0),
    "order1": ((8, 0, (1,) * 17, 3), 12, 442, (FEASIBLE,), 0),
    "free": (EDGE, 12, 451, (FEASIBLE,), 2),
    "independence": (EDGE, 300, 461, (FEASIBLE,), 0),
    "mixed": (EDGE, 12, 497, (FEASIBLE, FEASIBLE, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE), 0),
})
MIXED_CHANGED = (0, 4, 8)    # the members of "mixed" the GPU test spoils (feasible ones): an h block that is indefinite by 1e20, a
#                              variable nothing holds, a NaN in c
SMALL_BATCHES = sorted(k for k in BATCHES if k != "independence")


@functools.lru_cache(maxsize=None)
def batch(name):
    (n, ml, s, p), B, seed, kinds, free = BATCHES[name]
    return members(n, ml, s, p, B, seed, kinds, free)


@functools.lru_cache(maxsize=None)
def restated(name, precision="longdouble"):
    """The restated results of batch(name), computed once per process and left unchanged."""
    return restate(batch(name), None, getattr(np, precision))
