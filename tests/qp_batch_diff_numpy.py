"""The restatement kvxopt_amd.qpbatchdiff is tested against.  For one member of a batch from qp_batch_numpy.members and a given
x, y, s, z it has the matrix K = [P A' G'; A 0 0; G 0 -diag(s / z)] of the differentiated KKT conditions, a dense solve of it by
an elimination of its own in float64 or numpy.longdouble (numpy.linalg.solve is float64 only), the reduced Cholesky solve with
`refinement` steps in float64 as csrc/qp_batch_diff.hip does it, the right-hand sides of both modes, the gradient formulas, and
for a whole batch the per-member and summed gradients and the exit codes, in the layout of qp_batch_vjp / qp_batch_jvp."""
import types

import numpy as np

import qp_batch_numpy as R

NAMES = ("P", "q", "G", "h", "A", "b")

# ---- the batches of tests/test_qp_batch_diff_gpu.py beyond those of qp_batch_numpy: the staging-tile edges of the assembly
STAGING = [(5, 31, 0), (5, 32, 1), (5, 33, 2)]
SHAPES = R.SHAPES[:7] + STAGING
SEEDS = {shape: (R.SEEDS[shape] if shape in R.SEEDS else 200 + k) for k, shape in enumerate(SHAPES)}
# ---- central differences: the step, the tolerances of the longdouble solves, and those of the float64 end-to-end comparison
EPS = 1e-5
TIGHT_LONGDOUBLE = {"abstol": 1e-12, "reltol": 1e-12, "feastol": 1e-12}
FD_BATCHES = (((8, 17, 3), R.SHAPE_B, SEEDS[(8, 17, 3)]), ((16, 33, 2), R.SHAPE_B, R.INDEPENDENCE[2]))
E2E_SHAPE, E2E_TOL = (8, 17, 3), {"abstol": 1e-9, "reltol": 1e-9, "feastol": 1e-9}
# The largest distance between the float64 restatement (reduced solve, one refinement step) and central differences of float64
# solves at E2E_TOL over the batch of E2E_SHAPE, measured by tests/test_qp_batch_diff_cpu.py: 1.07e-3 (member 11, whose weakly
# active row makes it the member most sensitive to where on the central path the solver stops; the others 2e-9 .. 1e-5).
# tests/test_qp_batch_diff_gpu.py allows the device 10 x this.
E2E_ERROR = 1.07e-3


def member(M, k):
    """(P symmetric from its lower triangle, G, A) of member k; A with 0 rows when the batch has no equalities."""
    P = np.tril(M.P[k]) + np.tril(M.P[k], -1).T
    return P, M.G[k], (np.zeros((0, M.n)) if M.A is None else M.A[k])


def kkt_matrix(P, G, A, s, z, dtype=np.float64):
    """K with the unknowns in the order (uz, ux, uy): the diagonal block -diag(s / z) leads, so that the elimination meets its
    ml columns while they are still sparse."""
    n, ml, p = len(P), len(G), len(A)
    K = np.zeros((ml + n + p, ml + n + p), dtype=dtype)
    K[:ml, :ml] = -np.diag(np.asarray(s, dtype=dtype) / np.asarray(z, dtype=dtype))
    K[:ml, ml:ml + n] = G
    K[ml:ml + n, :ml] = G.T
    K[ml:ml + n, ml:ml + n] = P
    K[ml:ml + n, ml + n:] = A.T
    K[ml + n:, ml:ml + n] = A
    return K


def eliminate(K, r):
    """K^-1 r by Gaussian elimination with partial pivoting in the dtype of K; r a vector or a matrix of right-hand sides.
    A row whose multiplier is exactly zero and a column where the pivot row is exactly zero are passed over, which changes no
    result and lets the diagonal block of K cost what it holds."""
    K, r = K.copy(), np.asarray(r, dtype=K.dtype).copy()
    m = len(K)
    for j in range(m):
        i = j + int(np.argmax(np.abs(K[j:, j])))
        if not (np.abs(K[i, j]) > 0 and np.isfinite(K[i, j])):
            raise ArithmeticError("pivot %d" % j)
        if i != j:
            K[[j, i]] = K[[i, j]]
            r[[j, i]] = r[[i, j]]
        f = K[j + 1:, j] / K[j, j]
        rows = np.flatnonzero(f)
        cols = j + 1 + np.flatnonzero(K[j, j + 1:])
        if rows.size:
            K[np.ix_(j + 1 + rows, cols)] -= np.multiply.outer(f[rows], K[j, cols])
            r[j + 1 + rows] -= np.multiply.outer(f[rows], r[j])
    for j in range(m - 1, -1, -1):
        r[j] = (r[j] - K[j, j + 1:] @ r[j + 1:]) / K[j, j]
    return r


def reduced_solve(P, G, A, s, z, rhs, refinement=1):
    """(ux, uy, uz) as the kernel computes them, in float64: S = P + G' diag(z / s) G = L L', X = L^-1 A', K = X'X, the reduced
    solve of misc.py:1489-1563, and `refinement` times the residual of the full system and a solve with the same factors.
    ArithmeticError on a failed pivot."""
    p = len(A)
    di = np.sqrt(z / s)
    w = s / z
    L = R.cholesky(P + G.T @ ((di ** 2)[:, None] * G))
    if p:
        X = R.forward(L, A.T)
        Lk = R.cholesky(X.T @ X)

    def solve(bx, by, bz):
        bz = di * bz
        x = R.forward(L, bx + G.T @ (di * bz))
        y = by
        if p:
            y = R.backward(Lk, R.forward(Lk, X.T @ x - by))
            x = x - X @ y
        x = R.backward(L, x)
        return x, y, di * (di * (G @ x) - bz)

    bx, by, bz = (np.asarray(v, dtype=np.float64) for v in rhs)
    ux, uy, uz = solve(bx, by, bz)
    for _ in range(refinement):
        dx, dy, dz = solve(bx - (P @ ux + A.T @ uy + G.T @ uz), by - A @ ux, bz - (G @ ux - w * uz))
        ux, uy, uz = ux + dx, uy + dy, uz + dz
    return ux, uy, uz


def rhs_vjp(gx, ml, p):
    return -np.asarray(gx), np.zeros(p, dtype=np.asarray(gx).dtype), np.zeros(ml, dtype=np.asarray(gx).dtype)


def rhs_jvp(x, y, z, d, n, ml, p, dtype=np.float64):
    """The right-hand side of forward mode from the member's perturbations d = {'P': ..., 'q': ...}; a missing name is zero;
    only the lower triangle of d['P'] is read."""
    t = lambda v: np.asarray(v, dtype=dtype)                                          # noqa: E731
    x, y, z = t(x), t(y), t(z)
    dP = t(d["P"]) if d.get("P") is not None else np.zeros((n, n), dtype=dtype)
    dP = np.tril(dP) + np.tril(dP, -1).T
    dq = t(d["q"]) if d.get("q") is not None else np.zeros(n, dtype=dtype)
    dG = t(d["G"]) if d.get("G") is not None else np.zeros((ml, n), dtype=dtype)
    dh = t(d["h"]) if d.get("h") is not None else np.zeros(ml, dtype=dtype)
    dA = t(d["A"]) if p and d.get("A") is not None else np.zeros((p, n), dtype=dtype)
    db = t(d["b"]) if p and d.get("b") is not None else np.zeros(p, dtype=dtype)
    return -(dP @ x + dq + dG.T @ z + dA.T @ y), db - dA @ x, dh - dG @ x


def gradients(x, y, z, ux, uy, uz):
    """The six gradients of reverse mode from the solution and (ux, uy, uz)."""
    o = np.multiply.outer
    return {"P": 0.5 * (o(ux, x) + o(x, ux)), "q": ux, "G": o(uz, x) + o(z, ux), "h": -uz, "A": o(uy, x) + o(y, ux), "b": -uy}


def inner(grads, d):
    """<grads, d> over the six data; the symmetric dP is read by its lower triangle, as the entries read it."""
    t = 0.0
    for k, g in grads.items():
        if d.get(k) is None or g is None:
            continue
        v = np.asarray(d[k], dtype=np.asarray(g).dtype)
        if k == "P":
            v = np.tril(v) + np.tril(v, -1).T
        t = t + (np.asarray(g) * v).sum()
    return t


def member_exit(code, s, z):
    """The exit of the derivative of a member before any arithmetic: 1 skipped, 2 a bad s or z, 0 to be solved."""
    if code != 0:
        return 1
    ok = np.all((s > 0) & np.isfinite(s) & (z > 0) & np.isfinite(z))
    return 0 if ok else 2


def _solver(method, refinement):
    """solve(P, G, A, s, z, [rhs, ...]) -> [(ux, uy, uz), ...]; the dense elimination is done once for all right-hand sides."""
    if method == "reduced":
        return lambda P, G, A, s, z, many: [reduced_solve(P, G, A, s, z, rhs, refinement) for rhs in many]
    dtype = getattr(np, method)

    def solve(P, G, A, s, z, many):
        n, ml = len(P), len(G)
        r = np.stack([np.concatenate([np.asarray(v, dtype=dtype) for v in (bz, bx, by)]) for bx, by, bz in many], axis=1)
        u = eliminate(kkt_matrix(P, G, A, s, z, dtype), r)
        return [(u[ml:ml + n, c], u[ml + n:, c], u[:ml, c]) for c in range(len(many))]
    return solve


def derivatives(M, sol, gx=None, d=None, method="longdouble", refinement=1, shared=()):
    """(V, J): qp_batch_vjp for the cotangent gx and qp_batch_jvp for the perturbations d restated on the batch M at the
    solution `sol`; None for a mode whose input is None.  method: 'longdouble' or 'float64' (the dense elimination, done once
    per member for both modes) or 'reduced' (as the kernel, float64, with `refinement` steps).
    V: 'ux', 'uy', 'uz', 'exit' and the six gradients per member -- matrices (B, rows, n), columns rows x B -- except for the
    names in `shared`, which get the sum over the members with exit 0; the gradients of A and b are None when p = 0.
    J: 'x', 'y', 'z', 's', 'exit'; d maps names to per-member perturbations ((B, rows, n) or rows x B), a missing name is zero."""
    solve = _solver(method, refinement)
    B, n, ml, p = M.B, M.n, M.ml, M.p
    dt = np.float64 if method == "reduced" else getattr(np, method)
    V = {"ux": np.zeros((n, B), dt), "uy": np.zeros((p, B), dt), "uz": np.zeros((ml, B), dt), "exit": np.zeros(B, dtype=np.int64),
         "P": np.zeros((B, n, n), dt), "q": np.zeros((n, B), dt), "G": np.zeros((B, ml, n), dt), "h": np.zeros((ml, B), dt),
         "A": np.zeros((B, p, n), dt), "b": np.zeros((p, B), dt)}
    J = {"x": np.zeros((n, B), dt), "y": np.zeros((p, B), dt), "z": np.zeros((ml, B), dt), "s": np.zeros((ml, B), dt),
         "exit": np.zeros(B, dtype=np.int64)}
    for k in range(B):
        x, y, s, z = (sol[v][:, k] for v in ("x", "y", "s", "z"))
        code = member_exit(sol["exit"][k], s, z)
        if code == 0:
            P, G, A = member(M, k)
            many = ([rhs_vjp(gx[:, k].astype(dt), ml, p)] if gx is not None else []) + \
                   ([rhs_jvp(x, y, z, member_perturbation(d, k), n, ml, p, dt)] if d is not None else [])
            try:
                res = solve(P, G, A, s, z, many)
            except ArithmeticError:
                code = 2
        V["exit"][k] = J["exit"][k] = code
        if code:
            continue
        if gx is not None:
            ux, uy, uz = res[0]
            V["ux"][:, k], V["uy"][:, k], V["uz"][:, k] = ux, uy, uz
            g = gradients(x.astype(dt), y.astype(dt), z.astype(dt), ux, uy, uz)
            for name in NAMES:
                if name in "PGA":
                    V[name][k] = g[name]
                else:
                    V[name][:, k] = g[name]
        if d is not None:
            dx, dy, dz = res[-1]
            J["x"][:, k], J["y"][:, k], J["z"][:, k] = dx, dy, dz
            J["s"][:, k] = -(s.astype(dt) / z.astype(dt)) * dz
    for name in shared:
        V[name] = V[name].sum(axis=0) if name in "PGA" else V[name].sum(axis=1)
    if not p:
        V["A"] = V["b"] = None
    return (V if gx is not None else None), (J if d is not None else None)


def vjp_batch(M, sol, gx, method="longdouble", refinement=1, shared=()):
    return derivatives(M, sol, gx, None, method, refinement, shared)[0]


def jvp_batch(M, sol, d, method="longdouble", refinement=1):
    return derivatives(M, sol, None, d, method, refinement)[1]


def member_perturbation(d, k):
    return {name: (None if d.get(name) is None else (d[name][k] if name in "PGA" else d[name][:, k])) for name in NAMES}


def direction(M, seed, scale=1.0):
    """One random direction in all six data of the batch M, per member; dP symmetric."""
    rng = np.random.default_rng(seed)
    B, n, ml, p = M.B, M.n, M.ml, M.p
    dP = rng.standard_normal((B, n, n))
    d = {"P": scale * 0.5 * (dP + dP.transpose(0, 2, 1)), "q": scale * np.asfortranarray(rng.standard_normal((n, B))),
         "G": scale * rng.standard_normal((B, ml, n)), "h": scale * np.asfortranarray(rng.standard_normal((ml, B))),
         "A": scale * rng.standard_normal((B, p, n)) if p else None, "b": scale * np.asfortranarray(rng.standard_normal((p, B))) if p else None}
    return d


def moved(M, d, eps):
    """The batch M moved by eps along the direction d."""
    add = lambda a, v: a if v is None else a + eps * v                                   # noqa: E731
    return types.SimpleNamespace(n=M.n, ml=M.ml, p=M.p, B=M.B, P=add(M.P, d["P"]), q=add(M.q, d["q"]), G=add(M.G, d["G"]), h=add(M.h, d["h"]),
                                 A=None if M.A is None else add(M.A, d["A"]), b=None if M.b is None else add(M.b, d["b"]))


def solution(ref):
    """A list of qp_batch_numpy.solve_member results as the dictionary qp_batch returns (x, y, s, z, exit), in their dtype."""
    stack = lambda name: np.stack([getattr(r, name) for r in ref], axis=1)              # noqa: E731
    return {"x": stack("x"), "y": stack("y"), "s": stack("s"), "z": stack("z"), "exit": np.array([r.exit for r in ref], dtype=np.int64)}


def fd_errors(J, plus, minus, eps=EPS):
    """Per member: the largest relative 2-norm distance over x, y, s, z between the directional derivative J and the central
    difference of the two solutions (dictionaries as qp_batch returns them); nan where one of the three is not done."""
    B = len(J["exit"])
    out = np.full(B, np.nan)
    for k in range(B):
        if J["exit"][k] or plus["exit"][k] or minus["exit"][k]:
            continue
        worst = 0.0
        for v in ("x", "y", "s", "z"):
            fd = (plus[v][:, k] - minus[v][:, k]) / (2 * eps)
            if len(fd):
                worst = max(worst, float(np.linalg.norm((J[v][:, k] - fd).astype(np.float64)) / np.linalg.norm(fd.astype(np.float64))))
        out[k] = worst
    return out


def rule(got, ref):
    """|got - ref| in units of the project's bound 1e-6 max(|ref|, 1) in the 2-norm: passes when <= 1."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - ref) / (1e-6 * max(np.linalg.norm(ref), 1.0)))
