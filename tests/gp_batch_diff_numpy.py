"""The restatement kvxopt_amd.gpbatchdiff is tested against.  For one member of a batch from
gp_batch_numpy.members and a given x, y, znl, snl, zl, sl it has the point-dependent parts (the softmax weights y, zeta = (1, znl),
Df, H, J), the matrix K = [H A' J'; A 0 0; J 0 -diag(s / z)] of the differentiated optimality conditions in x, a dense solve of it
by the elimination of qp_batch_diff_numpy in numpy.longdouble, the reduced Cholesky solve with `refinement` steps in float64 as
csrc/gp_batch_diff.hip does it (S from the centred factors and the gradient rows, the residual with H u formed from F and never as
a matrix), the right-hand sides of both modes, the gradient formulas, and for a whole batch the per-member and summed gradients
and the exit codes in the layout of gp_batch_vjp / gp_batch_jvp.  Also the batches of tests/test_gp_batch_diff_gpu.py, the
refinement table and the central differences of tests/test_gp_batch_diff_cpu.py."""
import functools
import types

import numpy as np

import gp_batch_numpy as R
from qp_batch_diff_numpy import eliminate, rule  # noqa: F401
from qp_batch_numpy import backward, cholesky, forward

NAMES = ("F", "g", "G", "h", "A", "b")
MATRICES = ("F", "G", "A")
SOL_KEYS = ("x", "y", "znl", "snl", "zl", "sl")

# ---- the batches of tests/test_gp_batch_diff_gpu.py: those of gp_batch_numpy.EDGES, each for an edge of k_gp_batch_diff, and one
# more: block 0 stages no gradient row here, so blocks_tile_plus has TILE of them and this shape has TILE + 1 again.
EXTRA = {"grads_tile_plus": (3, [5] + [1] * (R.TILE + 1), 7, 0, 8, 3112)}
EDGE_NAMES = ("one_term_blocks", "k63_64_65", "l768", "mixed_one_term", "tile_minus", "tile_exact", "tile_plus", "blocks_tile_plus",
              "grads_tile_plus", "n63_p63", "N192_blocks", "N192_linear", "lds_corner", "spread700")
INDEPENDENT = (0, 63, 64, 299)                # the members of the independence batch that are compared
# ---- central differences: the step, the tolerances of the longdouble solves, the batches (shape, B, seed)
EPS = 1e-6
TIGHT_LONGDOUBLE = {"abstol": 1e-13, "reltol": 1e-13, "feastol": 1e-13}
FD_BATCHES = (((4, [5, 3], 8, 1), 8, 5101), ((6, [5, 3, 2], 12, 1), 8, 5102), ((3, [4, 1, 2], 0, 0), 8, 5103))


@functools.lru_cache(maxsize=None)
def named(name):
    if name in EXTRA:
        n, K, ml, p, B, seed = EXTRA[name]
        return R.members(n, K, ml, p, B, seed)
    return R.named(name)


@functools.lru_cache(maxsize=None)
def restated(name, precision="float64", maxiters=None, which=None):
    """The restated solutions of named(name), computed once per process and left unchanged."""
    if name not in EXTRA:
        return R.restated(name, precision, maxiters, which)
    return R.restate(named(name), {} if maxiters is None else {"maxiters": maxiters}, getattr(np, precision), which)


def solution(ref, m):
    """A list of gp_batch_numpy.solve_member results as the dictionary gp_batch returns (x, y, znl, snl, zl, sl, exit)."""
    stack = lambda name: np.stack([getattr(r, name) for r in ref], axis=1)              # noqa: E731
    s, z = stack("s"), stack("z")
    return {"x": stack("x"), "y": stack("y"), "znl": z[1:m], "snl": s[1:m], "zl": z[m:], "sl": s[m:],
            "exit": np.array([r.exit for r in ref], dtype=np.int64)}


def subset(M, which):
    """The members `which` of a batch as a batch."""
    K, F, g, G, h, A, b = R.batch_args(M, which)
    return types.SimpleNamespace(n=M.n, K=M.K, ml=M.ml, p=M.p, B=len(which), F=F, g=g, G=G, h=h, A=A, b=b)


# ---- one member ------------------------------------------------------------------------------------------------------------------
def member(M, k, dtype=np.float64):
    """(F, g, G, A) of member k; G and A with 0 rows where the batch has none."""
    t = lambda a, rows: np.zeros((rows, M.n), dtype) if a is None else np.asarray(a[k], dtype)       # noqa: E731
    return np.asarray(M.F[k], dtype), np.asarray(M.g[:, k], dtype), t(M.G, 0), t(M.A, 0)


def point(K, F, g, x, znl):
    """(off, blk, y, zeta, Df) at x in the dtype of F: the softmax weights per block (the maximum taken before exp), the weights
    zeta = (1, znl) of the blocks in H and the block gradients Df_i = y_i'F_i (m x n, row 0 the objective's)."""
    m = len(K)
    off = np.concatenate([[0], np.cumsum(K)]).astype(int)
    blk = np.repeat(np.arange(m), K)
    u = F @ x + g
    y = np.empty_like(u)
    for i in range(m):
        e = np.exp(u[off[i]:off[i + 1]] - u[off[i]:off[i + 1]].max())
        y[off[i]:off[i + 1]] = e / e.sum()
    zeta = np.concatenate([np.ones(1, F.dtype), np.asarray(znl, F.dtype)])
    Df = np.stack([y[off[i]:off[i + 1]] @ F[off[i]:off[i + 1]] for i in range(m)])
    return off, blk, y, zeta, Df


def block_sums(off, v):
    return np.array([v[off[i]:off[i + 1]].sum() for i in range(len(off) - 1)], dtype=v.dtype)


def hess_mul(F, off, blk, y, zeta, u, uznl0=None):
    """(w, c): with t = F u, c_i = y_i't_i and w_k = y_k (zeta_i (t_k - c_i) + uznl0_i), so that H u + Df'uznl0 = F'w;
    uznl0 has m entries, the first 0."""
    t = F @ u
    c = block_sums(off, y * t)
    w = y * (zeta[blk] * (t - c[blk]) + (0 if uznl0 is None else uznl0[blk]))
    return w, c


def kkt_matrix(F, G, A, off, blk, y, zeta, Df, s, z):
    """K with the unknowns in the order (uz, ux, uy), as qp_batch_diff_numpy.kkt_matrix; uz = (uznl, uzl)."""
    dtype = F.dtype
    Fc = np.sqrt(zeta[blk] * y)[:, None] * (F - Df[blk])
    H = Fc.T @ Fc
    J = np.vstack([Df[1:], G])
    n, r, p = F.shape[1], len(J), len(A)
    Kk = np.zeros((r + n + p, r + n + p), dtype=dtype)
    Kk[:r, :r] = -np.diag(np.asarray(s, dtype) / np.asarray(z, dtype))
    Kk[:r, r:r + n] = J
    Kk[r:r + n, :r] = J.T
    Kk[r:r + n, r:r + n] = H
    Kk[r:r + n, r + n:] = A.T
    Kk[r + n:, r:r + n] = A
    return Kk


def reduced_solve(F, G, A, off, blk, y, zeta, Df, s, z, many, refinement):
    """[(ux, uy, uz), ...] for the right-hand sides `many` as the kernel computes them, in float64: S = H + J' diag(z / s) J from
    the staged rows, its factor, X = L^-1 A', K = X'X, the reduced solve of misc.py:1489-1563 and `refinement` times the residual
    of the full system, H u formed from F, and a solve with the same factors.  Where S fails its factorisation and p > 0 it is
    factored on S + A'A.  ArithmeticError on a failed pivot after that."""
    p, m = len(A), len(off) - 1
    J = np.vstack([Df[1:], G])
    di = np.sqrt(z / s)
    w = s / z
    Fc = np.sqrt(zeta[blk] * y)[:, None] * (F - Df[blk])
    S, sing = Fc.T @ Fc + J.T @ ((di ** 2)[:, None] * J), False
    try:
        L = cholesky(S)
    except ArithmeticError:
        if not p:
            raise
        L, sing = cholesky(S + A.T @ A), True                                        # the repair of misc.py:1433-1458
    if p:
        X = forward(L, A.T)
        Lk = cholesky(X.T @ X)

    def solve(bx, by, bz):
        bz = di * bz
        x = forward(L, bx + J.T @ (di * bz) + (A.T @ by if sing else 0.0))
        yy = by
        if p:
            yy = backward(Lk, forward(Lk, X.T @ x - by))
            x = x - X @ yy
        x = backward(L, x)
        return x, yy, di * (di * (J @ x) - bz)

    out = []
    for bx, by, bz in many:
        bx, by, bz = (np.asarray(v, dtype=np.float64) for v in (bx, by, bz))
        ux, uy, uz = solve(bx, by, bz)
        for _ in range(refinement):
            wv, c = hess_mul(F, off, blk, y, zeta, ux, np.concatenate([[0.0], uz[:m - 1]]))
            rz = bz - (np.concatenate([c[1:], G @ ux]) - w * uz)
            dx, dy, dz = solve(bx - (F.T @ wv + G.T @ uz[m - 1:] + A.T @ uy), by - A @ ux, rz)
            ux, uy, uz = ux + dx, uy + dy, uz + dz
        out.append((ux, uy, uz))
    return out


def rhs_jvp(F, off, blk, y, zeta, x, yeq, zl, d, ml, p):
    """The right-hand side of forward mode from the member's perturbations d = {'F': ..., 'g': ...}; a missing name is zero."""
    dtype, (l, n) = F.dtype, F.shape
    get = lambda k, shape: np.asarray(d[k], dtype) if d.get(k) is not None else np.zeros(shape, dtype)       # noqa: E731
    dF, dg, dG, dh = get("F", (l, n)), get("g", l), get("G", (ml, n)), get("h", ml)
    dA, db = (get("A", (p, n)), get("b", p)) if p else (np.zeros((0, n), dtype), np.zeros(0, dtype))
    v = dF @ x + dg
    c = block_sums(off, y * v)
    bx = -(dF.T @ (zeta[blk] * y) + F.T @ (zeta[blk] * y * (v - c[blk])) + dG.T @ zl + dA.T @ yeq)
    return bx, db - dA @ x, np.concatenate([-c[1:], dh - dG @ x])


def gradients(F, off, blk, y, zeta, x, yeq, zl, ux, uy, uz):
    """The six gradients of reverse mode from the solution and (ux, uy, uz), uz = (uznl, uzl)."""
    o, m = np.multiply.outer, len(off) - 1
    gg, _ = hess_mul(F, off, blk, y, zeta, ux, np.concatenate([np.zeros(1, F.dtype), uz[:m - 1]]))
    uzl = uz[m - 1:]
    return {"F": o(zeta[blk] * y, ux) + o(gg, x), "g": gg, "G": o(uzl, x) + o(zl, ux), "h": -uzl, "A": o(uy, x) + o(yeq, ux), "b": -uy}


def member_exit(code, s, z):
    """The exit of the derivative of a member before any arithmetic: 1 skipped, 2 a bad s or z, 0 to be solved."""
    if code != 0:
        return 1
    return 0 if np.all((s > 0) & np.isfinite(s) & (z > 0) & np.isfinite(z)) else 2


# ---- a batch ---------------------------------------------------------------------------------------------------------------------
def derivatives(M, sol, gx=None, d=None, precision="longdouble", refinement=1, shared=(), ds="scaled"):
    """(V, J): gp_batch_vjp for the cotangent gx and gp_batch_jvp for the perturbations d restated on the batch M at the solution
    `sol`; None for a mode whose input is None.  precision 'float64': the reduced solve with `refinement` steps, as the kernel;
    'longdouble': the dense elimination of the full system, done once per member for both modes.
    V: 'ux', 'uy', 'uznl', 'uzl', 'exit' and the six gradients per member -- matrices (B, rows, n), columns rows x B -- except
    for the names in `shared`, which get the sum over the members with exit 0; None for G, h when ml = 0 and A, b when p = 0.
    J: 'x', 'y', 'znl', 'snl', 'zl', 'sl', 'exit'; d maps names to per-member perturbations, a missing name is zero.
    ds: 'scaled' for ds = -(s / z) dz, as the kernel; 'row' for the third block row ds = bz - J dx."""
    B, n, ml, p, K = M.B, M.n, M.ml, M.p, list(M.K)
    m, l = len(K), sum(K)
    dt = np.float64 if precision == "float64" else getattr(np, precision)
    zeros = lambda *shape: np.zeros(shape, dt)                                              # noqa: E731
    V = {"ux": zeros(n, B), "uy": zeros(p, B), "uznl": zeros(m - 1, B), "uzl": zeros(ml, B), "exit": np.zeros(B, dtype=np.int64),
         "F": zeros(B, l, n), "g": zeros(l, B), "G": zeros(B, ml, n), "h": zeros(ml, B), "A": zeros(B, p, n), "b": zeros(p, B)}
    J = {"x": zeros(n, B), "y": zeros(p, B), "znl": zeros(m - 1, B), "snl": zeros(m - 1, B), "zl": zeros(ml, B), "sl": zeros(ml, B),
         "exit": np.zeros(B, dtype=np.int64)}
    with np.errstate(all="ignore"):
        for k in range(B):
            x, yeq, znl, snl, zl, sl = (np.asarray(sol[v][:, k], dt) for v in SOL_KEYS)
            s, z = np.concatenate([snl, sl]), np.concatenate([znl, zl])
            code = member_exit(sol["exit"][k], s, z)
            if code == 0:
                F, g, G, A = member(M, k, dt)
                off, blk, y, zeta, Df = point(K, F, g, x, znl)
                many = ([(-np.asarray(gx[:, k], dt), zeros(p), zeros(m - 1 + ml))] if gx is not None else []) + \
                       ([rhs_jvp(F, off, blk, y, zeta, x, yeq, zl, member_perturbation(d, k), ml, p)] if d is not None else [])
                try:
                    if precision == "float64":
                        res = reduced_solve(F, G, A, off, blk, y, zeta, Df, s, z, many, refinement)
                    else:
                        r = m - 1 + ml
                        rr = np.stack([np.concatenate([bz, bx, by]) for bx, by, bz in many], axis=1)
                        u = eliminate(kkt_matrix(F, G, A, off, blk, y, zeta, Df, s, z), rr)
                        res = [(u[r:r + n, c], u[r + n:, c], u[:r, c]) for c in range(len(many))]
                    if not all(np.all(np.isfinite(np.concatenate(t))) for t in res):
                        raise ArithmeticError("not finite")
                except ArithmeticError:
                    code = 2
            V["exit"][k] = J["exit"][k] = code
            if code:
                continue
            if gx is not None:
                ux, uy, uz = res[0]
                V["ux"][:, k], V["uy"][:, k], V["uznl"][:, k], V["uzl"][:, k] = ux, uy, uz[:m - 1], uz[m - 1:]
                gr = gradients(F, off, blk, y, zeta, x, yeq, zl, ux, uy, uz)
                for name in NAMES:
                    if name in MATRICES:
                        V[name][k] = gr[name]
                    else:
                        V[name][:, k] = gr[name]
            if d is not None:
                dx, dy, dz = res[-1]
                dsv = -(s / z) * dz if ds == "scaled" else many[-1][2] - np.vstack([Df[1:], G]) @ dx
                J["x"][:, k], J["y"][:, k] = dx, dy
                J["znl"][:, k], J["zl"][:, k], J["snl"][:, k], J["sl"][:, k] = dz[:m - 1], dz[m - 1:], dsv[:m - 1], dsv[m - 1:]
    for name in shared:
        V[name] = V[name].sum(axis=0) if name in MATRICES else V[name].sum(axis=1)
    if not ml:
        V["G"] = V["h"] = None
    if not p:
        V["A"] = V["b"] = None
    return (V if gx is not None else None), (J if d is not None else None)


def member_perturbation(d, k):
    return {name: (None if d.get(name) is None else (d[name][k] if name in MATRICES else d[name][:, k])) for name in NAMES}


def inner(grads, d):
    """<grads, d> over the six data of one member."""
    t = 0.0
    for k, g in grads.items():
        if d.get(k) is None or g is None:
            continue
        t = t + (np.asarray(g) * np.asarray(d[k], dtype=np.asarray(g).dtype)).sum()
    return t


def member_gradients(V, k):
    return {name: (V[name][k] if name in MATRICES else V[name][:, k]) for name in NAMES if V[name] is not None}


def direction(M, seed, scale=1.0):
    """One random direction in all six data of the batch M, per member."""
    rng = np.random.default_rng(seed)
    B, n, ml, p, l = M.B, M.n, M.ml, M.p, sum(M.K)
    col = lambda r: scale * np.asfortranarray(rng.standard_normal((r, B)))                   # noqa: E731
    mat = lambda r: scale * rng.standard_normal((B, r, n))                                   # noqa: E731
    return {"F": mat(l), "g": col(l), "G": mat(ml) if ml else None, "h": col(ml) if ml else None, "A": mat(p) if p else None,
            "b": col(p) if p else None}


def moved(M, d, eps):
    """The batch M moved by eps along the direction d."""
    add = lambda a, v: a if a is None or v is None else a + eps * v                          # noqa: E731
    return types.SimpleNamespace(n=M.n, K=M.K, ml=M.ml, p=M.p, B=M.B, **{k: add(getattr(M, k), d[k]) for k in NAMES})


def fd_errors(J, runs, eps=EPS):
    """Per member: the largest distance |J - fd|_2 / max(|fd|_2, 1) over x, y, znl, snl, zl, sl between the directional
    derivative J and the central difference fd of the solutions at +eps and -eps -- the scaling of the project's rule, absolute
    below 1: a member without an active log-sum-exp row has znl and its derivative at 1e-18, where a relative distance says
    nothing; nan where a member is left out: one of the three runs (lists of
    gp_batch_numpy.solve_member results: at the point, at +eps, at -eps) did not end optimal, or their iteration counts differ."""
    at, plus, minus = runs
    m = len(at[0].K)
    P, Mi = solution(plus, m), solution(minus, m)
    out = np.full(len(at), np.nan)
    for k in range(len(at)):
        if J["exit"][k] or any(r[k].exit for r in runs) or len({r[k].iterations for r in runs}) != 1:
            continue
        worst = 0.0
        for v in SOL_KEYS:
            fd = ((P[v][:, k] - Mi[v][:, k]) / (2 * eps)).astype(np.float64)
            if len(fd):
                worst = max(worst, float(np.linalg.norm(J[v][:, k].astype(np.float64) - fd) / max(np.linalg.norm(fd), 1.0)))
        out[k] = worst
    return out


# ---- the refinement table ---------------------------------------------------------------------------------------------------------
def table_batches():
    """(name, batch, float64 solution) of every batch of tests/test_gp_batch_diff_gpu.py."""
    for name in EDGE_NAMES:
        M = named(name)
        yield name, M, solution(restated(name), len(M.K))
    M = R.named("independence")
    yield "independence", subset(M, INDEPENDENT), solution(R.restated("independence", "float64", None, INDEPENDENT), len(M.K))
    M = R.named("mixed")
    yield "mixed", M, solution(R.restated("mixed", "float64"), len(M.K))


V_KEYS = ("ux", "uy", "uznl", "uzl") + NAMES
J_KEYS = SOL_KEYS


def rule_errors(V, J, Vr, Jr, B):
    """Per member: the largest error over every output of both modes against the reference, in units of the rule."""
    out = np.zeros(B)
    for k in range(B):
        e = [0.0]
        for v in V_KEYS if V is not None else ():
            if V[v] is not None:
                e.append(rule(V[v][k], Vr[v][k]) if v in MATRICES else rule(V[v][:, k], Vr[v][:, k]))
        for v in J_KEYS if J is not None else ():
            e.append(rule(J[v][:, k], Jr[v][:, k]))
        out[k] = max(e)
    return out


@functools.lru_cache(maxsize=None)
def refinement_table():
    """name -> the largest error over the done members, in units of the rule, at 0, 1, 2 steps with ds = -(s / z) dz and at 0, 1,
    2 steps with ds from the third block row."""
    out = {}
    for name, M, sol in table_batches():
        gx = np.random.default_rng(5).standard_normal((M.n, M.B))
        d = direction(M, 6)
        Vr, Jr = derivatives(M, sol, gx, d, "longdouble")
        row = []
        for mode in ("scaled", "row"):
            Jm = Jr if mode == "scaled" else derivatives(M, sol, None, d, "longdouble", ds="row")[1]
            for steps in (0, 1, 2):
                V, J = derivatives(M, sol, gx, d, "float64", steps, ds=mode)
                assert list(V["exit"]) == list(Vr["exit"]), (name, V["exit"], Vr["exit"])
                row.append(float(rule_errors(V, J, Vr, Jm, M.B).max()))
        out[name] = tuple(row)
    return out
