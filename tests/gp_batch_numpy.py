"""The restatement kvxopt_amd.gpbatch is tested against: cvx._cpl (cvxprog.py:556-1356) at refinement 0 on cp's epigraph form of one
geometric program, one member at a time, in float64 or numpy.longdouble.  The variable is (x, t) with t in column n; the mnl + 1
log-sum-exp rows (objective first, f_0 - t) and the ml rows of G are one orthant block of N rows.  The KKT solve is misc.kkt_chol2
on dense matrices without the A'A repair: S = H + J' di^2 J = L L' with H = sum_i z_i H_i built from the centred factors
sqrt(z_i y_k) (F_k - Df_i) of cvxprog.py:2135-2150, X = L^-1 A', K = X'X, with the explicit column Cholesky of qp_batch_numpy that
raises ArithmeticError on a pivot <= 0 (or not finite).  Every backtracking loop leaves with exit 4 after 64 halvings of the step,
as the kernel does; the reference has no bound.  solve_member also counts which branches of the line search ran.

Also the seeded generator of feasible members and the batches tests/test_gp_batch_gpu.py runs, with the cache of their restated
results."""
import functools
import types

import numpy as np

from kvxopt_amd import _ipm
from qp_batch_numpy import backward, cholesky, forward

BETA, ALPHA, MAX_RELAXED_ITERS, MAX_HALVINGS = 0.5, 0.01, 8, 64
EXIT_OPTIMAL, EXIT_MAXITERS, EXIT_SINGULAR, EXIT_RANK, EXIT_LINESEARCH = range(5)
COUNTERS = ("backtracks", "saved", "relaxed_inc", "resumed", "restored", "max_halvings")


class _Halvings(Exception):
    pass


def solve_member(K, F, g, G=None, h=None, A=None, b=None, options=None, dtype=np.float64, linsolve=False, reverse=False):
    """One member: a namespace with status, exit (the codes of kvxopt_amd.gpbatch), iterations, x (n), y, s, z (N = mnl + 1 + ml,
    the objective row first), stats (gap, relgap, pcost, dcost, pres, dres, primal slack, dual slack) and counters.  linsolve=True
    replaces both factors by numpy.linalg.solve (float64 only), which moves every rounding and so shows whether an iteration count
    or a branch of the line search sits on a rounding edge.  reverse=True solves the same program with the terms of every block
    and the rows of G in reverse order, which moves every rounding too and keeps the Cholesky factors with their failed pivots."""
    if reverse:
        off = np.concatenate([[0], np.cumsum(K)]).astype(int)
        perm = np.concatenate([np.arange(off[i + 1] - 1, off[i] - 1, -1) for i in range(len(K))])
        F, g = np.asarray(F)[perm], np.asarray(g)[perm]
        G, h = (None, None) if G is None else (np.asarray(G)[::-1], np.asarray(h)[::-1])
    with np.errstate(all="ignore"):
        r = _solve(K, F, g, G, h, A, b, options, dtype, linsolve)
    if reverse:
        m = len(K)
        r.s, r.z = np.concatenate([r.s[:m], r.s[m:][::-1]]), np.concatenate([r.z[:m], r.z[m:][::-1]])
    return r


def _solve(K, F, g, G, h, A, b, options, dtype, linsolve):
    o = dict(options or {})
    o.setdefault("refinement", 0)
    opt = _ipm.options(o, {"l": 0, "q": [], "s": []})
    assert opt.refinement == 0
    T = dtype
    F, g = np.asarray(F, dtype=T), np.asarray(g, dtype=T)
    l, n = F.shape
    ne, m = n + 1, len(K)
    off = np.concatenate([[0], np.cumsum(K)]).astype(int)
    G = np.zeros((0, n), dtype=T) if G is None else np.asarray(G, dtype=T)
    h = np.zeros(0, dtype=T) if h is None else np.asarray(h, dtype=T)
    A = np.zeros((0, n), dtype=T) if A is None else np.asarray(A, dtype=T)
    b = np.zeros(0, dtype=T) if b is None else np.asarray(b, dtype=T)
    ml, p = len(h), len(b)
    N = m + ml
    Ge = np.hstack([G, np.zeros((ml, 1), dtype=T)])
    Ae = np.hstack([A, np.zeros((p, 1), dtype=T)])
    c = np.zeros(ne, dtype=T); c[n] = 1.0
    blk = np.repeat(np.arange(m), K)
    cnt = dict.fromkeys(COUNTERS, 0)
    nrm = lambda v: float(np.sqrt(v @ v))                                      # noqa: E731

    def lse(xe):
        u = F @ xe[:n] + g
        f, y = np.zeros(m, dtype=T), np.empty(l, dtype=T)
        for i in range(m):
            ui = u[off[i]:off[i + 1]]
            mx = ui.max()
            e = np.exp(ui - mx)
            sm = e.sum()
            f[i] = mx + np.log(sm)
            y[off[i]:off[i + 1]] = e / sm
        f[0] -= xe[n]
        return f, y

    def jac(y):
        Df = np.zeros((m, ne), dtype=T)
        for i in range(m):
            Df[i, :n] = y[off[i]:off[i + 1]] @ F[off[i]:off[i + 1]]
        Df[0, n] = -1.0
        return np.vstack([Df, Ge])

    st = types.SimpleNamespace()

    def factor(J, y, z, di):
        Fc = np.sqrt(z[blk] * y)[:, None] * (F - J[blk, :n])
        S = np.zeros((ne, ne), dtype=T)
        S[:n, :n] = Fc.T @ Fc
        S = S + J.T @ ((di ** 2)[:, None] * J)
        if linsolve:
            if not np.all(np.isfinite(S)):
                raise ArithmeticError("S is not finite")
            try:
                st.S, st.K = S, Ae @ np.linalg.solve(S, Ae.T)
            except np.linalg.LinAlgError:
                raise ArithmeticError("S is singular")
            return
        st.L = cholesky(S)
        if p:
            st.X = forward(st.L, Ae.T)
            st.Lk = cholesky(st.X.T @ st.X)

    def ksolve(J, di, bx, by, bz):
        bz = di * bz
        bx = bx + J.T @ (di * bz)
        if linsolve:
            u = np.linalg.solve(st.S, bx)
            by = np.linalg.solve(st.K, Ae @ u - by) if p else by
            bx = np.linalg.solve(st.S, bx - Ae.T @ by)
            return bx, by, di * (J @ bx) - bz
        bx = forward(st.L, bx)
        if p:
            by = backward(st.Lk, forward(st.Lk, st.X.T @ bx - by))
            bx = bx - st.X @ by
        bx = backward(st.L, bx)
        return bx, by, di * (J @ bx) - bz

    x, y_ = np.zeros(ne, dtype=T), np.zeros(p, dtype=T)
    s, z = np.ones(N, dtype=T), np.ones(N, dtype=T)
    relaxed_iters = 0
    sv = None
    phi0 = dphi0 = gap0 = step0 = dsdz0 = sigma0 = eta0 = 0.0

    def finish(code, iters, gap, relgap, pcost, dcost, pres, dres):
        if code == EXIT_RANK:
            zz = lambda k: np.zeros(k)                                         # noqa: E731
            return types.SimpleNamespace(status="unknown", exit=code, iterations=0, x=zz(n), y=zz(p), s=zz(N), z=zz(N),
                                         stats=(np.nan,) * 8, counters=cnt, K=list(K), ml=ml)
        stats = tuple(np.nan if v is None else float(v) for v in (gap, relgap, pcost, dcost, pres, dres, s.min(), z.min()))
        return types.SimpleNamespace(status="optimal" if code == EXIT_OPTIMAL else "unknown", exit=code, iterations=iters,
                                     x=x[:n].copy(), y=y_.copy(), s=s.copy(), z=z.copy(), stats=stats, counters=cnt, K=list(K), ml=ml)

    for iters in range(opt.maxiters + 1):
        f, yv = lse(x)
        J = jac(yv)
        gap = float(s @ z)
        rx = c + Ae.T @ y_ + J.T @ z
        resx = nrm(rx)
        ry = Ae @ x - b
        resy = nrm(ry)
        rz = s.copy()
        rz[:m] += f
        rz[m:] += Ge @ x - h
        resznl, reszl = nrm(rz[:m]), nrm(rz[m:])
        pcost = float(c @ x)
        dcost = pcost + float(y_ @ ry) + float(z @ rz) - gap
        relgap = _ipm.relgap(gap, pcost, dcost)
        pres = float(np.sqrt(resy ** 2 + resznl ** 2 + reszl ** 2))
        dres = resx
        if iters == 0:
            resx0, resznl0 = max(1.0, resx), max(1.0, resznl)
            pres0, dres0 = max(1.0, pres), max(1.0, dres)
            gap0 = gap
            theta1, theta2, theta3 = 1.0 / gap0, 1.0 / resx0, 1.0 / resznl0
        phi = theta1 * gap + theta2 * resx + theta3 * resznl
        pres, dres = pres / pres0, dres / dres0
        if iters == opt.maxiters:                                               # first, as in cvxprog.py:729
            return finish(EXIT_MAXITERS, iters, gap, relgap, pcost, dcost, pres, dres)
        if pres <= opt.feastol and dres <= opt.feastol and (gap <= opt.abstol or (relgap is not None and relgap <= opt.reltol)):
            return finish(EXIT_OPTIMAL, iters, gap, relgap, pcost, dcost, pres, dres)

        if iters == 0:
            d = np.sqrt(s / z); di = 1.0 / d; lmbda = np.sqrt(s * z)
        lmbdasq = lmbda * lmbda
        try:
            factor(J, yv, z, di)
        except ArithmeticError:
            singular = False
            if iters == 0:
                return finish(EXIT_RANK, 0, *(None,) * 6)
            elif 0 < relaxed_iters < MAX_RELAXED_ITERS:
                cnt["restored"] += 1
                phi, gap = phi0, gap0
                d, di = sv.d.copy(), sv.di.copy()
                x, y_, s, z = sv.x.copy(), sv.y.copy(), sv.s.copy(), sv.z.copy()
                lmbda = sv.lmbda.copy()                                          # lmbdasq stays (cvxprog.py:807)
                rx, ry, rz = sv.rx.copy(), sv.ry.copy(), sv.rz.copy()
                resx, resznl = nrm(rx), nrm(rz[:m])
                relaxed_iters = -1
                f, yv = lse(x)
                J = jac(yv)
                try:
                    factor(J, yv, z, di)
                except ArithmeticError:
                    singular = True
            else:
                singular = True
            if singular:
                return finish(EXIT_SINGULAR, iters, gap, relgap, pcost, dcost, pres, dres)

        sigma, eta = 0.0, 0.0
        try:
            for i in (0, 1):
                mu = gap / N
                ds = -lmbdasq + sigma * mu
                # f4_no_ir (cvxprog.py:858-883)
                ds = ds / lmbda
                dx, dy, dz = ksolve(J, di, (-1.0 + eta) * rx, (-1.0 + eta) * ry, (-1.0 + eta) * rz - d * ds)
                ds = ds - dz
                dsdz = float(ds @ dz)
                dz2, ds2 = di * dz, d * ds
                ds, dz = ds / lmbda, dz / lmbda
                t = max(0.0, float(max(-ds)), float(max(-dz)))
                step = _ipm.step_length(t, 1)
                phi = theta1 * gap + theta2 * resx + theta3 * resznl
                if i == 0:
                    dphi = -phi
                else:
                    dphi = -theta1 * (1 - sigma) * gap - theta2 * (1 - eta) * resx - theta3 * (1 - eta) * resznl
                halvings, backtrack = 0, True

                def halve():
                    nonlocal step, halvings
                    step *= BETA
                    halvings += 1
                    cnt["max_halvings"] = max(cnt["max_halvings"], halvings)
                    if halvings == MAX_HALVINGS:
                        raise _Halvings()

                while backtrack:
                    newx, newy = x + step * dx, y_ + step * dy
                    newz, news = z + step * dz2, s + step * ds2
                    newf, newyv = lse(newx)
                    newrx = c + Ae.T @ newy + jac(newyv).T @ newz
                    newresx = nrm(newrx)
                    newresznl = nrm(news[:m] + newf)
                    newgap = (1.0 - (1.0 - sigma) * step) * gap + step ** 2 * dsdz
                    newphi = theta1 * newgap + theta2 * newresx + theta3 * newresznl
                    if i == 0:
                        if newgap <= (1.0 - ALPHA * step) * gap and (0 <= relaxed_iters < MAX_RELAXED_ITERS or
                                                                       newphi <= phi + ALPHA * step * dphi):
                            backtrack = False
                            sigma = min(newgap / gap, (newgap / gap) ** _ipm.EXPON)
                            eta = 0.0
                        else:
                            halve()
                    else:
                        if relaxed_iters == -1:
                            if newphi <= phi + ALPHA * step * dphi:
                                backtrack = False
                            else:
                                halve()
                        elif relaxed_iters == 0:
                            if newphi <= phi + ALPHA * step * dphi:
                                relaxed_iters = 0
                            else:
                                cnt["saved"] += 1
                                phi0, dphi0, gap0, step0 = phi, dphi, gap, step
                                sv = types.SimpleNamespace(d=d.copy(), di=di.copy(), x=x.copy(), dx=dx.copy(), y=y_.copy(), dy=dy.copy(),
                                                           s=s.copy(), z=z.copy(), ds=ds.copy(), dz=dz.copy(), ds2=ds2.copy(),
                                                           dz2=dz2.copy(), lmbda=lmbda.copy(), lmbdasq=lmbdasq.copy(), rx=rx.copy(),
                                                           ry=ry.copy(), rz=rz.copy())
                                dsdz0, sigma0, eta0 = dsdz, sigma, eta
                                relaxed_iters = 1
                            backtrack = False
                        elif 0 <= relaxed_iters < MAX_RELAXED_ITERS:
                            if newphi <= phi0 + ALPHA * step0 * dphi0:
                                relaxed_iters = 0
                            else:
                                relaxed_iters += 1
                                cnt["relaxed_inc"] += 1
                            backtrack = False
                        elif relaxed_iters == MAX_RELAXED_ITERS:
                            if newphi <= phi0 + ALPHA * step0 * dphi0:
                                backtrack = False
                                relaxed_iters = 0
                            else:
                                cnt["resumed"] += 1
                                phi, dphi, gap, step = phi0, dphi0, gap0, step0
                                d, di = sv.d.copy(), sv.di.copy()
                                x, dx, y_, dy = sv.x.copy(), sv.dx.copy(), sv.y.copy(), sv.dy.copy()
                                s, z, ds, dz = sv.s.copy(), sv.z.copy(), sv.ds.copy(), sv.dz.copy()
                                ds2, dz2 = sv.ds2.copy(), sv.dz2.copy()
                                lmbda = sv.lmbda.copy()
                                dsdz, sigma, eta = dsdz0, sigma0, eta0
                                relaxed_iters = -1
                if halvings:
                    cnt["backtracks"] += 1
        except _Halvings:
            cnt["backtracks"] += 1
            return finish(EXIT_LINESEARCH, iters, gap, relgap, pcost, dcost, pres, dres)

        # the step and the scaling update (misc.py:444-464)
        x = x + step * dx
        y_ = y_ + step * dy
        rs, rzz = np.sqrt((1.0 + step * ds) * lmbda), np.sqrt((1.0 + step * dz) * lmbda)
        d = d * rs / rzz
        di = 1.0 / d
        lmbda = rs * rzz
        s, z = d * lmbda, di * lmbda
        gap = float(lmbda @ lmbda)
    raise AssertionError("unreachable")


# ---- members -------------------------------------------------------------------------------------------------------------------
def members(n, K, ml, p, B, seed, delta=0.5, spread=None, free=False):
    """B members with matrices of their own: F (B, l, n), g (l x B), G (B, ml, n), h (ml x B), A (B, p, n), b (p x B).  A point xbar
    is strictly feasible for every row: g is shifted block by block so that f_i(xbar) = -delta, h = G xbar + U(0.5, 1.5),
    b = A xbar.  One device keeps the optimum finite, the first that the shape allows: box rows [I; -I] at the head of G
    (ml >= 2n); a block of at least n + 1 terms whose rows are centred, so that its log-sum-exp grows in every direction; with
    one-term blocks only (a linear program) an objective row that is minus a positive combination of the constraint rows plus a
    combination of the rows of A, so that the dual is feasible; free=True asks for none of them (the program is then unbounded or
    its S singular).  The rows of A are orthonormal.  spread: (rows, values) added to g before the shift, the same for every member."""
    rng = np.random.default_rng(seed)
    K = list(K)
    l, m = sum(K), len(K)
    off = np.concatenate([[0], np.cumsum(K)]).astype(int)
    F = rng.standard_normal((B, l, n))
    g = rng.standard_normal((B, l))
    G = rng.standard_normal((B, ml, n))
    A = rng.standard_normal((B, p, n))
    if p:
        A = np.linalg.qr(A.transpose(0, 2, 1))[0].transpose(0, 2, 1)             # orthonormal rows
    big = [i for i in range(m) if K[i] >= n + 1]
    if ml >= 2 * n:
        G[:, :n] = np.eye(n); G[:, n:2 * n] = -np.eye(n)
    elif big:
        i = big[0]
        F[:, off[i]:off[i + 1]] -= F[:, off[i]:off[i + 1]].mean(axis=1, keepdims=True)
    elif m > 1 and max(K) == 1:
        lam, nu = rng.uniform(0.5, 1.5, (B, m - 1)), rng.standard_normal((B, p))
        F[:, 0] = -np.einsum("bi,bin->bn", lam, F[:, 1:]) - np.einsum("bi,bin->bn", nu, A)
    elif not free:
        raise ValueError("members: nothing bounds this shape")
    if spread is not None:
        g[:, spread[0]] += spread[1]
    xbar = 0.3 * rng.standard_normal((B, n))
    for i in range(1, m):
        u = np.einsum("bkn,bn->bk", F[:, off[i]:off[i + 1]], xbar) + g[:, off[i]:off[i + 1]]
        mx = u.max(axis=1, keepdims=True)
        g[:, off[i]:off[i + 1]] -= mx + np.log(np.exp(u - mx).sum(axis=1, keepdims=True)) + delta
    h = np.einsum("bkn,bn->bk", G, xbar) + rng.uniform(0.5, 1.5, (B, ml))
    b = np.einsum("bkn,bn->bk", A, xbar)
    return types.SimpleNamespace(n=n, K=K, ml=ml, p=p, B=B, F=F, g=np.asfortranarray(g.T), G=G if ml else None,
                                 h=np.asfortranarray(h.T) if ml else None, A=A if p else None, b=np.asfortranarray(b.T) if p else None)


def member_args(M, k):
    return (M.K, M.F[k], M.g[:, k], None if M.G is None else M.G[k], None if M.h is None else M.h[:, k],
            None if M.A is None else M.A[k], None if M.b is None else M.b[:, k])


def restate(M, options=None, dtype=np.float64, which=None, linsolve=False, reverse=False):
    return [solve_member(*member_args(M, k), options=options, dtype=dtype, linsolve=linsolve, reverse=reverse)
            for k in (range(M.B) if which is None else which)]


def batch_args(M, which=None):
    """The arguments of solvers.gp_batch for the members `which` (all by default) of a batch from members()."""
    w = list(range(M.B)) if which is None else list(which)
    sub = lambda a: None if a is None else np.ascontiguousarray(a[w])           # noqa: E731
    col = lambda a: None if a is None else np.asfortranarray(a[:, w])           # noqa: E731
    return M.K, sub(M.F), col(M.g), sub(M.G), col(M.h), sub(M.A), col(M.b)


# ---- the batches of tests/test_gp_batch_gpu.py; tests/test_gp_batch_cpu.py certifies them -------------------------------------------
TILE = 32                                                                     # GPB_TILE of csrc/gp_batch.hpp
CORNER_K = [300, 200, 140, 64, 64]                                            # l = 768
# name: (n, K, ml, p, B, seed)
EDGE_OPTIONS = {
    # A x = b pins x and no row of G is active, so cond(S) grows like 1 / gap^2: with the default tolerances float64 loses a pivot
    # of K in the last iteration where longdouble does not (exit 2 against 0).  The batch stops two digits earlier.
    "n63_p63": {"abstol": 1e-4, "reltol": 1e-3, "feastol": 1e-5},
}
EDGES = {
    "n1_k1": (1, [1], 0, 0, 8, 3001),                                         # S has rank 1 of 2: every member ends with exit 3
    "one_term_blocks": (2, [1, 1, 1], 0, 1, 8, 3002),
    "k63_64_65": (5, [63, 64, 65], 3, 0, 8, 3003),
    "l768": (6, [255, 256, 257], 0, 2, 8, 3004),
    "mixed_one_term": (4, [7, 1, 5, 1, 1, 9, 1], 9, 1, 10, 3005),
    "n63_p63": (63, [3, 2], 126, 63, 8, 3006),
    "N192_blocks": (3, [4] + [1, 2] * 95 + [1], 0, 0, 8, 3007),               # 192 blocks, l = 290
    "N192_linear": (6, [9, 3, 2], 189, 1, 8, 3008),
    "tile_minus": (4, [TILE - 6, 5], 8, 0, 8, 3009),                          # l = TILE - 1 staged Hessian rows
    "tile_exact": (4, [TILE - 5, 5], 8, 0, 8, 3010),
    "tile_plus": (4, [TILE - 4, 5], 8, 0, 8, 3011),
    "blocks_tile_plus": (3, [5] + [1] * TILE, 7, 0, 8, 3012),                 # TILE + 1 gradient rows
    "lds_corner": (63, CORNER_K, 192 - len(CORNER_K), 63, 8, 3013),
}
SPREAD = ("spread700", (3, [5, 1, 3, 4], 6, 1, 8, 3014), ([0, 1, 2, 5, 6, 7, 9, 12], [700.0, -700.0, 650.0, 720.0, -710.0, 705.0, -690.0, 700.0]))
INDEPENDENCE = ((6, [5, 3, 2], 12, 1), 300, 3015)
MIXED = ((4, [5, 3], 8, 1), 9, 3016)
# shape, B, seed, delta: found by search on the CPU.  Over BRANCHES the line search backtracks (up to 12 halvings), saves its state,
# counts relaxed iterations and resumes a saved line search at MAX_RELAXED_ITERS; over RESTORE a factorisation fails after a relaxed
# line search and the saved state is restored (cvxprog.py:778-840).  float64, longdouble and the float64 runs with other roundings
# (linsolve, and for the restore reverse, which keeps the failed pivot) take the same branches in every member.  A failed pivot sits
# on a rounding edge by its nature: of 600 seeds four passed all of that, each with one restore among its 8 members.
BRANCHES = ((8, [9, 3, 3, 2], 4, 1), 12, 4084, 5.0)
RESTORE = ((6, [7, 2, 2], 0, 2), 8, 4200, 5.0)
RESTORE2 = ((6, [7, 2, 2], 0, 2), 8, 4214, 5.0)
TIMING = (12, [6, 4, 4, 3, 3, 2], 24, 2)


@functools.lru_cache(maxsize=None)
def edge(name):
    n, K, ml, p, B, seed = EDGES[name]
    return members(n, K, ml, p, B, seed, free=name == "n1_k1")


@functools.lru_cache(maxsize=None)
def spread_batch():
    n, K, ml, p, B, seed = SPREAD[1]
    return members(n, K, ml, p, B, seed, spread=SPREAD[2])


@functools.lru_cache(maxsize=None)
def shaped(shape, B, seed, delta=0.5):
    n, K, ml, p = shape
    return members(n, tuple(K), ml, p, B, seed, delta=delta)


def named(name):
    if name == "spread700":
        return spread_batch()
    if name == "independence":
        return shaped((INDEPENDENCE[0][0], tuple(INDEPENDENCE[0][1])) + INDEPENDENCE[0][2:], *INDEPENDENCE[1:])
    if name == "mixed":
        return shaped((MIXED[0][0], tuple(MIXED[0][1])) + MIXED[0][2:], *MIXED[1:])
    if name in ("branches", "restore", "restore2"):
        spec = {"branches": BRANCHES, "restore": RESTORE, "restore2": RESTORE2}[name]
        return shaped((spec[0][0], tuple(spec[0][1])) + spec[0][2:], *spec[1:])
    return edge(name)


@functools.lru_cache(maxsize=None)
def restated(name, precision="longdouble", maxiters=None, which=None, linsolve=False, reverse=False):
    """The restated results of named(name), computed once per process and left unchanged."""
    opts = dict(EDGE_OPTIONS.get(name, {}))
    if maxiters is not None:
        opts["maxiters"] = maxiters
    return restate(named(name), opts, getattr(np, precision), which, linsolve, reverse)
