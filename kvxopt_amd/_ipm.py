"""Front matter shared by the interior-point drivers (lp.conelp, lp.coneqp, cone.conelp, cone.coneqp, and cvx.cpl for its
options, refinement wrapper and closing lines): option defaults and the reference's checks of them, conversion and size checks
of the problem data, the operators x -> G x, A x, the iterative-refinement wrappers around a driver's Newton solve, and the
result dictionaries with the progress and closing lines (coneprog.py:425-575, 1211-1235, 1768-1975, 2330-2347;
cvxprog.py:392-424, 939-956).  `options` and `problem` are pure host code: they run before a device is asked for."""
import types

import numpy as np

from . import base

_INT, _NUM = (int, np.integer), (float, int, np.floating, np.integer)
EXPON = 3          # coneprog.py:423
STEP = 0.99        # coneprog.py:424


def options(user, dims, qp=False):
    """Defaults updated by `user`, checked as the reference checks them (coneprog.py:425-455, 502-509 / 1768-1801, 1862-1868);
    the default of 'refinement' is 1 with 'q' or 's' cones and 0 without."""
    o = {"maxiters": 100, "abstol": 1e-7, "reltol": 1e-6, "feastol": 1e-7, "show_progress": False, "refinement": None,
         "use_correction": True}
    o.update(user or {})
    if not isinstance(o["maxiters"], _INT) or o["maxiters"] < 1:
        raise ValueError("options['maxiters'] must be a positive integer")
    for k in ("abstol", "reltol"):
        if not isinstance(o[k], _NUM):
            raise ValueError("options['%s'] must be a scalar" % k)
    if o["reltol"] <= 0.0 and o["abstol"] <= 0.0:
        raise ValueError("at least one of options['reltol'] and options['abstol'] must be positive")
    if not isinstance(o["feastol"], _NUM) or o["feastol"] <= 0.0:
        raise ValueError("options['feastol'] must be a positive scalar")
    ref = o["refinement"]
    if ref is None:
        ref = 1 if (dims.get("q") or dims.get("s")) else 0
    elif not isinstance(ref, _INT) or ref < 0:
        raise ValueError("options['refinement'] must be a nonnegative integer")
    return types.SimpleNamespace(maxiters=o["maxiters"], abstol=o["abstol"], reltol=o["reltol"], feastol=o["feastol"],
                                 show=o["show_progress"], refinement=int(ref), correction=bool(o["use_correction"]) if qp else None)


def check_dims(dims):
    """The cone dimensions as {'l', 'q', 's'} with the reference's checks (coneprog.py:494-500)."""
    dims = {"l": dims.get("l", 0), "q": list(dims.get("q") or []), "s": list(dims.get("s") or [])}
    if not isinstance(dims["l"], _INT) or dims["l"] < 0:
        raise TypeError("'dims['l']' must be a nonnegative integer")
    if [k for k in dims["q"] if not isinstance(k, _INT) or k < 1]:
        raise TypeError("'dims['q']' must be a list of positive integers")
    if [k for k in dims["s"] if not isinstance(k, _INT) or k < 0]:
        raise TypeError("'dims['s']' must be a list of nonnegative integers")
    return dims


def vector(v, name, size):
    a = base.flat(v)
    if a.size != size:
        raise TypeError("'%s' must be a 'd' matrix of size (%d,1)" % (name, size))
    return a


def problem(c, G, h, dims, A, b, P=None, qp=False):
    """The data of  minimize c'x [+ (1/2) x'Px]  s.t.  G x + s = h, A x = b  as contiguous float64 vectors and CCS triples
    (P by its lower triangle; A with p = 0 rows when absent), after the reference's size checks (coneprog.py:488-575,
    1836-1975).  dims None: the orthant of G's rows.  Returns a namespace n, p, dims, cdim, c, h, b, G, A, P."""
    c = base.flat(c)
    n = c.size
    Pl = base.lower_ccs(P, n) if qp else None
    Gm, Gn, Gp, Gi, Gx = base.ccs(G)
    dims = check_dims({"l": Gm} if dims is None else dims)
    cdim = dims["l"] + sum(dims["q"]) + sum(k * k for k in dims["s"])
    cdim_pckd = dims["l"] + sum(dims["q"]) + sum(k * (k + 1) // 2 for k in dims["s"])
    h = vector(h, "h", cdim)
    if (Gm, Gn) != (cdim, n):
        raise TypeError("'G' must be a 'd' matrix of size (%d, %d)" % (cdim, n))
    if A is None:
        p, Al = 0, (np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
    else:
        p, na, Ap, Ai, Ax = base.ccs(A)
        if na != n:
            raise TypeError("'A' must be a 'd' matrix with %d columns%s" % (n, "" if qp else " "))
        Al = (Ap, Ai, Ax)
    b = np.zeros(0) if b is None else base.flat(b)
    if b.size != p:
        raise TypeError("'b' must have length %d" % p)
    if p > n or (not qp and p + cdim_pckd < n):
        raise ValueError("Rank(A) < p or Rank([P; G; A]) < n" if qp else "Rank(A) < p or Rank([G; A]) < n")
    return types.SimpleNamespace(n=n, p=p, dims=dims, cdim=cdim, c=c, h=h, b=b, G=(Gp, Gi, Gx), A=Al, P=Pl)


class NoVec:
    """Stand-in for the empty y-blocks of p = 0: every vector operation is a no-op that launches nothing."""

    def __getattr__(self, name):
        return lambda *a, **k: self

    def dot(self, other):
        return 0.0

    def nrm2(self):
        return 0.0

    def get(self):
        return np.zeros(0)


def operators(Gd, Ad, trisc=None, tg=None):
    """Gf(u, v, trans, alpha, beta): v := alpha G u + beta v or alpha G' u + beta v; with 's' blocks (trisc: u -> trisc(u) in
    place, tg: a work vector) G' acts on the symmetric blocks as misc.sgemv does (misc.py:801-833).  Af likewise with A; p = 0
    (Ad None): v := beta v for trans 'T', nothing otherwise."""
    def Gf(u, v, trans="N", alpha=1.0, beta=0.0):
        if trans != "N" and trisc is not None:
            tg.copy_from(u)
            trisc(tg)
            u = tg
        Gd.gemv(u, v, trans=trans, alpha=alpha, beta=beta)

    def Af(u, v, trans="N", alpha=1.0, beta=0.0):
        if Ad is not None:
            Ad.gemv(u, v, trans=trans, alpha=alpha, beta=beta)
        elif trans == "T" and beta == 0.0:
            v.fill(0.0)
        elif trans == "T" and beta != 1.0:
            v.scal(beta)
    return Gf, Af


def f6(no_ir, res, nref, w, w2):
    """coneprog.py:1211-1235: f6_no_ir with nref steps of iterative refinement; w, w2: work (x, y, z, s) quadruples."""
    def f(bx, by, bz, btau, bs, bkappa):
        if nref:
            for t, u in zip(w, (bx, by, bz, bs)):
                t.copy_from(u)
            wtau, wkappa = btau[0], bkappa[0]
        no_ir(bx, by, bz, btau, bs, bkappa)
        for _ in range(nref):
            for t, u in zip(w2, w):
                t.copy_from(u)
            wx2, wy2, wz2, ws2 = w2
            wtau2, wkappa2 = [wtau], [wkappa]
            res(bx, by, bz, btau, bs, bkappa, wx2, wy2, wz2, wtau2, ws2, wkappa2)
            no_ir(wx2, wy2, wz2, wtau2, ws2, wkappa2)
            bx.axpy(wx2); by.axpy(wy2); bz.axpy(wz2)
            btau[0] += wtau2[0]
            bs.axpy(ws2)
            bkappa[0] += wkappa2[0]
    return f


def f4(no_ir, res, nref, w, w2):
    """coneprog.py:2330-2347: f4_no_ir with nref steps of iterative refinement; w, w2: work (x, y, z, s) quadruples."""
    def f(bx, by, bz, bs):
        if nref:
            for t, u in zip(w, (bx, by, bz, bs)):
                t.copy_from(u)
        no_ir(bx, by, bz, bs)
        for _ in range(nref):
            for t, u in zip(w2, w):
                t.copy_from(u)
            res(bx, by, bz, bs, *w2)
            no_ir(*w2)
            for t, u in zip((bx, by, bz, bs), w2):
                t.axpy(u)
    return f


def relgap(gap, pcost, dcost):
    """The relative gap of the reference's drivers (coneprog.py:898-903), None when neither objective has the sign it needs."""
    return gap / -pcost if pcost < 0.0 else (gap / dcost if dcost > 0.0 else None)


def step_length(t, i):
    """The step of direction i (0: predictor, 1: corrector) from the distance t to the boundary (coneprog.py:1322-1328)."""
    return 1.0 if t == 0.0 else (min(1.0, 1.0 / t) if i == 0 else min(1.0, STEP / t))


def progress(iters, pcost, dcost, gap, pres, dres, kt=None):
    """The reference's progress header and line (coneprog.py:904-910, 2205-2210); kt = kappa / tau for conelp."""
    if iters == 0:
        print("% 10s% 12s% 10s% 8s% 7s" % ("pcost", "dcost", "gap", "pres", "dres") + ("" if kt is None else " % 5s" % "k/t"))
    print("%2d: % 8.4e % 8.4e % 4.0e% 7.0e% 7.0e" % (iters, pcost, dcost, gap, pres, dres) + ("" if kt is None else "% 7.0e" % kt))


_CLOSING = {"optimal": "Optimal solution found.", "primal infeasible": "Certificate of primal infeasibility found.",
            "dual infeasible": "Certificate of dual infeasibility found."}
MAXITERS_MSG = "Terminated (maximum number of iterations reached)."
SINGULAR_MSG = "Terminated (singular KKT matrix)."


def _result(show, status, msg, x, y, s, z, stats, slacks, iters, nfactor, extra):
    if show:
        print(msg or _CLOSING[status])
    sol = {"x": x, "y": y, "s": s, "z": z, "status": status}
    sol.update(zip(("gap", "relative gap", "primal objective", "dual objective", "primal infeasibility", "dual infeasibility"), stats[:6]))
    sol["primal slack"], sol["dual slack"] = (None if t is None else -t for t in slacks)
    if len(stats) > 6:
        sol["residual as primal infeasibility certificate"], sol["residual as dual infeasibility certificate"] = stats[6:]
    sol.update({"iterations": iters, "factorizations": nfactor})
    sol.update(extra)
    return sol


def conelp_result(show, status, x, y, s, z, stats, ts, tz, iters, nfactor, msg=None, **extra):
    """The reference's result dictionary of conelp (coneprog.py:962-974 and its siblings) with numpy arrays; stats = (gap,
    relgap, pcost, dcost, pres, dres, pinfres, dinfres); x, s None for a primal, y, z None for a dual infeasibility certificate."""
    return _result(show, status, msg, x, y, s, z, stats, (ts, tz), iters, nfactor, extra)


def coneqp_result(show, status, x, y, s, z, stats, ts, tz, iters, nfactor, msg=None):
    """The reference's result dictionary of coneqp (coneprog.py:2216-2221); stats = (gap, relgap, pcost, dcost, pres, dres)."""
    return _result(show, status, msg, x, y, s, z, stats, (ts, tz), iters, nfactor, {})
