"""Front matter shared by the interior-point drivers (lp.conelp, lp.coneqp, cone.conelp, cone.coneqp, and cvx.cpl for its
options, refinement wrapper and closing lines): option defaults and the reference's checks of them, conversion and size checks
of the problem data, the operators x -> G x, A x, the iterative-refinement wrappers around a driver's Newton solve, and the
result dictionaries with the progress and closing lines (coneprog.py:425-575, 1211-1235, 1768-1975, 2330-2347;
cvxprog.py:392-424, 939-956).  `options` and `problem` are pure host code: they run before a device is asked for.

The two algorithms are written here once, on host scalars: `conelp_start` / `conelp_loop` (coneprog.py:662-1436) and `coneqp_start` /
`coneqp_loop` (coneprog.py:2044-2547).  The vectors and launches belong to an engine -- four in lp.py and one in cone.py for conelp,
one each for coneqp -- so this module never asks for a device either; tests/test_lp_loop_cpu.py and tests/test_qp_loop_cpu.py run
the loops on numpy engines.  Both starts ask an engine for what depends on the cone:
  factor_identity(needed)  the KKT factorisation with W = I (needed False: the caller gave both starting points)
  start_solve(x, y, z)     a KKT solve with that factor
  max_step(v), nrm2(v), dot(u, v), add_e(v, a), symm(v)
                           the largest step, the cone norm and inner product, v += a e, and the symmetrisation of 's' blocks."""
import collections
import math
import os
import sys
import time
import types

import numpy as np

from . import base

_TRACE = os.environ.get("KVX_LP_TRACE", "0") not in ("", "0")      # per-iteration wall times of conelp on stderr
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


# what an interior-point loop returns: stats = (gap, relgap, pcost, dcost, pres, dres[, pinfres, dinfres]); phase_seconds: conelp only
Outcome = collections.namedtuple("Outcome", "status iterations stats msg phase_seconds")


def conelp_start(e, opt, primalstart, dualstart, res0):
    """The starting point of conelp (coneprog.py:662-842) in the vectors of engine `e`: the KKT system with W = I, or what the caller
    gives.  Returns s'z, or the Outcome if the computed point is optimal already."""
    x, y, s, z, cv, bv, hv = e.x, e.y, e.s, e.z, e.cv, e.bv, e.hv
    try:
        e.factor_identity(primalstart is None or dualstart is None)
    except ArithmeticError:
        raise ValueError(e.rank_msg)
    if primalstart is None:
        x.fill(0.0); e.dy.copy_from(bv); s.copy_from(hv)
        e.start_solve(x, e.dy, s)
        s.scal(-1.0)
    else:                                                        # coneprog.py:703-705
        x.set(vector(primalstart["x"], "primalstart['x']", x.n)); s.set(vector(primalstart["s"], "primalstart['s']", s.n))
    ts = e.max_step(s)
    if ts >= 0 and primalstart is not None:
        raise ValueError("initial s is not positive")
    if dualstart is None:
        e.dx.copy_from(cv).scal(-1.0); y.fill(0.0); z.fill(0.0)
        e.start_solve(e.dx, y, z)
    else:                                                        # coneprog.py:731-733
        if e.p and "y" in dualstart:
            y.set(vector(dualstart["y"], "dualstart['y']", e.p))
        elif e.p:
            y.fill(0.0)
        z.set(vector(dualstart["z"], "dualstart['z']", z.n))
    tz = e.max_step(z)
    if tz >= 0 and dualstart is not None:
        raise ValueError("initial z is not positive")
    nrms, nrmz = e.nrm2(s), e.nrm2(z)
    if primalstart is None and dualstart is None:
        gap = e.dot(s, z)
        pcost = cv.dot(x)
        dcost = -bv.dot(y) - e.dot(hv, z)
        rgap = relgap(gap, pcost, dcost)
        if ts <= 0 and tz <= 0 and (gap <= opt.abstol or (rgap is not None and rgap <= opt.reltol)):
            rx, ry, rz = e.rx, e.ry, e.rz
            e.symm(s); e.symm(z)
            rx.copy_from(cv); e.Af(y, rx, trans="T", alpha=1.0, beta=1.0); e.Gf(z, rx, trans="T", alpha=1.0, beta=1.0)
            resx = rx.nrm2()
            ry.copy_from(bv); e.Af(x, ry, trans="N", alpha=1.0, beta=-1.0)
            resy = ry.nrm2()
            e.Gf(x, rz, trans="N"); rz.axpy(s); rz.axpy(hv, -1.0)
            resz = e.nrm2(rz)
            return Outcome("optimal", 0, (gap, rgap, pcost, dcost, max(resy / res0[1], resz / res0[2]), resx / res0[0], None, None),
                           None, [0.0, 0.0, 0.0])
    # (coneprog.py:806-842: a computed start is pushed into the cone, a given one is taken as it is)
    if primalstart is None and ts >= -1e-8 * max(nrms, 1.0):
        e.add_e(s, 1.0 + ts)
    if dualstart is None and tz >= -1e-8 * max(nrmz, 1.0):
        e.add_e(z, 1.0 + tz)
    e.lmbda.fill(0.0)
    return e.dot(s, z)


def conelp_loop(engine, opt, degree, gap, res0):
    """The interior-point loop of conelp (coneprog.py:859-1436) on a cone of the given degree, from a starting point with
    tau = kappa = 1 and s'z = gap; res0 = (resx0, resy0, resz0).  Host scalars only: the vectors belong to `engine`, which is asked for
      stats(tau)        the squared norms of hrx, rx, hry, ry, hrz, rz, then c'x, b'y, h'z and lmbda'lmbda
      scaling()         the NT scaling of the first iteration; returns lmbda'lmbda
      direction(i, ...) whatever of direction i (0: predictor, with the factorisation and the constant system; 1: corrector)
                        can report a failed factorisation, by ArithmeticError
      bounds(i)         the rest of direction i; returns (dtau, dkappa, max_step(ds), max_step(dz))
      update(step, tau) the step, the new scaling, and s, z of the next iteration; tau is the new one
      scale(a, b)       x, s *= a and y, z *= b (None: left alone)
    and returns an Outcome; the iterates are left scaled as the reference returns them."""
    resx0, resy0, resz0 = res0
    tau, kappa = 1.0, 1.0
    dg = dgi = lmbda_g = 1.0
    phase = [0.0, 0.0, 0.0]
    for iters in range(opt.maxiters + 1):
        # residuals (coneprog.py:861-896): their norms and the objectives
        v_hrx, v_rx, v_hry, v_ry, v_hrz, v_rz, cx, by, hz, lam2 = engine.stats(tau)
        t_now = time.perf_counter()
        if iters > 0:
            phase[2] += t_now - t_mark
        t_mark = t_now
        hresx, resx = math.sqrt(v_hrx), math.sqrt(v_rx) / tau
        hresy, resy = math.sqrt(v_hry), math.sqrt(v_ry) / tau
        hresz, resz = math.sqrt(v_hrz), math.sqrt(v_rz) / tau
        if iters > 0:
            gap = (math.sqrt(lam2) / tau) ** 2           # (coneprog.py:1436; lmbda of the previous update)
        rt = kappa + cx + by + hz
        pcost, dcost = cx / tau, -(by + hz) / tau
        rgap = relgap(gap, pcost, dcost)
        pres = max(resy / resy0, resz / resz0)
        dres = resx / resx0
        pinfres = hresx / resx0 / (-hz - by) if hz + by < 0.0 else None
        dinfres = max(hresy / resy0, hresz / resz0) / (-cx) if cx < 0.0 else None
        if opt.show:
            progress(iters, pcost, dcost, gap, pres, dres, kappa / tau)

        if (pres <= opt.feastol and dres <= opt.feastol and (gap <= opt.abstol or (rgap is not None and rgap <= opt.reltol))) \
                or iters == opt.maxiters:
            engine.scale(1.0 / tau, 1.0 / tau)
            if iters == opt.maxiters:
                return Outcome("unknown", iters, (gap, rgap, pcost, dcost, pres, dres, pinfres, dinfres), MAXITERS_MSG, phase)
            return Outcome("optimal", iters, (gap, rgap, pcost, dcost, pres, dres, None, None), None, phase)
        elif pinfres is not None and pinfres <= opt.feastol:
            engine.scale(None, 1.0 / (-hz - by))
            return Outcome("primal infeasible", iters, (None, None, None, 1.0, None, None, pinfres, None), None, phase)
        elif dinfres is not None and dinfres <= opt.feastol:
            engine.scale(1.0 / (-cx), None)
            return Outcome("dual infeasible", iters, (None, None, -1.0, None, None, None, None, dinfres), None, phase)

        # NT scaling at the first iteration (coneprog.py:1031-1043 -> misc.py:284-287)
        if iters == 0:
            lam2 = engine.scaling()
            dg = math.sqrt(kappa / tau)
            dgi = math.sqrt(tau / kappa)
            lmbda_g = math.sqrt(tau * kappa)
        mu = (lam2 + lmbda_g ** 2) / (1 + degree)
        sigma = wkappa3 = 0.0
        for i in (0, 1):
            try:
                engine.direction(i, sigma, mu, rt, dg, dgi, lmbda_g, wkappa3)
            except ArithmeticError:
                engine.scale(1.0 / tau, 1.0 / tau)
                return Outcome("unknown", iters, (gap, rgap, pcost, dcost, pres, dres, pinfres, dinfres), SINGULAR_MSG, phase)
            dtau, dkappa, ts, tz = engine.bounds(i)
            t_now = time.perf_counter()
            phase[i] += t_now - t_mark
            if _TRACE:
                print("conelp iteration %d direction %d: %.0f us" % (iters, i, 1e6 * (t_now - t_mark)), file=sys.stderr)
            t_mark = t_now
            if i == 0:
                wkappa3 = dtau * dkappa
            # step to the boundary (coneprog.py:1314-1331)
            tt, tk = -dtau / lmbda_g, -dkappa / lmbda_g
            step = step_length(max(0.0, ts, tz, tt, tk), i)
            if i == 0:
                sigma = (1.0 - step) ** EXPON

        # update (coneprog.py:1336-1436)
        dg *= math.sqrt(1.0 - step * tk) / math.sqrt(1.0 - step * tt)
        dgi = 1.0 / dg
        lmbda_g *= math.sqrt(1.0 - step * tt) * math.sqrt(1.0 - step * tk)
        kappa, tau = lmbda_g / dgi, lmbda_g * dgi
        engine.update(step, tau)
    raise AssertionError("unreachable")


def coneqp_start(e, initvals, label="initvals['{}']"):
    """The starting point of coneqp (coneprog.py:2044-2150) in the vectors of engine `e`: the KKT system with W = I and right-hand side
    (-q, b, h), s = -z, both pushed into the cone; or the caller's values, a missing x or y as 0 and a missing s or z as the cone's
    identity e.  `label` names a vector of the wrong size.  Returns s'z."""
    x, y, s, z = e.x, e.y, e.s, e.z
    if initvals is None:
        try:
            e.factor_identity(True)
        except ArithmeticError:
            raise ValueError("Rank(A) < p or Rank([P; A; G]) < n")
        x.copy_from(e.qv).scal(-1.0); y.copy_from(e.bv); z.copy_from(e.hv)
        try:
            e.start_solve(x, y, z)
        except ArithmeticError:
            raise ValueError("Rank(A) < p or Rank([P; G; A]) < n")
        s.copy_from(z).scal(-1.0)
        for v in (s, z):
            t = e.max_step(v)
            if t >= -1e-8 * max(e.nrm2(v), 1.0):
                e.add_e(v, 1.0 + t)
    else:
        for k, v, size in (("x", x, x.n), ("y", y, e.p)):
            if k in initvals and size:
                v.set(vector(initvals[k], label.format(k), size))
            else:
                v.fill(0.0)
        for k, v in (("s", s), ("z", z)):
            if k in initvals:
                v.set(vector(initvals[k], label.format(k), v.n))
                if e.max_step(v) >= 0:
                    raise ValueError("initial %s is not positive" % k)
            else:
                e.add_e(v.fill(0.0), 1.0)
    return e.dot(s, z)


def coneqp_loop(engine, opt, degree, gap, res0):
    """The interior-point loop of coneqp (coneprog.py:2160-2547) on a cone of the given degree from a starting point with s'z = gap;
    res0 = (resx0, resy0, resz0).  Host scalars only: the vectors belong to `engine`, which is asked for
      stats()           x'(Px + q), x'q, the squared norms of rx, ry, rz, then y'ry and z'rz
      scaling()         the NT scaling of the first iteration
      factor()          the KKT factorisation in the current scaling; ArithmeticError if it fails
      direction(i, sigma_mu, eta, correction)
                        direction i (0: affine scaling, 1: combined; with the Mehrotra term if `correction`) scaled by lmbda;
                        returns (ds'dz, max_step(ds), max_step(dz)); ArithmeticError if its solve fails
      update(step)      the step, the new scaling, and s, z of the next iteration; returns lmbda'lmbda
    and returns an Outcome.  A failed factorisation or solve is a ValueError at the first iteration and "unknown" later
    (coneprog.py:2236-2247, 2401-2412)."""
    resx0, resy0, resz0 = res0
    for iters in range(opt.maxiters + 1):
        # residuals and objectives (coneprog.py:2167-2203)
        xPq, xq, v_rx, v_ry, v_rz, yry, zrz = engine.stats()
        f0 = 0.5 * (xPq + xq)
        resx, resy, resz = math.sqrt(v_rx), math.sqrt(v_ry), math.sqrt(v_rz)
        pcost = f0
        dcost = f0 + yry + zrz - gap
        rgap = relgap(gap, pcost, dcost)
        pres, dres = max(resy / resy0, resz / resz0), resx / resx0
        if opt.show:
            progress(iters, pcost, dcost, gap, pres, dres)
        stats = (gap, rgap, pcost, dcost, pres, dres)
        if iters == opt.maxiters:
            return Outcome("unknown", iters, stats, MAXITERS_MSG, None)
        if pres <= opt.feastol and dres <= opt.feastol and (gap <= opt.abstol or (rgap is not None and rgap <= opt.reltol)):
            return Outcome("optimal", iters, stats, None, None)

        # scaling (coneprog.py:2230-2231), KKT factorisation, the two directions (coneprog.py:2367-2451)
        if iters == 0:
            engine.scaling()
        mu = gap / degree
        sigma, eta = 0.0, 0.0
        try:
            engine.factor()
            for i in (0, 1):
                dsdz, ts, tz = engine.direction(i, sigma * mu, eta, opt.correction)
                step = step_length(max(0.0, ts, tz), i)
                if i == 0:
                    sigma = min(1.0, max(0.0, 1.0 - step + dsdz / gap * step ** 2)) ** EXPON
                    eta = 0.0
        except ArithmeticError:
            if iters == 0:
                raise ValueError("Rank(A) < p or Rank([P; A; G]) < n")
            return Outcome("unknown", iters, stats, SINGULAR_MSG, None)
        gap = engine.update(step)
    raise AssertionError("unreachable")
