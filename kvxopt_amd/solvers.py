"""`kvxopt.solvers` names for the device-resident interior-point drivers of kvxopt_amd.lp (orthant cone) and kvxopt_amd.cone
(second-order and semidefinite cones):

    conelp(c, G, h, dims=None, A=None, b=None, primalstart=None, dualstart=None)     coneprog.py:420  (-> cone.conelp when dims
                                                                                     has 'q' or 's' blocks, coneprog.py:459, 504)
    socp(c, Gl, hl, Gq, hq, A=None, b=None, primalstart=None, dualstart=None)        coneprog.py:3044
    sdp(c, Gl, hl, Gs, hs, A=None, b=None, primalstart=None, dualstart=None)         coneprog.py:3597
    coneqp(P, q, G, h, dims=None, A=None, b=None, initvals=None)                     coneprog.py:1440 (-> cone.coneqp when dims
                                                                                     has 'q' or 's' blocks, coneprog.py:1806-1807)
    lp(c, G, h, A=None, b=None, primalstart=None, dualstart=None)                    coneprog.py:2551 (-> conelp)
    qp(P, q, G, h, A=None, b=None, initvals=None)                                    coneprog.py:4120 (-> coneqp)
    cpl(c, F, G=None, h=None, dims=None, A=None, b=None)                             cvxprog.py:35   (-> cvx.cpl, 'l' rows only)
    cp(F, G=None, h=None, dims=None, A=None, b=None)                                 cvxprog.py:1359 (-> cvx.cp: cpl on the epigraph form)
    gp(K, F, g, G=None, h=None, A=None, b=None)                                      cvxprog.py:1967 (-> cvx.gp: kvx_gp_eval_dev, cp)
    qp_batch(P, q, G, h, A=None, b=None, options=None)                               no counterpart: B small dense QPs in one launch
                                                                                     (-> qpbatch.qp_batch; reads its own `options` only)
    qp_batch_vjp(P, q, G, h, A=None, b=None, *, sol, gx, wrt=..., options=None)      no counterpart: the gradients of a loss through a
                                                                                     solved qp_batch, from its cotangent gx = dl/dx
    qp_batch_jvp(P, q, G, h, A=None, b=None, *, sol, dP=None, ..., db=None,          no counterpart: the directional derivative of the
                 options=None)                                                       solution of a solved qp_batch
                                                                                     (-> qpbatchdiff; options: 'refinement' 0..3 only)
    lp_batch(c, G, h, A=None, b=None, options=None)                                  no counterpart: B small dense LPs in one launch,
                                                                                     with conelp's infeasibility certificates
                                                                                     (-> lpbatch.lp_batch; reads its own `options` only)
    socp_batch(c, G, h, dims, A=None, b=None, options=None)                          no counterpart: B small dense SOCPs in one launch,
                                                                                     dims = {'l': ml, 'q': [...]} shared by the members
                                                                                     (-> socpbatch.socp_batch; reads its own `options` only)
    sdp_batch(c, G, h, dims, A=None, b=None, options=None)                           no counterpart: B small dense SDPs in one launch,
                                                                                     dims = {'l': ml, 's': [...]} shared by the members
                                                                                     (-> sdpbatch.sdp_batch; reads its own `options` only)
    conelp_batch(c, G, h, dims, A=None, b=None, options=None)                        no counterpart: B small dense cone programs in one
                                                                                     launch, dims = {'l': ml, 'q': [...], 's': [...]}
                                                                                     shared by the members
                                                                                     (-> conelpbatch.conelp_batch; reads its own `options` only)
    coneqp_batch(P, q, G, h, dims, A=None, b=None, options=None)                     no counterpart: B small dense cone QPs in one
                                                                                     launch, dims = {'l': ml, 'q': [...], 's': [...]}
                                                                                     shared by the members
                                                                                     (-> coneqpbatch.coneqp_batch; reads its own `options` only)
    coneqp_batch_vjp(P, q, G, h, dims, A=None, b=None, *, sol, gx, wrt=...,          no counterpart: the gradients of a loss through a
                     options=None)                                                   solved coneqp_batch, from its cotangent gx = dl/dx
    coneqp_batch_jvp(P, q, G, h, dims, A=None, b=None, *, sol, dP=None, ...,         no counterpart: the directional derivative of the
                     db=None, options=None)                                          solution of a solved coneqp_batch, after centring
                                                                                     (-> coneqpbatchdiff; options: 'refinement' 0..3,
                                                                                     'centering' 0..16 and 'centol' only)
    gp_batch(K, F, g, G=None, h=None, A=None, b=None, options=None)                  no counterpart: B small dense geometric programs
                                                                                     in one launch, K shared by the members
                                                                                     (-> gpbatch.gp_batch; reads its own `options` only)
    gp_batch_vjp(K, F, g, G=None, h=None, A=None, b=None, *, sol, gx, wrt=...,       no counterpart: the gradients of a loss through a
                 options=None)                                                       solved gp_batch, from its cotangent gx = dl/dx
    gp_batch_jvp(K, F, g, G=None, h=None, A=None, b=None, *, sol, dF=None, ...,      no counterpart: the directional derivative of the
                 db=None, options=None)                                              solution of a solved gp_batch
                                                                                     (-> gpbatchdiff; options: 'refinement' 0..3 only)
    options                                                                        the module-level dict of the reference

Like the reference, algorithm parameters come from `solvers.options` ('maxiters', 'abstol', 'reltol', 'feastol',
'refinement', 'show_progress'); a keyword `options=` overrides it per call.  `conelp / lp / coneqp / qp (..., kktsolver=f)`
take the reference's plug-in, a function `W -> g(x, y, z)` (coneprog.py:323-344, 1969-1981; host round trips per factorisation
and solve, lp.KKTUserHost) on the orthant; with 'q' / 's' cones the KKT system is misc.kkt_chol on the GPU (for coneqp with H = P)
and any `kktsolver` raises.  The named solvers ('ldl', 'ldl2', 'qr', 'chol', 'chol2') and `solver=` (external codes) are not part
of this path and raise -- except `lp / qp (..., solver='osqp')` (coneprog.py:2818-2906, 4391-4603), which run kvxopt_amd.osqp (ADMM on
one kept Cholesky factor) with the options of `options['osqp']`.  coneqp reads 'use_correction' as well.
"""
import numpy as np

from . import _ipm
from . import base as _base
from . import cone as _cone
from . import cvx as _cvx
from . import lp as _lp
from . import osqp as _osqp
from .conelpbatch import conelp_batch  # noqa: F401
from .coneqpbatch import coneqp_batch  # noqa: F401
from .coneqpbatchdiff import coneqp_batch_jvp, coneqp_batch_vjp  # noqa: F401
from .gpbatch import gp_batch  # noqa: F401
from .gpbatchdiff import gp_batch_jvp, gp_batch_vjp  # noqa: F401
from .lpbatch import lp_batch  # noqa: F401
from .qpbatch import qp_batch  # noqa: F401
from .qpbatchdiff import qp_batch_jvp, qp_batch_vjp  # noqa: F401
from .sdpbatch import sdp_batch  # noqa: F401
from .socpbatch import socp_batch  # noqa: F401

options = {}


def _opts(kw):
    o = {"show_progress": True}                          # the reference's default (coneprog.py:456, 1803)
    o.update(options)
    o.update(kw.pop("options", None) or {})
    if kw.pop("solver", None) is not None:
        raise NotImplementedError("kvxopt_amd.solvers runs misc.kkt_chol2 on the GPU; 'solver' is not selectable")
    if kw:
        raise TypeError("unexpected arguments: %s" % ", ".join(sorted(kw)))
    return o


def _kkt(kw):
    k = kw.pop("kktsolver", None)
    if k is not None and not callable(k):
        raise NotImplementedError("kvxopt_amd.solvers runs misc.kkt_chol2 on the GPU; the named KKT solver '%s' is not selectable "
                                  "(a function W -> f(x, y, z) is)" % k)
    return k


def conelp(c, G, h, dims=None, A=None, b=None, primalstart=None, dualstart=None, **kw):
    k = _kkt(kw)
    if dims is not None and (dims.get("q") or dims.get("s")):
        # the reference's own test for the general-cone path (coneprog.py:459, 504): misc.kkt_chol on the GPU
        if k is not None:
            raise NotImplementedError("conelp with 'q' / 's' cones runs misc.kkt_chol on the GPU; kktsolver is not selectable")
        return _cone.conelp(c, G, h, dims, A=A, b=b, options=_opts(kw), primalstart=primalstart, dualstart=dualstart)
    return _lp.conelp(c, G, h, dims=dims, A=A, b=b, options=_opts(kw), primalstart=primalstart, dualstart=dualstart, kktsolver=k)


def coneqp(P, q, G, h, dims=None, A=None, b=None, initvals=None, **kw):
    k = _kkt(kw)
    if dims is not None and (dims.get("q") or dims.get("s")):
        # the reference's default for these cones (coneprog.py:1806-1807): misc.kkt_chol with H = P, on the GPU
        if k is not None:
            raise NotImplementedError("coneqp with 'q' / 's' cones runs misc.kkt_chol on the GPU; kktsolver is not selectable")
        return _cone.coneqp(P, q, G, h, dims, A=A, b=b, initvals=initvals, options=_opts(kw))
    return _lp.coneqp(P, q, G, h, _opts(kw), None, A=A, b=b, initvals=initvals, kktsolver=k)


def _cvx_opts(kw):
    o = dict(options)
    o.update(kw.pop("options", None) or {})
    if kw:
        raise TypeError("unexpected arguments: %s" % ", ".join(sorted(kw)))
    return o


def cpl(c, F, G=None, h=None, dims=None, A=None, b=None, kktsolver=None, xnewcopy=None, xdot=None, xaxpy=None, xscal=None,
        ynewcopy=None, ydot=None, yaxpy=None, yscal=None, **kw):
    """solvers.cpl (cvxprog.py:35-1356): nonlinear convex program with a linear objective, 'l' rows only, on the GPU."""
    return _cvx.cpl(c, F, G, h, dims, A, b, kktsolver, xnewcopy, xdot, xaxpy, xscal, ynewcopy, ydot, yaxpy, yscal, options=_cvx_opts(kw))


def cp(F, G=None, h=None, dims=None, A=None, b=None, kktsolver=None, xnewcopy=None, xdot=None, xaxpy=None, xscal=None,
       ynewcopy=None, ydot=None, yaxpy=None, yscal=None, **kw):
    """solvers.cp (cvxprog.py:1359-1964): nonlinear convex program, through the epigraph form and cpl."""
    return _cvx.cp(F, G, h, dims, A, b, kktsolver, xnewcopy, xdot, xaxpy, xscal, ynewcopy, ydot, yaxpy, yscal, options=_cvx_opts(kw))


def gp(K, F, g, G=None, h=None, A=None, b=None, kktsolver=None, **kw):
    """solvers.gp (cvxprog.py:1967-2155): geometric program in convex form; F stays in HBM (kvx_gp_eval_dev)."""
    return _cvx.gp(K, F, g, G, h, A, b, kktsolver, options=_cvx_opts(kw))


def _osqp_args(kw):
    """The arguments of a `solver='osqp'` call: options['osqp'] of the keyword `options` or of the module's dict."""
    kw.pop("solver")
    kw.pop("kktsolver", None)                            # the reference ignores it on this path
    o = dict(options)
    o.update(kw.pop("options", None) or {})
    if kw:
        raise TypeError("unexpected arguments: %s" % ", ".join(sorted(kw)))
    return o.get("osqp", None)


def _sp(M):
    """A dense matrix as a sparse one with every entry stored (coneprog.py:2824-2827, 4398-4403); sparse and None unchanged."""
    if isinstance(M, np.ndarray):
        M = _base.matrix(np.asarray(M, dtype=np.float64).reshape(M.shape[0], -1))
    return _base._full_pattern(M)


def _mv(M, x, trans=False):
    """M x (or M'x) of a CCS matrix in numpy."""
    m, n, cp, ri, v = _base.ccs(M)
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(cp))
    if trans:
        return np.bincount(cols, weights=v * x[ri], minlength=n)
    return np.bincount(ri, weights=v * x[cols], minlength=m)


def _osqp_result(status, x, s, y, z, pcost, dcost, gap, relgap, pres, dres, pslack, dslack):
    return {"status": status, "x": x, "s": s, "y": y, "z": z, "primal objective": pcost, "dual objective": dcost, "gap": gap,
            "relative gap": relgap, "primal infeasibility": pres, "dual infeasibility": dres, "primal slack": pslack,
            "dual slack": dslack, "residual as primal infeasibility certificate": None,
            "residual as dual infeasibility certificate": None}


def _nrm2(v):
    return float(np.sqrt(np.dot(v, v)))


def _lp_osqp(c, G, h, A, b, opts):
    """solvers.lp(..., solver='osqp') (coneprog.py:2818-2906): osqp.qp, then the reference's dictionary from x, z, y."""
    G, A = _sp(G), _sp(A)
    status, x, z, y = _osqp.qp(c, G, h, A, b, options=opts)
    if status == "solved":
        status = "optimal"
    if status != "optimal":
        return _osqp_result(status, x, None, y, z, None, None, None, None, None, None, None, None)
    c, h = _flat(c), _flat(h)
    b = _flat(b) if A is not None and b is not None else np.zeros(0)
    pcost = float(np.dot(c, x))
    dcost = -float(np.dot(h, z)) - float(np.dot(b, y))
    s = h - _mv(G, x)
    gap = float(np.dot(s, z))
    rx = c + _mv(G, z, True) + (_mv(A, y, True) if b.size else 0.0)
    ry = b - _mv(A, x) if b.size else np.zeros(0)
    rz = _mv(G, x) + s - h
    pres = max(_nrm2(ry) / max(1.0, _nrm2(b)), _nrm2(rz) / max(1.0, _nrm2(h)))
    return _osqp_result(status, x, s, y, z, pcost, dcost, gap, _ipm.relgap(gap, pcost, dcost), pres, _nrm2(rx) / max(1.0, _nrm2(c)),
                        float(s.min()), float(z.min()))


def _qp_osqp(P, q, G, h, A, b, opts):
    """solvers.qp(..., solver='osqp') (coneprog.py:4391-4408, 4542-4603)."""
    if G is None:
        raise NotImplementedError("solvers.qp(..., solver='osqp') needs inequality constraints G x <= h (osqp.qp, osqp.c:455-460)")
    G, A, P = _sp(G), _sp(A), _sp(P)
    solsta, x, z, y = _osqp.qp(q, G, h, A, b, P, options=opts)
    if solsta != "solved":
        return _osqp_result("unknown", None, None, None, None, None, None, None, None, None, None, None, None)
    q, h = _flat(q), _flat(h)
    b = _flat(b) if A is not None and b is not None else np.zeros(0)
    s = h - _mv(G, x)
    n = q.size
    Pp, Pi, Px = _base.lower_ccs(P, n)                  # base.symv reads the lower triangle
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(Pp))
    off = Pi != cols
    rx = q + np.bincount(Pi, weights=Px * x[cols], minlength=n) + np.bincount(cols[off], weights=Px[off] * x[Pi[off]], minlength=n)
    pcost = 0.5 * (float(np.dot(x, rx)) + float(np.dot(x, q)))
    if b.size:
        rx = rx + _mv(A, y, True)
    rx = rx + _mv(G, z, True)
    ry = _mv(A, x) - b if b.size else np.zeros(0)
    rz = _mv(G, x) + s - h
    gap = float(np.dot(s, z))
    dcost = pcost + float(np.dot(y, ry)) + float(np.dot(z, rz)) - gap
    pres = max(_nrm2(ry) / max(1.0, _nrm2(b)), _nrm2(rz) / max(1.0, _nrm2(h)))
    return _osqp_result("optimal", x, s, y, z, pcost, dcost, gap, _ipm.relgap(gap, pcost, dcost), pres, _nrm2(rx) / max(1.0, _nrm2(q)),
                        float(s.min()), float(z.min()))


def lp(c, G, h, A=None, b=None, primalstart=None, dualstart=None, **kw):
    """solvers.lp (coneprog.py:2551-2790): conelp on the orthant, result keys as the reference returns them;
    solver='osqp': kvxopt_amd.osqp.qp with P = 0 (coneprog.py:2818-2906)."""
    if kw.get("solver", None) == "osqp":
        return _lp_osqp(c, G, h, A, b, _osqp_args(kw))
    sol = conelp(c, G, h, None, A, b, primalstart, dualstart, **kw)
    return sol


def qp(P, q, G, h, A=None, b=None, initvals=None, **kw):
    """solvers.qp (coneprog.py:4120-4330): coneqp on the orthant; solver='osqp': kvxopt_amd.osqp.qp (coneprog.py:4391-4603)."""
    if kw.get("solver", None) == "osqp":
        return _qp_osqp(P, q, G, h, A, b, _osqp_args(kw))
    return coneqp(P, q, G, h, None, A, b, initvals, **kw)


def _stack(blocks, n):
    """[B_0; B_1; ...] (dense or sparse, each with n columns) as one CCS spmatrix."""
    rows, cols, vals, off = [], [], [], 0
    for B in blocks:
        m, nb, cp, ri, v = _base.ccs(B)
        if nb != n:
            raise TypeError("the constraint matrices must have %d columns" % n)
        rows.append(ri + off)
        cols.append(np.repeat(np.arange(n, dtype=np.int64), np.diff(cp)))
        vals.append(v)
        off += m
    r = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    c = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    order = np.lexsort((r, c))
    cp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(c, minlength=n), out=cp[1:])
    return _base.spmatrix.from_ccs(off, n, cp, r[order], (np.concatenate(vals) if vals else np.zeros(0))[order])


_flat = _base.flat


def _nrows(B):
    return _base.ccs(B)[0]


def _common(sol, keys):
    out = {k: sol[k] for k in ("status", "x", "y", "gap", "relative gap", "primal objective", "dual objective",
                                "primal infeasibility", "dual infeasibility", "primal slack", "dual slack",
                                "residual as primal infeasibility certificate", "residual as dual infeasibility certificate",
                                "iterations")}
    out.update(keys)
    return out


def socp(c, Gl=None, hl=None, Gq=None, hq=None, A=None, b=None, kktsolver=None, solver=None, primalstart=None, dualstart=None, **kw):
    """solvers.socp (coneprog.py:3044-3596): minimize c'x s.t. Gl x <= hl, ||.||-cone constraints Gq[k] x + sq[k] = hq[k],
    A x = b; conelp with dims = {'l': rows of Gl, 'q': [rows of Gq[k]], 's': []}.  Returns x, y, sl, sq, zl, zq and the
    reference's status keys (numpy arrays)."""
    if solver is not None:
        raise NotImplementedError("kvxopt_amd.solvers runs misc.kkt_chol on the GPU; 'solver' is not selectable")
    n = _flat(c).size
    Gq, hq = list(Gq or []), list(hq or [])
    if len(Gq) != len(hq):
        raise TypeError("'Gq' and 'hq' must have the same length")
    ml = _nrows(Gl) if Gl is not None else 0
    qd = [_nrows(G) for G in Gq]
    G = _stack(([Gl] if Gl is not None else []) + Gq, n)
    h = np.concatenate([_flat(hl)] + [_flat(x) for x in hq]) if Gl is not None else \
        np.concatenate([_flat(x) for x in hq] or [np.zeros(0)])
    dims = {"l": ml, "q": qd, "s": []}
    ps = ds = None
    if primalstart is not None:
        ps = {"x": primalstart["x"], "s": np.concatenate([_flat(primalstart["sl"])] * (ml > 0) + [_flat(v) for v in primalstart["sq"]])}
    if dualstart is not None:
        ds = {"z": np.concatenate([_flat(dualstart["zl"])] * (ml > 0) + [_flat(v) for v in dualstart["zq"]])}
        if "y" in dualstart:
            ds["y"] = dualstart["y"]
    sol = conelp(c, G, h, dims, A=A, b=b, primalstart=ps, dualstart=ds, kktsolver=kktsolver, **kw)
    off = np.concatenate([[ml], ml + np.cumsum(qd)]).astype(int)

    def split(v):
        if v is None:
            return None, None
        return v[:ml].copy(), [v[off[k]:off[k + 1]].copy() for k in range(len(qd))]
    sl, sq = split(sol["s"])
    zl, zq = split(sol["z"])
    return _common(sol, {"sl": sl, "sq": sq, "zl": zl, "zq": zq})


def sdp(c, Gl=None, hl=None, Gs=None, hs=None, A=None, b=None, kktsolver=None, solver=None, primalstart=None, dualstart=None, **kw):
    """solvers.sdp (coneprog.py:3597-4186): minimize c'x s.t. Gl x <= hl, sum_j x_j mat(Gs[k][:, j]) <= hs[k] (semidefinite),
    A x = b; conelp with dims = {'l': rows of Gl, 'q': [], 's': [orders of hs[k]]}.  The 's' blocks of the result (ss, zs)
    are full symmetric m_k x m_k matrices, as the reference returns them."""
    if solver is not None:
        raise NotImplementedError("kvxopt_amd.solvers runs misc.kkt_chol on the GPU; 'solver' is not selectable")
    n = _flat(c).size
    Gs, hs = list(Gs or []), list(hs or [])
    if len(Gs) != len(hs):
        raise TypeError("'Gs' and 'hs' must have the same length")
    ml = _nrows(Gl) if Gl is not None else 0
    sd = []
    for k, H in enumerate(hs):
        m = int(round(np.sqrt(_flat(H).size)))
        if m * m != _flat(H).size or _nrows(Gs[k]) != m * m:
            raise TypeError("'Gs[%d]' must have %d rows and 'hs[%d]' must be square" % (k, m * m, k))
        sd.append(m)
    G = _stack(([Gl] if Gl is not None else []) + Gs, n)
    h = np.concatenate(([_flat(hl)] if Gl is not None else []) + [_flat(H) for H in hs] or [np.zeros(0)])
    dims = {"l": ml, "q": [], "s": sd}
    ps = ds = None
    if primalstart is not None:
        ps = {"x": primalstart["x"], "s": np.concatenate([_flat(primalstart["sl"])] * (ml > 0) + [_flat(v) for v in primalstart["ss"]])}
    if dualstart is not None:
        ds = {"z": np.concatenate([_flat(dualstart["zl"])] * (ml > 0) + [_flat(v) for v in dualstart["zs"]])}
        if "y" in dualstart:
            ds["y"] = dualstart["y"]
    sol = conelp(c, G, h, dims, A=A, b=b, primalstart=ps, dualstart=ds, kktsolver=kktsolver, **kw)
    off = np.concatenate([[ml], ml + np.cumsum([m * m for m in sd])]).astype(int)

    def split(v):
        if v is None:
            return None, None
        return v[:ml].copy(), [v[off[k]:off[k + 1]].reshape((m, m), order="F").copy() for k, m in enumerate(sd)]
    sl, ss = split(sol["s"])
    zl, zs = split(sol["z"])
    return _common(sol, {"sl": sl, "ss": ss, "zl": zl, "zs": zs})
