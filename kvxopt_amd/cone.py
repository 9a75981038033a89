"""Device-resident cone-LP and cone-QP interior-point drivers for general cones ('l' rows, 'q' second-order cones, 's'
semidefinite blocks):

    minimize c'x (conelp) or (1/2) x'Px + q'x (coneqp)  subject to  G x + s = h,  A x = b,  s in C = R^ml_+ x Q^q_1 x ... x S^m_1 x ...

A restatement of the reference's `coneprog.conelp` (src/python/coneprog.py:31-1436) with its KKT solver `misc.kkt_chol`
(misc.py:1213-1349): the reduced matrix S = Gs' Gs, Gs = pack2(W^-T G), assembled on a fixed sparsity pattern by
kvx_cone_assemble_dev (csrc/cone_api.cpp, csrc/kkt_cone.hip) and factored by the sparse supernodal Cholesky of this package on
one analysis.  Equality constraints are eliminated through K = A S^-1 A' (dense in HBM), as lp.KKTGenEqDev does; the reference
eliminates them by a QR factorisation of A' instead (same solution, different roundings).  Iterates, the scaling W (d, di, v,
beta, r, rti) and all work vectors stay in HBM; the host reads scalars only (inner products, step lengths).

`coneqp` restates the reference's `coneprog.coneqp` (coneprog.py:1440-2547) the same way, with the reduced matrix
S = P + Gs' Gs: the plan takes the lower pattern of P (kvx_cone_plan_h) and the gather of the assembly adds its values
(kvx_cone_assemble_h_dev).
"""
import ctypes
import math
import time

import numpy as np

from . import _ipm, _lib
from ._lib import lib, raise_for
from .base import ccs as _ccs, lower_ccs
from .chol import Factor
from .coneops import (Dims, WDev, compute_scaling as _compute_scaling, max_step, put_diag, scale, scale2, sdot, sinv, snrm2,
                      sprod, ssqr, step_and_update_scaling, tri)
from .devvec import DVec, SpMatDev, SymSpMatDev
from .lp import dense_schur



class ConePlan:
    """kvx_cone_plan / kvx_cone_plan_h: the pattern of S = Gs' Gs (+ H with a pattern Hp, Hi: the union with its lower triangle)
    and its assembly (host plan, device assembly)."""

    def __init__(self, D, n, Gp, Gi, Hp=None, Hi=None):
        h = ctypes.c_void_p()
        q = np.asarray(D.q, dtype=np.int64)
        s = np.asarray(D.s, dtype=np.int64)
        Gp = np.ascontiguousarray(Gp, dtype=np.int64)
        Gi = np.ascontiguousarray(Gi, dtype=np.int64)
        self.has_h = Hp is not None
        if self.has_h:
            Hp = np.ascontiguousarray(Hp, dtype=np.int64)
            Hi = np.ascontiguousarray(Hi, dtype=np.int64)
            if Hp.size != n + 1:
                raise TypeError("the pattern of H must have %d columns" % n)
            self.hnz = int(Hp[-1]) if n else 0
            raise_for(lib().kvx_cone_plan_h(D.ml, D.nq, _lib.pi(q) if q.size else None, D.ns, _lib.pi(s) if s.size else None, n,
                                            _lib.pi(Gp), _lib.pi(Gi) if Gi.size else None, _lib.pi(Hp), _lib.pi(Hi) if Hi.size else None,
                                            ctypes.byref(h)))
        else:
            raise_for(lib().kvx_cone_plan(D.ml, D.nq, _lib.pi(q) if q.size else None, D.ns, _lib.pi(s) if s.size else None, n,
                                          _lib.pi(Gp), _lib.pi(Gi) if Gi.size else None, ctypes.byref(h)))
        self._h = h
        snz = ctypes.c_int64()
        raise_for(lib().kvx_cone_pattern(h, ctypes.byref(snz), None, None))
        self.Sp = np.empty(n + 1, dtype=np.int64)
        Si = np.empty(max(snz.value, 1), dtype=np.int64)
        raise_for(lib().kvx_cone_pattern(h, ctypes.byref(snz), _lib.pi(self.Sp), _lib.pi(Si)))
        self.Si = Si[:snz.value].copy()

    def assemble(self, Gx_dev, W, Sx, Hx_dev=None):
        """Sx := Gs' Gs, or H + Gs' Gs with the values Hx_dev of a plan made with an H pattern."""
        if self.has_h:
            if Hx_dev is None:
                raise ValueError("the plan has an H pattern: its values are needed")
            raise_for(lib().kvx_cone_assemble_h_dev(self._h, Gx_dev.ptr, W.di.ptr, W.v.ptr, W.beta.ptr, W.rti.ptr,
                                                    Hx_dev.ptr if self.hnz else None, Sx.ptr))
        else:
            raise_for(lib().kvx_cone_assemble_dev(self._h, Gx_dev.ptr, W.di.ptr, W.v.ptr, W.beta.ptr, W.rti.ptr, Sx.ptr))

    def __del__(self):
        if getattr(self, "_h", None):
            lib().kvx_cone_free(self._h)
            self._h = None


class KKTConeDev:
    """misc.kkt_chol (misc.py:1213-1349) in HBM: factor(W) assembles S = Gs' Gs (kvx_cone_assemble_dev) and refactors it on the
    analysis made at construction; solve(x, y, z) overwrites (bx, by, bz) with (ux, uy, W uz):
        x := bx + G' W^-1 W^-T bz   ('s' part of G' in sgemv form: trisc),  ux = S^-1 x  (p = 0),
        uz := W^-T (G ux - bz).
    p > 0: u = S^-1 x, uy = K^-1 (A u - by) with K = A S^-1 A' dense, ux = S^-1 (x - A' uy)  (lp.KKTGenEqDev's elimination).

    With H = (Hp, Hi, Hx), a symmetric n x n matrix in CCS form whose lower triangle is used (coneqp: H = P; misc.py:1275-1277),
    the (1, 1) block of the KKT system is H and S = H + Gs' Gs on the union of the two patterns; the solve keeps its form.  S
    is then positive definite when Rank([H; G]) = n, which is weaker than the Rank(G) = n that the path without H needs."""

    BLOCK_BYTES = 1 << 30

    def __init__(self, D, n, Gp, Gi, Gx, p=0, Ap=None, Ai=None, Ax=None, chol_opts=None, Hp=None, Hi=None, Hx=None):
        self.D, self.n, self.p = D, n, p
        self.plan = ConePlan(D, n, Gp, Gi, Hp, Hi)
        self.Hx = None
        if Hp is not None:
            self.Hx = DVec(max(self.plan.hnz, 1))
            self.set_hessian(Hx)
        self.fac = Factor(n, self.plan.Sp, self.plan.Si, "L", None, chol_opts)
        self.G = SpMatDev(D.N, n, Gp, Gi, Gx)
        self.Sx = DVec(max(self.plan.Si.size, 1))
        self.t, self.u = DVec(D.N), DVec(D.N)
        self.W = None
        self.nfactor = 0
        if p:
            Ap = np.asarray(Ap, dtype=np.int64); Ai = np.asarray(Ai, dtype=np.int64); Ax = np.asarray(Ax, dtype=np.float64)
            self.A = SpMatDev(p, n, Ap, Ai, Ax)
            cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
            order = np.lexsort((cols, Ai))
            ATp = np.zeros(p + 1, dtype=np.int64)
            np.add.at(ATp, Ai + 1, 1)
            np.cumsum(ATp, out=ATp)
            self.AT = SpMatDev(n, p, ATp, cols[order], Ax[order])
            self.cols = max(1, min(p, self.BLOCK_BYTES // (8 * max(n, 1))))
            self.X = DVec(max(n * self.cols, 1))
            self.Kd = DVec(max(p * p, 1))
            self.Kx = DVec(max(p * (p + 1) // 2, 1))
            Kp = np.zeros(p + 1, dtype=np.int64)
            Kp[1:] = np.cumsum(np.arange(p, 0, -1))
            Ki = np.concatenate([np.arange(j, p, dtype=np.int64) for j in range(p)])
            self.kfac = Factor(p, Kp, Ki, "L", None, {"ordering": 1, "dbound": 1e-15, "dbound_drop": 1})
            self.kdiag = DVec(p)
            self.xs = DVec(n)
            self.kscale = 1.0

    def set_hessian(self, Hx):
        """New values of H on the pattern given at construction."""
        if self.Hx is None:
            raise ValueError("the KKT system was built without an H pattern")
        Hx = np.ascontiguousarray(Hx, dtype=np.float64).reshape(-1)
        if Hx.size != self.plan.hnz:
            raise TypeError("H has %d values, its pattern %d" % (Hx.size, self.plan.hnz))
        if Hx.size:
            self.Hx.set(Hx)

    def set_hessian_dev(self, src_ptr, map_dev, count):
        """New values of H from HBM: Hx[map[i]] := src[i] for the count entries of a device index map (kvx_vec_scatter_dev)."""
        if self.Hx is None:
            raise ValueError("the KKT system was built without an H pattern")
        if count:
            raise_for(lib().kvx_vec_scatter_dev(count, src_ptr, map_dev.ptr, self.Hx.ptr))

    def assemble(self, W):
        self.plan.assemble(self.G.vx, W, self.Sx, self.Hx)

    def factor(self, W):
        """ArithmeticError if S (or K) is not positive definite."""
        n, p = self.n, self.p
        self.assemble(W)
        self.fac.factorize_dev(self.Sx.ptr, sync=True)
        if p:
            kmax = dense_schur(self.fac, self.AT, self.X, self.Kd, self.Kx, self.kdiag, n, p, self.cols)
            self.fac.status()
            if not (kmax > 0.0) or not np.isfinite(kmax):
                raise ArithmeticError(0)
            self.kscale = 1.0 / kmax
            self.Kx.scal(self.kscale)
            self.kfac.factorize_dev(self.Kx.ptr, sync=True)
        self.W = W
        self.nfactor += 1

    def solve(self, x, y, z):
        D, W, n = self.D, self.W, self.n
        t = self.t
        t.copy_from(z)
        scale(D, W, t.ptr, trans="T", inverse="I")
        scale(D, W, t.ptr, trans="N", inverse="I")
        tri(D, t.ptr, 1)                                               # trisc: the 's' part of G' (misc.py:829)
        self.G.gemv(t, x, trans="T", alpha=1.0, beta=1.0)              # x := bx + G' W^-1 W^-T bz
        if self.p:
            self.xs.copy_from(x)
            self.fac.solve_dev(x.ptr, 0, 1, max(1, n))                 # u = S^-1 x
            self.A.gemv(x, y, trans="N", alpha=1.0, beta=-1.0)          # y := A u - by
            self.kfac.solve_dev(y.ptr, 0, 1, max(1, self.p))
            y.scal(self.kscale)                                        # uy = K^-1 (A u - by)
            x.copy_from(self.xs)
            self.A.gemv(y, x, trans="T", alpha=-1.0, beta=1.0)          # x - A' uy
        self.fac.solve_dev(x.ptr, 0, 1, max(1, n))
        self.G.gemv(x, self.u, trans="N")                              # u := G ux - bz
        self.u.axpy(z, -1.0)
        scale(D, W, self.u.ptr, trans="T", inverse="I")                # W^-T (G ux - bz) ('s': lower triangles)
        z.copy_from(self.u)


_vec = _ipm.vector


def compute_scaling(D, s, z, W, lmbda):
    if _compute_scaling(D, s, z, W, lmbda) is not None:
        raise ArithmeticError("compute_scaling: an 's' block of s or z is not positive definite")


def check_dims(dims, h_size=None):
    """coneprog.py:499-521: the dims checks and their TypeErrors."""
    _ipm.check_dims(dims)


def conelp(c, G, h, dims, A=None, b=None, options=None, primalstart=None, dualstart=None, kktsolver=None, chol_opts=None):
    """coneprog.conelp (coneprog.py:31-1436) for dims with 'q' / 's' cones, on the GPU.  Returns the reference's result dictionary
    with numpy arrays ('s' blocks of s and z as full symmetric matrices)."""
    if kktsolver is not None:
        raise NotImplementedError("conelp with 'q' / 's' cones runs misc.kkt_chol on the GPU; kktsolver is not selectable")
    opt = _ipm.options(options, dims)
    MAXITERS, ABSTOL, RELTOL, FEASTOL, REFINEMENT, show = opt.maxiters, opt.abstol, opt.reltol, opt.feastol, opt.refinement, opt.show
    pb = _ipm.problem(c, G, h, dims, A, b)
    n, p, cdim, c_h, h_h, b_h = pb.n, pb.p, pb.cdim, pb.c, pb.h, pb.b
    _lib.require_device()
    D = Dims(pb.dims)
    kkt = KKTConeDev(D, n, *pb.G, p, *pb.A, chol_opts)
    vec = DVec
    Gf, Af = _ipm.operators(kkt.G, kkt.A if p else None, (lambda t: tri(D, t.ptr, 1)) if D.tot2 else None, vec(cdim))
    cv, hv, bv = vec(n, c_h), vec(cdim, h_h), vec(p, b_h if p else None)
    ws3, wz3 = vec(cdim), vec(cdim)
    W = WDev(D)

    def res(ux, uy, uz, utau, us, ukappa, vx, vy, vz, vtau, vs, vkappa, dg, lmbda_g):   # coneprog.py:578-631
        Af(uy, vx, alpha=-1.0, beta=1.0, trans="T")
        wz3.copy_from(uz)
        scale(D, W, wz3.ptr, inverse="I")
        Gf(wz3, vx, alpha=-1.0, beta=1.0, trans="T")
        vx.axpy(cv, -utau[0] / dg)
        Af(ux, vy, alpha=1.0, beta=1.0)
        vy.axpy(bv, -utau[0] / dg)
        Gf(ux, vz, alpha=1.0, beta=1.0)
        vz.axpy(hv, -utau[0] / dg)
        ws3.copy_from(us)
        scale(D, W, ws3.ptr, trans="T")
        vz.axpy(ws3)
        vtau[0] += dg * ukappa[0] + cv.dot(ux) + bv.dot(uy) + sdot(D, hv.ptr, wz3.ptr)
        ws3.copy_from(us)
        ws3.axpy(uz)
        sprod(D, ws3.ptr, lmbda.ptr, diag="D")
        vs.axpy(ws3)
        vkappa[0] += lmbda_g * (utau[0] + ukappa[0])

    resx0 = max(1.0, math.sqrt(cv.dot(cv)))
    resy0 = max(1.0, math.sqrt(bv.dot(bv)))
    resz0 = max(1.0, snrm2(D, hv.ptr))
    x, y = vec(n).fill(0.0), vec(p).fill(0.0)                       # coneprog.py:655-656
    s, z = vec(cdim), vec(cdim)
    dx, dy = vec(n), vec(p)
    ds, dz = vec(cdim), vec(cdim)
    t_start = time.perf_counter()

    def finish(status, iters, gap, relgap, pcost, dcost, pres, dres, pinfres, dinfres, xs=True, zs=True, ts=None, tz=None, msg=None):
        return _ipm.conelp_result(show, status, x.get() if xs else None, y.get() if zs else None, s.get() if xs else None,
                                  z.get() if zs else None, (gap, relgap, pcost, dcost, pres, dres, pinfres, dinfres), ts, tz, iters,
                                  kkt.nfactor, msg, **{"loop seconds": time.perf_counter() - t_start})

    rank_msg = "Rank(A) < p or Rank([G; A]) < n"
    if p:
        # the elimination through S^-1 needs S = G' W^-1 W^-T G itself positive definite, i.e. Rank(G) = n; the reference's QR
        # elimination (misc.py:1244-1282) needs it on the null space of A only
        rank_msg += (", or Rank(G) < n: with equality constraints this path eliminates A through S^-1, S = G' W^-1 W^-T G, "
                     "which needs G to have full column rank")
    if primalstart is None or dualstart is None:
        W.identity()
        try:
            kkt.factor(W)
        except ArithmeticError:
            raise ValueError(rank_msg)
    if primalstart is None:
        x.fill(0.0)
        dy.copy_from(bv)
        s.copy_from(hv)
        try:
            kkt.solve(x, dy, s)
        except ArithmeticError:
            raise ValueError(rank_msg)
        s.scal(-1.0)
    else:
        x.set(_vec(primalstart["x"], "primalstart['x']", n))
        s.set(_vec(primalstart["s"], "primalstart['s']", cdim))
    ts = max_step(D, s.ptr)
    if ts >= 0 and primalstart:
        raise ValueError("initial s is not positive")
    if dualstart is None:
        dx.copy_from(cv).scal(-1.0)
        y.fill(0.0)
        z.fill(0.0)
        try:
            kkt.solve(dx, y, z)
        except ArithmeticError:
            raise ValueError(rank_msg)
    else:
        if "y" in dualstart and p:
            y.set(_vec(dualstart["y"], "dualstart['y']", p))
        z.set(_vec(dualstart["z"], "dualstart['z']", cdim))
    tz = max_step(D, z.ptr)
    if tz >= 0 and dualstart:
        raise ValueError("initial z is not positive")
    nrms, nrmz = snrm2(D, s.ptr), snrm2(D, z.ptr)

    if primalstart is None and dualstart is None:
        gap = sdot(D, s.ptr, z.ptr)
        pcost = cv.dot(x)
        dcost = -bv.dot(y) - sdot(D, hv.ptr, z.ptr)
        relgap = _ipm.relgap(gap, pcost, dcost)
        if ts <= 0 and tz <= 0 and (gap <= ABSTOL or (relgap is not None and relgap <= RELTOL)):
            tri(D, s.ptr, 0); tri(D, z.ptr, 0)
            rx = vec(n, c_h)
            Af(y, rx, beta=1.0, trans="T")
            Gf(z, rx, beta=1.0, trans="T")
            resx = math.sqrt(rx.dot(rx))
            ry = vec(p, b_h if p else None)
            Af(x, ry, alpha=-1.0, beta=1.0)
            resy = math.sqrt(ry.dot(ry))
            rz = vec(cdim)
            Gf(x, rz)
            rz.axpy(s)
            rz.axpy(hv, -1.0)
            resz = snrm2(D, rz.ptr)
            pres, dres = max(resy / resy0, resz / resz0), resx / resx0
            cx, by, hz = cv.dot(x), bv.dot(y), sdot(D, hv.ptr, z.ptr)
            return finish("optimal", 0, gap, relgap, cx, -(by + hz), pres, dres, None, None, ts=ts, tz=tz)
        if ts >= -1e-8 * max(nrms, 1.0):
            s.axpy(D.e, 1.0 + ts)
        if tz >= -1e-8 * max(nrmz, 1.0):
            z.axpy(D.e, 1.0 + tz)
    elif primalstart is None and dualstart is not None:
        if ts >= -1e-8 * max(nrms, 1.0):
            s.axpy(D.e, 1.0 + ts)
    elif primalstart is not None and dualstart is None:
        if tz >= -1e-8 * max(nrmz, 1.0):
            z.axpy(D.e, 1.0 + tz)

    tau, kappa = 1.0, 1.0
    rx, hrx = vec(n), vec(n)
    ry, hry = vec(p), vec(p)
    rz, hrz = vec(cdim), vec(cdim)
    sigs, sigz = vec(D.tot1), vec(D.tot1)
    lmbda, lmbdasq = vec(D.Nd), vec(D.Nd)
    lmbda_g = 0.0
    x1, y1, z1 = vec(n), vec(p), vec(cdim)
    th = vec(cdim)
    wx, wy, wz, ws = vec(n), vec(p), vec(cdim), vec(cdim)
    wx2, wy2, wz2, ws2 = vec(n), vec(p), vec(cdim), vec(cdim)
    gap = sdot(D, s.ptr, z.ptr)
    dg = dgi = 1.0
    ind = D.ind
    st = np.zeros(1, dtype=np.int32)

    for iters in range(MAXITERS + 1):
        # residuals (coneprog.py:861-896)
        Af(y, hrx, alpha=-1.0, trans="T")
        Gf(z, hrx, alpha=-1.0, beta=1.0, trans="T")
        hresx = math.sqrt(hrx.dot(hrx))
        rx.copy_from(hrx)
        rx.axpy(cv, -tau)
        resx = math.sqrt(rx.dot(rx)) / tau
        Af(x, hry)
        hresy = math.sqrt(hry.dot(hry))
        ry.copy_from(hry)
        ry.axpy(bv, -tau)
        resy = math.sqrt(ry.dot(ry)) / tau
        Gf(x, hrz)
        hrz.axpy(s)
        hresz = snrm2(D, hrz.ptr)
        rz.fill(0.0)
        rz.axpy(hrz)
        rz.axpy(hv, -tau)
        resz = snrm2(D, rz.ptr) / tau
        cx, by, hz = cv.dot(x), bv.dot(y), sdot(D, hv.ptr, z.ptr)
        rt = kappa + cx + by + hz
        pcost, dcost = cx / tau, -(by + hz) / tau
        relgap = _ipm.relgap(gap, pcost, dcost)
        pres = max(resy / resy0, resz / resz0)
        dres = resx / resx0
        pinfres = hresx / resx0 / (-hz - by) if hz + by < 0.0 else None
        dinfres = max(hresy / resy0, hresz / resz0) / (-cx) if cx < 0.0 else None
        if show:
            _ipm.progress(iters, pcost, dcost, gap, pres, dres, kappa / tau)

        if (pres <= FEASTOL and dres <= FEASTOL and (gap <= ABSTOL or (relgap is not None and relgap <= RELTOL))) or iters == MAXITERS:
            x.scal(1.0 / tau); y.scal(1.0 / tau); s.scal(1.0 / tau); z.scal(1.0 / tau)
            tri(D, s.ptr, 0); tri(D, z.ptr, 0)
            ts, tz = max_step(D, s.ptr), max_step(D, z.ptr)
            if iters == MAXITERS:
                return finish("unknown", iters, gap, relgap, pcost, dcost, pres, dres, pinfres, dinfres, ts=ts, tz=tz,
                              msg=_ipm.MAXITERS_MSG)
            return finish("optimal", iters, gap, relgap, pcost, dcost, pres, dres, None, None, ts=ts, tz=tz)
        elif pinfres is not None and pinfres <= FEASTOL:
            y.scal(1.0 / (-hz - by)); z.scal(1.0 / (-hz - by))
            tri(D, z.ptr, 0)
            tz = max_step(D, z.ptr)
            return finish("primal infeasible", iters, None, None, None, 1.0, None, None, pinfres, None, xs=False, tz=tz)
        elif dinfres is not None and dinfres <= FEASTOL:
            x.scal(1.0 / (-cx)); s.scal(1.0 / (-cx))
            tri(D, s.ptr, 0)
            ts = max_step(D, s.ptr)
            return finish("dual infeasible", iters, None, None, -1.0, None, None, None, None, dinfres, zs=False, ts=ts)

        if iters == 0:
            compute_scaling(D, s, z, W, lmbda)
            dg = math.sqrt(kappa / tau)
            dgi = math.sqrt(tau / kappa)
            lmbda_g = math.sqrt(tau * kappa)

        ssqr(D, lmbdasq.ptr, lmbda.ptr)
        lmbdasq_g = lmbda_g ** 2

        try:
            kkt.factor(W)
            x1.copy_from(cv).scal(-1.0)
            y1.copy_from(bv)
            z1.copy_from(hv)
            kkt.solve(x1, y1, z1)
            x1.scal(dgi); y1.scal(dgi); z1.scal(dgi)
        except ArithmeticError:
            if iters == 0 and primalstart and dualstart:
                raise ValueError(rank_msg)
            x.scal(1.0 / tau); y.scal(1.0 / tau); s.scal(1.0 / tau); z.scal(1.0 / tau)
            tri(D, s.ptr, 0); tri(D, z.ptr, 0)
            ts, tz = max_step(D, s.ptr), max_step(D, z.ptr)
            return finish("unknown", iters, gap, relgap, pcost, dcost, pres, dres, pinfres, dinfres, ts=ts, tz=tz,
                          msg=_ipm.SINGULAR_MSG)

        th.copy_from(hv)
        scale(D, W, th.ptr, trans="T", inverse="I")
        z1z1 = sdot(D, z1.ptr, z1.ptr)

        def f6_no_ir(bx, by_, bz, btau, bs, bkappa):                  # coneprog.py:1130-1195
            by_.scal(-1.0)
            sinv(D, bs.ptr, lmbda.ptr)
            bs.scal(-1.0)
            ws3.copy_from(bs)
            scale(D, W, ws3.ptr, trans="T")
            bz.axpy(ws3)
            bz.scal(-1.0)
            kkt.solve(bx, by_, bz)
            bkappa[0] = -bkappa[0] / lmbda_g
            btau[0] += bkappa[0] / dgi
            btau[0] = dgi * (btau[0] + cv.dot(bx) + bv.dot(by_) + sdot(D, th.ptr, bz.ptr)) / (1.0 + z1z1)
            bx.axpy(x1, btau[0]); by_.axpy(y1, btau[0]); bz.axpy(z1, btau[0])
            bs.axpy(bz, -1.0)
            bkappa[0] -= btau[0]

        f6 = _ipm.f6(f6_no_ir, lambda *a: res(*a, dg, lmbda_g), REFINEMENT, (wx, wy, wz, ws), (wx2, wy2, wz2, ws2))

        mu = lmbda.dot(lmbda) + 0.0
        mu = (mu + lmbda_g ** 2) / (1 + D.Nd)                          # blas.nrm2(lmbda)**2 / (1 + cdim_diag)
        sigma = 0.0
        wkappa3 = 0.0
        for i in (0, 1):
            put_diag(D, ds, lmbdasq.ptr)                              # coneprog.py:1273-1280
            dkappa = [lmbdasq_g]
            if i == 1:
                ds.axpy(ws3)
                ds.axpy(D.e, -sigma * mu)
                dkappa[0] += wkappa3 - sigma * mu
            dx.copy_from(rx).scal(1.0 - sigma)
            dy.copy_from(ry).scal(1.0 - sigma)
            dz.copy_from(rz).scal(1.0 - sigma)
            dtau = [(1.0 - sigma) * rt]
            f6(dx, dy, dz, dtau, ds, dkappa)
            if i == 0:
                ws3.copy_from(ds)
                sprod(D, ws3.ptr, dz.ptr)
                wkappa3 = dtau[0] * dkappa[0]
            scale2(D, lmbda.ptr, ds.ptr)
            scale2(D, lmbda.ptr, dz.ptr)
            if i == 0:
                ts, tz = max_step(D, ds.ptr), max_step(D, dz.ptr)
            else:
                ts, tz = max_step(D, ds.ptr, sigma=sigs), max_step(D, dz.ptr, sigma=sigz)
            tt = -dtau[0] / lmbda_g
            tk = -dkappa[0] / lmbda_g
            t = max([0.0, ts, tz, tt, tk])
            step = _ipm.step_length(t, i)
            if i == 0:
                sigma = (1.0 - step) ** _ipm.EXPON

        # update (coneprog.py:1336-1436)
        x.axpy(dx, step)
        y.axpy(dy, step)
        step_and_update_scaling(D, W, lmbda, ds, dz, sigs, sigz, step)
        dg *= math.sqrt(1.0 - step * tk) / math.sqrt(1.0 - step * tt)
        dgi = 1.0 / dg
        lmbda_g *= math.sqrt(1.0 - step * tt) * math.sqrt(1.0 - step * tk)
        put_diag(D, s, lmbda.ptr)
        scale(D, W, s.ptr, trans="T")
        put_diag(D, z, lmbda.ptr)
        scale(D, W, z.ptr, inverse="I")
        kappa, tau = lmbda_g / dgi, lmbda_g * dgi
        gap = (math.sqrt(lmbda.dot(lmbda)) / tau) ** 2
    raise AssertionError("unreachable")


def coneqp(P, q, G, h, dims, A=None, b=None, initvals=None, options=None, chol_opts=None):
    """coneprog.coneqp (coneprog.py:1440-2547) for dims with 'q' / 's' cones, on the GPU:

        minimize (1/2) x'Px + q'x  subject to  G x + s = h,  A x = b,  s in C,

    with the reference's kktsolver='chol' system (coneprog.py:1806-1809, 1969-1981): KKTConeDev with H = P, S = P + Gs' Gs.
    P: dense or sparse, its lower triangle is used (a dense P with its full lower pattern).  S must be positive definite, i.e.
    Rank([P; G]) = n (with equality constraints the reference needs that on the null space of A only).  Returns the reference's
    result dictionary (coneprog.py:2216-2221) with numpy arrays, the 's' blocks of s and z as full symmetric matrices, plus
    "factorizations"."""
    if G is None or dims is None:
        raise NotImplementedError("coneqp without G is not part of the general-cone path")
    for M in (P, G, A):
        if callable(M):
            raise ValueError("use of function valued P, G, A requires a user-provided kktsolver")
    opt = _ipm.options(options, dims, qp=True)
    MAXITERS, ABSTOL, RELTOL, FEASTOL, REFINEMENT, show = opt.maxiters, opt.abstol, opt.reltol, opt.feastol, opt.refinement, opt.show
    correction = opt.correction
    pb = _ipm.problem(q, G, h, dims, A, b, P, qp=True)
    n, p, cdim, q_h, h_h, b_h = pb.n, pb.p, pb.cdim, pb.c, pb.h, pb.b
    if cdim == 0:
        raise NotImplementedError("coneqp without cone constraints is not part of the general-cone path")
    _lib.require_device()
    D = Dims(pb.dims)
    kkt = KKTConeDev(D, n, *pb.G, p, *pb.A, chol_opts, *pb.P)
    Pd = SymSpMatDev(n, *pb.P)
    vec = DVec
    Gf, Af = _ipm.operators(kkt.G, kkt.A if p else None, (lambda t: tri(D, t.ptr, 1)) if D.tot2 else None, vec(cdim))

    qv, hv, bv = vec(n, q_h), vec(cdim, h_h), vec(p, b_h if p else None)
    ws3, wz3, dtmp = vec(cdim), vec(cdim), vec(cdim)
    W = WDev(D)
    lmbda, lmbdasq = vec(D.Nd), vec(D.Nd)

    def res(ux, uy, uz, us, vx, vy, vz, vs):                          # coneprog.py:1930-1960
        Pd.symv(ux, vx, alpha=-1.0, beta=1.0)
        Af(uy, vx, alpha=-1.0, beta=1.0, trans="T")
        wz3.copy_from(uz)
        scale(D, W, wz3.ptr, inverse="I")
        Gf(wz3, vx, alpha=-1.0, beta=1.0, trans="T")
        Af(ux, vy, alpha=-1.0, beta=1.0)
        Gf(ux, vz, alpha=-1.0, beta=1.0)
        ws3.copy_from(us)
        scale(D, W, ws3.ptr, trans="T")
        vz.axpy(ws3, -1.0)
        ws3.copy_from(us)
        ws3.axpy(uz)
        sprod(D, ws3.ptr, lmbda.ptr, diag="D")
        vs.axpy(ws3, -1.0)

    resx0 = max(1.0, math.sqrt(qv.dot(qv)))
    resy0 = max(1.0, math.sqrt(bv.dot(bv))) if p else 1.0
    resz0 = max(1.0, snrm2(D, hv.ptr))
    x, y = vec(n), vec(p)
    s, z = vec(cdim), vec(cdim)
    y.fill(0.0)

    def finish(status, iters, gap, relgap, pcost, dcost, pres, dres, msg):
        tri(D, s.ptr, 0); tri(D, z.ptr, 0)                            # misc.symm of the 's' blocks
        ts, tz = max_step(D, s.ptr), max_step(D, z.ptr)
        return _ipm.coneqp_result(show, status, x.get(), y.get() if p else np.zeros(0), s.get(), z.get(),
                                  (gap, relgap, pcost, dcost, pres, dres), ts, tz, iters, kkt.nfactor, msg)

    # ---- starting point (coneprog.py:2044-2150)
    if initvals is None:
        W.identity()
        try:
            kkt.factor(W)
        except ArithmeticError:
            raise ValueError("Rank(A) < p or Rank([P; A; G]) < n")
        x.copy_from(qv).scal(-1.0)
        y.copy_from(bv)
        z.copy_from(hv)
        try:
            kkt.solve(x, y, z)
        except ArithmeticError:
            raise ValueError("Rank(A) < p or Rank([P; G; A]) < n")
        s.copy_from(z).scal(-1.0)
        nrms = snrm2(D, s.ptr)
        ts = max_step(D, s.ptr)
        if ts >= -1e-8 * max(nrms, 1.0):
            s.axpy(D.e, 1.0 + ts)
        nrmz = snrm2(D, z.ptr)
        tz = max_step(D, z.ptr)
        if tz >= -1e-8 * max(nrmz, 1.0):
            z.axpy(D.e, 1.0 + tz)
    else:
        x.set(_vec(initvals["x"], "initvals['x']", n)) if "x" in initvals else x.fill(0.0)
        if "s" in initvals:
            s.set(_vec(initvals["s"], "initvals['s']", cdim))
            if max_step(D, s.ptr) >= 0:
                raise ValueError("initial s is not positive")
        else:
            s.copy_from(D.e)
        if "y" in initvals and p:
            y.set(_vec(initvals["y"], "initvals['y']", p))
        if "z" in initvals:
            z.set(_vec(initvals["z"], "initvals['z']", cdim))
            if max_step(D, z.ptr) >= 0:
                raise ValueError("initial z is not positive")
        else:
            z.copy_from(D.e)

    rx, ry, rz = vec(n), vec(p), vec(cdim)
    dx, dy = vec(n), vec(p)
    dz, ds = vec(cdim), vec(cdim)
    sigs, sigz = vec(D.tot1), vec(D.tot1)
    if REFINEMENT:
        wx, wy, wz, ws = vec(n), vec(p), vec(cdim), vec(cdim)
        wx2, wy2, wz2, ws2 = vec(n), vec(p), vec(cdim), vec(cdim)
    tmpx = vec(n)
    gap = sdot(D, s.ptr, z.ptr)

    def f4_no_ir(bx, by_, bz, bs):                                    # coneprog.py:2288-2316
        sinv(D, bs.ptr, lmbda.ptr)
        ws3.copy_from(bs)
        scale(D, W, ws3.ptr, trans="T")
        bz.axpy(ws3, -1.0)
        kkt.solve(bx, by_, bz)
        bs.axpy(bz, -1.0)

    f4 = _ipm.f4(f4_no_ir, res, REFINEMENT, (wx, wy, wz, ws) if REFINEMENT else (), (wx2, wy2, wz2, ws2) if REFINEMENT else ())

    for iters in range(MAXITERS + 1):
        # f0 = (1/2) x'Px + q'x, rx = Px + q + A'y + G'z, ry = Ax - b, rz = s + Gx - h  (coneprog.py:2169-2186)
        rx.copy_from(qv)
        Pd.symv(x, rx, alpha=1.0, beta=1.0)
        tmpx.copy_from(rx)
        f0 = 0.5 * (x.dot(tmpx) + x.dot(qv))
        Af(y, rx, beta=1.0, trans="T")
        Gf(z, rx, beta=1.0, trans="T")
        resx = math.sqrt(rx.dot(rx))
        ry.copy_from(bv)
        Af(x, ry, alpha=1.0, beta=-1.0)
        resy = math.sqrt(ry.dot(ry)) if p else 0.0
        rz.copy_from(s)
        rz.axpy(hv, -1.0)
        Gf(x, rz, beta=1.0)
        resz = snrm2(D, rz.ptr)
        pcost = f0
        dcost = f0 + (y.dot(ry) if p else 0.0) + sdot(D, z.ptr, rz.ptr) - gap
        relgap = _ipm.relgap(gap, pcost, dcost)
        pres = max(resy / resy0, resz / resz0)
        dres = resx / resx0
        if show:
            _ipm.progress(iters, pcost, dcost, gap, pres, dres)
        if (pres <= FEASTOL and dres <= FEASTOL and (gap <= ABSTOL or (relgap is not None and relgap <= RELTOL))) or iters == MAXITERS:
            if iters == MAXITERS:
                return finish("unknown", iters, gap, relgap, pcost, dcost, pres, dres, _ipm.MAXITERS_MSG)
            return finish("optimal", iters, gap, relgap, pcost, dcost, pres, dres, "Optimal solution found.")

        if iters == 0:
            compute_scaling(D, s, z, W, lmbda)
        ssqr(D, lmbdasq.ptr, lmbda.ptr)
        try:
            kkt.factor(W)
        except ArithmeticError:
            if iters == 0:
                raise ValueError("Rank(A) < p or Rank([P; A; G]) < n")
            return finish("unknown", iters, gap, relgap, pcost, dcost, pres, dres, _ipm.SINGULAR_MSG)

        mu = gap / (D.ml + D.nq + D.tot1)
        sigma, eta = 0.0, 0.0
        for i in (0, 1):
            # ds = -lmbdasq + sigma mu e (i = 0), -lmbdasq - dsa o dza + sigma mu e (i = 1)  (coneprog.py:2376-2392)
            ds.fill(0.0)
            if correction and i == 1:
                ds.axpy(ws3, -1.0)
            put_diag(D, dtmp, lmbdasq.ptr)
            ds.axpy(dtmp, -1.0)
            ds.axpy(D.e, sigma * mu)
            dx.fill(0.0).axpy(rx, -1.0 + eta)
            dy.fill(0.0).axpy(ry, -1.0 + eta)
            dz.fill(0.0).axpy(rz, -1.0 + eta)
            try:
                f4(dx, dy, dz, ds)
            except ArithmeticError:
                if iters == 0:
                    raise ValueError("Rank(A) < p or Rank([P; A; G]) < n")
                return finish("unknown", iters, gap, relgap, pcost, dcost, pres, dres, _ipm.SINGULAR_MSG)
            dsdz = sdot(D, ds.ptr, dz.ptr)
            if correction and i == 0:                                 # ds o dz for the Mehrotra correction
                ws3.copy_from(ds)
                sprod(D, ws3.ptr, dz.ptr)
            # step to the boundary; i = 1: also the eigen-decompositions of the 's' blocks of ds, dz (coneprog.py:2431-2456)
            scale2(D, lmbda.ptr, ds.ptr)
            scale2(D, lmbda.ptr, dz.ptr)
            if i == 0:
                ts, tz = max_step(D, ds.ptr), max_step(D, dz.ptr)
            else:
                ts, tz = max_step(D, ds.ptr, sigma=sigs), max_step(D, dz.ptr, sigma=sigz)
            t = max([0.0, ts, tz])
            step = _ipm.step_length(t, i)
            if i == 0:
                sigma = min(1.0, max(0.0, 1.0 - step + dsdz / gap * step ** 2)) ** _ipm.EXPON
                eta = 0.0

        # update (coneprog.py:2459-2547)
        x.axpy(dx, step)
        y.axpy(dy, step)
        step_and_update_scaling(D, W, lmbda, ds, dz, sigs, sigz, step)
        put_diag(D, s, lmbda.ptr)
        scale(D, W, s.ptr, trans="T")
        put_diag(D, z, lmbda.ptr)
        scale(D, W, z.ptr, inverse="I")
        gap = lmbda.dot(lmbda)
    raise AssertionError("unreachable")
