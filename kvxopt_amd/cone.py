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

Both loops and both starting points are those of _ipm.py (`conelp_loop`, `coneqp_loop`), written once for every cone; this module
holds the engines that own the vectors and the launches on general cones, `_ConeEngine` and `_ConeQpEngine`.  They stay apart from
the orthant engines of lp.py: those scale with the `mul(d)` / `div(lmbda)` kernels, these with `scale` / `sinv`, and the two have not
been shown to round alike.
"""
import ctypes
import time

import numpy as np

from . import _ipm, _lib
from ._lib import lib, raise_for
from .base import ccs as _ccs, lower_ccs                        # noqa: F401  (cone._ccs, cone.lower_ccs: tools and tests)
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


def compute_scaling(D, s, z, W, lmbda):
    if _compute_scaling(D, s, z, W, lmbda) is not None:
        raise ArithmeticError("compute_scaling: an 's' block of s or z is not positive definite")


class _ConeOps:
    """What the starting points of _ipm ask an engine for, on a product of 'l', 'q' and 's' cones, and what the two engines below
    have in common: the scaling W, the operators with G and A, and the end of an iteration."""

    def __init__(self, kkt, pb, D):
        self.kkt, self.D, self.W, self.n, self.p = kkt, D, WDev(D), pb.n, pb.p
        self.Gf, self.Af = _ipm.operators(kkt.G, kkt.A if pb.p else None, (lambda t: tri(D, t.ptr, 1)) if D.tot2 else None, DVec(D.N))
        self.hv, self.bv = DVec(D.N, pb.h), DVec(pb.p, pb.b if pb.p else None)
        self.x, self.dx, self.rx = (DVec(pb.n) for _ in range(3))
        self.y, self.dy, self.ry = (DVec(pb.p) for _ in range(3))
        self.s, self.z, self.ds, self.dz, self.rz, self.ws3, self.wz3 = (DVec(D.N) for _ in range(7))
        self.sigs, self.sigz = DVec(D.tot1), DVec(D.tot1)
        self.lmbda, self.lmbdasq = DVec(D.Nd), DVec(D.Nd)
        self.y.fill(0.0)

    def factor_identity(self, needed):
        if needed:
            self.W.identity()
            self.kkt.factor(self.W)

    def start_solve(self, x, y, z):
        self.kkt.solve(x, y, z)

    def max_step(self, v):
        return max_step(self.D, v.ptr)

    def nrm2(self, v):
        return snrm2(self.D, v.ptr)

    def dot(self, u, v):
        return sdot(self.D, u.ptr, v.ptr)

    def add_e(self, v, a):
        v.axpy(self.D.e, a)

    def symm(self, v):
        tri(self.D, v.ptr, 0)

    def scaled_bounds(self, i):
        """ds, dz scaled by lmbda (misc.scale2) and their largest steps; at the second direction also the eigenvalues and
        eigenvectors of their 's' blocks, which step() consumes (coneprog.py:1308-1321, 2431-2456)."""
        D, ds, dz = self.D, self.ds, self.dz
        scale2(D, self.lmbda.ptr, ds.ptr)
        scale2(D, self.lmbda.ptr, dz.ptr)
        if i == 0:
            return max_step(D, ds.ptr), max_step(D, dz.ptr)
        return max_step(D, ds.ptr, sigma=self.sigs), max_step(D, dz.ptr, sigma=self.sigz)

    def step(self, step):
        """x, y, the scaling and lmbda after the step, s = W' lmbda and z = W^-1 lmbda (coneprog.py:1336-1431, 2459-2545);
        returns lmbda'lmbda."""
        D, W, s, z, lmbda = self.D, self.W, self.s, self.z, self.lmbda
        self.x.axpy(self.dx, step)
        self.y.axpy(self.dy, step)
        step_and_update_scaling(D, W, lmbda, self.ds, self.dz, self.sigs, self.sigz, step)
        put_diag(D, s, lmbda.ptr)
        scale(D, W, s.ptr, trans="T")
        put_diag(D, z, lmbda.ptr)
        scale(D, W, z.ptr, inverse="I")
        return lmbda.dot(lmbda)


class _ConeEngine(_ConeOps):
    """The device vectors and launches of one conelp run (the protocol of _ipm.conelp_loop), to be read top to bottom as the launch
    order of an iteration.  The Newton systems are solved as the reference solves them (coneprog.py:578-631 res, :1130-1195 f6_no_ir,
    :1211-1235 f6), operation by operation; the scalars (tau, kappa blocks) travel in one-element lists."""

    def __init__(self, kkt, pb, D, nref, starts_given):
        super().__init__(kkt, pb, D)
        n, p, N = pb.n, pb.p, D.N
        self.cv = DVec(n, pb.c)
        self.x.fill(0.0)                                                 # coneprog.py:655-656
        self.x1, self.hrx = DVec(n), DVec(n)
        self.y1, self.hry = DVec(p), DVec(p)
        self.z1, self.hrz, self.th = DVec(N), DVec(N), DVec(N)
        w, w2 = ((DVec(n), DVec(p), DVec(N), DVec(N)) for _ in range(2))
        self.f6 = _ipm.f6(self.f6_no_ir, self.res, nref, w, w2)
        self.lam2 = 0.0
        self.unfactored = starts_given                                   # no factorisation has succeeded yet (coneprog.py:1078)
        self.rank_msg = "Rank(A) < p or Rank([G; A]) < n"
        if p:
            # the elimination through S^-1 needs S = G' W^-1 W^-T G itself positive definite, i.e. Rank(G) = n; the reference's QR
            # elimination (misc.py:1244-1282) needs it on the null space of A only
            self.rank_msg += (", or Rank(G) < n: with equality constraints this path eliminates A through S^-1, S = G' W^-1 W^-T G, "
                              "which needs G to have full column rank")

    def start_solve(self, x, y, z):
        try:
            self.kkt.solve(x, y, z)
        except ArithmeticError:
            raise ValueError(self.rank_msg)

    def stats(self, tau):
        e, D = self, self.D                                               # residuals (coneprog.py:861-896)
        e.Af(e.y, e.hrx, alpha=-1.0, trans="T")
        e.Gf(e.z, e.hrx, alpha=-1.0, beta=1.0, trans="T")
        v_hrx = e.hrx.dot(e.hrx)
        e.rx.copy_from(e.hrx)
        e.rx.axpy(e.cv, -tau)
        v_rx = e.rx.dot(e.rx)
        e.Af(e.x, e.hry)
        v_hry = e.hry.dot(e.hry)
        e.ry.copy_from(e.hry)
        e.ry.axpy(e.bv, -tau)
        v_ry = e.ry.dot(e.ry)
        e.Gf(e.x, e.hrz)
        e.hrz.axpy(e.s)
        v_hrz = sdot(D, e.hrz.ptr, e.hrz.ptr)
        e.rz.fill(0.0)
        e.rz.axpy(e.hrz)
        e.rz.axpy(e.hv, -tau)
        v_rz = sdot(D, e.rz.ptr, e.rz.ptr)
        return v_hrx, v_rx, v_hry, v_ry, v_hrz, v_rz, e.cv.dot(e.x), e.bv.dot(e.y), sdot(D, e.hv.ptr, e.z.ptr), e.lam2

    def scaling(self):
        compute_scaling(self.D, self.s, self.z, self.W, self.lmbda)
        return self.lmbda.dot(self.lmbda)

    def scale(self, primal, dual):
        if primal is not None:
            self.x.scal(primal); self.s.scal(primal)
            self.symm(self.s)
        if dual is not None:
            self.y.scal(dual); self.z.scal(dual)
            self.symm(self.z)

    def f6_no_ir(self, bx, by, bz, btau, bs, bkappa):                     # coneprog.py:1130-1195
        e, D = self, self.D
        by.scal(-1.0)
        sinv(D, bs.ptr, e.lmbda.ptr)
        bs.scal(-1.0)
        e.ws3.copy_from(bs)
        scale(D, e.W, e.ws3.ptr, trans="T")
        bz.axpy(e.ws3)
        bz.scal(-1.0)
        e.kkt.solve(bx, by, bz)
        bkappa[0] = -bkappa[0] / e.lmbda_g
        btau[0] += bkappa[0] / e.dgi
        btau[0] = e.dgi * (btau[0] + e.cv.dot(bx) + e.bv.dot(by) + sdot(D, e.th.ptr, bz.ptr)) / (1.0 + e.z1z1)
        bx.axpy(e.x1, btau[0]); by.axpy(e.y1, btau[0]); bz.axpy(e.z1, btau[0])
        bs.axpy(bz, -1.0)
        bkappa[0] -= btau[0]

    def res(self, ux, uy, uz, utau, us, ukappa, vx, vy, vz, vtau, vs, vkappa):   # coneprog.py:578-631
        e, D, dg, ws3, wz3 = self, self.D, self.dg, self.ws3, self.wz3
        e.Af(uy, vx, alpha=-1.0, beta=1.0, trans="T")
        wz3.copy_from(uz)
        scale(D, e.W, wz3.ptr, inverse="I")
        e.Gf(wz3, vx, alpha=-1.0, beta=1.0, trans="T")
        vx.axpy(e.cv, -utau[0] / dg)
        e.Af(ux, vy, alpha=1.0, beta=1.0)
        vy.axpy(e.bv, -utau[0] / dg)
        e.Gf(ux, vz, alpha=1.0, beta=1.0)
        vz.axpy(e.hv, -utau[0] / dg)
        ws3.copy_from(us)
        scale(D, e.W, ws3.ptr, trans="T")
        vz.axpy(ws3)
        vtau[0] += dg * ukappa[0] + e.cv.dot(ux) + e.bv.dot(uy) + sdot(D, e.hv.ptr, wz3.ptr)
        ws3.copy_from(us)
        ws3.axpy(uz)
        sprod(D, ws3.ptr, e.lmbda.ptr, diag="D")
        vs.axpy(ws3)
        vkappa[0] += e.lmbda_g * (utau[0] + ukappa[0])

    def direction(self, i, sigma, mu, rt, dg, dgi, lmbda_g, wkappa3):
        e, D = self, self.D
        e.sigma, e.mu, e.rt, e.dg, e.dgi, e.lmbda_g, e.wkappa3 = sigma, mu, rt, dg, dgi, lmbda_g, wkappa3
        if i == 1:
            return
        unfactored, e.unfactored = e.unfactored, False
        ssqr(D, e.lmbdasq.ptr, e.lmbda.ptr)
        try:                                                              # factor, and the constant system (coneprog.py:1066-1128)
            e.kkt.factor(e.W)
            e.x1.copy_from(e.cv).scal(-1.0)
            e.y1.copy_from(e.bv)
            e.z1.copy_from(e.hv)
            e.kkt.solve(e.x1, e.y1, e.z1)
            e.x1.scal(dgi); e.y1.scal(dgi); e.z1.scal(dgi)
        except ArithmeticError:
            if unfactored:
                raise ValueError(e.rank_msg)
            raise
        e.th.copy_from(e.hv)
        scale(D, e.W, e.th.ptr, trans="T", inverse="I")
        e.z1z1 = sdot(D, e.z1.ptr, e.z1.ptr)

    def bounds(self, i):
        e, D, sigma = self, self.D, self.sigma                            # right-hand side (coneprog.py:1250-1298), f6, ws3
        put_diag(D, e.ds, e.lmbdasq.ptr)
        dkappa = [e.lmbda_g ** 2]
        if i == 1:
            e.ds.axpy(e.ws3)
            e.ds.axpy(D.e, -sigma * e.mu)
            dkappa[0] += e.wkappa3 - sigma * e.mu
        e.dx.copy_from(e.rx).scal(1.0 - sigma)
        e.dy.copy_from(e.ry).scal(1.0 - sigma)
        e.dz.copy_from(e.rz).scal(1.0 - sigma)
        dtau = [(1.0 - sigma) * e.rt]
        e.f6(e.dx, e.dy, e.dz, dtau, e.ds, dkappa)
        if i == 0:
            e.ws3.copy_from(e.ds)
            sprod(D, e.ws3.ptr, e.dz.ptr)
        return (dtau[0], dkappa[0]) + e.scaled_bounds(i)

    def update(self, step, tau):
        self.lam2 = self.step(step)


def conelp(c, G, h, dims, A=None, b=None, options=None, primalstart=None, dualstart=None, kktsolver=None, chol_opts=None):
    """coneprog.conelp (coneprog.py:31-1436) for dims with 'q' / 's' cones, on the GPU.  Returns the reference's result dictionary
    with numpy arrays ('s' blocks of s and z as full symmetric matrices)."""
    if kktsolver is not None:
        raise NotImplementedError("conelp with 'q' / 's' cones runs misc.kkt_chol on the GPU; kktsolver is not selectable")
    opt = _ipm.options(options, dims)
    pb = _ipm.problem(c, G, h, dims, A, b)
    _lib.require_device()
    D = Dims(pb.dims)
    kkt = KKTConeDev(D, pb.n, *pb.G, pb.p, *pb.A, chol_opts)
    e = _ConeEngine(kkt, pb, D, opt.refinement, bool(primalstart and dualstart))
    res0 = (max(1.0, e.cv.nrm2()), max(1.0, e.bv.nrm2()), max(1.0, e.nrm2(e.hv)))
    t_start = time.perf_counter()
    out = _ipm.conelp_start(e, opt, primalstart, dualstart, res0)
    if not isinstance(out, _ipm.Outcome):
        out = _ipm.conelp_loop(e, opt, D.Nd, out, res0)
    xs, zs = out.status != "primal infeasible", out.status != "dual infeasible"      # a certificate comes without the other half
    return _ipm.conelp_result(
        opt.show, out.status, e.x.get() if xs else None, e.y.get() if zs else None, e.s.get() if xs else None, e.z.get() if zs else None,
        out.stats, e.max_step(e.s) if xs else None, e.max_step(e.z) if zs else None, out.iterations, kkt.nfactor, out.msg,
        **{"loop seconds": time.perf_counter() - t_start})


class _ConeQpEngine(_ConeOps):
    """The device vectors and launches of one coneqp run (the protocol of _ipm.coneqp_loop), to be read top to bottom as the launch
    order of an iteration."""

    def __init__(self, kkt, pb, D, nref):
        super().__init__(kkt, pb, D)
        n, p, N = pb.n, pb.p, D.N
        self.P = SymSpMatDev(n, *pb.P)
        self.qv, self.tmpx, self.dtmp = DVec(n, pb.c), DVec(n), DVec(N)
        w, w2 = ((DVec(n), DVec(p), DVec(N), DVec(N)) for _ in range(2)) if nref else ((), ())
        self.f4 = _ipm.f4(self.f4_no_ir, self.res, nref, w, w2)

    def f4_no_ir(self, bx, by, bz, bs):                                   # coneprog.py:2288-2316
        sinv(self.D, bs.ptr, self.lmbda.ptr)
        self.ws3.copy_from(bs)
        scale(self.D, self.W, self.ws3.ptr, trans="T")
        bz.axpy(self.ws3, -1.0)
        self.kkt.solve(bx, by, bz)
        bs.axpy(bz, -1.0)

    def res(self, ux, uy, uz, us, vx, vy, vz, vs):                        # coneprog.py:1930-1960
        e, D, ws3, wz3 = self, self.D, self.ws3, self.wz3
        e.P.symv(ux, vx, alpha=-1.0, beta=1.0)
        e.Af(uy, vx, alpha=-1.0, beta=1.0, trans="T")
        wz3.copy_from(uz)
        scale(D, e.W, wz3.ptr, inverse="I")
        e.Gf(wz3, vx, alpha=-1.0, beta=1.0, trans="T")
        e.Af(ux, vy, alpha=-1.0, beta=1.0)
        e.Gf(ux, vz, alpha=-1.0, beta=1.0)
        ws3.copy_from(us)
        scale(D, e.W, ws3.ptr, trans="T")
        vz.axpy(ws3, -1.0)
        ws3.copy_from(us)
        ws3.axpy(uz)
        sprod(D, ws3.ptr, e.lmbda.ptr, diag="D")
        vs.axpy(ws3, -1.0)

    def stats(self):
        # rx = Px + q + A'y + G'z, ry = Ax - b, rz = s + Gx - h  (coneprog.py:2169-2186)
        e, x, y, z, rx, ry, rz = self, self.x, self.y, self.z, self.rx, self.ry, self.rz
        rx.copy_from(e.qv)
        e.P.symv(x, rx, alpha=1.0, beta=1.0)
        e.tmpx.copy_from(rx)
        xPq, xq = x.dot(e.tmpx), x.dot(e.qv)
        e.Af(y, rx, beta=1.0, trans="T")
        e.Gf(z, rx, beta=1.0, trans="T")
        v_rx = rx.dot(rx)
        ry.copy_from(e.bv)
        e.Af(x, ry, alpha=1.0, beta=-1.0)
        v_ry = ry.dot(ry)
        rz.copy_from(e.s)
        rz.axpy(e.hv, -1.0)
        e.Gf(x, rz, beta=1.0)
        v_rz = e.dot(rz, rz)
        return xPq, xq, v_rx, v_ry, v_rz, y.dot(ry), e.dot(z, rz)

    def scaling(self):
        compute_scaling(self.D, self.s, self.z, self.W, self.lmbda)

    def factor(self):
        ssqr(self.D, self.lmbdasq.ptr, self.lmbda.ptr)
        self.kkt.factor(self.W)

    def direction(self, i, sigma_mu, eta, correction):
        # ds = -lmbdasq + sigma mu e (i = 0), -lmbdasq - dsa o dza + sigma mu e (i = 1)  (coneprog.py:2376-2392)
        e, D, ds, dz = self, self.D, self.ds, self.dz
        ds.fill(0.0)
        if correction and i == 1:
            ds.axpy(e.ws3, -1.0)
        put_diag(D, e.dtmp, e.lmbdasq.ptr)
        ds.axpy(e.dtmp, -1.0)
        ds.axpy(D.e, sigma_mu)
        e.dx.fill(0.0).axpy(e.rx, -1.0 + eta)
        e.dy.fill(0.0).axpy(e.ry, -1.0 + eta)
        dz.fill(0.0).axpy(e.rz, -1.0 + eta)
        e.f4(e.dx, e.dy, dz, ds)
        dsdz = e.dot(ds, dz)
        if correction and i == 0:                                         # ds o dz for the Mehrotra correction
            e.ws3.copy_from(ds)
            sprod(D, e.ws3.ptr, dz.ptr)
        return (dsdz,) + e.scaled_bounds(i)

    update = _ConeOps.step


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
    pb = _ipm.problem(q, G, h, dims, A, b, P, qp=True)
    if pb.cdim == 0:
        raise NotImplementedError("coneqp without cone constraints is not part of the general-cone path")
    _lib.require_device()
    D = Dims(pb.dims)
    kkt = KKTConeDev(D, pb.n, *pb.G, pb.p, *pb.A, chol_opts, *pb.P)
    e = _ConeQpEngine(kkt, pb, D, opt.refinement)
    res0 = (max(1.0, e.qv.nrm2()), max(1.0, e.bv.nrm2()), max(1.0, e.nrm2(e.hv)))
    out = _ipm.coneqp_loop(e, opt, D.ml + D.nq + D.tot1, _ipm.coneqp_start(e, initvals), res0)
    e.symm(e.s); e.symm(e.z)                                              # misc.symm of the 's' blocks
    return _ipm.coneqp_result(opt.show, out.status, e.x.get(), e.y.get() if pb.p else np.zeros(0), e.s.get(), e.z.get(), out.stats,
                              e.max_step(e.s), e.max_step(e.z), out.iterations, kkt.nfactor, out.msg)
