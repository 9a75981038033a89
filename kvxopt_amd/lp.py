"""Device-resident cone-LP and cone-QP interior-point drivers for the orthant cone:

    minimize c'x [+ (1/2) x'Px]  subject to  G x + s = h,  A x = b,  s >= 0          (G sparse, ml x n; A sparse, p x n, p >= 0)

A restatement of the reference's `coneprog.conelp` / `coneqp` (src/python/coneprog.py:31-2547) specialised to dims = {'l': ml, 'q': [],
's': []}, with the default KKT solver `misc.kkt_chol2` (src/python/misc.py:1352-1567) or a caller's `kktsolver`.  Every vector lives in
HBM for the whole solve; per iteration the host sees only scalars (gap, residual norms, step lengths).  Per iteration, as in the
reference: 1 numeric refactorisation of S = G' diag(di^2) G on a fixed symbolic analysis, 3 KKT solves, 2 products with G
and 2 with G', the NT-scaling update -- all HIP kernels of libkvxhip.so.  No CPU fallback.  KKT objects: KKTChol2Dev (p = 0), KKTDiagEqDev
(p > 0, diagonal S, sparse K = A S^{-1} A' on a fixed pattern), KKTGenEqDev (p > 0, general S, dense K in HBM); `misc.kkt_chol2` is built
on the same classes.

Both loops and both starting points are written once, on host scalars, in _ipm.py (`conelp_loop`, `coneqp_loop`); this module holds the
engines that own the vectors and the launches.  conelp has four, all with the same arithmetic and roundings (tests/test_kkt_gpu.py
compares them bit for bit): `_CIssued`, the default for p = 0 (fused kernels, an iteration in four C calls); `_PythonIssued`,
KVX_LP_PYCALLS=1 (the same launches, one ctypes call each); `_PerOperation`, KVX_LP_UNFUSED=1, p > 0 or a user's kktsolver (one launch
per BLAS-1-sized operation); `_Refined`, options['refinement'] > 0 (iterative refinement of the Newton systems).  coneqp has one,
`_QpEngine`.  cone.py holds the engines of the general cones.
"""
import collections
import ctypes
import os
import time

import numpy as np

from . import _ipm, _lib, base
from ._lib import lib, raise_for
from .chol import Factor
from .devvec import DVec, SpMatDev, SymSpMatDev, reduce_multi      # noqa: F401  (lp.DVec, lp.SpMatDev, ... are public names)

# the schedule of conelp's iteration (module docstring); the library reads KVX_LP_UNFUSED too
_UNFUSED = os.environ.get("KVX_LP_UNFUSED", "0") not in ("", "0")
_PYCALLS = os.environ.get("KVX_LP_PYCALLS", "0") not in ("", "0")


def _sides(items):
    """ctypes array of kvx_kkt_side from (xin, xscale, zin, xout, xoscale, zout, zoscale) tuples of DVecs and floats."""
    arr = (_lib.KktSide * 2)()
    for k, (xin, xs, zin, xout, xos, zout, zos) in enumerate(items):
        a = arr[k]
        a.xin, a.xscale, a.zin = xin.ptr, float(xs), zin.ptr
        a.xout, a.xoscale, a.zout, a.zoscale = xout.ptr, float(xos), zout.ptr, float(zos)
    return arr


class KKTChol2Dev:
    """Device-resident `misc.kkt_chol2` for sparse G and p = 0 (misc.py:1389-1563)."""

    def __init__(self, ml, n, Gp, Gi, Gx, chol_opts=None, Pp=None, Pi=None, Px=None):
        """Pp, Pi, Px: optional lower-triangular CCS of the QP Hessian H (coneqp): S = H + G' W^-1 W^-T G
        (misc.py:1425-1426, 1454-1455)."""
        self.ml, self.n = ml, n
        Gp = np.ascontiguousarray(Gp, dtype=np.int64)
        Gi = np.ascontiguousarray(Gi, dtype=np.int64)
        h = ctypes.c_void_p()
        self.Px = None
        if Pp is not None:
            Pp = np.ascontiguousarray(Pp, dtype=np.int64)
            Pi = np.ascontiguousarray(Pi, dtype=np.int64)
            self.Px = DVec(max(len(Px), 1), Px if len(Px) else None)
            raise_for(lib().kvx_atda_plan(ml, n, _lib.pi(Gp), _lib.pi(Gi), _lib.pi(Pp), _lib.pi(Pi), ctypes.byref(h)))
        else:
            raise_for(lib().kvx_atda_plan(ml, n, _lib.pi(Gp), _lib.pi(Gi), None, None, ctypes.byref(h)))
        self._plan = h
        snz = ctypes.c_int64()
        raise_for(lib().kvx_atda_pattern(h, ctypes.byref(snz), None, None))
        self.Sp = np.empty(n + 1, dtype=np.int64)
        Si = np.empty(max(snz.value, 1), dtype=np.int64)
        raise_for(lib().kvx_atda_pattern(h, ctypes.byref(snz), _lib.pi(self.Sp), _lib.pi(Si)))
        self.Si = Si[:snz.value].copy()
        # first call of the reference fixes the pattern of S and analyses it once (misc.py:1422-1432)
        self.fac = Factor(n, self.Sp, self.Si, "L", None, chol_opts)
        self.G = SpMatDev(ml, n, Gp, Gi, Gx)
        self.w = DVec(ml)
        self.t = DVec(ml)
        self.Sx = DVec(self.Si.size)
        self.di = None
        self.nfactor = 0
        self.async_solves = False      # True: solves are only enqueued; check() after the next host synchronisation

    def __del__(self):
        if getattr(self, "_plan", None):
            lib().kvx_atda_free(self._plan)
            self._plan = None

    def reset(self, Gx, Px=None):
        """New values of G (and H) on the patterns given at construction: the object -- product map, analysis of S, captured
        launch graphs -- serves another problem of the same structure (see `_kkt_for`)."""
        self.G.set_values(Gx)
        if Px is not None:
            self.set_hessian(Px)
        self.di = None
        self.nfactor = 0
        self.async_solves = False

    def set_hessian(self, Px):
        """New values of H on the pattern given at construction (cvxprog: H changes at every iteration)."""
        if self.Px is not None and len(Px):
            self.Px.set(Px)

    def factor(self, di, sync=True):
        """S = G' diag(di)^2 G on the fixed pattern, numeric refactorisation (misc.py:1418-1462).
        Raises ArithmeticError when S is not positive definite -- with sync=False only the NEXT solve does (the solve
        is queued behind the factorisation without a host round trip)."""
        self._assemble(di)
        self.fac.factorize_dev(self.Sx.ptr, sync=sync)
        self.di = di
        self.nfactor += 1

    def _assemble(self, di):
        if _UNFUSED:
            self.w.sqr_of(di)
            raise_for(lib().kvx_atda_assemble_dev(self._plan, self.G.vx.ptr, self.w.ptr,
                                                  None if self.Px is None else self.Px.ptr, self.Sx.ptr))
        else:                                            # the square is taken while G is scaled: one launch less
            raise_for(lib().kvx_atda_assemble_sq_dev(self._plan, self.G.vx.ptr, di.ptr,
                                                     None if self.Px is None else self.Px.ptr, self.Sx.ptr))

    def _x2buf(self):
        if getattr(self, "_x2", None) is None:
            self._x2 = DVec(2 * max(self.n, 1))
        return self._x2

    def _pre(self, sides, nrhs):
        G = self.G
        raise_for(lib().kvx_kkt_solve_pre_dev(self.ml, self.n, G.cp.ptr, G.ri.ptr, G.vx.ptr, G.max_col, self.di.ptr, nrhs, sides,
                                              self._x2buf().ptr, max(1, self.n)))

    def _post(self, sides, nrhs):
        G = self.G
        raise_for(lib().kvx_kkt_solve_post_dev(self.ml, self.n, G.tcp.ptr, G.tri.ptr, G.tvx.ptr, G.max_row, self.di.ptr, nrhs, sides,
                                               self._x2buf().ptr, max(1, self.n)))

    def solve_sides(self, items):
        """One or two KKT solves with the current factor, each side given as (xin, xscale, zin, xout, xoscale, zout, zoscale):
        x2 := xscale*xin + Gs' W^-1 zin ; x2 := S^-1 x2 ; xout := xoscale*x2 ; zout := zoscale*(Gs x2 - W^-1 zin)
        (misc.py:1489-1563 with p = 0) in three enqueues: kvx_kkt_solve_pre_dev, the triangular solves, kvx_kkt_solve_post_dev."""
        nrhs = len(items)
        sides = _sides(items)
        self._pre(sides, nrhs)
        self.fac.solve_dev(self._x2buf().ptr, 0, nrhs, max(1, self.n), sync=not self.async_solves)
        self._post(sides, nrhs)

    def factor_solve_sides(self, di, items):
        """factor(di) and solve_sides(items) with the factorisation and the triangular solves as ONE enqueue
        (kvx_chol_factorize_solve_async_dev).  Enqueue only -- check() after the next host synchronisation."""
        nrhs = len(items)
        sides = _sides(items)
        self._assemble(di)
        self.di = di
        self.nfactor += 1
        self._pre(sides, nrhs)
        self.fac.factorize_solve_async_dev(self.Sx.ptr, self._x2buf().ptr, nrhs, max(1, self.n))
        self._post(sides, nrhs)

    def factor_solve2(self, di, xa, za, xb, zb):
        """factor(di) and solve2(xa, za, xb, zb) as ONE enqueue (kvx_chol_factorize_solve_async_dev): the two right-hand sides
        do not depend on the factor, so they are formed first and the forward sweep runs beside the factorisation of the top of
        the tree.  Same kernels, same order: bitwise what factor() followed by solve2() gives.  Enqueue only -- check() after
        the next host synchronisation."""
        n = self.n
        if not _UNFUSED:
            return self.factor_solve_sides(di, [(xa, 1.0, za, xa, 1.0, za, 1.0), (xb, 1.0, zb, xb, 1.0, zb, 1.0)])
        self._x2buf()
        self._assemble(di)
        self.di = di
        self.nfactor += 1
        for k, (x, z) in enumerate(((xa, za), (xb, zb))):
            z.mul(di)
            self.t.xmy(1.0, di, z)
            self.G.gemv(self.t, x, trans="T", alpha=1.0, beta=1.0)
            raise_for(lib().kvx_vec_copy_dev(n, x.ptr, self._x2.ptr + 8 * n * k))
        self.fac.factorize_solve_async_dev(self.Sx.ptr, self._x2.ptr, 2, max(1, n))
        for k, (x, z) in enumerate(((xa, za), (xb, zb))):
            raise_for(lib().kvx_vec_copy_dev(n, self._x2.ptr + 8 * n * k, x.ptr))
            self.G.gemv(x, self.t, trans="N")
            z.xmy(1.0, di, self.t, -1.0)

    def check(self):
        """Raise ArithmeticError if the last (asynchronous) factorisation failed; synchronises the factor's stream."""
        self.fac.status()

    def solve(self, x, z):
        """Overwrites (x, z) with (ux, W*uz) (misc.py:1489-1563 with p = 0)."""
        di = self.di
        if not _UNFUSED:
            return self.solve_sides([(x, 1.0, z, x, 1.0, z, 1.0)])
        z.mul(di)                                        # z := W^{-1} z                (misc.py:1513)
        self.t.xmy(1.0, di, z)                           # t := di .* z
        self.G.gemv(self.t, x, trans="T", alpha=1.0, beta=1.0)   # x += Gs' z       (misc.py:1524)
        self.fac.solve_dev(x.ptr, 0, 1, max(1, self.n), sync=not self.async_solves)  # x := S^{-1} x (sys 7,4 then 5,8: misc.py:1531-1558)
        self.G.gemv(x, self.t, trans="N")                # t := G x
        z.xmy(1.0, di, self.t, -1.0)                     # z := Gs x - z                (misc.py:1563)

    def solve2(self, xa, za, xb, zb):
        """Two KKT systems with the same factor in ONE two-column triangular solve (the interior-point iteration has
        two right-hand sides that do not depend on each other: the (-c, h) system and the predictor)."""
        di, n = self.di, self.n
        if not _UNFUSED:
            return self.solve_sides([(xa, 1.0, za, xa, 1.0, za, 1.0), (xb, 1.0, zb, xb, 1.0, zb, 1.0)])
        self._x2buf()
        for k, (x, z) in enumerate(((xa, za), (xb, zb))):
            z.mul(di)
            self.t.xmy(1.0, di, z)
            self.G.gemv(self.t, x, trans="T", alpha=1.0, beta=1.0)
            raise_for(lib().kvx_vec_copy_dev(n, x.ptr, self._x2.ptr + 8 * n * k))
        self.fac.solve_dev(self._x2.ptr, 0, 2, max(1, n), sync=not self.async_solves)
        for k, (x, z) in enumerate(((xa, za), (xb, zb))):
            raise_for(lib().kvx_vec_copy_dev(n, self._x2.ptr + 8 * n * k, x.ptr))
            self.G.gemv(x, self.t, trans="N")
            z.xmy(1.0, di, self.t, -1.0)


class KKTUserHost:
    """The reference's plug-in point `kktsolver(W) -> f(x, y, z)` (coneprog.py:323-344, 571-585) under the device-resident
    conelp: the caller's factory is handed the scaling on the host (W['d'], W['di'] as base.matrix; the other fields of the
    'l'-cone scaling empty, as misc.compute_scaling leaves them) at every factorisation, and its f the right-hand sides as
    base.matrix columns at every solve; (ux, uy, W uz) go back to HBM.  Functional, not fast -- every solve crosses PCIe --
    and the place where `kvxopt_amd.misc.kkt_chol2` (host-array mirror of the reference's default) or any user solver plugs in."""

    def __init__(self, ml, n, Gp, Gi, Gx, p, Ap, Ai, Ax, factory):
        self.ml, self.n, self.p = ml, n, p
        self.G = SpMatDev(ml, n, Gp, Gi, Gx)
        self.A = SpMatDev(p, n, Ap, Ai, Ax) if p else None
        self.factory = factory
        self.f = None
        self.di = None
        self.nfactor = 0
        self.async_solves = False

    def factor(self, di, sync=True):
        dih = di.get()
        empty = base.matrix(0.0, (0, 1))
        W = {"d": base.matrix(1.0 / dih), "di": base.matrix(dih), "dnl": empty, "dnli": base.matrix(0.0, (0, 1)),
             "v": [], "beta": [], "r": [], "rti": []}
        self.f = self.factory(W)                          # ArithmeticError / ValueError of the caller's factorisation pass through
        self.di = di
        self.nfactor += 1

    def solve(self, x, y, z):
        xm = base.matrix(x.get())
        ym = base.matrix(y.get()) if self.p else base.matrix(0.0, (0, 1))
        zm = base.matrix(z.get())
        self.f(xm, ym, zm)
        x.set(xm._a)
        if self.p:
            y.set(ym._a)
        z.set(zm._a)

    def check(self):
        pass


class KKTDiagEqDev:
    """Device-resident `misc.kkt_chol2` with equality constraints (p > 0) for a G whose columns have disjoint row
    supports (every row of G holds at most one entry -- G = -I of a standard-form LP).  Then
    S = G' W^-1 W^-T G is DIAGONAL and the reference's K = A S^-1 A' (misc.py:1483-1487, 1545: sparse triangular
    solves with the factor of S, then a syrk) is one more fixed-pattern assembly, K = sum_k (1/S_kk) A[:,k] A[:,k]',
    factored numerically on a symbolic analysis done once (the reference re-analyses K at every call, misc.py:1486)."""

    def __init__(self, ml, n, Gp, Gi, Gx, p, Ap, Ai, Ax, chol_opts=None):
        self.ml, self.n, self.p = ml, n, p
        Gi = np.ascontiguousarray(Gi, dtype=np.int64)
        if Gi.size and np.bincount(Gi, minlength=ml).max() > 1:
            raise NotImplementedError("device-resident conelp with equality constraints needs a G with at most one "
                                      "entry per row (diagonal S); use kvxopt_amd.misc.kkt_chol2 (host arrays) otherwise")
        self.G = SpMatDev(ml, n, Gp, Gi, Gx)
        self.G2 = SpMatDev(ml, n, Gp, Gi, np.asarray(Gx, dtype=np.float64) ** 2)
        self.A = SpMatDev(p, n, Ap, Ai, Ax)
        # CCS of A' (n x p) = CSR of A
        Ap = np.asarray(Ap, dtype=np.int64); Ai = np.asarray(Ai, dtype=np.int64); Ax = np.asarray(Ax, dtype=np.float64)
        cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
        order = np.lexsort((cols, Ai))
        self._at_order = order
        ATi, ATx = cols[order], Ax[order]
        ATp = np.zeros(p + 1, dtype=np.int64)
        np.add.at(ATp, Ai + 1, 1)
        np.cumsum(ATp, out=ATp)
        h = ctypes.c_void_p()
        raise_for(lib().kvx_atda_plan(n, p, _lib.pi(ATp), _lib.pi(np.ascontiguousarray(ATi)), None, None, ctypes.byref(h)))
        self._plan = h
        self.A2 = SpMatDev(p, n, Ap, Ai, Ax ** 2)                     # diag(K) = (A o A) S^-1
        self.kd = DVec(max(p, 1))
        self.kscale = 1.0
        knz = ctypes.c_int64()
        raise_for(lib().kvx_atda_pattern(h, ctypes.byref(knz), None, None))
        self.Kp = np.empty(p + 1, dtype=np.int64)
        Ki = np.empty(max(knz.value, 1), dtype=np.int64)
        raise_for(lib().kvx_atda_pattern(h, ctypes.byref(knz), _lib.pi(self.Kp), _lib.pi(Ki)))
        self.Ki = Ki[:knz.value].copy()
        # K is factored after scaling to max(diag K) = 1 with the pivot rule "d <= 1e-30 -> 1e128" (cholmod's dbound in its
        # drop-the-row form): near the solution S^-1 = diag(x ./ z) spans twenty orders of magnitude and K = A S^-1 A' loses
        # rank in floating point; the reference stops there with status 'unknown' (coneprog.py:1078-1109), interior-point
        # codes built on normal equations zero the affected multipliers instead.
        ko = {"dbound": 1e-15, "dbound_drop": 1}
        ko.update(chol_opts or {})
        self.fac = Factor(p, self.Kp, self.Ki, "L", None, ko)
        self.ATx = DVec(max(ATx.size, 1), ATx if ATx.size else None)
        self.Kx = DVec(self.Ki.size)
        self.w, self.t = DVec(ml), DVec(ml)
        self.sdiag, self.sinv, self.u = DVec(n), DVec(n), DVec(n)
        self.di = None
        self.nfactor = 0
        self.async_solves = False

    def __del__(self):
        if getattr(self, "_plan", None):
            lib().kvx_atda_free(self._plan)
            self._plan = None

    def reset(self, Gx, Ax):
        """New values of G and A on the patterns given at construction (see `_kkt_for`)."""
        Gx = np.asarray(Gx, dtype=np.float64); Ax = np.asarray(Ax, dtype=np.float64)
        self.G.set_values(Gx); self.G2.set_values(Gx ** 2)
        self.A.set_values(Ax); self.A2.set_values(Ax ** 2)
        if Ax.size:
            self.ATx.set(Ax[self._at_order])
        self.kscale = 1.0
        self.di = None
        self.nfactor = 0
        self.async_solves = False

    def factor(self, di, sync=True):
        self.w.sqr_of(di)
        self.G2.gemv(self.w, self.sdiag, trans="T")                   # S_kk = sum_i di_i^2 G_ik^2
        self.sinv.fill(1.0).div(self.sdiag)
        self.A2.gemv(self.sinv, self.kd, trans="N", alpha=-1.0)       # -diag(K)
        smin, kmax = reduce_multi([("max", self.sdiag), ("max", self.kd)])   # one host round trip: -min S_kk, max diag K
        if -smin <= 0.0 or not (kmax > 0.0) or not np.isfinite(kmax):  # S singular / K = 0
            raise ArithmeticError(0)
        self.kscale = 1.0 / kmax
        self.sinv.scal(self.kscale)                                   # K' = A (S^-1 / max diag K) A'
        raise_for(lib().kvx_atda_assemble_dev(self._plan, self.ATx.ptr, self.sinv.ptr, None, self.Kx.ptr))
        self.sinv.scal(kmax)
        self.fac.factorize_dev(self.Kx.ptr, sync=sync)
        self.di = di
        self.nfactor += 1

    def check(self):
        self.fac.status()

    def solve(self, x, y, z):
        """Overwrites (x, y, z) = (bx, by, bz) with (ux, uy, uz) of misc.py:1489-1563."""
        di = self.di
        z.mul(di)
        self.t.xmy(1.0, di, z)
        self.G.gemv(self.t, x, trans="T", alpha=1.0, beta=1.0)        # x := bx + G' W^-1 W^-T bz
        self.u.xmy(1.0, self.sinv, x)                                 # u := S^-1 x
        self.A.gemv(self.u, y, trans="N", alpha=1.0, beta=-1.0)       # y := A S^-1 x - by
        self.fac.solve_dev(y.ptr, 0, 1, max(1, self.p), sync=not self.async_solves)   # y := K'^-1 y
        y.scal(self.kscale)                                           # K^-1 = K'^-1 / max diag K: uy
        self.A.gemv(y, x, trans="T", alpha=-1.0, beta=1.0)
        x.mul(self.sinv)                                              # x := S^-1 (x - A' uy) = ux
        self.G.gemv(x, self.t, trans="N")
        z.xmy(1.0, di, self.t, -1.0)                                  # z := W^-T (G ux - bz) = uz

    def solve2(self, xa, ya, za, xb, yb, zb):
        """Two KKT systems, one two-column solve with the factor of K (see KKTChol2Dev.solve2)."""
        di, p = self.di, self.p
        if getattr(self, "_y2", None) is None:
            self._y2 = DVec(2 * max(p, 1))
        for k, (x, y, z) in enumerate(((xa, ya, za), (xb, yb, zb))):
            z.mul(di)
            self.t.xmy(1.0, di, z)
            self.G.gemv(self.t, x, trans="T", alpha=1.0, beta=1.0)
            self.u.xmy(1.0, self.sinv, x)
            self.A.gemv(self.u, y, trans="N", alpha=1.0, beta=-1.0)
            raise_for(lib().kvx_vec_copy_dev(p, y.ptr, self._y2.ptr + 8 * p * k))
        self.fac.solve_dev(self._y2.ptr, 0, 2, max(1, p), sync=not self.async_solves)
        self._y2.scal(self.kscale)
        for k, (x, y, z) in enumerate(((xa, ya, za), (xb, yb, zb))):
            raise_for(lib().kvx_vec_copy_dev(p, self._y2.ptr + 8 * p * k, y.ptr))
            self.A.gemv(y, x, trans="T", alpha=-1.0, beta=1.0)
            x.mul(self.sinv)
            self.G.gemv(x, self.t, trans="N")
            z.xmy(1.0, di, self.t, -1.0)


def dense_schur(Sfac, AT, X, Kd, Kx, kdiag, n, p, cols):
    """K = A S^-1 A' as a dense p x p matrix in HBM from the factor of S (misc.py:1476-1487 written with S^-1): X = S^-1 A' in
    column blocks of `cols` (AT: the CCS of A', n x p), K = A X, its lower triangle packed into Kx, -diag(K) into kdiag.  Returns
    max diag(K) (one host round trip); the solves with S are only enqueued, a failed factorisation of S surfaces in its status."""
    for c0 in range(0, p, cols):                                       # column blocks of X = S^-1 A' and of K = A X
        nb = min(cols, p - c0)
        raise_for(lib().kvx_dense_from_ccs_dev(n, nb, AT.cp.ptr + 8 * c0, AT.ri.ptr, AT.vx.ptr, X.ptr, n))
        Sfac.solve_dev(X.ptr, 0, nb, n, sync=False)
        raise_for(lib().kvx_spmm_t_dev(p, nb, AT.cp.ptr, AT.ri.ptr, AT.vx.ptr, X.ptr, n, Kd.ptr + 8 * c0 * p, p))
    raise_for(lib().kvx_pack_lower_dev(p, Kd.ptr, p, Kx.ptr))
    # scale to max diag K = 1 (one host round trip; it also surfaces a failed factorisation of S)
    raise_for(lib().kvx_vec_copy_strided_dev(p, Kd.ptr, p + 1, kdiag.ptr))
    kdiag.scal(-1.0)
    return kdiag.max_step()


class KKTGenEqDev:
    """Device-resident `misc.kkt_chol2` with equality constraints and a GENERAL sparse G (S not diagonal), for a moderate
    number p of equality rows.  The reference forms Asct = L^-1 P A' by sparse triangular solves, K = Asct' Asct by a sparse
    syrk and re-analyses K at every call (misc.py:1476-1487).  Here X = S^-1 A' is one multi-right-hand-side solve with the
    factor of S (n x p dense), K = A X a dense p x p matrix (one gather mat-mat), factored as a single dense front by the
    same Cholesky (dense lower pattern, analysed once).  KKT solve (misc.py:1489-1563 written with S^-1):
    u = S^-1 (bx + G' W^-1 W^-T bz), uy = K^-1 (A u - by), ux = S^-1 (bx + G'.. - A' uy), uz = W^-T (G ux - bz)."""

    BLOCK_BYTES = 1 << 30        # X = S^-1 A' is formed in column blocks of about this size (n x cols doubles)

    def __init__(self, ml, n, Gp, Gi, Gx, p, Ap, Ai, Ax, chol_opts=None, Pp=None, Pi=None, Px=None):
        """Pp, Pi, Px: optional lower-triangular CCS of the QP Hessian (coneqp): S = P + G' W^-1 W^-T G.
        Any p: K = A S^-1 A' is structurally dense whenever S is irreducible (every column of L^-1 P A' reaches the root of
        the elimination tree), so it is held as a dense p x p matrix in HBM (20 GB at p = 50 000) and X = S^-1 A' is formed
        and consumed in column blocks -- never as a whole."""
        self.ml, self.n, self.p = ml, n, p
        self.cols = max(1, min(max(p, 1), self.BLOCK_BYTES // (8 * max(n, 1))))
        self.S = KKTChol2Dev(ml, n, Gp, Gi, Gx, chol_opts, Pp, Pi, Px)
        self.G = self.S.G
        self.A = SpMatDev(p, n, Ap, Ai, Ax)
        # CCS of A' (n x p) = CSR of A
        Ap = np.asarray(Ap, dtype=np.int64); Ai = np.asarray(Ai, dtype=np.int64); Ax = np.asarray(Ax, dtype=np.float64)
        cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
        order = np.lexsort((cols, Ai))
        self._at_order = order
        ATp = np.zeros(p + 1, dtype=np.int64)
        np.add.at(ATp, Ai + 1, 1)
        np.cumsum(ATp, out=ATp)
        self.AT = SpMatDev(n, p, ATp, cols[order], Ax[order])
        self.X = DVec(max(n * self.cols, 1))
        self.x_whole = p <= self.cols and os.environ.get("KVX_KKT_NO_X") != "1"     # X = S^-1 A' of the last factorisation is held as a whole
        self.Kd = DVec(max(p * p, 1))
        self.Kx = DVec(max(p * (p + 1) // 2, 1))
        Kp = np.zeros(p + 1, dtype=np.int64)
        Kp[1:] = np.cumsum(np.arange(p, 0, -1))
        Ki = np.concatenate([np.arange(j, p, dtype=np.int64) for j in range(p)]) if p else np.zeros(0, np.int64)
        # K is dense: natural order, one front; scaled to max diag = 1 with the pivot floor of KKTDiagEqDev
        self.fac = Factor(p, Kp, Ki, "L", None, {"ordering": 1, "dbound": 1e-15, "dbound_drop": 1})
        self.kdiag = DVec(max(p, 1))
        self.u, self.r = DVec(n), DVec(n)
        self.t = self.S.t
        self.kscale = 1.0
        self.di = None
        self.nfactor = 0
        self._async = False

    def reset(self, Gx, Ax, Px=None):
        """New values of G, A (and H) on the patterns given at construction (see `_kkt_for`)."""
        Ax = np.asarray(Ax, dtype=np.float64)
        self.S.reset(Gx, Px)
        self.A.set_values(Ax)
        self.AT.set_values(Ax[self._at_order])
        self.kscale = 1.0
        self.di = None
        self.nfactor = 0
        self.async_solves = False

    @property
    def async_solves(self):
        return self._async

    @async_solves.setter
    def async_solves(self, v):
        self._async = v
        self.S.async_solves = v

    def factor(self, di, sync=True):
        n, p = self.n, self.p
        self.S.factor(di, sync=False)                                  # S = G' W^-1 W^-T G: assembly + numeric refactorisation
        kmax = dense_schur(self.S.fac, self.AT, self.X, self.Kd, self.Kx, self.kdiag, n, p, self.cols)
        self.S.check()
        if not (kmax > 0.0) or not np.isfinite(kmax):
            raise ArithmeticError(0)
        self.kscale = 1.0 / kmax
        self.Kx.scal(self.kscale)
        self.fac.factorize_dev(self.Kx.ptr, sync=sync)
        self.di = di
        self.nfactor += 1

    def check(self):
        self.S.check()
        self.fac.status()

    def solve(self, x, y, z):
        """Overwrites (x, y, z) = (bx, by, bz) with (ux, uy, uz)."""
        self._solve_cols(((x, y, z),))

    def solve2(self, xa, ya, za, xb, yb, zb):
        """Two KKT systems: their solves with S and with K are two-column solves (see KKTChol2Dev.solve2)."""
        self._solve_cols(((xa, ya, za), (xb, yb, zb)))

    def _solve_cols(self, systems):
        # u = S^-1 (bx + G' W^-1 W^-T bz), uy = K^-1 (A u - by), ux = u - X uy with X = S^-1 A' of the last factorisation when the
        # whole of it is at hand (p columns fit one block): S^-1 (b - A' uy) = S^-1 b - X uy, a dense product (80 MB at n = 50 000,
        # p = 200: 20 us) instead of a second sweep through the factor of S (0.5 ms).  Otherwise the second solve as in misc.py:1545-1553.
        di, n, p = self.di, self.n, self.p
        nc = len(systems)
        if getattr(self, "_u2", None) is None:
            self._u2 = DVec(2 * max(n, 1))
            self._y2 = DVec(2 * max(p, 1))
        U, Y = self._u2, self._y2
        for c, (x, y, z) in enumerate(systems):
            z.mul(di)
            self.t.xmy(1.0, di, z)
            self.G.gemv(self.t, x, trans="T", alpha=1.0, beta=1.0)    # x := bx + G' W^-1 W^-T bz
            raise_for(lib().kvx_vec_copy_dev(n, x.ptr, U.ptr + 8 * n * c))
        self.S.fac.solve_dev(U.ptr, 0, nc, max(1, n), sync=not self._async)           # u := S^-1 x
        for c, (x, y, z) in enumerate(systems):
            raise_for(lib().kvx_vec_copy_dev(n, U.ptr + 8 * n * c, self.u.ptr))
            self.A.gemv(self.u, y, trans="N", alpha=1.0, beta=-1.0)   # y := A u - by
            raise_for(lib().kvx_vec_copy_dev(p, y.ptr, Y.ptr + 8 * p * c))
        self.fac.solve_dev(Y.ptr, 0, nc, max(1, p), sync=not self._async)
        for c, (x, y, z) in enumerate(systems):
            raise_for(lib().kvx_vec_copy_dev(p, Y.ptr + 8 * p * c, y.ptr))
            y.scal(self.kscale)                                       # uy = K^-1 (A u - by)
        if self.x_whole:
            for c, (x, y, z) in enumerate(systems):
                raise_for(lib().kvx_vec_copy_dev(n, U.ptr + 8 * n * c, x.ptr))
                raise_for(lib().kvx_dense_gemv_dev(n, p, 1, -1.0, self.X.ptr, n, y.ptr, p, 1.0, x.ptr, n))   # ux = u - X uy
        else:
            for c, (x, y, z) in enumerate(systems):
                self.A.gemv(y, x, trans="T", alpha=-1.0, beta=1.0)    # x := x - A' uy
                raise_for(lib().kvx_vec_copy_dev(n, x.ptr, U.ptr + 8 * n * c))
            self.S.fac.solve_dev(U.ptr, 0, nc, max(1, n), sync=not self._async)       # ux = S^-1 (...)
            for c, (x, y, z) in enumerate(systems):
                raise_for(lib().kvx_vec_copy_dev(n, U.ptr + 8 * n * c, x.ptr))
        for c, (x, y, z) in enumerate(systems):
            self.G.gemv(x, self.t, trans="N")
            z.xmy(1.0, di, self.t, -1.0)                              # uz = W^-T (G ux - bz)


# The KKT objects of the last few constraint structures are kept: a sequence of cone programs on the same patterns of G, A (and
# P) -- the usual way an interior-point solver is deployed: receding-horizon control, parameter sweeps, branch and bound -- pays
# for the product map, the analysis of S (and K), the device set-up and the capture of the launch graphs once; only the values
# are refreshed.  cholmod.linsolve / klu.linsolve keep their analyses the same way.  `clear_cache()` releases them.
_KKT_CACHE = collections.OrderedDict()
_KKT_CACHE_MAX = 4


def clear_cache():
    """Release the cached KKT objects (device memory, analyses, launch graphs)."""
    _KKT_CACHE.clear()


_lib.register_cache(clear_cache)


def _opts_key(chol_opts):
    """Hashable key of an options dict whatever the value types (numpy integers, bools, floats): sorted (name, repr) pairs."""
    return tuple(sorted((str(k), repr(v.item() if hasattr(v, "item") else v)) for k, v in (chol_opts or {}).items()))


def _pattern_key(*arrays):
    return _lib.pattern_digest(*[np.ascontiguousarray(a, dtype=np.int64) for a in arrays])


def _kkt_for(kind, dims_key, patterns, chol_opts, build, refresh):
    """The cached KKT object of this structure with its values refreshed, or a new one (build())."""
    if os.environ.get("KVX_LP_NO_CACHE") == "1":
        return build()
    # the device is part of the key: the buffers, streams and launch graphs of a KKT object live on the device it was built on
    key = (kind, dims_key, _pattern_key(*patterns), _opts_key(chol_opts), _lib.current_device())
    kkt = _KKT_CACHE.pop(key, None)
    if kkt is None:
        kkt = _lib.retry_after_release(build)
    else:
        refresh(kkt)
    _KKT_CACHE[key] = kkt
    while len(_KKT_CACHE) > _KKT_CACHE_MAX:
        _KKT_CACHE.popitem(last=False)
    return kkt


class _Orthant:
    """What the starting points of _ipm ask an engine for, on the orthant: W = diag(d), e = 1, every vector a DVec."""
    rank_msg = "Rank(A) < p or Rank([G; A]) < n"

    def __init__(self, kkt, pb):
        self.kkt, self.ml, self.n, self.p = kkt, pb.cdim, pb.n, pb.p
        self.xz = isinstance(kkt, KKTChol2Dev)           # p = 0 on the device: its solves take (x, z)
        self.G = kkt.G
        self.Gf, self.Af = _ipm.operators(kkt.G, kkt.A if pb.p else None)
        self.d, self.di = DVec(pb.cdim), DVec(pb.cdim)

    def ksolve(self, x, y, z):
        self.kkt.solve(*((x, z) if self.xz else (x, y, z)))

    start_solve = ksolve

    def factor_identity(self, needed):                   # (the orthant drivers factor whether or not the start needs it)
        self.d.fill(1.0); self.di.fill(1.0)
        self.kkt.factor(self.di)

    def max_step(self, v):
        return v.max_step()

    def nrm2(self, v):
        return v.nrm2()

    def dot(self, u, v):
        return u.dot(v)

    def add_e(self, v, a):
        v.addc(a)

    def symm(self, v):
        pass


class _Engine(_Orthant):
    """The device vectors of one conelp run and what the schedules below have in common.  Each schedule is one subclass, to be read
    top to bottom as its launch order; all four do the same arithmetic with the same roundings."""

    def __init__(self, kkt, pb):
        super().__init__(kkt, pb)
        ml, n, p = pb.cdim, pb.n, pb.p
        self.cv, self.hv = DVec(n, pb.c), DVec(ml, pb.h)
        self.x, self.dx, self.x1, self.rx, self.hrx = (DVec(n) for _ in range(5))
        self.bv = DVec(p, pb.b) if p else _ipm.NoVec()   # p = 0: the y-blocks of the algorithm are empty
        self.y, self.dy, self.y1, self.ry, self.hry = (DVec(p) for _ in range(5)) if p else [self.bv] * 5
        self.s, self.z, self.ds, self.dz, self.z1, self.rz, self.hrz, self.th, self.ws3, self.lmbda = (DVec(ml) for _ in range(10))
        self.out4 = (ctypes.c_double * 4)()              # dtau, z1'z1, max_step(ds), max_step(dz) of the last direction

    def reduce(self):
        e = self
        return reduce_multi([("dot", e.hrx, e.hrx), ("dot", e.rx, e.rx), ("dot", e.hry, e.hry), ("dot", e.ry, e.ry), ("dot", e.hrz, e.hrz),
                             ("dot", e.rz, e.rz), ("dot", e.cv, e.x), ("dot", e.bv, e.y), ("dot", e.hv, e.z), ("dot", e.lmbda, e.lmbda)])

    def scaling(self):
        raise_for(lib().kvx_nt_compute_scaling_dev(self.ml, self.s.ptr, self.z.ptr, self.d.ptr, self.di.ptr, self.lmbda.ptr))
        return self.lmbda.dot(self.lmbda)

    def scale(self, primal, dual):
        if primal is not None:
            self.x.scal(primal); self.s.scal(primal)
        if dual is not None:
            self.y.scal(dual); self.z.scal(dual)

    def begin(self, i, sigma, mu, rt, dg, dgi, lmbda_g, wkappa3):
        """The tau and kappa entries of the right-hand side of direction i (coneprog.py:1250-1298), the same after the first half of
        f6_no_ir (:1130-1160), and the scalars its launches take."""
        self.sigma, self.smu, self.dgi, self.lmbda_g = sigma, (sigma * mu if i == 1 else 0.0), dgi, lmbda_g
        self.rtau = (1.0 - sigma) * rt
        self.rkappa = lmbda_g ** 2
        if i == 1:
            self.rkappa += wkappa3 - sigma * mu
        self.dkappa = -self.rkappa / lmbda_g
        self.dtau0 = self.rtau + self.dkappa / dgi

    def newton_rhs(self, i, lmbdasq):
        """ds := -(lmbdasq (+ ws3 - sigma mu)) o\\ lmbda,  dz := -((1 - sigma) rz + W' ds): one kernel; lmbdasq None: formed inside."""
        raise_for(lib().kvx_lp_newton_rhs_dev(self.ml, lmbdasq, self.ws3.ptr if i == 1 else None, self.smu, 1.0 - self.sigma,
                                              self.rz.ptr, self.lmbda.ptr, self.d.ptr, self.ds.ptr, self.dz.ptr))

    def second_half(self, i):
        """Second half of f6_no_ir (coneprog.py:1162-1195), dz += dtau z1, ds -= dz, [ws3 := ds o dz (:1303-1306)], the scaling by lmbda and
        the step bounds (:1314-1321): dtau is formed on the device from the inner products, ONE host round trip per direction."""
        e, p = self, self.p
        raise_for(lib().kvx_lp_second_half_dev(e.ml, e.n, p, e.cv.ptr, e.bv.ptr if p else None, e.th.ptr, e.x1.ptr, e.y1.ptr if p else None,
                                               e.z1.ptr, e.lmbda.ptr, e.dx.ptr, e.dy.ptr if p else None, e.dz.ptr, e.ds.ptr,
                                               e.ws3.ptr if i == 0 else None, e.dgi, e.dtau0, -1.0 if i == 0 else e.out4[1], e.out4))

    def bounds(self, i):
        dtau, _, ts, tz = self.out4                      # (z1'z1 comes with the first direction and is handed to the second)
        return dtau, self.dkappa - dtau, ts, tz


class _CIssued(_Engine):
    """p = 0, the default: the fused launches of an iteration issued from C in four calls (kvx_lp_iter_*) -- a direction up to its
    scalars is ONE call: what newton_rhs, factor_solve_sides / solve_sides, th.xmy and second_half enqueue in _PythonIssued, in that order."""

    def __init__(self, kkt, pb):
        super().__init__(kkt, pb)
        e, G = self, self.G
        self.ctx = _lib.LpCtx(e.ml, e.n, G.cp.ptr, G.ri.ptr, G.vx.ptr, G.max_col, G.tcp.ptr, G.tri.ptr, G.tvx.ptr, G.max_row,
                              kkt._plan, kkt.fac._h, kkt.Sx.ptr, kkt._x2buf().ptr, e.x.ptr, e.s.ptr, e.z.ptr, e.cv.ptr, e.hv.ptr, e.hrx.ptr,
                              e.rx.ptr, e.hrz.ptr, e.rz.ptr, e.lmbda.ptr, e.d.ptr, e.di.ptr, e.ds.ptr, e.dz.ptr, e.dx.ptr, e.x1.ptr, e.z1.ptr,
                              e.th.ptr, e.ws3.ptr)
        self.out10 = (ctypes.c_double * 10)()
        self.fresh = False                               # out10 holds the statistics of the coming iteration

    def stats(self, tau):
        if not self.fresh:
            raise_for(lib().kvx_lp_iter_residuals(ctypes.byref(self.ctx), tau, self.out10))
        self.fresh = False
        return tuple(self.out10)

    def direction(self, i, *scalars):
        self.begin(i, *scalars)
        if i == 0:
            self.kkt.di = self.di
            self.kkt.nfactor += 1
            raise_for(lib().kvx_lp_iter_predictor(ctypes.byref(self.ctx), self.dgi, self.dtau0, self.out4))
        else:
            self.kkt.check()                             # the stream is idle by now: no extra wait
            raise_for(lib().kvx_lp_iter_corrector(ctypes.byref(self.ctx), self.smu, 1.0 - self.sigma, self.dgi, self.dtau0, self.out4[1], self.out4))

    def update(self, step, tau):
        # the update, the residuals of the next iteration (with the new tau) and their reductions in ONE call
        raise_for(lib().kvx_lp_iter_update(ctypes.byref(self.ctx), step, tau, self.out10))
        self.fresh = True


class _PythonIssued(_Engine):
    """p = 0, KVX_LP_PYCALLS=1: the same fused launches, one ctypes call each."""

    def stats(self, tau):
        e, G = self, self.G
        raise_for(lib().kvx_lp_residuals_dev(e.ml, e.n, G.cp.ptr, G.ri.ptr, G.vx.ptr, G.max_col, G.tcp.ptr, G.tri.ptr, G.tvx.ptr, G.max_row,
                                             e.x.ptr, e.z.ptr, e.s.ptr, e.cv.ptr, e.hv.ptr, tau, e.hrx.ptr, e.rx.ptr, e.hrz.ptr, e.rz.ptr))
        return self.reduce()

    def direction(self, i, *scalars):
        e = self
        e.begin(i, *scalars)
        if i == 1:
            return e.kkt.check()                         # the stream is idle by now: no extra wait
        e.kkt.async_solves = True                        # enqueue only: the host runs ahead of the GPU up to the next scalar
        e.newton_rhs(0, None)
        # factorisation and both solves in one enqueue; x1 := -c, z1 := h, their scaling by dgi and dx := (1 - sigma) rx inside its launches
        e.kkt.factor_solve_sides(e.di, [(e.cv, -1.0, e.hv, e.x1, e.dgi, e.z1, e.dgi), (e.rx, 1.0 - e.sigma, e.dz, e.dx, 1.0, e.dz, 1.0)])
        e.th.xmy(1.0, e.hv, e.di)

    def bounds(self, i):
        e = self
        if i == 1:
            e.newton_rhs(1, None)
            e.kkt.solve_sides([(e.rx, 1.0 - e.sigma, e.dz, e.dx, 1.0, e.dz, 1.0)])
        e.second_half(i)
        return super().bounds(i)

    def update(self, step, tau):
        e = self
        raise_for(lib().kvx_lp_update_x_dev(e.ml, e.n, step, e.ds.ptr, e.dz.ptr, e.d.ptr, e.di.ptr, e.lmbda.ptr, e.s.ptr, e.z.ptr, e.dx.ptr, e.x.ptr))


class _PerOperation(_Engine):
    """KVX_LP_UNFUSED=1, equality constraints or a user's kktsolver: one launch per operation."""

    def stats(self, tau):
        e = self
        e.Af(e.y, e.hrx, trans="T", alpha=-1.0, beta=0.0)
        e.G.gemv(e.z, e.hrx, trans="T", alpha=-1.0, beta=1.0)
        e.rx.lincomb(1.0, e.hrx, -tau, e.cv)
        e.Af(e.x, e.hry, trans="N")
        e.ry.lincomb(1.0, e.hry, -tau, e.bv)
        e.G.gemv(e.x, e.hrz, trans="N"); e.hrz.axpy(e.s)
        e.rz.lincomb(1.0, e.hrz, -tau, e.hv)
        return e.reduce()

    def scaling(self):
        lam2 = super().scaling()
        self.lmbdasq = DVec(self.ml).sqr_of(self.lmbda)  # lmbda o lmbda, renewed with lmbda
        return lam2

    def rhs(self, i):
        self.newton_rhs(i, self.lmbdasq.ptr)
        self.dx.lincomb(1.0 - self.sigma, self.rx)
        self.dy.lincomb(-(1.0 - self.sigma), self.ry)

    def direction(self, i, *scalars):
        e, kkt = self, self.kkt
        e.begin(i, *scalars)
        if i == 1:
            return kkt.check()                           # the stream is idle by now: no extra wait
        # factor + the two solves that do not depend on each other (coneprog.py:1066-1077 and the predictor's f3)
        kkt.async_solves = True                          # enqueue only: the host runs ahead of the GPU up to the next scalar
        if not e.xz:
            kkt.factor(e.di, sync=False)                 # a failed factorisation surfaces in the solve right below
        e.x1.lincomb(-1.0, e.cv); e.y1.copy_from(e.bv); e.z1.copy_from(e.hv)
        e.rhs(0)
        if e.xz:                                         # with the factorisation in one enqueue: the right-hand sides do not depend on it
            kkt.factor_solve2(e.di, e.x1, e.z1, e.dx, e.dz)
        elif isinstance(kkt, KKTUserHost):
            kkt.solve(e.x1, e.y1, e.z1)
            kkt.solve(e.dx, e.dy, e.dz)
        else:                                            # one two-column triangular solve with the new factor
            kkt.solve2(e.x1, e.y1, e.z1, e.dx, e.dy, e.dz)
        e.x1.scal(e.dgi); e.y1.scal(e.dgi); e.z1.scal(e.dgi)
        e.th.copy_from(e.hv).mul(e.di)                   # th = W^{-T} h      (coneprog.py:1126-1128)

    def bounds(self, i):
        if i == 1:
            self.rhs(1)
            self.ksolve(self.dx, self.dy, self.dz)
        self.second_half(i)
        return super().bounds(i)

    def update(self, step, tau):
        e = self
        e.x.axpy(e.dx, step)
        e.y.axpy(e.dy, step)
        raise_for(lib().kvx_lp_update_dev(e.ml, step, e.ds.ptr, e.dz.ptr, e.d.ptr, e.di.ptr, e.lmbda.ptr, e.s.ptr, e.z.ptr))
        e.lmbdasq.sqr_of(e.lmbda)


class _Refined(_PerOperation):
    """options['refinement'] > 0: the Newton systems with iterative refinement (coneprog.py:599-631 res(), :1110-1195 f6_no_ir,
    :1211-1235 f6), operation by operation; the scalars (tau, kappa blocks) travel in one-element lists.  For the orthant cone
    W = diag(d): scale(., W, inverse='I') multiplies by di, scale(., W, trans='T') by d."""

    def __init__(self, kkt, pb, nref):
        super().__init__(kkt, pb)
        self.rs3, self.rz3 = DVec(self.ml), DVec(self.ml)
        w, w2 = ((DVec(self.n), DVec(self.p) if self.p else self.y, DVec(self.ml), DVec(self.ml)) for _ in range(2))
        self.f6 = _ipm.f6(self.f6_no_ir, self.res, nref, w, w2)

    def f6_no_ir(self, bx, by, bz, btau, bs, bkappa):
        e = self
        by.scal(-1.0)
        bs.div(e.lmbda).scal(-1.0)                       # s := -lmbda o\ bs
        e.rs3.copy_from(bs).mul(e.d)
        bz.axpy(e.rs3).scal(-1.0)                        # z := -(bz + W' s)
        e.ksolve(bx, by, bz)
        bkappa[0] = -bkappa[0] / e.lmbda_g
        btau[0] += bkappa[0] / e.dgi
        btau[0] = e.dgi * (btau[0] + e.cv.dot(bx) + e.bv.dot(by) + e.th.dot(bz)) / (1.0 + e.z1.dot(e.z1))
        bx.axpy(e.x1, btau[0]); by.axpy(e.y1, btau[0]); bz.axpy(e.z1, btau[0])
        bs.axpy(bz, -1.0)
        bkappa[0] -= btau[0]

    def res(self, ux, uy, uz, utau, us, ukappa, vx, vy, vz, vtau, vs, vkappa):
        e, dg = self, 1.0 / self.dgi                     # (not the loop's dg: the rounding this engine has always had)
        e.Af(uy, vx, trans="T", alpha=-1.0, beta=1.0)
        e.rz3.copy_from(uz).mul(e.di)                    # W^{-1} uz
        e.G.gemv(e.rz3, vx, trans="T", alpha=-1.0, beta=1.0)
        vx.axpy(e.cv, -utau[0] / dg)
        e.Af(ux, vy, trans="N", alpha=1.0, beta=1.0)
        vy.axpy(e.bv, -utau[0] / dg)
        e.G.gemv(ux, vz, trans="N", alpha=1.0, beta=1.0)
        vz.axpy(e.hv, -utau[0] / dg)
        e.rs3.copy_from(us).mul(e.d)
        vz.axpy(e.rs3)
        vtau[0] += dg * ukappa[0] + e.cv.dot(ux) + e.bv.dot(uy) + e.hv.dot(e.rz3)
        e.rs3.copy_from(us).axpy(uz).mul(e.lmbda)
        vs.axpy(e.rs3)
        vkappa[0] += e.lmbda_g * (utau[0] + ukappa[0])

    def direction(self, i, *scalars):
        e = self
        e.begin(i, *scalars)
        if i == 0:
            e.kkt.async_solves = True
            e.kkt.factor(e.di, sync=False)               # (the directions are solved one by one inside f6)
            e.x1.lincomb(-1.0, e.cv); e.y1.copy_from(e.bv); e.z1.copy_from(e.hv)
            e.ksolve(e.x1, e.y1, e.z1)
            e.x1.scal(e.dgi); e.y1.scal(e.dgi); e.z1.scal(e.dgi)
            e.th.copy_from(e.hv).mul(e.di)
            e.kkt.check()                                # (a failed factorisation must not be refined)

    def bounds(self, i):
        e = self                                         # right-hand side as the reference sets it up (coneprog.py:1250-1333)
        e.ds.copy_from(e.lmbdasq)
        if i == 1:
            e.ds.axpy(e.ws3).addc(-e.smu)
        e.dx.lincomb(1.0 - e.sigma, e.rx); e.dy.lincomb(1.0 - e.sigma, e.ry); e.dz.lincomb(1.0 - e.sigma, e.rz)
        dtau, dkappa = [e.rtau], [e.rkappa]
        e.f6(e.dx, e.dy, e.dz, dtau, e.ds, dkappa)
        if i == 0:
            e.ws3.copy_from(e.ds).mul(e.dz)
        e.ds.div(e.lmbda); e.dz.div(e.lmbda)             # misc.scale2(lmbda, .) on the orthant
        return dtau[0], dkappa[0], e.ds.max_step(), e.dz.max_step()


def conelp(c, G, h, dims=None, A=None, b=None, options=None, chol_opts=None, primalstart=None, dualstart=None, kktsolver=None):
    """Solve the LP  minimize c'x  s.t.  Gx <= h, Ax = b  on the GPU.  c: (n,), h: (ml,), G: spmatrix-like
    (ml x n, sparse); A (p x n, sparse), b (p,) optional -- with equality constraints either G has at most one entry per
    row (standard form: KKTDiagEqDev, sparse K on a fixed pattern) or any other sparse G (KKTGenEqDev, dense K in HBM).  primalstart = {'x', 's'},
    dualstart = {'y', 'z'} (y optional) as in the reference (coneprog.py:683-737): s and z must be strictly positive.  Returns the reference's result dictionary (coneprog.py:962-974) with numpy arrays."""
    opt = _ipm.options(options, {})
    pb = _ipm.problem(c, G, h, None, A, b)
    n, p, ml = pb.n, pb.p, pb.cdim
    (Gp, Gi, Gx), (Ap, Ai, Ax) = pb.G, pb.A
    if dims is not None and (dims.get("q") or dims.get("s") or dims.get("l", ml) != ml):
        raise NotImplementedError("only the orthant cone dims = {'l': G.size[0], 'q': [], 's': []} runs on the GPU")
    _lib.require_device()

    if kktsolver is not None:
        # the reference's plug-in point (coneprog.py:323-344): kktsolver(W) returns f(x, y, z); host round trips per call
        if not callable(kktsolver):
            raise ValueError("kktsolver must be a function W -> f(x, y, z) (the reference's named solvers 'ldl', 'ldl2', 'qr', "
                             "'chol', 'chol2' are not part of this path: 'chol2' is what runs on the GPU by default)")
        kkt = KKTUserHost(ml, n, Gp, Gi, Gx, p, Ap, Ai, Ax, kktsolver)
    elif p > 0:
        Gi64 = np.asarray(Gi, dtype=np.int64)
        diag_s = not (Gi64.size and np.bincount(Gi64, minlength=ml).max() > 1)
        cls = KKTDiagEqDev if diag_s else KKTGenEqDev
        kkt = _kkt_for(cls.__name__, (ml, n, p), (Gp, Gi, Ap, Ai), chol_opts,
                       lambda: cls(ml, n, Gp, Gi, Gx, p, Ap, Ai, Ax, chol_opts), lambda k: k.reset(Gx, Ax))
    else:
        kkt = _kkt_for("KKTChol2Dev", (ml, n, 0), (Gp, Gi), chol_opts,
                       lambda: KKTChol2Dev(ml, n, Gp, Gi, Gx, chol_opts), lambda k: k.reset(Gx))
    if opt.refinement:
        engine = _Refined(kkt, pb, opt.refinement)
    elif _UNFUSED or not isinstance(kkt, KKTChol2Dev):
        engine = _PerOperation(kkt, pb)
    else:                                                # p = 0: the short launches of an iteration fused (kkt.hip, "round 3")
        engine = (_PythonIssued if _PYCALLS else _CIssued)(kkt, pb)
    res0 = (max(1.0, engine.cv.nrm2()), max(1.0, engine.bv.nrm2()), max(1.0, engine.hv.nrm2()))

    out, t_loop = _ipm.conelp_start(engine, opt, primalstart, dualstart, res0), time.perf_counter()
    looped = not isinstance(out, _ipm.Outcome)
    if looped:
        out = _ipm.conelp_loop(engine, opt, ml, out, res0)
    e, xs, zs = engine, out.status != "primal infeasible", out.status != "dual infeasible"      # a certificate comes without the other half
    return _ipm.conelp_result(
        opt.show, out.status, e.x.get() if xs else None, e.y.get() if zs else None, e.s.get() if xs else None, e.z.get() if zs else None,
        out.stats, e.s.max_step() if xs else None, e.z.max_step() if zs else None, out.iterations, kkt.nfactor, out.msg, **{
            # wall time of the loop proper (coneprog.py:859-1436): no symbolic analysis, no starting point; not a key of the reference's
            "loop seconds": (time.perf_counter() - t_loop) if looped else 0.0,
            # the same, split at the three host synchronisations of an iteration: [-> first direction, -> second, -> next residual norms]
            "phase seconds": list(out.phase_seconds)})


class _QpEngine(_Orthant):
    """The device vectors and launches of one coneqp run (the protocol of _ipm.coneqp_loop), for p = 0 and p > 0 and any of
    KKTChol2Dev, KKTGenEqDev and KKTUserHost; to be read top to bottom as the launch order of an iteration."""

    def __init__(self, kkt, pb, nref):
        super().__init__(kkt, pb)
        ml, n, p = pb.cdim, pb.n, pb.p
        self.P = SymSpMatDev(n, *pb.P)
        self.qv, self.hv = DVec(n, pb.c), DVec(ml, pb.h)
        self.bv = DVec(p, pb.b) if p else _ipm.NoVec()   # p = 0: the y-blocks of the algorithm are empty
        self.y, self.dy, self.ry = (DVec(p) for _ in range(3)) if p else [self.bv] * 3
        self.x, self.dx, self.rx, self.tmpx = (DVec(n) for _ in range(4))
        self.s, self.z, self.ds, self.dz, self.rz, self.ws3, self.tmp, self.lmbda, self.lmbdasq = (DVec(ml) for _ in range(9))
        w, w2 = ((DVec(n), DVec(p) if p else self.y, DVec(ml), DVec(ml)) for _ in range(2)) if nref else ((), ())
        self.f4 = _ipm.f4(self.f4_no_ir, self.res, nref, w, w2)

    def start_solve(self, x, y, z):
        self.ksolve(x, y, z)
        if self.p:
            self.kkt.check()

    def f4_no_ir(self, bx, by, bz, bs):
        # [P A' G'; A 0 0; G 0 -W'W][ux; uy; W^-1 uz] = [bx; by; bz - W'(lmbda o\ bs)],  us = lmbda o\ bs - uz   (coneprog.py:2283-2313)
        bs.div(self.lmbda)
        self.tmp.xmy(1.0, bs, self.d)
        bz.axpy(self.tmp, -1.0)
        self.ksolve(bx, by, bz)
        bs.axpy(bz, -1.0)

    def res(self, ux, uy, uz, us, vx, vy, vz, vs):
        # residual of the Newton equations (coneprog.py:1929-1960)
        e, tmp = self, self.tmp
        e.P.symv(ux, vx, alpha=-1.0, beta=1.0)
        e.Af(uy, vx, trans="T", alpha=-1.0, beta=1.0)
        e.Af(ux, vy, trans="N", alpha=-1.0, beta=1.0)
        tmp.xmy(1.0, uz, e.di)
        e.G.gemv(tmp, vx, trans="T", alpha=-1.0, beta=1.0)
        e.G.gemv(ux, vz, trans="N", alpha=-1.0, beta=1.0)
        tmp.xmy(1.0, us, e.d)
        vz.axpy(tmp, -1.0)
        tmp.lincomb(1.0, us, 1.0, uz)
        tmp.mul(e.lmbda)
        vs.axpy(tmp, -1.0)

    def stats(self):
        # rx = P x + q + A'y + G'z, ry = A x - b, rz = s + G x - h; ONE reduction call for the seven inner products
        e, x, y, z, rx, ry, rz = self, self.x, self.y, self.z, self.rx, self.ry, self.rz
        rx.copy_from(e.qv)
        e.P.symv(x, rx, alpha=1.0, beta=1.0)
        e.tmpx.copy_from(rx)                             # P x + q, for f0
        e.Af(y, rx, trans="T", alpha=1.0, beta=1.0)
        ry.copy_from(e.bv)
        e.Af(x, ry, trans="N", alpha=1.0, beta=-1.0)
        e.G.gemv(z, rx, trans="T", alpha=1.0, beta=1.0)
        rz.lincomb(1.0, e.s, -1.0, e.hv)
        e.G.gemv(x, rz, trans="N", alpha=1.0, beta=1.0)
        xPq, xq, v_rx, v_rz, zrz, v_ry, yry = reduce_multi([("dot", x, e.tmpx), ("dot", x, e.qv), ("dot", rx, rx), ("dot", rz, rz),
                                                             ("dot", z, rz), ("dot", ry, ry), ("dot", y, ry)])
        return xPq, xq, v_rx, v_ry, v_rz, yry, zrz

    def scaling(self):
        raise_for(lib().kvx_nt_compute_scaling_dev(self.ml, self.s.ptr, self.z.ptr, self.d.ptr, self.di.ptr, self.lmbda.ptr))

    def factor(self):
        self.lmbdasq.sqr_of(self.lmbda)
        self.kkt.factor(self.di)
        if self.p:
            self.kkt.check()

    def direction(self, i, sigma_mu, eta, correction):
        e, ds, dz = self, self.ds, self.dz               # right-hand sides (coneprog.py:2367-2390)
        ds.fill(0.0)
        if correction and i == 1:
            ds.axpy(e.ws3, -1.0)
        ds.axpy(e.lmbdasq, -1.0).addc(sigma_mu)
        e.dx.lincomb(-1.0 + eta, e.rx)
        e.dy.lincomb(-1.0 + eta, e.ry)
        dz.lincomb(-1.0 + eta, e.rz)
        e.f4(e.dx, e.dy, dz, ds)
        dsdz = ds.dot(dz)
        if correction and i == 0:
            e.ws3.xmy(1.0, ds, dz)
        ds.div(e.lmbda); dz.div(e.lmbda)                 # misc.scale2(lmbda, .) on the orthant (coneprog.py:2431-2451)
        return (dsdz,) + tuple(reduce_multi([("max", ds), ("max", dz)]))

    def update(self, step):
        e, ds, dz = self, self.ds, self.dz               # iterates and scaling (coneprog.py:2454-2545)
        e.x.axpy(e.dx, step)
        e.y.axpy(e.dy, step)
        ds.scal(step).addc(1.0); dz.scal(step).addc(1.0)
        ds.mul(e.lmbda); dz.mul(e.lmbda)
        raise_for(lib().kvx_nt_update_scaling_dev(e.ml, ds.ptr, dz.ptr, e.d.ptr, e.di.ptr, e.lmbda.ptr))
        e.s.xmy(1.0, e.lmbda, e.d)
        e.z.xmy(1.0, e.lmbda, e.di)
        return e.lmbda.dot(e.lmbda)


def coneqp(P, q, G, h, options=None, chol_opts=None, A=None, b=None, initvals=None, kktsolver=None):
    """Solve the convex QP  minimize (1/2) x'Px + q'x  s.t.  Gx <= h, Ax = b  on the GPU (orthant cone): the reference's coneqp (coneprog.py:1440-2547) with its default KKT solver for sparse G,
    misc.kkt_chol2 with H = P.  P: spmatrix-like, its lower triangle is used.  Returns the reference's result
    dictionary (coneprog.py:2216-2221) with numpy arrays, plus "factorizations"."""
    opt = _ipm.options(options, {}, qp=True)                                    # coneprog.py:1768-1781, 1862-1865
    pb = _ipm.problem(q, G, h, None, A, b, P, qp=True)
    n, p, ml = pb.n, pb.p, pb.cdim
    (Gp, Gi, Gx), (Ap, Ai, Ax), (Pp, Pi, Px) = pb.G, pb.A, pb.P
    if ml == 0:
        raise ValueError("coneqp on the GPU needs at least one inequality (dims['l'] > 0)")
    _lib.require_device()
    if kktsolver is not None:
        # the reference's plug-in point (coneprog.py:1969-1981): kktsolver(W) returns f(x, y, z) for the system with H = P; host
        # round trips per factorisation and solve (KKTUserHost, as under conelp)
        if not callable(kktsolver):
            raise ValueError("kktsolver must be a function W -> f(x, y, z) (the reference's named solvers are not part of this path: "
                             "'chol2' is what runs on the GPU by default)")
        kkt = KKTUserHost(ml, n, Gp, Gi, Gx, p, Ap, Ai, Ax, kktsolver)
    elif p > 0:
        kkt = _kkt_for("KKTGenEqDev+P", (ml, n, p), (Gp, Gi, Ap, Ai, Pp, Pi), chol_opts,
                       lambda: KKTGenEqDev(ml, n, Gp, Gi, Gx, p, Ap, Ai, Ax, chol_opts, Pp, Pi, Px), lambda k: k.reset(Gx, Ax, Px))
    else:
        kkt = _kkt_for("KKTChol2Dev+P", (ml, n, 0), (Gp, Gi, Pp, Pi), chol_opts,
                       lambda: KKTChol2Dev(ml, n, Gp, Gi, Gx, chol_opts, Pp, Pi, Px), lambda k: k.reset(Gx, Px))
    e = _QpEngine(kkt, pb, opt.refinement)
    res0 = (max(1.0, e.qv.nrm2()), max(1.0, e.bv.nrm2()), max(1.0, e.hv.nrm2()))
    out = _ipm.coneqp_loop(e, opt, ml, _ipm.coneqp_start(e, initvals, "initvals"), res0)
    return _ipm.coneqp_result(opt.show, out.status, e.x.get(), e.y.get(), e.s.get(), e.z.get(), out.stats, e.s.max_step(), e.z.max_step(),
                              out.iterations, kkt.nfactor, out.msg)
