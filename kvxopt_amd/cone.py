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

from . import _lib, base
from ._lib import DeviceBuffer, lib, raise_for
from .chol import Factor
from .lp import DVec, SpMatDev, SymSpMatDev, _lower_ccs, dense_schur

EXPON = 3          # coneprog.py:423
STEP = 0.99        # coneprog.py:424


def _i64dev(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    return DeviceBuffer.from_array(a) if a.size else DeviceBuffer(8)


class Dims:
    """Offsets of the blocks of a cone vector and the device tables of the kvx_ntq_* / kvx_nts_* entries."""

    def __init__(self, dims):
        self.ml = int(dims["l"])
        self.q = [int(k) for k in dims["q"]]
        self.s = [int(k) for k in dims["s"]]
        self.nq, self.ns = len(self.q), len(self.s)
        self.mq = sum(self.q)
        self.ind = self.ml + self.mq                                   # start of the 's' section
        self.tot2 = sum(m * m for m in self.s)
        self.tot1 = sum(self.s)
        self.N = self.ind + self.tot2                                  # cdim
        self.Nd = self.ind + self.tot1                                 # cdim_diag
        self.Np = self.ind + sum(m * (m + 1) // 2 for m in self.s)     # cdim_pckd
        qoff = np.zeros(self.nq + 1, dtype=np.int64)
        np.cumsum(np.asarray(self.q, dtype=np.int64), out=qoff[1:])
        self.qoff = qoff
        self.d_qoff = _i64dev(qoff)
        sd = np.asarray(self.s, dtype=np.int64)
        self.off2 = np.zeros(self.ns + 1, dtype=np.int64)
        self.off1 = np.zeros(self.ns + 1, dtype=np.int64)
        np.cumsum(sd * sd, out=self.off2[1:])
        np.cumsum(sd, out=self.off1[1:])
        self.d_off2, self.d_off1 = _i64dev(self.off2), _i64dev(self.off1)
        # identity e: 1 on the 'l' entries, the heads of the 'q' cones and the diagonals of the 's' blocks
        e = np.zeros(self.N)
        e[:self.ml] = 1.0
        e[self.ml + qoff[:-1]] = 1.0
        self.sdiag = np.concatenate([self.off2[k] + np.arange(m) * (m + 1) for k, m in enumerate(self.s)]).astype(np.int64) \
            if self.tot1 else np.zeros(0, dtype=np.int64)
        e[self.ind + self.sdiag] = 1.0
        self.e = DVec(self.N, e)
        self.d_sdiag = _i64dev(self.sdiag)
        self.work = DVec(max(4 * self.tot2, 3 * self.tot2 + 2 * self.tot1, 1))
        self.out = DVec(max(self.ns, self.nq, 1))

    def key(self):
        return (self.ml, tuple(self.q), tuple(self.s))


class WDev:
    """The Nesterov-Todd scaling W in HBM: d, di ('l'), v (the 'q' vectors back to back), beta (nq), r, rti (the 's' blocks)."""

    def __init__(self, D):
        self.D = D
        self.d, self.di = DVec(D.ml), DVec(D.ml)
        self.v, self.beta = DVec(D.mq), DVec(D.nq)
        self.r, self.rti = DVec(D.tot2), DVec(D.tot2)

    def identity(self):
        """W = I (coneprog.py:662-672)."""
        D = self.D
        self.d.fill(1.0); self.di.fill(1.0)
        v = np.zeros(D.mq)
        v[D.qoff[:-1]] = 1.0
        self.v.set(v); self.beta.fill(1.0)
        r = np.zeros(D.tot2)
        r[D.sdiag] = 1.0
        self.r.set(r); self.rti.set(r)

    def set_host(self, W):
        """From the reference's dictionary W (host matrices)."""
        D = self.D
        cat = lambda xs: np.concatenate([np.asarray(base._dense_buffer(x)[0], dtype=np.float64) for x in xs]) if xs else np.zeros(0)
        if D.ml:
            self.d.set(base._dense_buffer(W["d"])[0]); self.di.set(base._dense_buffer(W["di"])[0])
        if D.nq:
            self.v.set(cat(W["v"])); self.beta.set(np.asarray(W["beta"], dtype=np.float64))
        if D.tot2:
            self.r.set(cat(W["r"])); self.rti.set(cat(W["rti"]))


# ---- the operations of misc on device vectors (pointer + the layout of Dims) -------------------------------------------------
def scale(D, W, xp, trans="N", inverse="N"):
    """misc.scale (misc_solvers.c:85-240) of one vector at xp."""
    inv = inverse != "N"
    if D.ml:
        raise_for(lib().kvx_nt_scale_dev(D.ml, 1, D.N, xp, (W.di if inv else W.d).ptr))
    if D.nq:
        raise_for(lib().kvx_ntq_scale_dev(D.nq, D.d_qoff.ptr, W.v.ptr, W.beta.ptr, xp + 8 * D.ml, D.N, 1, 1 if inv else 0))
    if D.tot2:
        R = W.rti if inv else W.r
        form = 1 if (inverse == "N") == (trans == "T") else 0
        raise_for(lib().kvx_nts_scale_dev(D.ns, D.d_off2.ptr, D.d_off1.ptr, R.ptr, xp + 8 * D.ind, D.N, 1, form, D.work.ptr, D.tot2))


def scale2(D, lp_, xp, inverse="N"):
    """misc.scale2 (misc_solvers.c:256-397); lp_: lmbda (cdim_diag layout)."""
    inv = 1 if inverse == "I" else 0
    if D.ml:
        raise_for(lib().kvx_nt_scale2_dev(D.ml, lp_, xp, inv))
    if D.nq:
        raise_for(lib().kvx_ntq_scale2_dev(D.nq, D.d_qoff.ptr, lp_ + 8 * D.ml, xp + 8 * D.ml, inv))
    if D.tot2:
        raise_for(lib().kvx_nts_scale2_dev(D.ns, D.d_off2.ptr, D.d_off1.ptr, lp_ + 8 * D.ind, xp + 8 * D.ind, inv))


def sprod(D, xp, yp, diag="N"):
    """misc.sprod (misc_solvers.c:634-770): x := y o x; diag 'D': the 's' part of y holds diagonals only."""
    if D.ml:
        raise_for(lib().kvx_nt_sprod_dev(D.ml, xp, yp))
    if D.nq:
        raise_for(lib().kvx_ntq_prod_dev(D.nq, D.d_qoff.ptr, xp + 8 * D.ml, yp + 8 * D.ml, 0))
    if D.tot2:
        if diag == "N":
            raise_for(lib().kvx_nts_prod_dev(D.ns, D.d_off2.ptr, D.d_off1.ptr, xp + 8 * D.ind, yp + 8 * D.ind, 0, D.work.ptr))
        else:
            raise_for(lib().kvx_nts_prod_dev(D.ns, D.d_off2.ptr, D.d_off1.ptr, xp + 8 * D.ind, yp + 8 * D.ind, 1, None))


def sinv(D, xp, yp):
    """misc.sinv (misc_solvers.c:775-882), y in the cdim_diag layout."""
    if D.ml:
        raise_for(lib().kvx_nt_sinv_dev(D.ml, xp, yp))
    if D.nq:
        raise_for(lib().kvx_ntq_prod_dev(D.nq, D.d_qoff.ptr, xp + 8 * D.ml, yp + 8 * D.ml, 1))
    if D.tot2:
        raise_for(lib().kvx_nts_prod_dev(D.ns, D.d_off2.ptr, D.d_off1.ptr, xp + 8 * D.ind, yp + 8 * D.ind, 2, None))


def ssqr(D, xp, yp):
    """misc.ssqr (misc.py:945-959), both in the cdim_diag layout."""
    if D.ml:
        raise_for(lib().kvx_nt_ssqr_dev(D.ml, xp, yp))
    if D.nq:
        raise_for(lib().kvx_ntq_prod_dev(D.nq, D.d_qoff.ptr, xp + 8 * D.ml, yp + 8 * D.ml, 2))
    if D.tot1:
        raise_for(lib().kvx_nt_ssqr_dev(D.tot1, xp + 8 * D.ind, yp + 8 * D.ind))


def sdot(D, xp, yp):
    """misc.sdot (misc_solvers.c:991-1046)."""
    a = 0.0
    if D.ind:
        r = ctypes.c_double()
        raise_for(lib().kvx_nt_sdot_dev(D.ind, xp, yp, ctypes.byref(r)))
        a = r.value
    if D.tot2:
        raise_for(lib().kvx_nts_dot_dev(D.ns, D.d_off2.ptr, D.d_off1.ptr, xp + 8 * D.ind, yp + 8 * D.ind, D.out.ptr))
        for v in D.out.get()[:D.ns]:
            a += float(v)
    return a


def snrm2(D, xp):
    return math.sqrt(sdot(D, xp, xp))


def max_step(D, xp, sigma=None):
    """misc.max_step (misc_solvers.c:1052-1160); with sigma (a DVec of sum(dims['s'])) the eigenvalues of the 's' blocks are
    stored there and their eigenvectors replace the blocks of x."""
    if D.ind + D.tot2 == 0:
        return 0.0
    t = -np.finfo(np.float32).max
    if D.ml:
        r = ctypes.c_double()
        raise_for(lib().kvx_nt_max_step_dev(D.ml, xp, ctypes.byref(r)))
        t = max(t, r.value)
    if D.nq:
        raise_for(lib().kvx_ntq_max_step_dev(D.nq, D.d_qoff.ptr, xp + 8 * D.ml, D.out.ptr))
        t = max(t, float(D.out.get()[:D.nq].max()))
    if D.tot2:
        raise_for(lib().kvx_nts_max_step_dev(D.ns, D.d_off2.ptr, D.d_off1.ptr, xp + 8 * D.ind, sigma.ptr if sigma is not None else None,
                                             D.out.ptr, D.work.ptr))
        t = max(t, float(D.out.get()[:D.ns].max()))
    return t


def tri(D, xp, mode):
    """mode 0: misc.symm of every 's' block, 1: trisc, 2: triusc (misc_solvers.c:610-632, 887-988)."""
    if D.tot2:
        raise_for(lib().kvx_nts_tri_dev(D.ns, D.d_off2.ptr, D.d_off1.ptr, xp + 8 * D.ind, mode))


def put_diag(D, dst, srcp):
    """dst := src ('l' and 'q' entries), 's' blocks := diag(src_k) (coneprog.py:1273-1280, 1413-1421)."""
    if D.ind:
        raise_for(lib().kvx_vec_copy_dev(D.ind, srcp, dst.ptr))
    if D.tot2:
        raise_for(lib().kvx_vec_fill_dev(D.tot2, 0.0, dst.ptr + 8 * D.ind))
        raise_for(lib().kvx_vec_scatter_dev(D.tot1, srcp + 8 * D.ind, D.d_sdiag.ptr, dst.ptr + 8 * D.ind))


def compute_scaling(D, s, z, W, lmbda):
    """misc.compute_scaling (misc.py:250-419): W and lmbda from the interior points s, z."""
    ind = D.ind
    if D.ml:
        raise_for(lib().kvx_nt_compute_scaling_dev(D.ml, s.ptr, z.ptr, W.d.ptr, W.di.ptr, lmbda.ptr))
    if D.nq:
        raise_for(lib().kvx_ntq_compute_scaling_dev(D.nq, D.d_qoff.ptr, s.ptr + 8 * D.ml, z.ptr + 8 * D.ml, W.v.ptr,
                                                    W.beta.ptr, lmbda.ptr + 8 * D.ml))
    if D.tot2:
        stb = DeviceBuffer.from_array(np.array([2 ** 31 - 1], dtype=np.int32))
        raise_for(lib().kvx_nts_compute_scaling_dev(D.ns, D.d_off2.ptr, D.d_off1.ptr, s.ptr + 8 * ind, z.ptr + 8 * ind,
                                                    W.r.ptr, W.rti.ptr, lmbda.ptr + 8 * ind, D.work.ptr, stb.ptr))
        if int(stb.download(np.int32, 1)[0]) != 2 ** 31 - 1:
            raise ArithmeticError("compute_scaling: an 's' block of s or z is not positive definite")


def step_and_update_scaling(D, W, lmbda, ds, dz, sigs, sigz, step):
    """The end of an iteration (coneprog.py:1336-1431, 2463-2519): ds, dz (scaled by scale2, their 's' blocks replaced by the
    eigenvectors whose eigenvalues are in sigs, sigz) become the updated iterates in the current scaling, then
    misc.update_scaling (misc.py:422-634) refreshes W and lmbda."""
    ind = D.ind
    if ind:
        raise_for(lib().kvx_vec_scal_dev(ind, step, ds.ptr))
        raise_for(lib().kvx_vec_scal_dev(ind, step, dz.ptr))
        raise_for(lib().kvx_vec_axpy_dev(ind, 1.0, D.e.ptr, ds.ptr))
        raise_for(lib().kvx_vec_axpy_dev(ind, 1.0, D.e.ptr, dz.ptr))
    scale2(D, lmbda.ptr, ds.ptr, inverse="I")
    scale2(D, lmbda.ptr, dz.ptr, inverse="I")
    if D.tot1:
        for sg in (sigs, sigz):
            sg.scal(step)
            sg.addc(1.0)
            raise_for(lib().kvx_nt_sinv_dev(D.tot1, sg.ptr, lmbda.ptr + 8 * ind))     # blas.tbsv(lmbda, sig, k = 0)
        raise_for(lib().kvx_nts_colscale_dev(D.ns, D.d_off2.ptr, D.d_off1.ptr, ds.ptr + 8 * ind, sigs.ptr))
        raise_for(lib().kvx_nts_colscale_dev(D.ns, D.d_off2.ptr, D.d_off1.ptr, dz.ptr + 8 * ind, sigz.ptr))
    if D.ml:
        raise_for(lib().kvx_nt_update_scaling_dev(D.ml, ds.ptr, dz.ptr, W.d.ptr, W.di.ptr, lmbda.ptr))
    if D.nq:
        raise_for(lib().kvx_ntq_update_scaling_dev(D.nq, D.d_qoff.ptr, ds.ptr + 8 * D.ml, dz.ptr + 8 * D.ml, W.v.ptr, W.beta.ptr,
                                                   lmbda.ptr + 8 * D.ml))
    if D.tot2:
        raise_for(lib().kvx_nts_update_scaling_dev(D.ns, D.d_off2.ptr, D.d_off1.ptr, ds.ptr + 8 * ind, dz.ptr + 8 * ind, W.r.ptr,
                                                   W.rti.ptr, lmbda.ptr + 8 * ind, D.work.ptr))


def _ccs(M):
    """CCS of a dense or sparse matrix (ours or kvxopt's, or a 2-D numpy array); a dense matrix keeps every entry."""
    from .misc import _full_pattern
    if isinstance(M, np.ndarray):
        M = base.matrix(np.asarray(M, dtype=np.float64).reshape(M.shape[0], -1))
    m, n, cp, ri, v = base._as_ccs(_full_pattern(M))
    return m, n, np.ascontiguousarray(cp, dtype=np.int64), np.ascontiguousarray(ri, dtype=np.int64), np.ascontiguousarray(v, dtype=np.float64)


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


def _vec(v, name, size):
    a = np.ascontiguousarray(np.asarray(base._dense_buffer(v)[0] if not isinstance(v, np.ndarray) else v, dtype=np.float64).reshape(-1))
    if a.size != size:
        raise TypeError("'%s' must be a 'd' matrix of size (%d,1)" % (name, size))
    return a


def check_dims(dims, h_size=None):
    """coneprog.py:499-521: the dims checks and their TypeErrors."""
    if not isinstance(dims.get("l"), (int, np.integer)) or dims["l"] < 0:
        raise TypeError("'dims['l']' must be a nonnegative integer")
    if [k for k in dims.get("q", []) if not isinstance(k, (int, np.integer)) or k < 1]:
        raise TypeError("'dims['q']' must be a list of positive integers")
    if [k for k in dims.get("s", []) if not isinstance(k, (int, np.integer)) or k < 0]:
        raise TypeError("'dims['s']' must be a list of nonnegative integers")


def conelp(c, G, h, dims, A=None, b=None, options=None, primalstart=None, dualstart=None, kktsolver=None, chol_opts=None):
    """coneprog.conelp (coneprog.py:31-1436) for dims with 'q' / 's' cones, on the GPU.  Returns the reference's result dictionary
    with numpy arrays ('s' blocks of s and z as full symmetric matrices)."""
    _lib.require_device()
    if kktsolver is not None:
        raise NotImplementedError("conelp with 'q' / 's' cones runs misc.kkt_chol on the GPU; kktsolver is not selectable")
    opts = {"maxiters": 100, "abstol": 1e-7, "reltol": 1e-6, "feastol": 1e-7, "show_progress": False, "refinement": None}
    opts.update(options or {})
    MAXITERS, ABSTOL, RELTOL, FEASTOL = opts["maxiters"], opts["abstol"], opts["reltol"], opts["feastol"]
    if not isinstance(MAXITERS, (int, np.integer)) or MAXITERS < 1:
        raise ValueError("options['maxiters'] must be a positive integer")
    if RELTOL <= 0.0 and ABSTOL <= 0.0:
        raise ValueError("at least one of options['reltol'] and options['abstol'] must be positive")
    if FEASTOL <= 0.0:
        raise ValueError("options['feastol'] must be a positive scalar")
    show = opts["show_progress"]
    dims = {"l": dims.get("l", 0), "q": list(dims.get("q") or []), "s": list(dims.get("s") or [])}
    check_dims(dims)
    REFINEMENT = opts["refinement"]
    if REFINEMENT is None:
        REFINEMENT = 1 if (dims["q"] or dims["s"]) else 0            # coneprog.py:502-507
    elif not isinstance(REFINEMENT, (int, np.integer)) or REFINEMENT < 0:
        raise ValueError("options['refinement'] must be a nonnegative integer")
    D = Dims(dims)
    cdim = D.N
    c_h = np.asarray(base._dense_buffer(c)[0] if not isinstance(c, np.ndarray) else c, dtype=np.float64).reshape(-1)
    n = c_h.size
    h_h = _vec(h, "h", cdim)
    Gm, Gn, Gp, Gi, Gx = _ccs(G)
    if (Gm, Gn) != (cdim, n):
        raise TypeError("'G' must be a 'd' matrix of size (%d, %d)" % (cdim, n))
    p = 0
    Ap = Ai = Ax = None
    if A is not None:
        p, na, Ap, Ai, Ax = _ccs(A)
        if na != n:
            raise TypeError("'A' must be a 'd' matrix with %d columns " % n)
    b_h = np.zeros(0) if b is None else np.asarray(base._dense_buffer(b)[0] if not isinstance(b, np.ndarray) else b, dtype=np.float64).reshape(-1)
    if b_h.size != p:
        raise TypeError("'b' must have length %d" % p)
    if p > n or p + D.Np < n:
        raise ValueError("Rank(A) < p or Rank([G; A]) < n")           # coneprog.py:565-566
    kkt = KKTConeDev(D, n, Gp, Gi, Gx, p, Ap, Ai, Ax, chol_opts)
    Gd = kkt.G

    def Gf(u, v, trans="N", alpha=1.0, beta=0.0):                     # misc.sgemv (misc.py:801-833)
        if trans == "N":
            Gd.gemv(u, v, trans="N", alpha=alpha, beta=beta)
        else:
            tg.copy_from(u)
            if alpha:
                tri(D, tg.ptr, 1)
            Gd.gemv(tg, v, trans="T", alpha=alpha, beta=beta)

    def Af(u, v, trans="N", alpha=1.0, beta=0.0):                     # base.gemv with A (p x n)
        if p:
            kkt.A.gemv(u, v, trans=trans, alpha=alpha, beta=beta)
        elif trans == "T":
            if beta == 0.0:
                v.fill(0.0)
            else:
                v.scal(beta)

    def vec(nn, init=None):
        return DVec(nn, init)

    tg = vec(cdim)
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
        if show:
            print(msg or {"optimal": "Optimal solution found.", "primal infeasible": "Certificate of primal infeasibility found.",
                          "dual infeasible": "Certificate of dual infeasibility found."}[status])
        return {"x": x.get() if xs else None, "y": y.get() if zs else None, "s": s.get() if xs else None, "z": z.get() if zs else None,
                "status": status, "gap": gap, "relative gap": relgap, "primal objective": pcost, "dual objective": dcost,
                "primal infeasibility": pres, "dual infeasibility": dres,
                "primal slack": -ts if ts is not None else None, "dual slack": -tz if tz is not None else None,
                "residual as primal infeasibility certificate": pinfres, "residual as dual infeasibility certificate": dinfres,
                "iterations": iters, "factorizations": kkt.nfactor, "loop seconds": time.perf_counter() - t_start}

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
        relgap = gap / -pcost if pcost < 0.0 else (gap / dcost if dcost > 0.0 else None)
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
        relgap = gap / -pcost if pcost < 0.0 else (gap / dcost if dcost > 0.0 else None)
        pres = max(resy / resy0, resz / resz0)
        dres = resx / resx0
        pinfres = hresx / resx0 / (-hz - by) if hz + by < 0.0 else None
        dinfres = max(hresy / resy0, hresz / resz0) / (-cx) if cx < 0.0 else None
        if show:
            if iters == 0:
                print("% 10s% 12s% 10s% 8s% 7s % 5s" % ("pcost", "dcost", "gap", "pres", "dres", "k/t"))
            print("%2d: % 8.4e % 8.4e % 4.0e% 7.0e% 7.0e% 7.0e" % (iters, pcost, dcost, gap, pres, dres, kappa / tau))

        if (pres <= FEASTOL and dres <= FEASTOL and (gap <= ABSTOL or (relgap is not None and relgap <= RELTOL))) or iters == MAXITERS:
            x.scal(1.0 / tau); y.scal(1.0 / tau); s.scal(1.0 / tau); z.scal(1.0 / tau)
            tri(D, s.ptr, 0); tri(D, z.ptr, 0)
            ts, tz = max_step(D, s.ptr), max_step(D, z.ptr)
            if iters == MAXITERS:
                return finish("unknown", iters, gap, relgap, pcost, dcost, pres, dres, pinfres, dinfres, ts=ts, tz=tz,
                              msg="Terminated (maximum number of iterations reached).")
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
                          msg="Terminated (singular KKT matrix).")

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

        def f6(bx, by_, bz, btau, bs, bkappa):                        # coneprog.py:1211-1235
            if REFINEMENT:
                wx.copy_from(bx); wy.copy_from(by_); wz.copy_from(bz); ws.copy_from(bs)
                wtau, wkappa = btau[0], bkappa[0]
            f6_no_ir(bx, by_, bz, btau, bs, bkappa)
            for _ in range(REFINEMENT):
                wx2.copy_from(wx); wy2.copy_from(wy); wz2.copy_from(wz); ws2.copy_from(ws)
                wtau2, wkappa2 = [wtau], [wkappa]
                res(bx, by_, bz, btau, bs, bkappa, wx2, wy2, wz2, wtau2, ws2, wkappa2, dg, lmbda_g)
                f6_no_ir(wx2, wy2, wz2, wtau2, ws2, wkappa2)
                bx.axpy(wx2); by_.axpy(wy2); bz.axpy(wz2)
                btau[0] += wtau2[0]
                bs.axpy(ws2)
                bkappa[0] += wkappa2[0]

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
            if t == 0.0:
                step = 1.0
            else:
                step = min(1.0, 1.0 / t) if i == 0 else min(1.0, STEP / t)
            if i == 0:
                sigma = (1.0 - step) ** EXPON

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


def lower_ccs(M, n, name="P"):
    """Lower triangle (i >= j) of an n x n matrix (dense `matrix` or 2-D numpy array: every entry of the triangle stored; or an
    spmatrix) as CCS; what lies above the diagonal is ignored, as the reference's symmetric kernels ignore it."""
    from .misc import _full_pattern
    if isinstance(M, np.ndarray):
        M = base.matrix(np.asarray(M, dtype=np.float64).reshape(M.shape[0], -1))
    return _lower_ccs(_full_pattern(M), n, name)


def coneqp(P, q, G, h, dims, A=None, b=None, initvals=None, options=None, chol_opts=None):
    """coneprog.coneqp (coneprog.py:1440-2547) for dims with 'q' / 's' cones, on the GPU:

        minimize (1/2) x'Px + q'x  subject to  G x + s = h,  A x = b,  s in C,

    with the reference's kktsolver='chol' system (coneprog.py:1806-1809, 1969-1981): KKTConeDev with H = P, S = P + Gs' Gs.
    P: dense or sparse, its lower triangle is used (a dense P with its full lower pattern).  S must be positive definite, i.e.
    Rank([P; G]) = n (with equality constraints the reference needs that on the null space of A only).  Returns the reference's
    result dictionary (coneprog.py:2216-2221) with numpy arrays, the 's' blocks of s and z as full symmetric matrices, plus
    "factorizations"."""
    _lib.require_device()
    opts = {"maxiters": 100, "abstol": 1e-7, "reltol": 1e-6, "feastol": 1e-7, "show_progress": False, "use_correction": True}
    opts.update(options or {})
    num = (float, int, np.floating, np.integer)
    correction = opts["use_correction"]
    MAXITERS, ABSTOL, RELTOL, FEASTOL = opts["maxiters"], opts["abstol"], opts["reltol"], opts["feastol"]
    if not isinstance(MAXITERS, (int, np.integer)) or MAXITERS < 1:
        raise ValueError("options['maxiters'] must be a positive integer")
    if not isinstance(ABSTOL, num):
        raise ValueError("options['abstol'] must be a scalar")
    if not isinstance(RELTOL, num):
        raise ValueError("options['reltol'] must be a scalar")
    if RELTOL <= 0.0 and ABSTOL <= 0.0:
        raise ValueError("at least one of options['reltol'] and options['abstol'] must be positive")
    if not isinstance(FEASTOL, num) or FEASTOL <= 0.0:
        raise ValueError("options['feastol'] must be a positive scalar")
    show = opts["show_progress"]
    if G is None or dims is None:
        raise NotImplementedError("coneqp without G is not part of the general-cone path")
    for M in (P, G, A):
        if callable(M):
            raise ValueError("use of function valued P, G, A requires a user-provided kktsolver")
    dims = {"l": dims.get("l", 0), "q": list(dims.get("q") or []), "s": list(dims.get("s") or [])}
    check_dims(dims)
    if "refinement" not in opts or opts["refinement"] is None:
        REFINEMENT = 1 if (dims["q"] or dims["s"]) else 0            # coneprog.py:1862-1865
    else:
        REFINEMENT = opts["refinement"]
        if not isinstance(REFINEMENT, (int, np.integer)) or REFINEMENT < 0:
            raise ValueError("options['refinement'] must be a nonnegative integer")
    D = Dims(dims)
    cdim = D.N
    if cdim == 0:
        raise NotImplementedError("coneqp without cone constraints is not part of the general-cone path")
    q_h = np.ascontiguousarray(np.asarray(base._dense_buffer(q)[0] if not isinstance(q, np.ndarray) else q, dtype=np.float64).reshape(-1))
    n = q_h.size
    Pp, Pi, Px = lower_ccs(P, n)
    h_h = _vec(h, "h", cdim)
    Gm, Gn, Gp, Gi, Gx = _ccs(G)
    if (Gm, Gn) != (cdim, n):
        raise TypeError("'G' must be a 'd' matrix of size (%d, %d)" % (cdim, n))
    p = 0
    Ap = Ai = Ax = None
    if A is not None:
        p, na, Ap, Ai, Ax = _ccs(A)
        if na != n:
            raise TypeError("'A' must be a 'd' matrix with %d columns" % n)
    b_h = np.zeros(0) if b is None else np.asarray(base._dense_buffer(b)[0] if not isinstance(b, np.ndarray) else b, dtype=np.float64).reshape(-1)
    if b_h.size != p:
        raise TypeError("'b' must have length %d" % p)
    if p > n:
        raise ValueError("Rank(A) < p or Rank([P; G; A]) < n")        # coneprog.py:1970-1971
    kkt = KKTConeDev(D, n, Gp, Gi, Gx, p, Ap, Ai, Ax, chol_opts, Pp, Pi, Px)
    Gd, Pd = kkt.G, SymSpMatDev(n, Pp, Pi, Px)
    vec = DVec
    tg = vec(cdim)

    def Gf(u, v, trans="N", alpha=1.0, beta=0.0):                     # misc.sgemv (misc.py:801-833)
        if trans == "N":
            Gd.gemv(u, v, trans="N", alpha=alpha, beta=beta)
        else:
            tg.copy_from(u)
            tri(D, tg.ptr, 1)
            Gd.gemv(tg, v, trans="T", alpha=alpha, beta=beta)

    def Af(u, v, trans="N", alpha=1.0, beta=0.0):                     # base.gemv with A (p x n); p = 0: v := beta v
        if p:
            kkt.A.gemv(u, v, trans=trans, alpha=alpha, beta=beta)
        elif trans == "T" and beta == 0.0:
            v.fill(0.0)
        elif trans == "T" and beta != 1.0:
            v.scal(beta)

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
        if show:
            print(msg)
        return {"x": x.get(), "y": y.get() if p else np.zeros(0), "s": s.get(), "z": z.get(), "status": status, "gap": gap,
                "relative gap": relgap, "primal objective": pcost, "dual objective": dcost, "primal infeasibility": pres,
                "dual infeasibility": dres, "primal slack": -ts, "dual slack": -tz, "iterations": iters,
                "factorizations": kkt.nfactor}

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

    def f4(bx, by_, bz, bs):                                          # coneprog.py:2330-2347
        if REFINEMENT:
            wx.copy_from(bx); wy.copy_from(by_); wz.copy_from(bz); ws.copy_from(bs)
        f4_no_ir(bx, by_, bz, bs)
        for _ in range(REFINEMENT):
            wx2.copy_from(wx); wy2.copy_from(wy); wz2.copy_from(wz); ws2.copy_from(ws)
            res(bx, by_, bz, bs, wx2, wy2, wz2, ws2)
            f4_no_ir(wx2, wy2, wz2, ws2)
            bx.axpy(wx2); by_.axpy(wy2); bz.axpy(wz2); bs.axpy(ws2)

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
        relgap = gap / -pcost if pcost < 0.0 else (gap / dcost if dcost > 0.0 else None)
        pres = max(resy / resy0, resz / resz0)
        dres = resx / resx0
        if show:
            if iters == 0:
                print("% 10s% 12s% 10s% 8s% 7s" % ("pcost", "dcost", "gap", "pres", "dres"))
            print("%2d: % 8.4e % 8.4e % 4.0e% 7.0e% 7.0e" % (iters, pcost, dcost, gap, pres, dres))
        if (pres <= FEASTOL and dres <= FEASTOL and (gap <= ABSTOL or (relgap is not None and relgap <= RELTOL))) or iters == MAXITERS:
            if iters == MAXITERS:
                return finish("unknown", iters, gap, relgap, pcost, dcost, pres, dres, "Terminated (maximum number of iterations reached).")
            return finish("optimal", iters, gap, relgap, pcost, dcost, pres, dres, "Optimal solution found.")

        if iters == 0:
            compute_scaling(D, s, z, W, lmbda)
        ssqr(D, lmbdasq.ptr, lmbda.ptr)
        try:
            kkt.factor(W)
        except ArithmeticError:
            if iters == 0:
                raise ValueError("Rank(A) < p or Rank([P; A; G]) < n")
            return finish("unknown", iters, gap, relgap, pcost, dcost, pres, dres, "Terminated (singular KKT matrix).")

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
                return finish("unknown", iters, gap, relgap, pcost, dcost, pres, dres, "Terminated (singular KKT matrix).")
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
            if t == 0:
                step = 1.0
            else:
                step = min(1.0, 1.0 / t) if i == 0 else min(1.0, STEP / t)
            if i == 0:
                sigma = min(1.0, max(0.0, 1.0 - step + dsdz / gap * step ** 2)) ** EXPON
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
