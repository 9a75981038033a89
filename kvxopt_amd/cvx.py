"""Device-resident drivers for nonlinear convex programs: `cpl`, `cp` and `gp`, a restatement of the reference's
`cvxprog.cpl / cp / gp` (src/python/cvxprog.py:35-1356, 1359-1964, 1967-2155) for dims = {'l': ml, 'q': [], 's': []}:

    minimize c'x   subject to  f_k(x) <= 0 (k = 0..mnl-1),  G x <= h,  A x = b.

Iterates, the scaling (dnl, dnli, d, di: one orthant block of mnl + ml entries), residuals and the saved line-search state stay
in HBM; the host reads scalars only.  The KKT system is the reduced one of cone.KKTConeDev, S = H + J' diag(dnli, di)^2 J with
J = [Df; G] stacked as mnl + ml orthant rows and equalities eliminated through K = A S^-1 A'.  The patterns of Df and H are
fixed at plan time; their values are refreshed every iteration by index maps (SpMatDev.scatter_values, KKTConeDev.set_hessian_dev).

F comes in two internal forms: the evaluator of a geometric program (kvx_gp_eval_dev: device pointers, no host trip) and a user
callback with the reference's protocol F(), F(x), F(x, z) (x handed over as a base.matrix, results uploaded; a sparse return
fixes the pattern at its first evaluation, and a later entry outside it rebuilds the plan).

`cp` is `cpl` on the epigraph form  minimize t  s.t.  f_0(x) - t <= 0  (cvxprog.py:1746-1964): the variable t is carried as
column n of the same device plan (Df gets the entry -1 in row 0, H, G and A an empty column), which is the system the
reference solves after eliminating t in closed form (cvxprog.py:1908-1941)."""
import ctypes
import math
import types

import numpy as np

from . import _ipm, _lib, base
from ._lib import DeviceBuffer, lib, raise_for
from .cone import KKTConeDev
from .coneops import (Dims, WDev, compute_scaling, max_step, scale, scale2, sdot, sinv, sprod, ssqr, step_and_update_scaling)
from .devvec import DVec, SpMatDev

BETA, ALPHA, MAX_RELAXED_ITERS = 0.5, 0.01, 8          # cvxprog.py:384-388
RANK_MSG = "Rank(A) < p or Rank([H(x); A; Df(x); G]) < n"


class _Replan(Exception):
    """A callback returned an entry outside the planned pattern; the evaluator now holds the union pattern."""


class _View:
    """n entries of a device vector starting at a byte address (the operand of SpMatDev.gemv and the kvx_vec_* entries)."""

    def __init__(self, ptr, n):
        self.ptr, self.n = ptr, n


def _dot(n, xp, yp):
    if n == 0:
        return 0.0
    r = ctypes.c_double()
    raise_for(lib().kvx_nt_sdot_dev(n, xp, yp, ctypes.byref(r)))
    return r.value


# ---- evaluators: nrows functions of n variables; the patterns of Df and tril(H) as (row, column) lists in value order -----------
class GPEval:
    """The log-sum-exp blocks of a geometric program in HBM (kvx_gp_plan / kvx_gp_eval_dev, cvxprog.py:2094-2153)."""

    def __init__(self, K, n, Fp, Fi, Fx, g):
        K = np.ascontiguousarray(K, dtype=np.int64)
        Fp = np.ascontiguousarray(Fp, dtype=np.int64); Fi = np.ascontiguousarray(Fi, dtype=np.int64)
        h = ctypes.c_void_p()
        raise_for(lib().kvx_gp_plan(K.size, _lib.pi(K), n, _lib.pi(Fp), _lib.pi(Fi) if Fi.size else None, ctypes.byref(h)))
        self._h = h
        self.nrows, self.n, self.x0 = int(K.size), int(n), np.zeros(n)
        dnz, hnz = ctypes.c_int64(), ctypes.c_int64()
        raise_for(lib().kvx_gp_pattern(h, ctypes.byref(dnz), None, None, ctypes.byref(hnz), None, None))
        self.Dfp, self.Hp = np.empty(n + 1, dtype=np.int64), np.empty(n + 1, dtype=np.int64)
        Dfi, Hi = np.empty(max(dnz.value, 1), dtype=np.int64), np.empty(max(hnz.value, 1), dtype=np.int64)
        raise_for(lib().kvx_gp_pattern(h, None, _lib.pi(self.Dfp), _lib.pi(Dfi), None, _lib.pi(self.Hp), _lib.pi(Hi)))
        self.Dfi, self.Hi = Dfi[:dnz.value].copy(), Hi[:hnz.value].copy()
        cols = lambda cp: np.repeat(np.arange(n, dtype=np.int64), np.diff(cp))
        self.df_pattern = (self.Dfi, cols(self.Dfp))
        self.h_pattern = (self.Hi, cols(self.Hp))
        self.Fx, self.g = np.ascontiguousarray(Fx, dtype=np.float64), np.ascontiguousarray(g, dtype=np.float64)
        self._dev = None

    def eval_ptr(self, xp, zp, fp, dfp, hp):
        if self._dev is None:
            _lib.require_device()
            self._dev = (DVec(self.Fx.size, self.Fx if self.Fx.size else None), DVec(self.g.size, self.g))
        raise_for(lib().kvx_gp_eval_dev(self._h, self._dev[0].ptr, self._dev[1].ptr, xp, zp, fp, dfp, hp))

    def eval(self, x, z, f, Dfx, Hx):
        self.eval_ptr(x.ptr, None if z is None else z.ptr, f.ptr, Dfx.ptr, None if z is None else Hx.ptr)
        return True

    def __del__(self):
        if getattr(self, "_h", None):
            lib().kvx_gp_free(self._h)
            self._h = None


def _entries(M, m, n, what, lower=False):
    """(rows, columns, values) of a callback's return: a dense matrix is its full pattern, a sparse one its stored entries."""
    if callable(M):
        raise NotImplementedError("cpl: operator-form (function valued) %s needs a user kktsolver, which this path does not take" % what)
    if isinstance(M, (int, float)):
        M = np.array([[float(M)]])
    if isinstance(M, np.ndarray) and M.ndim == 1:
        M = M.reshape(1, -1)
    mm, nn, cp, ri, v = base.ccs(M)
    if (mm, nn) != (m, n):
        raise TypeError("%s output argument of F() must be a 'd' matrix of size (%d,%d)" % (what, m, n))
    cj = np.repeat(np.arange(n, dtype=np.int64), np.diff(cp))
    if lower:
        keep = ri >= cj
        ri, cj, v = ri[keep], cj[keep], v[keep]
    return ri, cj, v


class CallbackEval:
    """A user callback with the reference's protocol (cvxprog.py:56-80): F() -> (mnl, x0), F(x) -> (f, Df) or None outside the
    domain, F(x, z) -> (f, Df, H).  x and z are handed over as base.matrix; f, Df, H are uploaded."""

    def __init__(self, F, n=None):
        try:
            mnl, x0 = F()
        except Exception:
            raise ValueError("function call 'F()' failed")
        self.F, self.nrows = F, int(mnl)
        self.x0 = base.flat(x0).copy()
        self.n = self.x0.size
        if n is not None and self.n != n:
            raise TypeError("'c' must be a 'd' matrix of size (%d,1)" % self.n)
        r = F(base.matrix(self.x0.copy()), base.matrix(np.ones(max(self.nrows, 1))[:self.nrows], (self.nrows, 1), "d"))
        if r is None or r[0] is None:
            raise ValueError("F(x0) is not in the domain of f")
        dr, dc, _ = _entries(r[1], self.nrows, self.n, "second")
        hr, hc, _ = _entries(r[2], self.n, self.n, "third", lower=True)
        self._set_patterns(dr * self.n + dc, hr * self.n + hc)

    def _set_patterns(self, dkey, hkey):
        n = max(self.n, 1)
        self.dkey, self.hkey = np.unique(dkey), np.unique(hkey)
        self.df_pattern = (self.dkey // n, self.dkey % n)
        self.h_pattern = (self.hkey // n, self.hkey % n)

    def _place(self, keys, planned, v):
        pos = np.searchsorted(planned, keys)
        pos[pos == planned.size] = 0
        if keys.size and not np.array_equal(planned[pos] if planned.size else keys + 1, keys):
            return None
        out = np.zeros(planned.size)
        out[pos] = v
        return out

    def eval(self, x, z, f, Dfx, Hx):
        xm = base.matrix(x.get()[:self.n].copy())
        r = self.F(xm) if z is None else self.F(xm, base.matrix(z.get()[:self.nrows].copy(), (self.nrows, 1), "d"))
        if r is None or r[0] is None:
            return False
        fv = base.flat(r[0] if not isinstance(r[0], (int, float)) else [float(r[0])])
        if fv.size != self.nrows:
            raise TypeError("first output argument of F() must be a 'd' matrix of size (%d, %d)" % (self.nrows, 1))
        dr, dc, dv = _entries(r[1], self.nrows, self.n, "second")
        dkey = dr * self.n + dc
        dvals = self._place(dkey, self.dkey, dv)
        hvals, hkey = True, self.hkey
        if z is not None:
            hr, hc, hv = _entries(r[2], self.n, self.n, "third", lower=True)
            hkey = hr * self.n + hc
            hvals = self._place(hkey, self.hkey, hv)
        if dvals is None or hvals is None:
            self._set_patterns(np.concatenate([self.dkey, dkey]), np.concatenate([self.hkey, hkey]))
            raise _Replan()
        if self.nrows:
            f.buf.upload(fv)
        if dvals.size:
            Dfx.buf.upload(dvals)
        if z is not None and hvals.size:
            Hx.buf.upload(hvals)
        return True


class Epigraph:
    """F_e(x, t) = (f_0(x) - t, f_1(x), ...) of cp's epigraph form (cvxprog.py:1762-1817): t is variable n; Df gains the entry
    (0, n) = -1 (kept last in the value order and written once), H an empty column."""

    def __init__(self, ev):
        self.ev, self.nrows, self.n = ev, ev.nrows, ev.n + 1
        self.x0 = np.concatenate([ev.x0, [0.0]])
        self._patterns()

    def _patterns(self):
        dr, dc = self.ev.df_pattern
        self.dnz = dr.size
        self.df_pattern = (np.concatenate([dr, [0]]).astype(np.int64), np.concatenate([dc, [self.n - 1]]).astype(np.int64))
        self.h_pattern = self.ev.h_pattern

    def eval(self, x, z, f, Dfx, Hx):
        try:
            ok = self.ev.eval(x, z, f, Dfx, Hx)
        except _Replan:
            self._patterns()
            raise
        if ok:
            raise_for(lib().kvx_vec_axpy_dev(1, -1.0, x.ptr + 8 * (self.n - 1), f.ptr))
            raise_for(lib().kvx_vec_fill_dev(1, -1.0, Dfx.ptr + 8 * self.dnz))
        return ok


# ---- the plan of one pattern: J = [Df; G], tril(H), the KKT object and the index maps that refresh their values ----------------
def _ccs_of(rows, cols, n):
    """CCS of the entries (rows, cols) in value order: colptr, rowind and the CCS position of every entry."""
    order = np.lexsort((rows, cols))
    cp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n), out=cp[1:])
    where = np.empty(order.size, dtype=np.int64)
    where[order] = np.arange(order.size, dtype=np.int64)
    return cp, np.ascontiguousarray(rows[order], dtype=np.int64), where


def _plan(ev, n, ml, G, p, A):
    mnl = ev.nrows
    Gp, Gi, Gx = G
    dr, dc = ev.df_pattern
    gc = np.repeat(np.arange(n, dtype=np.int64), np.diff(Gp))
    Jp, Ji, where = _ccs_of(np.concatenate([dr, Gi + mnl]), np.concatenate([dc, gc]), n)
    Jx = np.zeros(Ji.size)
    Jx[where[dr.size:]] = Gx
    hr, hc = ev.h_pattern
    Hp, Hi, hwhere = _ccs_of(hr, hc, n)
    k = types.SimpleNamespace()
    D = Dims({"l": mnl + ml, "q": [], "s": []})
    k.kkt = KKTConeDev(D, n, Jp, Ji, Jx, p, *A, None, Hp, Hi, np.zeros(Hi.size))
    k.J = k.kkt.G
    k.Jn = SpMatDev(mnl + ml, n, Jp, Ji, Jx)                          # J at the trial point of the line search
    k.jmaps, k.jnmaps = k.J.value_maps(where[:dr.size]), k.Jn.value_maps(where[:dr.size])
    k.hmap = DeviceBuffer.from_array(hwhere) if hwhere.size else None
    k.hnz = int(hwhere.size)
    # H u = L u + (L - diag) ' u with L = tril(H): two copies of the lower triangle, the second with a zero diagonal
    k.Hl, k.Hs = SpMatDev(n, n, Hp, Hi, np.zeros(Hi.size)), SpMatDev(n, n, Hp, Hi, np.zeros(Hi.size))
    k.hlmaps, k.hsmaps = k.Hl.value_maps(hwhere), k.Hs.value_maps(hwhere)
    diag = np.flatnonzero(Hi == np.repeat(np.arange(n, dtype=np.int64), np.diff(Hp)))
    k.hdiag = k.Hs.value_maps(diag)
    k.zeros = DVec(max(diag.size, 1)).fill(0.0)
    k.Dfx, k.nDfx, k.Hx = DVec(dr.size), DVec(dr.size), DVec(hr.size)
    k.factored = False                                                # S of this plan has been factored
    return k


def _refresh(k):
    """The values k.Dfx, k.Hx (in the evaluator's order) into J, the KKT object's H and the two copies of tril(H)."""
    k.J.scatter_values(k.Dfx.ptr, k.jmaps)
    if k.hnz:
        k.kkt.set_hessian_dev(k.Hx.ptr, k.hmap, k.hnz)
        k.Hl.scatter_values(k.Hx.ptr, k.hlmaps)
        k.Hs.scatter_values(k.Hx.ptr, k.hsmaps)
        k.Hs.scatter_values(k.zeros.ptr, k.hdiag)


def _cpl(c_h, ev, ml, G, h_h, p, A, b_h, opt):
    """cvxprog.cpl (cvxprog.py:556-1356) on the device; c_h, h_h, b_h: host vectors; G, A: CCS triples; ev: an evaluator."""
    MAXITERS, ABSTOL, RELTOL, FEASTOL, REFINEMENT, show = opt.maxiters, opt.abstol, opt.reltol, opt.feastol, opt.refinement, opt.show
    _lib.require_device()
    n, mnl = ev.n, ev.nrows
    N = mnl + ml
    D = Dims({"l": N, "q": [], "s": []})
    vec = DVec
    k = _plan(ev, n, ml, G, p, A)
    Gd = SpMatDev(ml, n, *G) if ml else None
    cv, hv, bv = vec(n, c_h), vec(ml, h_h if ml else None), vec(p, b_h if p else None)
    W, W0 = WDev(D), WDev(D)
    x, y = vec(n, ev.x0), vec(p).fill(0.0)
    z, s = vec(N).fill(1.0), vec(N).fill(1.0)                         # cvxprog.py:557-570
    f, newf = vec(mnl), vec(mnl)
    rx, ry, rz = vec(n), vec(p), vec(N)
    dx, dy, dz, ds = vec(n), vec(p), vec(N), vec(N)
    lmbda, lmbdasq = vec(N), vec(N)
    dz2, ds2 = vec(N), vec(N)
    newx, newy, newz, news, newrx, newrznl = vec(n), vec(p), vec(N), vec(N), vec(n), vec(mnl)
    rx0, ry0, rz0 = vec(n), vec(p), vec(N)
    x0, dx0, y0, dy0 = vec(n), vec(n), vec(p), vec(p)
    z0, dz0, dz20, s0, ds0, ds20 = vec(N), vec(N), vec(N), vec(N), vec(N), vec(N)
    lmbda0, lmbdasq0 = vec(N), vec(N)
    ws3, wz3, wz2 = vec(N), vec(N), vec(N)
    sigs = sigz = vec(0)
    if REFINEMENT:
        wx, wy, wz, ws = vec(n), vec(p), vec(N), vec(N)
        wx2, wy2, wz2r, ws2 = vec(n), vec(p), vec(N), vec(N)
    lo = lambda v: _View(v.ptr + 8 * mnl, ml)                         # the 'l' part of an (mnl + ml)-vector

    def Af(u, v, trans="N", alpha=1.0, beta=0.0):
        if p:
            k.kkt.A.gemv(u, v, trans=trans, alpha=alpha, beta=beta)

    def copy_W(src, dst):
        dst.d.copy_from(src.d); dst.di.copy_from(src.di)

    refresh = lambda: _refresh(k)

    def replan():
        """A new plan on the evaluator's widened patterns; the new KKT object continues the count of factorisations."""
        nfactor = k.kkt.nfactor
        k.__dict__.update(_plan(ev, n, ml, G, p, A).__dict__)
        k.kkt.nfactor = nfactor

    def F_at_x():
        """f, Df, H at (x, z[:mnl]) into the plan's matrices (cvxprog.py:625-629 and the F(x, z) of kktsolver, :535-537)."""
        try:
            ok = ev.eval(x, z, f, k.Dfx, k.Hx)
        except _Replan:
            replan()
            ok = ev.eval(x, z, f, k.Dfx, k.Hx)
        if not ok:
            raise ValueError("F(x, z) failed at an iterate inside the domain")
        refresh()

    def F_new():
        """f, Df at newx into newf and Jn; False outside the domain.  A return outside the planned pattern rebuilds the plan:
        f, Df, H at x go into the new matrices and, inside an iteration, the new S is factored with the current scaling."""
        try:
            ok = ev.eval(newx, None, newf, k.nDfx, None)
        except _Replan:
            refactor = k.factored
            replan()
            F_at_x()
            if refactor:
                k.kkt.factor(W)
                k.factored = True
            ok = ev.eval(newx, None, newf, k.nDfx, None)
        if ok:
            k.Jn.scatter_values(k.nDfx.ptr, k.jnmaps)
        return ok

    def Hf(u, v, alpha, beta):
        if k.hnz:
            k.Hl.gemv(u, v, trans="N", alpha=alpha, beta=beta)
            k.Hs.gemv(u, v, trans="T", alpha=alpha, beta=1.0)
        elif beta != 1.0:
            v.scal(beta)

    def finish(status, iters, gap, relgap, pcost, dcost, pres, dres, msg):
        ts, tz = max_step(D, s.ptr), max_step(D, z.ptr)
        if show:
            print(msg)
        sh, zh = s.get(), z.get()
        return {"status": status, "x": x.get(), "y": y.get() if p else np.zeros(0), "znl": zh[:mnl].copy(), "zl": zh[mnl:].copy(),
                "snl": sh[:mnl].copy(), "sl": sh[mnl:].copy(), "gap": gap, "relative gap": relgap, "primal objective": pcost,
                "dual objective": dcost, "primal slack": -ts, "dual slack": -tz, "primal infeasibility": pres,
                "dual infeasibility": dres, "iterations": iters, "factorizations": k.kkt.nfactor}

    def f4_no_ir(bx, by_, bz, bs):                                    # cvxprog.py:858-883
        sinv(D, bs.ptr, lmbda.ptr)
        ws3.copy_from(bs)
        scale(D, W, ws3.ptr, trans="T")
        bz.axpy(ws3, -1.0)
        k.kkt.solve(bx, by_, bz)
        bs.axpy(bz, -1.0)

    def res(ux, uy, uz, us, vx, vy, vz, vs):                          # cvxprog.py:889-923
        Hf(ux, vx, -1.0, 1.0)
        Af(uy, vx, alpha=-1.0, beta=1.0, trans="T")
        wz3.copy_from(uz)
        scale(D, W, wz3.ptr, inverse="I")
        k.J.gemv(wz3, vx, trans="T", alpha=-1.0, beta=1.0)
        Af(ux, vy, alpha=-1.0, beta=1.0)
        k.J.gemv(ux, wz2, trans="N")
        vz.axpy(wz2, -1.0)
        ws3.copy_from(us)
        scale(D, W, ws3.ptr, trans="T")
        vz.axpy(ws3, -1.0)
        ws3.copy_from(us)
        ws3.axpy(uz)
        sprod(D, ws3.ptr, lmbda.ptr, diag="D")
        vs.axpy(ws3, -1.0)

    f4 = _ipm.f4(f4_no_ir, res, REFINEMENT, (wx, wy, wz, ws) if REFINEMENT else (), (wx2, wy2, wz2r, ws2) if REFINEMENT else ())

    if show:
        print("% 10s% 12s% 10s% 8s% 7s" % ("pcost", "dcost", "gap", "pres", "dres"))
    relaxed_iters = 0
    phi0 = dphi0 = gap0 = step0 = dsdz0 = sigma0 = eta0 = 0.0
    for iters in range(MAXITERS + 1):
        F_at_x()
        gap = sdot(D, s.ptr, z.ptr)
        rx.copy_from(cv)                                              # rx = c + A'y + Df'z[:mnl] + G'z[mnl:]
        Af(y, rx, beta=1.0, trans="T")
        k.J.gemv(z, rx, trans="T", alpha=1.0, beta=1.0)
        resx = math.sqrt(rx.dot(rx))
        ry.copy_from(bv)                                              # ry = A x - b
        Af(x, ry, alpha=1.0, beta=-1.0)
        resy = math.sqrt(ry.dot(ry)) if p else 0.0
        rz.copy_from(s)                                               # rznl = s[:mnl] + f, rzl = s[mnl:] + G x - h
        if mnl:
            raise_for(lib().kvx_vec_axpy_dev(mnl, 1.0, f.ptr, rz.ptr))
        if ml:
            raise_for(lib().kvx_vec_axpy_dev(ml, -1.0, hv.ptr, lo(rz).ptr))
            Gd.gemv(x, lo(rz), beta=1.0)
        resznl = math.sqrt(_dot(mnl, rz.ptr, rz.ptr))
        reszl = math.sqrt(_dot(ml, lo(rz).ptr, lo(rz).ptr))
        pcost = cv.dot(x)
        dcost = pcost + (y.dot(ry) if p else 0.0) + _dot(mnl, z.ptr, rz.ptr) + _dot(ml, lo(z).ptr, lo(rz).ptr) - gap
        relgap = _ipm.relgap(gap, pcost, dcost)
        pres = math.sqrt(resy ** 2 + resznl ** 2 + reszl ** 2)
        dres = resx
        if iters == 0:
            resx0, resznl0 = max(1.0, resx), max(1.0, resznl)
            pres0, dres0 = max(1.0, pres), max(1.0, dres)
            gap0 = gap
            theta1, theta2, theta3 = 1.0 / gap0, 1.0 / resx0, 1.0 / resznl0
        phi = theta1 * gap + theta2 * resx + theta3 * resznl
        pres, dres = pres / pres0, dres / dres0
        if show:
            print("%2d: % 8.4e % 8.4e % 4.0e% 7.0e% 7.0e" % (iters, pcost, dcost, gap, pres, dres))

        if (pres <= FEASTOL and dres <= FEASTOL and (gap <= ABSTOL or (relgap is not None and relgap <= RELTOL))) or iters == MAXITERS:
            if iters == MAXITERS:                                     # cvxprog.py:729-755
                return finish("unknown", iters, gap, relgap, pcost, dcost, pres, dres, _ipm.MAXITERS_MSG)
            return finish("optimal", iters, gap, relgap, pcost, dcost, pres, dres, "Optimal solution found.")

        if iters == 0:
            compute_scaling(D, s, z, W, lmbda)
        ssqr(D, lmbdasq.ptr, lmbda.ptr)

        try:
            k.kkt.factor(W)                                           # H, Df at (x, z[:mnl]) are in place (F_at_x above)
            k.factored = True
        except ArithmeticError:                                       # cvxprog.py:778-840
            singular = False
            if iters == 0:
                raise ValueError(RANK_MSG)
            elif 0 < relaxed_iters < MAX_RELAXED_ITERS > 0:
                # the failure may come from a relaxed line search: restore the saved state, ask for a standard line search
                phi, gap = phi0, gap0
                copy_W(W0, W)
                x.copy_from(x0); y.copy_from(y0); s.copy_from(s0); z.copy_from(z0)
                lmbda.copy_from(lmbda0)
                lmbdasq0.copy_from(lmbdasq)                           # (as the reference has it, cvxprog.py:807)
                rx.copy_from(rx0); ry.copy_from(ry0)
                resx = math.sqrt(rx.dot(rx))
                rz.copy_from(rz0)
                resznl = math.sqrt(_dot(mnl, rz.ptr, rz.ptr))
                relaxed_iters = -1
                try:
                    F_at_x()
                    k.kkt.factor(W)
                except ArithmeticError:
                    singular = True
            else:
                singular = True
            if singular:
                return finish("unknown", iters, gap, relgap, pcost, dcost, pres, dres, _ipm.SINGULAR_MSG)

        sigma, eta = 0.0, 0.0
        for i in (0, 1):
            mu = gap / N if N else 0.0
            ds.copy_from(lmbdasq).scal(-1.0).addc(sigma * mu)         # ds = -lmbdasq + sigma mu e
            dx.fill(0.0).axpy(rx, -1.0 + eta)
            dy.fill(0.0).axpy(ry, -1.0 + eta)
            dz.fill(0.0).axpy(rz, -1.0 + eta)
            try:
                f4(dx, dy, dz, ds)
            except ArithmeticError:                                   # cvxprog.py:1004-1026
                if iters == 0:
                    raise ValueError(RANK_MSG)
                return finish("unknown", iters, gap, relgap, pcost, dcost, pres, dres, _ipm.SINGULAR_MSG)

            dsdz = sdot(D, ds.ptr, dz.ptr)
            dz2.copy_from(dz)
            scale(D, W, dz2.ptr, inverse="I")
            ds2.copy_from(ds)
            scale(D, W, ds2.ptr, trans="T")
            scale2(D, lmbda.ptr, ds.ptr)
            ts = max_step(D, ds.ptr)
            scale2(D, lmbda.ptr, dz.ptr)
            tz = max_step(D, dz.ptr)
            t = max([0.0, ts, tz])
            step = _ipm.step_length(t, 1)

            while True:                                               # backtrack until newx is in the domain of f
                newx.copy_from(x).axpy(dx, step)
                if F_new():
                    break
                step *= BETA

            phi = theta1 * gap + theta2 * resx + theta3 * resznl
            if i == 0:
                dphi = -phi
            else:
                dphi = -theta1 * (1 - sigma) * gap - theta2 * (1 - eta) * resx - theta3 * (1 - eta) * resznl

            # line search: relaxed (one step) and standard (backtracking) iterations, cvxprog.py:1081-1261
            backtrack = True
            while backtrack:
                newx.copy_from(x).axpy(dx, step)
                newy.copy_from(y).axpy(dy, step)
                newz.copy_from(z).axpy(dz2, step)
                news.copy_from(s).axpy(ds2, step)
                if not F_new():
                    raise ValueError("F(x) left the domain of f inside the line search")
                newrx.copy_from(cv)
                Af(newy, newrx, beta=1.0, trans="T")
                k.Jn.gemv(newz, newrx, trans="T", alpha=1.0, beta=1.0)
                newresx = math.sqrt(newrx.dot(newrx))
                if mnl:
                    raise_for(lib().kvx_vec_copy_dev(mnl, news.ptr, newrznl.ptr))
                    newrznl.axpy(newf)
                newresznl = math.sqrt(newrznl.dot(newrznl)) if mnl else 0.0
                newgap = (1.0 - (1.0 - sigma) * step) * gap + step ** 2 * dsdz
                newphi = theta1 * newgap + theta2 * newresx + theta3 * newresznl

                if i == 0:
                    if newgap <= (1.0 - ALPHA * step) * gap and (0 <= relaxed_iters < MAX_RELAXED_ITERS or
                                                                   newphi <= phi + ALPHA * step * dphi):
                        backtrack = False
                        sigma = min(newgap / gap, (newgap / gap) ** _ipm.EXPON)
                        eta = 0.0
                    else:
                        step *= BETA
                else:
                    if relaxed_iters == -1 or (relaxed_iters == 0 == MAX_RELAXED_ITERS):
                        if newphi <= phi + ALPHA * step * dphi:       # a standard line search
                            backtrack = False                         # (relaxed_iters stays, as in the reference: cvxprog.py:1178)
                        else:
                            step *= BETA
                    elif relaxed_iters == 0 < MAX_RELAXED_ITERS:
                        if newphi <= phi + ALPHA * step * dphi:
                            relaxed_iters = 0                         # the relaxed line search gives a sufficient decrease
                        else:                                         # save the state
                            phi0, dphi0, gap0, step0 = phi, dphi, gap, step
                            copy_W(W, W0)
                            x0.copy_from(x); dx0.copy_from(dx); y0.copy_from(y); dy0.copy_from(dy)
                            s0.copy_from(s); z0.copy_from(z); ds0.copy_from(ds); dz0.copy_from(dz)
                            ds20.copy_from(ds2); dz20.copy_from(dz2)
                            lmbda0.copy_from(lmbda); lmbdasq0.copy_from(lmbdasq)
                            dsdz0, sigma0, eta0 = dsdz, sigma, eta
                            rx0.copy_from(rx); ry0.copy_from(ry); rz0.copy_from(rz)
                            relaxed_iters = 1
                        backtrack = False
                    elif 0 <= relaxed_iters < MAX_RELAXED_ITERS > 0:
                        if newphi <= phi0 + ALPHA * step0 * dphi0:
                            relaxed_iters = 0
                        else:
                            relaxed_iters += 1
                        backtrack = False
                    elif relaxed_iters == MAX_RELAXED_ITERS > 0:
                        if newphi <= phi0 + ALPHA * step0 * dphi0:
                            backtrack = False
                            relaxed_iters = 0
                        else:                                         # resume the last saved line search
                            phi, dphi, gap, step = phi0, dphi0, gap0, step0
                            copy_W(W0, W)
                            x.copy_from(x0); dx.copy_from(dx0); y.copy_from(y0); dy.copy_from(dy0)
                            s.copy_from(s0); z.copy_from(z0); ds.copy_from(ds0); dz.copy_from(dz0)
                            ds2.copy_from(ds20); dz2.copy_from(dz20)
                            lmbda.copy_from(lmbda0)
                            dsdz, sigma, eta = dsdz0, sigma0, eta0
                            relaxed_iters = -1

        # update (cvxprog.py:1264-1355)
        x.axpy(dx, step)
        y.axpy(dy, step)
        step_and_update_scaling(D, W, lmbda, ds, dz, sigs, sigz, step)
        s.copy_from(lmbda)
        scale(D, W, s.ptr, trans="T")
        z.copy_from(lmbda)
        scale(D, W, z.ptr, inverse="I")
        gap = lmbda.dot(lmbda)
    raise AssertionError("unreachable")


# ---- front matter ----------------------------------------------------------------------------------------------------------------
def _options(options):
    o = dict(options or {})
    o.setdefault("refinement", 1)                                     # cvxprog.py:422
    o.setdefault("show_progress", True)                               # cvxprog.py:420
    return _ipm.options(o, {"l": 0, "q": [], "s": []})


def _refuse(dims, kktsolver, G, A, hooks):
    if dims and (dims.get("q") or dims.get("s")):
        raise NotImplementedError("cpl / cp with 'q' or 's' cones in dims: misc.kkt_chol with mnl > 0 is not built on the GPU")
    if kktsolver is not None:
        raise NotImplementedError("cpl / cp run misc.kkt_chol2 on the GPU; kktsolver (a function or the named solver %r) is not "
                                  "selectable" % (kktsolver,))
    if callable(G) or callable(A):
        raise NotImplementedError("cpl / cp with operator-form (function valued) G or A need a user kktsolver, which this path does "
                                  "not take")
    if any(hk is not None for hk in hooks):
        raise NotImplementedError("cpl / cp with the custom vector hooks xnewcopy, xdot, xaxpy, xscal, ynewcopy, ydot, yaxpy, yscal "
                                  "are not carried: x and y are device vectors")


def _linear(n, G, h, dims, A, b, extra_col=False):
    """G, h, A, b of cpl / cp as CCS triples and host vectors after the reference's size checks (cvxprog.py:464-513); with
    extra_col an empty column n is appended to G and A (the epigraph variable)."""
    h = np.zeros(0) if h is None else base.flat(h)
    ml = h.size if not dims else int(dims.get("l", 0))
    if h.size != ml:
        raise TypeError("'h' must be a 'd' matrix of size (%d,1)" % ml)
    if G is None:
        Gm, Gn, Gp, Gi, Gx = 0, n, np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)
    else:
        Gm, Gn, Gp, Gi, Gx = base.ccs(G)
    if (Gm, Gn) != (ml, n):
        raise TypeError("'G' must be a 'd' matrix with size (%d, %d)" % (ml, n))
    if A is None:
        p, An, Ap, Ai, Ax = 0, n, np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)
    else:
        p, An, Ap, Ai, Ax = base.ccs(A)
    if An != n:
        raise TypeError("'A' must be a 'd' matrix with %d columns" % n)
    b = np.zeros(0) if b is None else base.flat(b)
    if b.size != p:
        raise TypeError("'b' must have length %d" % p)
    if extra_col:
        Gp, Ap = np.concatenate([Gp, Gp[-1:]]), np.concatenate([Ap, Ap[-1:]])
    return ml, (Gp, Gi, Gx), h, p, (Ap, Ai, Ax), b


def cpl(c, F, G=None, h=None, dims=None, A=None, b=None, kktsolver=None, xnewcopy=None, xdot=None, xaxpy=None, xscal=None,
        ynewcopy=None, ydot=None, yaxpy=None, yscal=None, options=None):
    """cvxprog.cpl (cvxprog.py:35-1356) on the GPU for dims = {'l': ml, 'q': [], 's': []}.  Returns the reference's result
    dictionary with numpy arrays, plus 'iterations' and 'factorizations'."""
    _refuse(dims, kktsolver, G, A, (xnewcopy, xdot, xaxpy, xscal, ynewcopy, ydot, yaxpy, yscal))
    opt = _options(options)
    c = base.flat(c)
    ev = F if isinstance(F, (GPEval, CallbackEval, Epigraph)) else CallbackEval(F, c.size)
    if ev.n != c.size:
        raise TypeError("'c' must be a 'd' matrix of size (%d,1)" % ev.n)
    ml, Gc, h, p, Ac, b = _linear(ev.n, G, h, dims, A, b)
    return _cpl(c, ev, ml, Gc, h, p, Ac, b, opt)


def cp(F, G=None, h=None, dims=None, A=None, b=None, kktsolver=None, xnewcopy=None, xdot=None, xaxpy=None, xscal=None,
       ynewcopy=None, ydot=None, yaxpy=None, yscal=None, options=None):
    """cvxprog.cp (cvxprog.py:1359-1964) on the GPU: cpl on the epigraph form with t as an extra column of the same plan.
    x, znl, snl have the reference's shapes (the objective row dropped)."""
    _refuse(dims, kktsolver, G, A, (xnewcopy, xdot, xaxpy, xscal, ynewcopy, ydot, yaxpy, yscal))
    opt = _options(options)
    inner = F if isinstance(F, (GPEval, CallbackEval)) else _CpCallback(F)
    ev = Epigraph(inner)
    n = inner.n
    ml, Gc, h, p, Ac, b = _linear(n, G, h, dims, A, b, extra_col=True)
    c = np.zeros(n + 1)
    c[n] = 1.0
    sol = _cpl(c, ev, ml, Gc, h, p, Ac, b, opt)
    sol["x"] = sol["x"][:n].copy()
    sol["znl"], sol["snl"] = sol["znl"][1:].copy(), sol["snl"][1:].copy()
    return sol


class _CpCallback(CallbackEval):
    """cp's callback: F() returns the number of constraints mnl, F(x) returns mnl + 1 values with the objective first."""

    def __init__(self, F):
        def shifted(*a):
            if not a:
                m, x0 = F()
                return m + 1, x0
            return F(*a)
        try:
            F()
        except Exception:
            raise ValueError("function call 'F()' failed")
        super().__init__(shifted)


def _is_mat(M):
    return isinstance(M, (base.matrix, base.spmatrix)) or (isinstance(M, np.ndarray) and M.ndim == 2)


def _is_col(v, size):
    if isinstance(v, base.matrix):
        return v.typecode == "d" and v.size == (size, 1)
    return isinstance(v, np.ndarray) and v.dtype == np.float64 and v.shape in ((size,), (size, 1))


def gp_problem(K, F, g, G=None, h=None, A=None, b=None):
    """The argument checks of cvxprog.gp (cvxprog.py:2056-2092) with their TypeErrors; returns (K, l, n, ml, p)."""
    if type(K) is not list or [k for k in K if type(k) is not int or k <= 0]:
        raise TypeError("'K' must be a list of positive integers")
    l = sum(K)
    tc = lambda M: getattr(M, "typecode", "d") == "d" and (not isinstance(M, np.ndarray) or M.dtype == np.float64)
    rows = lambda M: M.size[0] if not isinstance(M, np.ndarray) else M.shape[0]
    ncol = lambda M: M.size[1] if not isinstance(M, np.ndarray) else M.shape[1]
    if not _is_mat(F) or not tc(F) or rows(F) != l:
        raise TypeError("'F' must be a dense or sparse 'd' matrix with %d rows" % l)
    if not _is_col(g, l):
        raise TypeError("'g' must be a dene 'd' matrix of size (%d,1)" % l)
    n = ncol(F)
    ml = 0
    if G is not None:
        if not _is_mat(G) or not tc(G) or ncol(G) != n:
            raise TypeError("'G' must be a dense or sparse 'd' matrix with %d columns" % n)
        ml = rows(G)
    if (h is None and ml) or (h is not None and not _is_col(h, ml)):
        raise TypeError("'h' must be a dense 'd' matrix of size (%d,1)" % ml)
    p = 0
    if A is not None:
        if not _is_mat(A) or not tc(A) or ncol(A) != n:
            raise TypeError("'A' must be a dense or sparse 'd' matrix with %d columns" % n)
        p = rows(A)
    if (b is None and p) or (b is not None and not _is_col(b, p)):
        raise TypeError("'b' must be a dense 'd' matrix of size (%d,1)" % p)
    return K, l, n, ml, p


def gp(K, F, g, G=None, h=None, A=None, b=None, kktsolver=None, options=None):
    """cvxprog.gp (cvxprog.py:1967-2155) on the GPU: the blocks of F stay in HBM (GPEval), the program runs through cp from
    x0 = 0."""
    K, l, n, ml, p = gp_problem(K, F, g, G, h, A, b)
    if kktsolver is not None:
        _refuse(None, kktsolver, None, None, ())
    _, _, Fp, Fi, Fx = base.ccs(F)
    return cp(GPEval(K, n, Fp, Fi, Fx, base.flat(g)), G if ml else None, h if ml else None, None, A if p else None,
              b if p else None, options=options)
