"""`kvxopt.misc` / `kvxopt.misc_solvers` on MI355X -- the Nesterov-Todd scaling operations for the nonlinear, 'l', 'q' and
's' blocks and the storage helpers of the 's' blocks -- plus the KKT solver factory `kkt_chol2`: same names, argument
meaning and in-place semantics as the reference (src/python/misc.py, src/C/misc_solvers.c).  kkt_chol2 itself takes
'l' (and nonlinear) blocks only, as in the reference (misc.py:1381-1384).  The nonlinear block of cvxprog (`mnl` leading
entries scaled by W['dnl'], misc.py:262-270, 432-442, 48-60) is one more diagonal block in front of the 'l' block, so
every kernel simply runs over mnl + ml entries.

Host-array compatibility layer: arguments are host `matrix` objects (ours or kvxopt's); every operation uploads its
vectors whole, calls the device operation of `kvxopt_amd.coneops` on the cached layout (`Dims`) of the cone vector and
downloads what the reference's function modifies, with one synchronisation.  The device-resident paths for whole
interior-point iterations are `kvxopt_amd.lp` and `kvxopt_amd.cone`.
"""
import numpy as np

from . import _lib, base, cone, coneops, lp
from ._lib import lib, raise_for
from .base import _full_pattern
from .coneops import WDev, dims_for, dims_of
from .devvec import DVec, SpMatDev


def _buf(x):
    return base._dense_buffer(x)[0]


def _dims(dims, mnl=0):
    """The device layout of a cone vector; the mnl leading nonlinear entries are more 'l' entries."""
    _lib.require_device()
    return dims_for(int(mnl or 0) + dims["l"], dims.get("q") or [], dims.get("s") or [])


def _sync():
    raise_for(lib().kvx_dev_sync())


def _copy_without_s(x, y, dims, mnl, offsetx, offsety):
    """Without 's' blocks pack / unpack are the plain copy y := x, which needs no device; True when that was all."""
    if any(dims.get("s") or []):
        return False
    n = mnl + dims["l"] + sum(dims.get("q") or [])
    _buf(y)[offsety:offsety + n] = _buf(x)[offsetx:offsetx + n]
    return True


def compute_scaling(s, z, lmbda, dims, mnl=None):
    """misc.py:250-419: W['d'] = sqrt(s./z), W['di'] = 1./d, lmbda = sqrt(s.*z) on the 'l' entries; with mnl given (cvxprog),
    the first mnl entries make W['dnl'], W['dnli'] by the same formulas; for every second-order cone the unit-hyperbolic-norm
    vector W['v'][k] and W['beta'][k] with (beta_k (2 v_k v_k' - J)) z_k = lambda_k; for every 's' block r_k, rti_k = r_k^-T with
    r_k' z_k r_k = r_k^-1 s_k r_k^-T = diag(lambda_k).  ArithmeticError (lapack.potrf's) on a block that is not positive
    definite."""
    D = _dims(dims, mnl)
    W, lm = WDev(D), DVec(D.Nd)
    ds, dz = DVec(D.N, _buf(s)[:D.N]), DVec(D.N, _buf(z)[:D.N])
    bad = coneops.compute_scaling(D, ds, dz, W, lm)
    _sync()
    if bad is not None:
        raise ArithmeticError(bad + 1)
    _buf(lmbda)[:D.Nd] = lm.get()
    return W.to_host(mnl)


def update_scaling(W, lmbda, s, z):
    """misc.py:422-634, in place: W, lmbda and s, z (which leave as the reference leaves them: sqrt's on the 'l' entries, st / a
    and zt / b in the 'q' cones, the singular vectors U and V' in the 's' blocks)."""
    _lib.require_device()
    D, k = dims_of(W)
    Wd, lm = WDev(D).set_host(W), DVec(D.Nd, _buf(lmbda)[:D.Nd])
    ds, dz = DVec(D.N, _buf(s)[:D.N]), DVec(D.N, _buf(z)[:D.N])
    coneops.update_scaling(D, Wd, lm, ds, dz)
    _sync()
    _buf(s)[:D.N], _buf(z)[:D.N], _buf(lmbda)[:D.Nd] = ds.get(), dz.get(), lm.get()
    for key, new in Wd.to_host(k if "dnl" in W else None).items():
        if key == "beta":
            W["beta"][:] = new
        elif isinstance(new, list):
            for old, blk in zip(W[key], new):
                _buf(old)[:] = blk._a
        else:
            _buf(W[key])[:] = new._a


def scale(x, W, trans="N", inverse="N"):
    """misc_solvers.c:85-240 / misc.py:36-164, every column of x: the 'l' (and nonlinear) entries times d or di, the 'q' cones by
    beta_k (2 v_k v_k' - J) or its inverse, the 's' blocks x_k := r' X r ('N','N'), r X r' ('T','N'), rti X rti' ('N','I'),
    rti' X rti ('T','I') with X the symmetric matrix in the lower triangle of x_k (only that triangle is written)."""
    _lib.require_device()
    D, _ = dims_of(W)
    xb, size = base._dense_buffer(x)
    if D.N == 0:
        return
    dx, Wd = DVec(xb.size, xb), WDev(D).set_host(W)
    coneops.scale(D, Wd, dx.ptr, trans, inverse, ncols=size[1], ld=size[0])
    _sync()
    xb[:] = dx.get()


def _apply(op, D, x, nx, y, ny, **kw):
    """x[:nx] := op(x[:nx], y[:ny]) through the device."""
    dx, dy = DVec(nx, _buf(x)[:nx]), DVec(ny, _buf(y)[:ny])
    op(D, dx.ptr, dy.ptr, **kw)
    _sync()
    _buf(x)[:nx] = dx.get()
    return dy


def scale2(lmbda, x, dims, mnl=0, inverse="N"):
    """misc_solvers.c:256-397: x := x./lmbda ('N') or x.*lmbda ('I') on the 'l' entries, the hyperbolic form in the 'q' cones,
    x_k(i, j) divided or multiplied by sqrt(l_i) sqrt(l_j) in the 's' blocks."""
    D = _dims(dims, mnl)
    _apply(lambda D, xp, lp_: coneops.scale2(D, lp_, xp, inverse), D, x, D.N, lmbda, D.Nd)


def sprod(x, y, dims, mnl=0, diag="N"):
    """misc_solvers.c:634-770: x := y o x; the 's' blocks of y are full (diag 'N'; their upper triangles are filled in as the
    reference does) or diagonals only (diag 'D')."""
    D = _dims(dims, mnl)
    dy = _apply(coneops.sprod, D, x, D.N, y, D.N if diag == "N" else D.Nd, diag=diag)
    if diag == "N":
        _buf(y)[:D.N] = dy.get()


def sinv(x, y, dims, mnl=0):
    """misc_solvers.c:775-882: the inverse of x := y o x; y holds only the diagonals of its 's' blocks."""
    D = _dims(dims, mnl)
    _apply(coneops.sinv, D, x, D.N, y, D.Nd)


def ssqr(x, y, dims, mnl=0):
    """misc.py:945-959: x := y o y; the 's' components of x and y are diagonal and only the diagonals are stored."""
    D = _dims(dims, mnl)
    _apply(coneops.ssqr, D, x, D.Nd, y, D.Nd)


def sdot(x, y, dims, mnl=0):
    """misc_solvers.c:991-1046: sum_i x_i*y_i over the nonlinear, 'l' and 'q' entries plus, per 's' block, the trace inner
    product of the symmetric matrices stored in the lower triangles."""
    D = _dims(dims, mnl)
    dx, dy = DVec(D.N, _buf(x)[:D.N]), DVec(D.N, _buf(y)[:D.N])      # (held until the result is on the host)
    return coneops.sdot(D, dx.ptr, dy.ptr) if D.N else 0.0


def max_step(x, dims, mnl=0, sigma=None):
    """misc_solvers.c:1052-1160: min {t | x + t e >= 0}; 0.0 for an empty x.  With `sigma` the eigenvalues of the 's' blocks
    (ascending) are stored there and their eigenvectors replace the blocks of x."""
    D = _dims(dims, mnl)
    dx = DVec(D.N, _buf(x)[:D.N])
    dsg = DVec(D.tot1) if sigma is not None else None
    t = coneops.max_step(D, dx.ptr, sigma=dsg)
    if sigma is not None and D.tot2:
        _buf(sigma)[:D.tot1] = dsg.get()
        _buf(x)[:D.N] = dx.get()
    return t


# ---- storage helpers of the 's' blocks (misc_solvers.c:412-632, 887-988) -------------------------------------------------
def pack(x, y, dims, mnl=0, offsetx=0, offsety=0):
    """misc_solvers.c:412-468: y := x with the 's' blocks in packed storage (lower triangles by columns, off-diagonal
    entries scaled by sqrt(2))."""
    if _copy_without_s(x, y, dims, mnl, offsetx, offsety):
        return
    D = _dims(dims, mnl)
    dx, dy = DVec(D.N, _buf(x)[offsetx:offsetx + D.N]), DVec(D.Np)
    coneops.pack(D, dx.ptr, dy.ptr, 0)
    _sync()
    _buf(y)[offsety:offsety + D.Np] = dy.get()


def pack2(x, dims, mnl=0):
    """misc_solvers.c:476-544: in-place pack of every column of the matrix x (the diagonal entries are copied as they are)."""
    if not any(dims.get("s") or []):
        return
    D = _dims(dims, mnl)
    xb, size = base._dense_buffer(x)
    X = xb.reshape(size, order="F")
    dx, dp = DVec(xb.size, xb), DVec(D.Np)
    for c in range(size[1]):
        coneops.pack(D, dx.ptr + 8 * c * size[0], dp.ptr, 2)
        X[:D.Np, c] = dp.get()


def unpack(x, y, dims, mnl=0, offsetx=0, offsety=0):
    """misc_solvers.c:552-608: y := x with the 's' blocks unpacked into the lower triangles (off-diagonal entries scaled by
    1/sqrt(2)); the strict upper triangles of y are not touched."""
    if _copy_without_s(x, y, dims, mnl, offsetx, offsety):
        return
    D = _dims(dims, mnl)
    dx, dy = DVec(D.Np, _buf(x)[offsetx:offsetx + D.Np]), DVec(D.N, _buf(y)[offsety:offsety + D.N])
    coneops.pack(D, dy.ptr, dx.ptr, 1)
    _sync()
    _buf(y)[offsety:offsety + D.N] = dy.get()


def _tri(x, dims, offset, mode):
    if not any(dims.get("s") or []):
        return
    D = _dims(dims)
    d = DVec(D.N, _buf(x)[offset:offset + D.N])
    coneops.tri(D, d.ptr, mode)
    _sync()
    _buf(x)[offset:offset + D.N] = d.get()


def symm(x, n, offset=0):
    """misc_solvers.c:610-632: fills in the upper triangle of the n x n symmetric matrix stored at x[offset:] ('L' storage)."""
    _tri(x, {"l": 0, "s": [int(n)]}, offset, 0)


def trisc(x, dims, offset=0):
    """misc_solvers.c:887-938: upper triangles of the 's' blocks := 0, strict lower triangles scaled by 2."""
    _tri(x, dims, offset, 1)


def triusc(x, dims, offset=0):
    """misc_solvers.c:940-988: strict lower triangles of the 's' blocks scaled by 1/2."""
    _tri(x, dims, offset, 2)


class _Chol2Device:
    """Device side of one `kkt_chol2` factory: the stacked constraint matrix J = [Df; G] (plus the rows of A when S turned out
    singular), its row weights, the assembly plan of S = J' diag(w^2) J + H and the KKT object of kvxopt_amd.lp that owns
    the Cholesky factors.  Built at the first factor() call -- the call that fixes the sparsity patterns in the reference
    too (misc.py:1405-1432) -- and refilled with new values afterwards."""

    def __init__(self, G, A, mnl, Df, H, with_A_rows):
        gm, n, gcp, gri, gv = base._as_ccs(G)
        self.n, self.ml, self.mnl = n, gm, mnl
        self.p = A.size[0]
        am, an, acp, ari, av = base._as_ccs(A)
        blocks = []                                   # (row offset, colptr, rowind, value count) of every block of J
        if mnl:
            dm, dn, dcp, dri, dv = base._as_ccs(Df)
            if (dm, dn) != (mnl, n):
                raise TypeError("Df must be an mnl x n sparse matrix")
            blocks.append((0, dcp, dri, dv.size))
        blocks.append((mnl, gcp, gri, gv.size))
        if with_A_rows:
            blocks.append((mnl + gm, acp, ari, av.size))
        rows = np.concatenate([ri + off for off, cp, ri, cnt in blocks]) if blocks else np.zeros(0, np.int64)
        cols = np.concatenate([np.repeat(np.arange(n, dtype=np.int64), np.diff(cp)) for off, cp, ri, cnt in blocks])
        self._perm = np.lexsort((rows, cols))         # J's CCS order; also the gather of its value array from the blocks'
        self.Jp = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(cols, minlength=n), out=self.Jp[1:])
        self.Ji = np.ascontiguousarray(rows[self._perm])
        self.mj = mnl + gm + (am if with_A_rows else 0)
        self.with_A_rows = with_A_rows
        self._gv, self._av = gv, av
        Hp = Hi = Hx = None
        self._hkeep = None
        if H is not None:
            hm, hn, hcp, hri, hv = base._as_ccs(H)
            hcol = np.repeat(np.arange(hn, dtype=np.int64), np.diff(hcp))
            self._hkeep = hri >= hcol                 # S is stored by its lower triangle: that part of H is added
            Hp = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(np.bincount(hcol[self._hkeep], minlength=n), out=Hp[1:])
            Hi, Hx = np.ascontiguousarray(hri[self._hkeep]), np.ascontiguousarray(hv[self._hkeep])
            self._hpat = (hcp.copy(), hri.copy())
        Jx = self._values(Df)
        diag_s = (self.p > 0 and H is None and mnl == 0 and not with_A_rows and
                  (self.Ji.size == 0 or np.bincount(self.Ji, minlength=max(self.mj, 1)).max() <= 1))
        if self.p == 0:
            self.kkt = lp.KKTChol2Dev(self.mj, n, self.Jp, self.Ji, Jx, None, Hp, Hi, Hx)
            self.J, self.chol = self.kkt.G, self.kkt
        elif diag_s:
            self.kkt = lp.KKTDiagEqDev(self.mj, n, self.Jp, self.Ji, Jx, self.p, acp, ari, av)
            self.J, self.chol = None, None
        else:
            self.kkt = lp.KKTGenEqDev(self.mj, n, self.Jp, self.Ji, Jx, self.p, acp, ari, av, None, Hp, Hi, Hx)
            self.J, self.chol = self.kkt.G, self.kkt.S
        self.Adev = SpMatDev(am, an, acp, ari, av) if (with_A_rows and self.p) else None
        self.w = DVec(max(self.mj, 1))
        self.x, self.z = DVec(max(n, 1)), DVec(max(self.mj, 1))
        self.y = DVec(max(self.p, 1))
        self._first = True

    def _values(self, Df):
        parts = []
        if self.mnl:
            parts.append(base._as_ccs(Df)[4])
        parts.append(self._gv)
        if self.with_A_rows:
            parts.append(self._av)
        return np.ascontiguousarray(np.concatenate(parts)[self._perm]) if parts else np.zeros(0)

    def refactor(self, W, H, Df):
        """New weights (and Df / H values) on the fixed patterns; numeric refactorisation.  ArithmeticError if S (or K) is
        not positive definite."""
        wl = [np.asarray(_buf(W["dnli"]), dtype=np.float64)[:self.mnl]] if self.mnl else []
        wl.append(np.asarray(_buf(W["di"]), dtype=np.float64)[:self.ml])
        if self.with_A_rows:
            wl.append(np.ones(self.p))
        w = np.concatenate(wl) if self.mj else np.zeros(1)
        if w.size != max(self.mj, 1) and self.mj:
            raise TypeError("W['di'] does not match the number of inequality rows")
        self.w.set(w)
        if self.mnl and not self._first and self.J is not None:
            self.J.set_values(self._values(Df))
        if H is not None:
            if self._hkeep is None:
                raise ValueError("kkt_chol2: H appeared after the first call fixed the pattern of S without it")
            hm, hn, hcp, hri, hv = base._as_ccs(H)
            if hri.size != self._hpat[1].size or not np.array_equal(hcp, self._hpat[0]) or not np.array_equal(hri, self._hpat[1]):
                raise ValueError("kkt_chol2: H must keep the sparsity pattern of the first call")
            if not self._first and self.chol is not None:
                self.chol.set_hessian(np.ascontiguousarray(hv[self._hkeep]))
        self._first = False
        self.kkt.factor(self.w, sync=True)

    def solve(self, x, y, z):
        """(x, y, z) := (ux, uy, W uz) of the KKT system, host vectors in and out; the arithmetic stays on the device."""
        xb, yb, zb = _buf(x), _buf(y), _buf(z)
        n, p, m = self.n, self.p, self.mnl + self.ml
        self.x.set(xb[:n])
        zz = np.zeros(max(self.mj, 1))
        zz[:m] = zb[:m]
        self.z.set(zz)                                   # (the rows of A appended to J carry no right-hand side)
        if p:
            self.y.set(yb[:p])
            if self.with_A_rows:
                self.Adev.gemv(self.y, self.x, trans="T", alpha=1.0, beta=1.0)   # singular S: bx + A' by (misc.py:1525-1526)
            self.kkt.solve(self.x, self.y, self.z)
            yb[:p] = self.y.get()[:p]
        else:
            self.kkt.solve(self.x, self.z)
        xb[:n] = self.x.get()[:n]
        zb[:m] = self.z.get()[:m]


def kkt_chol2(G, dims, A, mnl=0):
    """KKT solver factory of the reference for sparse G (misc.py:1352-1567): returns factor(W, H=None, Df=None), which
    returns solve(x, y, z) overwriting the right-hand side (bx, by, bz) with (ux, uy, W uz) of

        [ H   A'  J' ] [ux]   [bx]
        [ A   0   0  ] [uy] = [by],      J = [Df; G]  (Df: the mnl x n Jacobian block of cvxprog, absent for cone LPs / QPs).
        [ J   0 -W'W ] [uz]   [bz]

    Same contract as the reference: the first factor() call fixes the sparsity patterns (of G, Df, H -- hence of
    S = J' W^-1 W^-T J + H) and analyses S once, later calls refactor numerically (misc.py:1405-1462); if the first S is not
    positive definite, A'A is added to it from then on and the solves compensate (misc.py:1433-1447, 1525-1526); a failing
    factorisation raises ArithmeticError.  Not the reference's program: everything between the host vectors of the caller
    and the result runs in HBM on kvxopt_amd.lp's device classes -- S assembled by one gather kernel on a product map,
    K = A S^-1 A' as a fixed-pattern assembly when S is diagonal and as a dense matrix otherwise (the reference rebuilds
    Asct = L^-1 P A' by sparse triangular solves and re-analyses K at every call, misc.py:1483-1487), both Cholesky factors
    resident between factor() and solve().  Dense G, A, H or Df (the reference's LAPACK branches) are taken as matrices with
    every entry stored and run through the same kernels."""
    if dims.get("q") or dims.get("s"):
        raise ValueError("kktsolver option 'kkt_chol2' is implemented only for problems with no "
                         "second-order or semidefinite cone constraints")
    p, n = A.size
    # dense operands (the reference's LAPACK branches, misc.py:1401-1404, 1428-1429, 1464-1481): every entry stored, the same
    # kernels on a full pattern -- S is then one dense front
    G = _full_pattern(G)
    A = _full_pattern(A)
    state = {"dev": None}

    def factor(W, H=None, Df=None):
        H = _full_pattern(H, lower=True)          # (the lower triangle is what the factorisation reads)
        if mnl:
            Df = _full_pattern(Df)
            if not hasattr(Df, "CCS"):
                raise TypeError("Df must be a 'd' matrix or spmatrix")
        _lib.require_device()
        if state["dev"] is None:
            dev = _Chol2Device(G, A, mnl, Df, H, with_A_rows=False)
            try:
                dev.refactor(W, H, Df)
            except ArithmeticError:
                if p == 0:
                    raise
                dev = _Chol2Device(G, A, mnl, Df, H, with_A_rows=True)      # S singular: S + A'A from now on
                dev.refactor(W, H, Df)
            state["dev"] = dev
        else:
            state["dev"].refactor(W, H, Df)
        return state["dev"].solve

    return factor


def kkt_chol(G, dims, A, mnl=0):
    """KKT solver factory of the reference for general cones (misc.py:1213-1349): returns factor(W, H=None, Df=None), which
    returns solve(x, y, z) overwriting (bx, by, bz) with (ux, uy, W uz) of

        [ H   A'  G'   ] [ux]   [bx]
        [ A   0   0    ] [uy] = [by],      H = 0 for cone LPs, H = P for coneqp
        [ G   0  -W'W  ] [uz]   [bz]

    with S = H + Gs' Gs, Gs = pack2(W^-T G), assembled on the fixed pattern of the cliques of the 'l' rows, 'q' cones and 's'
    blocks united with the lower pattern of H (kvx_cone_assemble_dev / kvx_cone_assemble_h_dev) and factored by the sparse
    Cholesky on one analysis; p > 0 is eliminated with K = A S^-1 A' (the reference uses a QR factorisation of A' there: the same
    solution, other roundings).  H: dense `matrix`, spmatrix or 2-D numpy array, its lower triangle is used (misc.py:1275-1277).
    The first call fixes the pattern of H; a later call with the same pattern refreshes its values only, one with another pattern
    (or H appearing or disappearing) builds a new plan and analysis.  Host vectors in and out, arithmetic on the device.  The
    nonlinear block (mnl > 0) and Df are not part of this path."""
    if mnl:
        raise NotImplementedError("misc.kkt_chol on the GPU: the nonlinear block (mnl > 0) is not supported")
    dims = {"l": dims["l"], "q": list(dims.get("q") or []), "s": list(dims.get("s") or [])}
    D = coneops.Dims(dims)
    _, n, Gp, Gi, Gx = base.ccs(G)
    p, _, Ap, Ai, Ax = base.ccs(A)
    state = {"kkt": None, "W": None, "hpat": None}

    def factor(W, H=None, Df=None):
        if Df is not None:
            raise NotImplementedError("misc.kkt_chol on the GPU: Df (cvxprog) is not supported")
        _lib.require_device()
        Hp = Hi = Hx = hpat = None
        if H is not None:
            Hp, Hi, Hx = base.lower_ccs(H, n, "H")
            hpat = (Hp.tobytes(), Hi.tobytes())
        if state["kkt"] is None or hpat != state["hpat"]:
            state["kkt"] = cone.KKTConeDev(D, n, Gp, Gi, Gx, p, Ap, Ai, Ax, None, Hp, Hi, Hx)
            state["hpat"] = hpat
            state["W"] = WDev(D)
            state["x"], state["y"], state["z"] = DVec(n), DVec(p), DVec(D.N)
        elif H is not None:
            state["kkt"].set_hessian(Hx)
        state["W"].set_host(W)
        state["kkt"].factor(state["W"])

        def solve(x, y, z):
            xb, yb, zb = _buf(x), _buf(y), _buf(z)
            X, Y, Z = state["x"], state["y"], state["z"]
            X.set(xb[:n]); Z.set(zb[:D.N])
            if p:
                Y.set(yb[:p])
            state["kkt"].solve(X, Y, Z)
            xb[:n] = X.get()
            zb[:D.N] = Z.get()
            if p:
                yb[:p] = Y.get()
        return solve

    return factor
