"""The Nesterov-Todd cone operations of `misc` on device vectors: the block layout `Dims` of a cone vector, the scaling `WDev`
in HBM and scale, scale2, sprod, sinv, ssqr, sdot, snrm2, max_step, tri, pack, put_diag, compute_scaling and
step_and_update_scaling over the kvx_nt_* ('l' entries), kvx_ntq_* ('q' cones) and kvx_nts_* ('s' blocks) entry points.
The one layer over those entry points: the interior-point drivers of kvxopt_amd.cone call it on their resident vectors,
kvxopt_amd.misc wraps it for host arrays (upload, operation, download)."""
import collections
import ctypes
import math

import numpy as np

from . import _lib, base
from ._lib import DeviceBuffer, lib, raise_for
from .devvec import DVec

NOFAIL = 2 ** 31 - 1           # status word of kvx_nts_compute_scaling_dev when every block was positive definite


def _i64dev(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    return DeviceBuffer.from_array(a) if a.size else DeviceBuffer(8)


class Dims:
    """Offsets of the blocks of a cone vector and the device tables of the kvx_ntq_* / kvx_nts_* entries."""

    def __init__(self, dims):
        self.ml = int(dims["l"])
        self.q = [int(k) for k in dims["q"]]
        self.s = [int(k) for k in dims["s"]]
        if any(m < 0 or m > 4096 for m in self.s):
            raise ValueError("semidefinite blocks must have an order between 0 and 4096 (one workgroup per block)")
        self.nq, self.ns = len(self.q), len(self.s)
        self.mq = sum(self.q)
        self.ind = self.ml + self.mq                                   # start of the 's' section
        self.tot2 = sum(m * m for m in self.s)
        self.tot1 = sum(self.s)
        self.N = self.ind + self.tot2                                  # cdim
        self.Nd = self.ind + self.tot1                                 # cdim_diag
        self.totp = sum(m * (m + 1) // 2 for m in self.s)
        self.Np = self.ind + self.totp                                 # cdim_pckd
        qoff = np.zeros(self.nq + 1, dtype=np.int64)
        np.cumsum(np.asarray(self.q, dtype=np.int64), out=qoff[1:])
        self.qoff = qoff
        self.d_qoff = _i64dev(qoff)
        sd = np.asarray(self.s, dtype=np.int64)
        self.off2 = np.zeros(self.ns + 1, dtype=np.int64)
        self.off1 = np.zeros(self.ns + 1, dtype=np.int64)
        np.cumsum(sd * sd, out=self.off2[1:])
        np.cumsum(sd, out=self.off1[1:])
        self.offp = np.zeros(self.ns + 1, dtype=np.int64)              # packed lower triangles
        np.cumsum(sd * (sd + 1) // 2, out=self.offp[1:])
        self.d_off2, self.d_off1, self.d_offp = _i64dev(self.off2), _i64dev(self.off1), _i64dev(self.offp)
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


# Layouts met before keep their device tables and work space (misc's host-array calls come by the thousand on a few layouts).
_DIMS_CACHE = collections.OrderedDict()
_DIMS_CACHE_MAX = 8


def dims_for(ml, q=(), s=()):
    """The cached `Dims` of this layout on the current device."""
    key = (int(ml), tuple(int(k) for k in q), tuple(int(k) for k in s), _lib.current_device())
    D = _DIMS_CACHE.pop(key, None)
    if D is None:
        D = Dims({"l": key[0], "q": key[1], "s": key[2]})
    _DIMS_CACHE[key] = D
    while len(_DIMS_CACHE) > _DIMS_CACHE_MAX:
        _DIMS_CACHE.popitem(last=False)
    return D


_lib.register_cache(_DIMS_CACHE.clear)


def _hostcat(xs):
    return np.concatenate([np.asarray(base._dense_buffer(x)[0], dtype=np.float64) for x in xs]) if xs else np.zeros(0)


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
        """From the reference's dictionary W (host matrices); the nonlinear entries W['dnl'] lead the 'l' block."""
        D = self.D
        if D.ml:
            self.d.set(_hostcat(([W["dnl"]] if "dnl" in W else []) + [W["d"]]))
            self.di.set(_hostcat(([W["dnli"]] if "dnl" in W else []) + [W["di"]]))
        if D.nq:
            self.v.set(_hostcat(W["v"])); self.beta.set(np.asarray(W["beta"], dtype=np.float64))
        if D.tot2:
            self.r.set(_hostcat(W["r"])); self.rti.set(_hostcat(W["rti"]))
        return self

    def to_host(self, mnl=None):
        """The reference's dictionary W (misc.py:250-283); with mnl the leading mnl entries of d, di make W['dnl'], W['dnli']."""
        D, k, mat = self.D, int(mnl or 0), base.matrix
        d, di = self.d.get(), self.di.get()
        W = {} if mnl is None else {"dnl": mat(d[:k].copy(), (k, 1)), "dnli": mat(di[:k].copy(), (k, 1))}
        W.update({"d": mat(d[k:].copy(), (D.ml - k, 1)), "di": mat(di[k:].copy(), (D.ml - k, 1)), "v": [], "beta": [], "r": [], "rti": []})
        if D.nq:
            v = self.v.get()
            W["v"] = [mat(v[D.qoff[i]:D.qoff[i + 1]].copy(), (m, 1)) for i, m in enumerate(D.q)]
            W["beta"] = [float(b) for b in self.beta.get()]
        if D.tot2:
            for key, a in (("r", self.r.get()), ("rti", self.rti.get())):
                W[key] = [mat(a[D.off2[i]:D.off2[i + 1]].copy(), (m, m)) for i, m in enumerate(D.s)]
        return W


def dims_of(W):
    """The cached `Dims` that a dictionary W implies (nonlinear entries counted with the 'l' block) and the number of
    nonlinear entries."""
    size = lambda x: base._dense_buffer(x)[1][0]
    k = size(W["dnl"]) if "dnl" in W else 0
    return dims_for(k + size(W["d"]), [size(v) for v in W.get("v") or []], [size(r) for r in W.get("r") or []]), k


# ---- the operations of misc on device vectors (pointer + the layout of Dims) -------------------------------------------------
def scale(D, W, xp, trans="N", inverse="N", ncols=1, ld=None):
    """misc.scale (misc_solvers.c:85-240) of the ncols columns (leading dimension ld, default cdim) at xp."""
    inv = inverse != "N"
    ld = D.N if ld is None else ld
    if D.ml:
        raise_for(lib().kvx_nt_scale_dev(D.ml, ncols, ld, xp, (W.di if inv else W.d).ptr))
    if D.nq:
        raise_for(lib().kvx_ntq_scale_dev(D.nq, D.d_qoff.ptr, W.v.ptr, W.beta.ptr, xp + 8 * D.ml, ld, ncols, 1 if inv else 0))
    if D.tot2:
        R = W.rti if inv else W.r
        form = 1 if (inverse == "N") == (trans == "T") else 0
        work = D.work if ncols * D.tot2 <= D.work.n else DVec(ncols * D.tot2)
        raise_for(lib().kvx_nts_scale_dev(D.ns, D.d_off2.ptr, D.d_off1.ptr, R.ptr, xp + 8 * D.ind, ld, ncols, form, work.ptr, D.tot2))


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


def pack(D, fullp, pkp, mode):
    """mode 0: misc.pack, packed := full ('s' blocks as lower triangles by columns, off-diagonal entries scaled by sqrt(2));
    1: misc.unpack, full := packed (strict upper triangles untouched); 2: a column of misc.pack2 (as 0, the copy unscaled)
    (misc_solvers.c:412-608).  The 'l' and 'q' entries are copied."""
    src, dst = (pkp, fullp) if mode == 1 else (fullp, pkp)
    if D.ind:
        raise_for(lib().kvx_vec_copy_dev(D.ind, src, dst))
    if D.tot2:
        raise_for(lib().kvx_nts_pack_dev(D.ns, D.d_off2.ptr, D.d_off1.ptr, D.d_offp.ptr, fullp + 8 * D.ind, pkp + 8 * D.ind, mode))


def put_diag(D, dst, srcp):
    """dst := src ('l' and 'q' entries), 's' blocks := diag(src_k) (coneprog.py:1273-1280, 1413-1421)."""
    if D.ind:
        raise_for(lib().kvx_vec_copy_dev(D.ind, srcp, dst.ptr))
    if D.tot2:
        raise_for(lib().kvx_vec_fill_dev(D.tot2, 0.0, dst.ptr + 8 * D.ind))
        raise_for(lib().kvx_vec_scatter_dev(D.tot1, srcp + 8 * D.ind, D.d_sdiag.ptr, dst.ptr + 8 * D.ind))


def compute_scaling(D, s, z, W, lmbda):
    """misc.compute_scaling (misc.py:250-419): W and lmbda from the interior points s, z.  Returns None, or the index of the
    first 's' block of s or z that is not positive definite (W and lmbda are then not to be used)."""
    ind = D.ind
    if D.ml:
        raise_for(lib().kvx_nt_compute_scaling_dev(D.ml, s.ptr, z.ptr, W.d.ptr, W.di.ptr, lmbda.ptr))
    if D.nq:
        raise_for(lib().kvx_ntq_compute_scaling_dev(D.nq, D.d_qoff.ptr, s.ptr + 8 * D.ml, z.ptr + 8 * D.ml, W.v.ptr,
                                                    W.beta.ptr, lmbda.ptr + 8 * D.ml))
    if D.tot2:
        stb = DeviceBuffer.from_array(np.array([NOFAIL], dtype=np.int32))
        raise_for(lib().kvx_nts_compute_scaling_dev(D.ns, D.d_off2.ptr, D.d_off1.ptr, s.ptr + 8 * ind, z.ptr + 8 * ind,
                                                    W.r.ptr, W.rti.ptr, lmbda.ptr + 8 * ind, D.work.ptr, stb.ptr))
        bad = int(stb.download(np.int32, 1)[0])
        if bad != NOFAIL:
            return bad
    return None


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
    update_scaling(D, W, lmbda, ds, dz)


def update_scaling(D, W, lmbda, s, z):
    """misc.update_scaling (misc.py:422-634): W and lmbda from the new iterates s, z in the current scaling ('s' blocks as
    Cholesky factors); s and z are overwritten as the reference overwrites them."""
    ind = D.ind
    if D.ml:
        raise_for(lib().kvx_nt_update_scaling_dev(D.ml, s.ptr, z.ptr, W.d.ptr, W.di.ptr, lmbda.ptr))
    if D.nq:
        raise_for(lib().kvx_ntq_update_scaling_dev(D.nq, D.d_qoff.ptr, s.ptr + 8 * D.ml, z.ptr + 8 * D.ml, W.v.ptr, W.beta.ptr,
                                                   lmbda.ptr + 8 * D.ml))
    if D.tot2:
        raise_for(lib().kvx_nts_update_scaling_dev(D.ns, D.d_off2.ptr, D.d_off1.ptr, s.ptr + 8 * ind, z.ptr + 8 * ind, W.r.ptr,
                                                   W.rti.ptr, lmbda.ptr + 8 * ind, D.work.ptr))

