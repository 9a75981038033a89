"""Device containers of the interior-point drivers: `DVec` (a float64 vector in HBM with the BLAS-1 and orthant NT operations
of the C ABI), `reduce_multi` (several reductions, one host synchronisation), `SpMatDev` (a CCS matrix and its transpose in
HBM) and `SymSpMatDev` (a symmetric matrix given by its lower triangle).  kvxopt_amd.coneops, lp, cone and misc build on them."""
import ctypes
import math

import numpy as np

from ._lib import DeviceBuffer, lib, raise_for


class DVec:
    """A float64 vector in HBM with the BLAS-1 / NT-scaling operations of the C ABI."""

    def __init__(self, n, init=None):
        self.n = int(n)
        self.buf = DeviceBuffer(8 * max(self.n, 1))
        if init is not None:
            self.set(init)

    @property
    def ptr(self):
        return self.buf.ptr

    def set(self, a):
        self.buf.upload(np.ascontiguousarray(a, dtype=np.float64).reshape(-1))
        return self

    def get(self):
        return self.buf.download(np.float64, self.n)

    def fill(self, v):
        raise_for(lib().kvx_vec_fill_dev(self.n, float(v), self.ptr)); return self

    def copy_from(self, x):
        raise_for(lib().kvx_vec_copy_dev(self.n, x.ptr, self.ptr)); return self

    def axpy(self, x, alpha=1.0):                       # self += alpha * x
        raise_for(lib().kvx_vec_axpy_dev(self.n, float(alpha), x.ptr, self.ptr)); return self

    def lincomb(self, a, x, b=0.0, y=None):             # self := a * x + b * y (one pass; copy + axpy / copy + scal)
        raise_for(lib().kvx_vec_lincomb_dev(self.n, float(a), x.ptr, float(b) if y is not None else 0.0,
                                            (y if y is not None else x).ptr, self.ptr)); return self

    def scal(self, alpha):
        raise_for(lib().kvx_vec_scal_dev(self.n, float(alpha), self.ptr)); return self

    def addc(self, c):
        raise_for(lib().kvx_vec_addc_dev(self.n, float(c), self.ptr)); return self

    def mul(self, y):                                   # self .*= y   (misc.scale / sprod / scale2 'I')
        raise_for(lib().kvx_nt_sprod_dev(self.n, self.ptr, y.ptr)); return self

    def div(self, y):                                   # self ./= y   (sinv / scale2 'N')
        raise_for(lib().kvx_nt_sinv_dev(self.n, self.ptr, y.ptr)); return self

    def sqr_of(self, y):                                # self := y.*y  (misc.ssqr)
        raise_for(lib().kvx_nt_ssqr_dev(self.n, self.ptr, y.ptr)); return self

    def xmy(self, a, x, y, b=0.0):                      # self := a * x.*y + b * self
        raise_for(lib().kvx_vec_xmy_dev(self.n, float(a), x.ptr, y.ptr, float(b), self.ptr)); return self

    def dot(self, y):
        if self.n == 0:
            return 0.0
        r = ctypes.c_double()
        raise_for(lib().kvx_nt_sdot_dev(self.n, self.ptr, y.ptr, ctypes.byref(r)))
        return r.value

    def nrm2(self):
        return math.sqrt(self.dot(self))

    def max_step(self):                                 # misc.max_step 'l' block: max_i(-x_i)
        r = ctypes.c_double()
        raise_for(lib().kvx_nt_max_step_dev(self.n, self.ptr, ctypes.byref(r)))
        return r.value


def reduce_multi(items):
    """Several reductions with ONE host synchronisation (kvx_nt_reduce_multi_dev).  items: ("dot", x, y) or ("max", x)
    with DVec operands; entries whose operand is not a DVec (the empty y-blocks of p = 0) yield 0.0.  Bitwise the values
    of DVec.dot / DVec.max_step."""
    live = [(k, it) for k, it in enumerate(items) if isinstance(it[1], DVec) and it[1].n > 0]
    out = [0.0] * len(items)
    if not live:
        return out
    m = len(live)
    kind = (ctypes.c_int32 * m)(*[0 if it[0] == "dot" else 1 for _, it in live])
    n = (ctypes.c_int64 * m)(*[it[1].n for _, it in live])
    xs = (ctypes.c_void_p * m)(*[it[1].ptr for _, it in live])
    ys = (ctypes.c_void_p * m)(*[(it[2].ptr if it[0] == "dot" else None) for _, it in live])
    res = (ctypes.c_double * m)()
    raise_for(lib().kvx_nt_reduce_multi_dev(m, kind, n, xs, ys, res))
    for j, (k, _) in enumerate(live):
        out[k] = float(res[j])
    return out


class SpMatDev:
    """CCS matrix resident in HBM (int64 indices as in the reference, kvxopt.h:46), together with the CCS of its
    transpose: both directions of the mat-vec then run as row gathers (kvx_spmv_dev 'T') -- the column-scatter form of
    'N' needs FP64 atomics, whose rounding depends on the order of arrival: with it two runs of the interior-point loop
    differ in the last bits, without it they are bitwise identical (like the factorisation and the solves)."""

    def __init__(self, m, n, colptr, rowind, values):
        self.m, self.n = int(m), int(n)
        colptr = np.ascontiguousarray(colptr, dtype=np.int64)
        rowind = np.ascontiguousarray(rowind, dtype=np.int64)
        values = np.ascontiguousarray(values, dtype=np.float64)
        self.cp = DeviceBuffer.from_array(colptr)
        self.ri = DeviceBuffer.from_array(rowind) if len(rowind) else DeviceBuffer(8)
        self.vx = DeviceBuffer.from_array(values) if len(values) else DeviceBuffer(8)
        cols = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(colptr))
        # (row, column) order: the entries come column by column, so a STABLE sort by row is the two-key sort; counts by bincount
        # (lexsort + np.add.at were 6 of the 8 ms this constructor took for 400 000 entries)
        order = np.argsort(rowind, kind="stable")
        self._order = order                               # CCS position of every entry of the transposed copy
        tp = np.zeros(self.m + 1, dtype=np.int64)
        if len(rowind):
            np.cumsum(np.bincount(rowind, minlength=self.m), out=tp[1:])
        self.max_row = int(np.diff(tp).max()) if self.m else 0         # most entries in a row / column (the fused kernels size
        self.max_col = int(np.diff(colptr).max()) if self.n else 0     # their lane groups by them)
        self.tcp = DeviceBuffer.from_array(tp)
        self.tri = DeviceBuffer.from_array(cols[order]) if len(rowind) else DeviceBuffer(8)
        self.tvx = DeviceBuffer.from_array(values[order]) if len(values) else DeviceBuffer(8)

    def set_values(self, values):
        """New values on the same pattern (both copies)."""
        values = np.ascontiguousarray(values, dtype=np.float64)
        if values.size:
            self.vx.upload(values)
            self.tvx.upload(np.ascontiguousarray(values[self._order]))

    def value_maps(self, positions):
        """Device index maps of the entries at the CCS `positions`, into the values and into the transposed copy: the operand of
        scatter_values for a caller whose values of those entries live in HBM (kvxopt_amd.cvx: the rows Df of [Df; G])."""
        positions = np.ascontiguousarray(positions, dtype=np.int64)
        inv = np.empty(self._order.size, dtype=np.int64)
        inv[self._order] = np.arange(self._order.size, dtype=np.int64)
        up = lambda a: DeviceBuffer.from_array(a) if a.size else DeviceBuffer(8)
        return up(positions), up(inv[positions]), int(positions.size)

    def scatter_values(self, src_ptr, maps):
        """values[positions[i]] := src[i] in both copies (kvx_vec_scatter_dev), src a device address; the other entries stay."""
        a, b, count = maps
        if count:
            raise_for(lib().kvx_vec_scatter_dev(count, src_ptr, a.ptr, self.vx.ptr))
            raise_for(lib().kvx_vec_scatter_dev(count, src_ptr, b.ptr, self.tvx.ptr))

    def gemv(self, x, y, trans="N", alpha=1.0, beta=0.0):
        """y := alpha*op(A)*x + beta*y  (base.gemv -> sparse.c:1073-1104)."""
        if trans == "N":                                  # A x = (A')' x: gather over the rows of A
            raise_for(lib().kvx_spmv_dev(ord("T"), self.n, self.m, self.tcp.ptr, self.tri.ptr, self.tvx.ptr,
                                         float(alpha), x.ptr, float(beta), y.ptr))
        else:
            raise_for(lib().kvx_spmv_dev(ord("T"), self.m, self.n, self.cp.ptr, self.ri.ptr, self.vx.ptr,
                                         float(alpha), x.ptr, float(beta), y.ptr))



class SymSpMatDev:
    """Symmetric sparse matrix resident in HBM, given by its lower triangle (the 'L' storage base.symv reads for
    the quadratic term, coneprog.py:1889-1893): y := alpha*P*x + beta*y as one pass over the lower triangle and one
    transposed pass over its strictly lower part."""

    def __init__(self, n, colptr, rowind, values):
        colptr = np.ascontiguousarray(colptr, dtype=np.int64)
        rowind = np.ascontiguousarray(rowind, dtype=np.int64)
        values = np.ascontiguousarray(values, dtype=np.float64)
        cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(colptr))
        if np.any(rowind < cols):
            raise ValueError("P must be given by its lower triangle")
        strict = rowind > cols
        sp = np.zeros(n + 1, dtype=np.int64)
        np.add.at(sp, cols[strict] + 1, 1)
        np.cumsum(sp, out=sp)
        self.low = SpMatDev(n, n, colptr, rowind, values)
        self.strict = SpMatDev(n, n, sp, rowind[strict], values[strict])

    def symv(self, x, y, alpha=1.0, beta=0.0):
        self.low.gemv(x, y, trans="N", alpha=alpha, beta=beta)
        self.strict.gemv(x, y, trans="T", alpha=alpha, beta=1.0)
