"""Drop-in for `kvxopt.umfpack` on MI355X: same functions, argument meaning and error behaviour as the reference's
src/C/umfpack.c (method table umfpack.c:728-737), backed by the HIP multifrontal LU of libkvxhip.so (kvx_lu_*).
No CPU fallback: numeric calls raise RuntimeError without a GPU.

    linsolve(A, B, trans='N', nrhs=-1, ldB=0, offsetB=0)        umfpack.c:98-230
    symbolic(A) -> Fs                                            umfpack.c:240-290
    numeric(A, Fs) -> Fn                                         umfpack.c:304-367
    get_numeric(A, Fn) -> L, U, P, Q, R                          umfpack.c:378-557   (P R A Q = L U)
    solve(A, F, B, trans='N', nrhs=-1, ldB=0, offsetB=0)         umfpack.c:582-668
    get_det(A, Fs, Fn) -> float                                  umfpack.c:684-726

Shared with `kvxopt_amd.klu`: the engine (analysis, fronts, threshold pivoting inside a front, the triangular sweeps), the real
embedding of complex matrices and the packing of right-hand sides.  Two things differ, as UMFPACK differs from KLU:

  * no block triangular form: every analysis made here carries KVX_LU_FLAG_NO_BTF, so P R A Q = L U has no off-diagonal part.  The
    choice belongs to the analysis; a `klu` analysis in the same process keeps its blocks.
  * every solve is refined on the device (kvx_lu_solve_refine with 2 steps, UMFPACK's default UMFPACK_IRSTEP): after x = solve(b) a
    correction d = solve(b - op(A) x) is kept only if it lowers the componentwise backward error
    omega = max_i |r_i| / (|op(A)| |x| + |b|)_i of its column.  The residual uses the values the factor was made from (the factor's
    device copy), not the A handed to `solve`: as in the reference, they are meant to be the same matrix.

Not the reference's: R is the engine's row scaling by max |a_ij| (UMFPACK's default is the row sum; the identity holds with either),
no column pre-ordering of UMFPACK's, square matrices only (`symbolic` of a rectangular A raises NotImplementedError).

Complex ('z') matrices are SOLVED -- `linsolve`, `symbolic`, `numeric`, `solve` with trans 'N', 'T', 'C' -- through the real
2n x 2n embedding, exactly as in `klu`; the refinement and its omega are those of the EMBEDDED real system (the componentwise
backward error of [[Re A, -Im A], [Im A, Re A]] [Re x; Im x] = [Re b; Im b], not that of the complex system).  `get_numeric` /
`get_det` of a complex factor raise NotImplementedError.
"""
import numpy as np

from . import base
from .base import spmatrix
from .klu import _embed, _rhs_args, _same_pattern, _solve_packed
from .lu import LuSymbolic, LuNumeric

IRSTEP = 2                      # UMFPACK_IRSTEP's default: refinement steps of every solve


class _Fs:
    """Opaque symbolic factor (the reference returns a PyCapsule named 'UMFPACK SYM D FACTOR', umfpack.c:42-43)."""

    def __init__(self, sym, pattern, tc):
        self.sym = sym
        self.pattern = pattern
        self.tc = tc
        self.name = "UMFPACK SYM %s FACTOR" % tc.upper()


class _Fn:
    """Opaque numeric factor ('UMFPACK NUM D FACTOR', umfpack.c:45-46)."""

    def __init__(self, num, n, tc):
        self.num = num
        self.n = n
        self.tc = tc
        self.name = "UMFPACK NUM %s FACTOR" % tc.upper()


def _sp(A, msg):
    """(rows, columns, colptr, rowind, values, typecode) of a sparse 'd' or 'z' matrix, else TypeError(msg)."""
    if not (isinstance(A, spmatrix) or hasattr(A, "CCS")) or getattr(A, "typecode", "d") not in ("d", "z"):
        raise TypeError(msg)
    m, n, cp, ri, v = base._as_ccs(A)
    return m, n, cp, ri, v, "z" if v.dtype.kind == "c" else "d"


def _check_fn(F, tc):
    if not isinstance(F, _Fn) or F.tc != tc:             # (a klu factor, a symbolic factor, the other type: TypeCheck_Capsule)
        raise TypeError("F is not the UMFPACK numeric factor of a '%s' matrix" % tc)


def symbolic(A):
    m, n, cp, ri, v, tc = _sp(A, "A must be a sparse matrix")
    if m == 0 or n == 0:
        raise ValueError("A must have at least one row and column")
    if m != n:
        raise NotImplementedError("umfpack.symbolic of a %d x %d matrix: the engine factors square matrices only "
                                  "(the reference accepts rectangular A)" % (m, n))
    args = _embed(n, cp, ri, v) if tc == "z" else (n, cp, ri, v)
    return _Fs(LuSymbolic(*args, btf=False), (cp.copy(), ri.copy()), tc)


def numeric(A, Fs):
    m, n, cp, ri, v, tc = _sp(A, "A must be a sparse matrix")
    if not isinstance(Fs, _Fs) or Fs.tc != tc:
        raise TypeError("Fs is not the UMFPACK symbolic factor of a '%s' matrix" % tc)
    if m != n or not _same_pattern(Fs, cp, ri):
        raise ValueError("UMFPACK ERROR -11")               # UMFPACK_ERROR_different_pattern
    if tc == "z":
        v = _embed(n, cp, ri, v)[3]
    return _Fn(LuNumeric(Fs.sym, v), n, tc)                  # ArithmeticError("singular matrix") as umfpack.c:358-359


def _refined(num):
    def call(buf, trans, nrhs, ldB, offset):
        return num.solve_refine(buf, trans=trans, nrhs=nrhs, ldB=ldB, offset=offset, steps=IRSTEP, berr=False)
    return call


def solve(A, F, B, trans="N", nrhs=-1, ldB=0, offsetB=0):
    m, n, cp, ri, v, tc = _sp(A, "A must a square sparse matrix")
    if m != n:
        raise TypeError("A must a square sparse matrix")
    _check_fn(F, tc)
    buf, nrhs, ldB = _rhs_args(n, B, trans, nrhs, ldB, offsetB, tc)
    if nrhs == 0:
        return
    if F.n != n:
        raise ValueError("UMFPACK ERROR -8")                 # UMFPACK_ERROR_invalid_matrix: not the factored order
    _solve_packed(_refined(F.num), n, buf, nrhs, ldB, offsetB, trans, tc == "z")


def linsolve(A, B, trans="N", nrhs=-1, ldB=0, offsetB=0):
    m, n, cp, ri, v, tc = _sp(A, "A must be a square sparse matrix")
    if m != n:
        raise TypeError("A must be a square sparse matrix")
    buf, nrhs_, ldB_ = _rhs_args(n, B, trans, nrhs, ldB, offsetB, tc)
    if nrhs_ == 0:
        return
    # the reference analyses and factors at every call (umfpack.c:142-198); so does this one
    Fn = numeric(A, symbolic(A))
    _solve_packed(_refined(Fn.num), n, buf, nrhs_, ldB_, offsetB, trans, tc == "z")


def get_numeric(A, Fn):
    m, n, cp, ri, v, tc = _sp(A, "A must be a sparse matrix")
    _check_fn(Fn, tc)
    if tc == "z":
        raise NotImplementedError("get_numeric of a complex factor: complex systems are solved through their real embedding, "
                                  "whose factors are not the complex L, U")
    e = Fn.num.extract()
    n = Fn.n
    ar = np.arange(n, dtype=np.int64)
    L = spmatrix.from_ccs(n, n, *e["L"])
    U = spmatrix.from_ccs(n, n, *e["U"])
    # umfpack.c:492-514: R = diag of the row multipliers (already reciprocated), by ORIGINAL row; P(i, Pt[i]) = 1; Q(Qt[j], j) = 1.
    # The engine's scale vector is in pivotal order (R_k P A Q = L U): R[P[k]] = 1 / Rs[k] gives P R A Q = L U.
    r = np.empty(n)
    r[e["P"]] = 1.0 / e["Rs"]
    R = spmatrix(r, ar, ar, (n, n))
    P = spmatrix(np.ones(n), ar, e["P"], (n, n))
    Q = spmatrix(np.ones(n), e["Q"], ar, (n, n))
    return L, U, P, Q, R


def get_det(A, Fs, Fn):
    m, n, cp, ri, v, tc = _sp(A, "A must be a sparse matrix")
    _check_fn(Fn, tc)
    if not isinstance(Fs, _Fs) or Fs.tc != tc:
        raise TypeError("Fs is not the UMFPACK symbolic factor of a '%s' matrix" % tc)
    if tc == "z":
        raise NotImplementedError("get_det of a complex factor (the embedding only gives |det A|^2)")
    return Fn.num.det()
