"""CPU-side checks of the `kvxopt.umfpack` mirror: the per-analysis choice "no block triangular form" (KVX_LU_FLAG_NO_BTF through
`LuSymbolic(..., btf=False)`), every argument error that is raised before a device is needed (src/C/umfpack.c:98-130, 240-260,
304-324, 582-624, 684-710) and the factor type checks (TypeCheck_Capsule: a `klu` factor, 'd' against 'z').  None of it needs a GPU;
the numeric phase must fail loudly here."""
import os

import numpy as np
import pytest

from kvxopt_amd import _lib, klu, umfpack
from kvxopt_amd.base import matrix, spmatrix
from kvxopt_amd.lu import LuSymbolic

# spsolvers.rst:112-125
DOC_V = [2, 3, 3, -1, 4, 4, -3, 1, 2, 2, 6, 1]
DOC_I = [0, 1, 0, 2, 4, 1, 2, 3, 4, 2, 1, 4]
DOC_J = [0, 0, 1, 1, 1, 2, 2, 2, 2, 3, 4, 4]


def load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    return int(z["n"]), z["colptr"], z["rowind"], z["values"]


def test_block_form_is_chosen_per_analysis(golden_dir):
    """btf=False: one block, one block level, every column in block 0 -- and nothing of it stays behind in the process: the default
    analysis has bp_800's 492 blocks (tests/test_klu_cpu.py) before AND after a flagged one."""
    n, cp, ri, v = load(golden_dir, "bp_800")
    assert LuSymbolic(n, cp, ri, v).btf()[0] == 492
    nb, nlev, blk = LuSymbolic(n, cp, ri, v, btf=False).btf()
    assert (nb, nlev) == (1, 1) and blk.shape == (n,) and not blk.any()
    nb, nlev, blk = LuSymbolic(n, cp, ri, v).btf()
    assert nb == 492 and 1 < nlev <= 64 and sorted(set(blk)) == list(range(492))
    assert LuSymbolic(n, cp, ri, None, btf=False).btf()[:2] == (1, 1)            # pattern-only analysis too
    # the same analysis otherwise: the matching does not depend on the block form
    assert np.array_equal(LuSymbolic(n, cp, ri, v, btf=False).matching(), LuSymbolic(n, cp, ri, v).matching())


def test_umfpack_symbolic_has_no_blocks_and_klu_keeps_its_own(golden_dir):
    n, cp, ri, v = load(golden_dir, "bp_800")
    A = spmatrix.from_ccs(n, n, cp, ri, v)
    assert klu.symbolic(A).sym.btf()[0] == 492
    Fs = umfpack.symbolic(A)
    assert Fs.sym.btf()[:2] == (1, 1) and Fs.name == "UMFPACK SYM D FACTOR"
    assert klu.symbolic(A).sym.btf()[0] == 492
    Fz = umfpack.symbolic(spmatrix.from_ccs(n, n, cp, ri, v * (1.0 + 1.0j)))
    assert Fz.name == "UMFPACK SYM Z FACTOR" and Fz.sym.n == 2 * n and Fz.sym.btf()[:2] == (1, 1)


def test_symbolic_argument_errors():
    with pytest.raises(TypeError, match="A must be a sparse matrix"):
        umfpack.symbolic(matrix(np.eye(2)))                                      # umfpack.c:248
    with pytest.raises(TypeError, match="A must be a sparse matrix"):
        umfpack.symbolic(np.eye(2))
    with pytest.raises(ValueError, match="at least one row and column"):
        umfpack.symbolic(spmatrix([], [], [], (0, 0)))                           # umfpack.c:249-252
    with pytest.raises(ValueError):
        umfpack.symbolic(spmatrix([], [], [], (0, 3)))
    with pytest.raises(NotImplementedError, match="square matrices only"):
        umfpack.symbolic(spmatrix([1.0, 2.0], [0, 1], [0, 1], (2, 3)))           # the reference accepts rectangular A


def test_numeric_argument_errors():
    A = spmatrix(DOC_V, DOC_I, DOC_J)
    Az = spmatrix(np.array(DOC_V) * (1.0 + 1.0j), DOC_I, DOC_J)
    Fs, Fsz = umfpack.symbolic(A), umfpack.symbolic(Az)
    with pytest.raises(TypeError, match="A must be a sparse matrix"):
        umfpack.numeric(matrix(np.eye(5)), Fs)                                   # umfpack.c:314
    with pytest.raises(TypeError):
        umfpack.numeric(A, Fs, None)                                             # two arguments: no refactorisation form
    with pytest.raises(TypeError, match="Fs is not the UMFPACK symbolic factor of a 'd' matrix"):
        umfpack.numeric(A, "not a factor")
    with pytest.raises(TypeError, match="Fs is not the UMFPACK symbolic factor of a 'd' matrix"):
        umfpack.numeric(A, klu.symbolic(A))                                      # a klu factor handed to umfpack
    with pytest.raises(TypeError, match="Fs is not the UMFPACK symbolic factor of a 'd' matrix"):
        umfpack.numeric(A, Fsz)                                                  # 'd' matrix, 'z' analysis
    with pytest.raises(TypeError, match="Fs is not the UMFPACK symbolic factor of a 'z' matrix"):
        umfpack.numeric(Az, Fs)
    with pytest.raises(ValueError, match="UMFPACK ERROR"):
        umfpack.numeric(spmatrix([1.0, 2.0], [0, 1], [0, 1], (5, 5)), Fs)        # not the analysed pattern


def test_solve_and_linsolve_argument_errors():
    A = spmatrix(DOC_V, DOC_I, DOC_J)
    Az = spmatrix(np.array(DOC_V) * (1.0 + 1.0j), DOC_I, DOC_J)
    F = umfpack._Fn(None, 5, "d")                                                # an opaque numeric factor: no error below reaches the device
    Fz = umfpack._Fn(None, 5, "z")
    assert F.name == "UMFPACK NUM D FACTOR" and Fz.name == "UMFPACK NUM Z FACTOR"
    b = matrix(np.ones(5))
    with pytest.raises(TypeError, match="A must a square sparse matrix"):
        umfpack.solve(matrix(np.eye(5)), F, b)                                   # umfpack.c:598-599
    with pytest.raises(TypeError, match="A must a square sparse matrix"):
        umfpack.solve(spmatrix([1.0, 2.0], [0, 1], [0, 1], (2, 3)), F, b)
    with pytest.raises(TypeError, match="A must be a square sparse matrix"):
        umfpack.linsolve(spmatrix([1.0, 2.0], [0, 1], [0, 1], (2, 3)), b)        # umfpack.c:115-116
    with pytest.raises(TypeError, match="A must be a square sparse matrix"):
        umfpack.linsolve(np.eye(5), b)
    # factor type mismatches (TypeCheck_Capsule, umfpack.c:602-610)
    with pytest.raises(TypeError, match="F is not the UMFPACK numeric factor of a 'd' matrix"):
        umfpack.solve(A, klu._Fn(None), b)                                       # a klu numeric factor
    with pytest.raises(TypeError, match="F is not the UMFPACK numeric factor of a 'd' matrix"):
        umfpack.solve(A, umfpack.symbolic(A), b)                                 # the symbolic factor (klu's signature has Fs here)
    with pytest.raises(TypeError, match="F is not the UMFPACK numeric factor of a 'd' matrix"):
        umfpack.solve(A, Fz, b)
    with pytest.raises(TypeError, match="F is not the UMFPACK numeric factor of a 'z' matrix"):
        umfpack.solve(Az, F, matrix(np.ones(5) * 1j))
    # right-hand side: type, ldB, offsetB, length, trans -- as klu.py::_rhs_args (umfpack.c:613-624)
    for call in (lambda B, **kw: umfpack.solve(A, F, B, **kw), lambda B, **kw: umfpack.linsolve(A, B, **kw)):
        with pytest.raises(TypeError, match="B must a dense matrix of the same numeric type as A"):
            call("not a matrix")
        with pytest.raises(TypeError, match="B must a dense matrix of the same numeric type as A"):
            call(matrix(np.ones(5) * 1j))                                        # complex B with a real A
        with pytest.raises(ValueError, match="ldB"):
            call(np.ones(12), ldB=3)
        with pytest.raises(ValueError, match="offsetB"):
            call(np.ones(12), offsetB=-1)
        with pytest.raises(TypeError, match="length of B is too small"):
            call(np.ones(4), ldB=5)
        with pytest.raises(TypeError, match="length of B is too small"):
            call(np.ones(12), nrhs=2, ldB=7, offsetB=1)
        with pytest.raises(ValueError, match="trans"):
            call(np.ones(5), trans="X")
        assert call(np.ones(5), nrhs=0) is None                                  # nothing to do (umfpack.c:617)
    with pytest.raises(TypeError, match="B must a dense matrix of the same numeric type as A"):
        umfpack.linsolve(Az, b)                                                  # real B with a complex A


def test_get_numeric_and_get_det_argument_errors():
    A = spmatrix(DOC_V, DOC_I, DOC_J)
    Az = spmatrix(np.array(DOC_V) * (1.0 + 1.0j), DOC_I, DOC_J)
    Fs, Fsz = umfpack.symbolic(A), umfpack.symbolic(Az)
    F, Fz = umfpack._Fn(None, 5, "d"), umfpack._Fn(None, 5, "z")
    with pytest.raises(TypeError, match="A must be a sparse matrix"):
        umfpack.get_numeric(np.eye(5), F)
    with pytest.raises(TypeError, match="F is not the UMFPACK numeric factor of a 'd' matrix"):
        umfpack.get_numeric(A, klu._Fn(None))
    with pytest.raises(TypeError, match="F is not the UMFPACK numeric factor of a 'd' matrix"):
        umfpack.get_numeric(A, Fz)
    with pytest.raises(TypeError, match="F is not the UMFPACK numeric factor of a 'z' matrix"):
        umfpack.get_numeric(Az, F)
    with pytest.raises(TypeError):
        umfpack.get_numeric(A, Fs, F)                                            # umfpack's signature: (A, Fn), not klu's (A, Fs, Fn)
    with pytest.raises(NotImplementedError, match="real embedding"):
        umfpack.get_numeric(Az, Fz)                                              # klu.py's reason
    with pytest.raises(TypeError, match="A must be a sparse matrix"):
        umfpack.get_det(np.eye(5), Fs, F)
    with pytest.raises(TypeError, match="F is not the UMFPACK numeric factor of a 'd' matrix"):
        umfpack.get_det(A, Fs, klu._Fn(None))
    with pytest.raises(TypeError, match="Fs is not the UMFPACK symbolic factor of a 'd' matrix"):
        umfpack.get_det(A, klu.symbolic(A), F)
    with pytest.raises(TypeError, match="F is not the UMFPACK numeric factor of a 'd' matrix"):
        umfpack.get_det(A, Fs, Fz)
    with pytest.raises(NotImplementedError, match="det"):
        umfpack.get_det(Az, Fsz, Fz)


def test_module_is_exported_and_documents_the_reference_ranges():
    import kvxopt_amd
    assert "umfpack" in kvxopt_amd.__all__
    for rng in ("umfpack.c:98-230", "umfpack.c:240-290", "umfpack.c:304-367", "umfpack.c:378-557", "umfpack.c:582-668", "umfpack.c:684"):
        assert rng in umfpack.__doc__
    assert "embedded" in umfpack.__doc__.lower()                                # whose omega the complex refinement reports


def test_numeric_phase_fails_loudly_without_a_gpu():
    if _lib.lib().kvx_device_count() > 0:
        return                                                                   # (tests/test_umfpack_gpu.py runs it there)
    A = spmatrix(DOC_V, DOC_I, DOC_J)
    with pytest.raises(RuntimeError):
        umfpack.numeric(A, umfpack.symbolic(A))
    with pytest.raises(RuntimeError):
        umfpack.linsolve(A, matrix(np.arange(5.0)))
