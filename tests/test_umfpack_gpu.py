"""GPU tests of the `kvxopt.umfpack` mirror and of the refined solve under it (kvx_lu_solve_refine, csrc/lu_refine.hip): the
reference's TestUMFPACK (tests/test_sparse_solvers.py:101-211) restated on its four matrices, the documented answers
(doc/source/spsolvers.rst:126-138, 211-230), the per-analysis choice of the block form, the determinant, and the refinement
itself: bits of steps = 0, the reported backward errors against a recomputation, a matrix on which refinement strictly helps,
determinism, and the row lengths at which the 16-lane row groups of k_lu_resid change shape.

The backward error omega = max_i |r_i| / (|op(A)| |x| + |b|)_i is recomputed here with an EXACT residual (error-free products,
math.fsum): the device sums the residual in about twice the working precision, so both agree far inside rtol 1e-6 even where
omega is at rounding level."""
import math
import os

import numpy as np
import pytest
import scipy.sparse as sp

from kvxopt_amd import _lib, klu, umfpack
from kvxopt_amd.base import matrix, spmatrix
from kvxopt_amd.lu import LuSymbolic, LuNumeric

pytestmark = pytest.mark.gpu

CASES = ["ACTIVSg2000", "bcsstk13", "bcsstk24", "bp_800"]          # test_sparse_solvers.py:29-30
DOC_V = [2, 3, 3, -1, 4, 4, -3, 1, 2, 2, 6, 1]                     # spsolvers.rst:112-125
DOC_VB = [4, 3, 3, -1, 4, 4, -3, 1, 2, 2, 6, 2]
DOC_I = [0, 1, 0, 2, 4, 1, 2, 3, 4, 2, 1, 4]
DOC_J = [0, 0, 1, 1, 1, 2, 2, 2, 2, 3, 4, 4]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


def to_sp(S):
    return sp.csc_matrix((S.values, S.rowind, S.colptr), shape=S.size)


_LOADED = {}


def load(golden_dir, name):
    if name not in _LOADED:
        z = np.load(os.path.join(golden_dir, name + ".npz"))
        n = int(z["n"])
        _LOADED[name] = spmatrix.from_ccs(n, n, z["colptr"], z["rowind"], z["values"])
    return _LOADED[name]


def from_dense(D):
    A = sp.csc_matrix(D); A.sort_indices()
    return spmatrix.from_ccs(D.shape[0], D.shape[1], A.indptr, A.indices, A.data)


def omega_exact(M, x, b):
    """max_i |b - M x|_i / (|M| |x| + |b|)_i with 0 / 0 = 0, the residual rounded once from its exact value: every product
    M_ik x_k is split into hi + lo without error (Veltkamp / Dekker), math.fsum adds b_i and the parts exactly."""
    M = sp.csr_matrix(M)
    a, xc = M.data, x[M.indices]
    p = a * xc
    sa = 134217729.0 * a; ah = sa - (sa - a); al = a - ah
    sx = 134217729.0 * xc; xh = sx - (sx - xc); xl = xc - xh
    e = ((ah * xh - p) + ah * xl + al * xh) + al * xl
    r = np.array([math.fsum([b[i]] + list(-p[s:t]) + list(-e[s:t])) for i, (s, t) in enumerate(zip(M.indptr[:-1], M.indptr[1:]))])
    den = abs(M) @ np.abs(x) + np.abs(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(den > 0, np.abs(r) / den, np.where(np.abs(r) > 0, np.inf, 0.0))
    return float(q.max())


def refined(num, b, trans, steps):
    """(x, berr) of a refined solve of the columns of b; b is left alone."""
    n, k = b.shape
    x = np.asfortranarray(b.copy())
    w = num.solve_refine(x.reshape(-1, order="F"), trans=trans, nrhs=k, ldB=n, steps=steps, berr=True)
    return x, w


def plain_numeric(A, btf=True):
    return LuNumeric(LuSymbolic(A.size[0], A.colptr, A.rowind, A.values, btf=btf), A.values)


# ---- 1. documented answers ----------------------------------------------------------------------------------------------------
def test_doc_known_answers():
    A = spmatrix(DOC_V, DOC_I, DOC_J)
    x = matrix(np.ones(5))
    umfpack.linsolve(A, x)                                              # spsolvers.rst:126-138
    assert np.allclose(x._a, [0.579, -0.0526, 1.00, 1.97, -0.789], rtol=5e-3)
    Bm = spmatrix(DOC_VB, DOC_I, DOC_J)                                 # spsolvers.rst:211-230: x = A^-T B^-1 A^-1 1
    Fs = umfpack.symbolic(A)
    FA = umfpack.numeric(A, Fs)
    FB = umfpack.numeric(Bm, Fs)
    x = matrix(np.ones(5))
    umfpack.solve(A, FA, x)
    umfpack.solve(Bm, FB, x)
    umfpack.solve(A, FA, x, trans="T")
    assert np.allclose(x._a, [0.581, -0.237, 1.63, 8.07, -0.131], rtol=5e-3)
    assert FA.name == "UMFPACK NUM D FACTOR" and Fs.name == "UMFPACK SYM D FACTOR"


# ---- 2. TestUMFPACK on the four matrices --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_lu_identity(golden_dir, name):
    """test_sparse_solvers.py:103-121: norm(P*R*A*Q - L*U, 1) == 0 to 7 places; all five results are spmatrix."""
    A = load(golden_dir, name)
    n = A.size[0]
    Fn = umfpack.numeric(A, umfpack.symbolic(A))
    res = umfpack.get_numeric(A, Fn)
    assert len(res) == 5 and all(isinstance(M, spmatrix) and M.size == (n, n) for M in res)
    L, U, P, Q, R = (to_sp(M) for M in res)
    rho = abs(P @ R @ to_sp(A) @ Q - L @ U).sum(axis=0).max()
    print("%s: |P R A Q - L U|_1 = %.3e" % (name, rho))
    assert rho < 5e-8
    assert abs(sp.triu(L, 1)).sum() == 0 and np.all(L.diagonal() == 1.0)            # unit lower triangular, diagonal stored
    assert abs(sp.tril(U, -1)).sum() == 0
    for M in (P, Q):                                                                # permutation matrices
        assert M.nnz == n and np.all(M.data == 1.0) and np.all(M.sum(axis=0) == 1) and np.all(M.sum(axis=1) == 1)
    assert R.nnz == n and abs(R - sp.diags(R.diagonal())).sum() == 0 and np.all(R.diagonal() > 0)
    assert np.allclose(R.diagonal(), 1.0 / abs(to_sp(A)).max(axis=1).toarray().ravel(), rtol=1e-14)   # multipliers by ORIGINAL row


@pytest.mark.parametrize("name", CASES)
def test_linsolve_and_solve(golden_dir, name):
    """test_sparse_solvers.py:123-171: op(A) x reproduces b to 7 places, for linsolve and for symbolic / numeric / solve."""
    A = load(golden_dir, name)
    As = to_sp(A)
    n = A.size[0]
    b = np.random.default_rng(3).standard_normal((n, 3))
    Fn = umfpack.numeric(A, umfpack.symbolic(A))
    for tran, M in (("N", As), ("T", As.T)):
        x = matrix(b.copy())
        umfpack.linsolve(A, x, trans=tran)
        e1 = np.abs(M @ np.array(x._a).reshape(n, 3, order="F") - b).max()
        y = matrix(b.copy())
        umfpack.solve(A, Fn, y, trans=tran)
        e2 = np.abs(M @ np.array(y._a).reshape(n, 3, order="F") - b).max()
        print("%s %s: max|op(A)x - b| linsolve %.3e solve %.3e" % (name, tran, e1, e2))
        assert e1 < 5e-8 and e2 < 5e-8


@pytest.mark.parametrize("name", CASES)
def test_complex_linsolve_and_solve(golden_dir, name):
    """test_sparse_solvers.py:86-95 with `_complex = True`: A := A + 1j*A, b := 1j*normal, trans in 'N', 'T', 'C'."""
    A = load(golden_dir, name)
    n = A.size[0]
    Az = spmatrix.from_ccs(n, n, A.colptr, A.rowind, A.values * (1.0 + 1.0j))
    As = sp.csc_matrix((Az.values, Az.rowind, Az.colptr), shape=(n, n))
    b = np.random.default_rng(4).standard_normal((n, 3)) * 1j
    Fs = umfpack.symbolic(Az)
    Fn = umfpack.numeric(Az, Fs)
    assert Fs.name == "UMFPACK SYM Z FACTOR" and Fn.name == "UMFPACK NUM Z FACTOR"
    for tran, M in (("N", As), ("T", As.T), ("C", As.conj().T)):
        x = matrix(b.copy())
        umfpack.linsolve(Az, x, trans=tran)
        e1 = np.abs(M @ np.array(x._a).reshape(n, 3, order="F") - b).max()
        y = matrix(b.copy())
        umfpack.solve(Az, Fn, y, trans=tran)
        e2 = np.abs(M @ np.array(y._a).reshape(n, 3, order="F") - b).max()
        print("%s z %s: max|op(A)x - b| linsolve %.3e solve %.3e" % (name, tran, e1, e2))
        assert e1 < 5e-8 and e2 < 5e-8
    with pytest.raises(NotImplementedError):
        umfpack.get_numeric(Az, Fn)
    with pytest.raises(NotImplementedError):
        umfpack.get_det(Az, Fs, Fn)
    with pytest.raises(TypeError):
        umfpack.solve(A, Fn, matrix(np.ones(n)))                        # a 'z' factor with a 'd' matrix


# ---- 3. no block form, per call -----------------------------------------------------------------------------------------------
def test_no_block_form_per_call(golden_dir):
    A = load(golden_dir, "bp_800")
    n = A.size[0]

    def klu_blocks():
        Fs = klu.symbolic(A)
        out = klu.get_numeric(A, Fs, klu.numeric(A, Fs))
        return to_sp(out[5]).nnz, len(out[6]) - 1

    assert klu_blocks()[1] == 492 and klu_blocks()[0] > 0
    Fs = umfpack.symbolic(A)
    assert Fs.sym.btf()[:2] == (1, 1)
    Fn = umfpack.numeric(A, Fs)
    assert Fn.num.extract()["F"][1].size == 0 and list(Fn.num.extract()["r"]) == [0, n]     # nothing is left outside L U
    L, U, P, Q, R = (to_sp(M) for M in umfpack.get_numeric(A, Fn))
    assert abs(P @ R @ to_sp(A) @ Q - L @ U).sum(axis=0).max() < 5e-8
    x = matrix(np.ones(n))
    umfpack.linsolve(A, x)
    fnz, nb = klu_blocks()                                               # ... and klu still has its blocks afterwards
    assert nb == 492 and fnz > 0


# ---- 4. determinant -----------------------------------------------------------------------------------------------------------
def perm_sign(M):
    p = np.asarray(sp.csr_matrix(M).indices)                             # row i -> the column of its 1
    seen, sign = np.zeros(p.size, bool), 1
    for i in range(p.size):
        k, j = 0, i
        while not seen[j]:
            seen[j] = True; j = p[j]; k += 1
        if k and k % 2 == 0:
            sign = -sign
    return sign


def test_get_det():
    """test_sparse_solvers.py:173-197 (7 places)."""
    A = spmatrix(DOC_V, DOC_I, DOC_J)
    Fs = umfpack.symbolic(A)
    Fn = umfpack.numeric(A, Fs)
    d = umfpack.get_det(A, Fs, Fn)
    assert isinstance(d, float) and abs(d - np.linalg.det(to_sp(A).toarray())) < 5e-8
    # 6 x 6: a symmetric pentadiagonal matrix of determinant 210 with two rows exchanged -- determinant -210; the matching puts
    # the rows back, so the factorisation's row permutation is that exchange times the (even) fill-reducing order: odd
    D = 3.0 * np.eye(6) - np.eye(6, k=1) - np.eye(6, k=-1) - 0.5 * np.eye(6, k=2) - 0.5 * np.eye(6, k=-2)
    D[[1, 4]] = D[[4, 1]]
    M = from_dense(D)
    Fs = umfpack.symbolic(M)
    Fn = umfpack.numeric(M, Fs)
    d = umfpack.get_det(M, Fs, Fn)
    L, U, P, Q, R = umfpack.get_numeric(M, Fn)
    print("det 6x6: %.17g (numpy %.17g), sign(P) %d sign(Q) %d" % (d, np.linalg.det(D), perm_sign(to_sp(P)), perm_sign(to_sp(Q))))
    assert d < 0 and abs(d - np.linalg.det(D)) < 5e-8 and abs(d + 210.0) < 5e-8
    assert perm_sign(to_sp(P)) == -1                                     # the row permutation is odd


# ---- 5. refinement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", "NT")
@pytest.mark.parametrize("k", [1, 3])
def test_steps_zero_is_the_plain_solve_bit_for_bit(golden_dir, trans, k):
    A = load(golden_dir, "ACTIVSg2000")
    n = A.size[0]
    num = plain_numeric(A)
    b = np.random.default_rng(6).standard_normal((n, k))
    x0 = np.asfortranarray(b.copy())
    num.solve(x0.reshape(-1, order="F"), trans=trans, nrhs=k, ldB=n)
    x1 = np.asfortranarray(b.copy())
    assert num.solve_refine(x1.reshape(-1, order="F"), trans=trans, nrhs=k, ldB=n, steps=0, berr=False) is None
    assert x1.tobytes() == x0.tobytes()
    x2, w = refined(num, b, trans, 0)                                    # with the backward error asked for: the same solution
    assert x2.tobytes() == x0.tobytes() and np.array_equal(w[:, 0], w[:, 1])
    M = to_sp(A) if trans == "N" else to_sp(A).T
    for j in range(k):
        assert np.isclose(w[j, 0], omega_exact(M, x0[:, j], b[:, j]), rtol=1e-6, atol=0)


@pytest.mark.parametrize("name", CASES)
def test_backward_error_never_grows_and_is_what_numpy_computes(golden_dir, name):
    A = load(golden_dir, name)
    n = A.size[0]
    num = umfpack.numeric(A, umfpack.symbolic(A)).num
    b = np.random.default_rng(7).standard_normal((n, 3))
    for trans, M in (("N", to_sp(A)), ("T", to_sp(A).T)):
        x0, _ = refined(num, b, trans, 0)
        x2, w = refined(num, b, trans, 2)
        for j in range(3):
            before, after = omega_exact(M, x0[:, j], b[:, j]), omega_exact(M, x2[:, j], b[:, j])
            print("%s %s column %d: omega %.6e -> %.6e (recomputed %.6e -> %.6e)" % (name, trans, j, w[j, 0], w[j, 1], before, after))
            assert w[j, 1] <= w[j, 0]
            assert np.isclose(w[j, 0], before, rtol=1e-6, atol=0) and np.isclose(w[j, 1], after, rtol=1e-6, atol=0)


def weak_diagonal(n=64, diag=0.0011):
    """Unit off-diagonals, a diagonal just above the pivot tolerance 0.001 of the column maximum: analysed by its PATTERN (the
    transversal is then the diagonal; with the values the matching would move the ones there), the factorisation keeps every
    diagonal pivot it may keep and the factor grows by 1 / diag."""
    D = np.ones((n, n)) - (1.0 - diag) * np.eye(n)
    return D, from_dense(D)


def solve_longdouble(D, b):
    """Gaussian elimination with partial pivoting in numpy.longdouble."""
    A = np.array(D, dtype=np.longdouble)
    x = np.array(b, dtype=np.longdouble)
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, p]] = A[[p, k]]; x[[k, p]] = x[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= np.outer(f, A[k, k:])
        x[k + 1:] -= np.outer(f, x[k])
    for k in range(n - 1, -1, -1):
        x[k] = (x[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def test_refinement_strictly_helps_where_the_kept_pivots_let_the_factor_grow():
    """Matrix used: order 64, ones off the diagonal, 0.0011 on it (the first one tried).  Measured on MI355X:
    omega before 9.8e-15, 2.3e-14, 3.8e-14, after 8.7e-18, 8.9e-18, 3.6e-18; max |x - x_exact| 1.7e-12 before, 1.4e-16 after."""
    D, A = weak_diagonal()
    n = 64
    num = LuNumeric(LuSymbolic(n, A.colptr, A.rowind, None, btf=False), A.values)
    assert np.array_equal(num.sym.matching(), np.arange(n))              # the weak diagonal is what gets eliminated
    b = np.random.default_rng(12).standard_normal((n, 3))
    xe = solve_longdouble(D, b)
    x0, _ = refined(num, b, "N", 0)
    x2, w = refined(num, b, "N", 2)
    e0 = float(np.abs(x0 - xe).max()); e2 = float(np.abs(x2 - xe).max())
    print("weak diagonal n=64 diag=0.0011: omega before %s after %s; max|x - x_exact| before %.3e after %.3e" % (w[:, 0], w[:, 1], e0, e2))
    assert np.all(w[:, 1] <= w[:, 0]) and np.any(w[:, 1] < w[:, 0])
    assert w[:, 0].max() > 16 * np.finfo(float).eps                       # the matrix shows a backward error above rounding level
    for j in range(3):
        assert np.isclose(w[j, 0], omega_exact(D, x0[:, j], b[:, j]), rtol=1e-6, atol=0)
        assert np.isclose(w[j, 1], omega_exact(D, x2[:, j], b[:, j]), rtol=1e-6, atol=0)
    assert e2 <= e0


def test_two_runs_give_identical_bytes(golden_dir):
    """No floating-point atomics, fixed trees: the same bytes of x and of berr, launch by launch and from the replayed graph (the
    third call with the same buffer replays what the second one captured)."""
    A = load(golden_dir, "ACTIVSg2000")
    n = A.size[0]
    num = plain_numeric(A, btf=False)
    b = np.random.default_rng(8).standard_normal((n, 3))
    for trans in "NT":
        buf = np.empty(3 * n)
        runs = []
        for _ in range(3):
            buf[:] = b.reshape(-1, order="F")
            w = num.solve_refine(buf, trans=trans, nrhs=3, ldB=n, steps=2, berr=True)
            runs.append((buf.tobytes(), w.tobytes()))
        assert runs[0] == runs[1] == runs[2]
    other = plain_numeric(A, btf=False)                                   # ... and from another factor object
    buf[:] = b.reshape(-1, order="F")
    w2 = other.solve_refine(buf, trans="T", nrhs=3, ldB=n, steps=2, berr=True)
    assert (buf.tobytes(), w2.tobytes()) == runs[0]


def test_device_entry_point_and_the_factors_own_copy_of_the_values(golden_dir):
    """kvx_lu_solve_refine_dev gives the bytes of the host entry point; the residual uses the factor's own copy of A, which
    kvx_lu_refactor_dev refreshes for an analysis with KVX_LU_FLAG_KEEP_VALUES -- and a factor made from device values without
    the flag refuses a refined solve instead of refining against stale values."""
    A = load(golden_dir, "ACTIVSg2000")
    n, nnz = A.size[0], A.values.size
    b = np.random.default_rng(9).standard_normal((n, 2))
    num = LuNumeric(LuSymbolic(n, A.colptr, A.rowind, A.values, btf=False, keep_values=True), A.values)
    xh, wh = refined(num, b, "T", 2)
    buf = _lib.DeviceBuffer.from_array(b.reshape(-1, order="F"))
    wd = num.solve_refine_dev(buf.ptr, "T", nrhs=2, ldB=n, steps=2)
    assert buf.download(np.float64, 2 * n).tobytes() == xh.reshape(-1, order="F").tobytes() and wd.tobytes() == wh.tobytes()
    vals = _lib.DeviceBuffer.from_array(A.values * 2.0)
    num.refactor_dev(vals.ptr, nnz)
    x2, w2 = refined(num, b, "N", 2)
    M2 = 2.0 * to_sp(A)
    for j in range(2):                                                   # omega of (2 A) x = b: the copy followed the refactorisation
        assert w2[j, 1] <= w2[j, 0] < 1e-12 and np.isclose(w2[j, 1], omega_exact(M2, x2[:, j], b[:, j]), rtol=1e-6, atol=0)
    other = plain_numeric(A)
    other.refactor_dev(vals.ptr, nnz)
    with pytest.raises(ValueError, match="KVX_LU_FLAG_KEEP_VALUES"):
        refined(other, b, "N", 2)
    x0 = np.asfortranarray(b.copy())
    other.solve_refine(x0.reshape(-1, order="F"), nrhs=2, ldB=n, steps=0, berr=False)      # the plain solve needs no values
    assert np.abs(M2 @ x0 - b).max() < 5e-8
    other.refactor(A.values)                                             # host values: the copy is there again
    assert np.all(refined(other, b, "N", 2)[1] < 1e-12)


def row_group_matrix():
    """Order 72: rows of 1, 16 and 17 entries and a dense last row of 72 (a dense row appended to a sparse 40 x 40 matrix would
    have 41 entries -- not longer than the 64 lanes of a wave --, so the sparse part has order 71), diagonally dominant."""
    n = 72
    rng = np.random.default_rng(21)
    D = np.zeros((n, n))
    for i in range(n - 1):                                               # sparse part: one or two off-diagonal entries per row
        D[i, (i + 1) % (n - 1)] = rng.standard_normal()
        if i % 3 == 0:
            D[i, (i + 7) % (n - 1)] = rng.standard_normal()
    for i, k in ((5, 0), (20, 15), (33, 16), (n - 1, n - 1)):            # off-diagonal entries of the rows of 1, 16, 17 and 72
        D[i, :] = 0.0
        D[i, rng.choice(np.delete(np.arange(n), i), k, replace=False)] = rng.uniform(0.5, 1.5, k) * rng.choice([-1.0, 1.0], k)
    D[np.arange(n), np.arange(n)] = 1.0 + np.abs(D).sum(axis=1)
    return D


def test_row_lengths_that_exercise_the_row_groups():
    D = row_group_matrix()
    n = D.shape[0]
    cnt = np.count_nonzero(D, axis=1)
    assert cnt[5] == 1 and cnt[20] == 16 and cnt[33] == 17 and cnt[-1] == 72 > 64
    b = np.random.default_rng(22).standard_normal((n, 2))
    # 'N' reads the rows of D through the index map; D' with 'T' reads the same rows as the columns of the stored matrix
    for trans, S in (("N", D), ("T", D.T.copy())):
        A = from_dense(S)
        num = umfpack.numeric(A, umfpack.symbolic(A)).num
        x0, _ = refined(num, b, trans, 0)
        x2, w = refined(num, b, trans, 2)
        for j in range(2):
            print("row groups %s column %d: omega %.6e -> %.6e" % (trans, j, w[j, 0], w[j, 1]))
            assert w[j, 1] <= w[j, 0]
            assert np.isclose(w[j, 0], omega_exact(D, x0[:, j], b[:, j]), rtol=1e-6, atol=0)
            assert np.isclose(w[j, 1], omega_exact(D, x2[:, j], b[:, j]), rtol=1e-6, atol=0)
        assert np.abs(D @ x2 - b).max() < 1e-12 * max(1.0, np.abs(x2).max()) * np.abs(D).sum(axis=1).max()
    # a column without right-hand side and without solution entries: 0 / 0 counts as 0
    A = from_dense(D)
    num = umfpack.numeric(A, umfpack.symbolic(A)).num
    x, w = refined(num, np.zeros((n, 1)), "N", 2)
    assert not x.any() and np.array_equal(w, np.zeros((1, 2)))
