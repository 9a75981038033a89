"""The host side of osqp.Problem.solve_batch ("A batch on the kept factor"): the argument, bound and
rho-class checks of osqp._check_batch need no device."""
import numpy as np
import pytest

from kvxopt_amd import osqp
from kvxopt_amd.base import matrix

N_, M_ = 3, 4
E = np.array([0.5, 1.0, 2.0, 1.5])
KL = np.array([-1.0, -2.0, 0.25, -osqp.INFTY])        # row 0, 1 two-sided, row 2 an equality, row 3 free
KU = np.array([1.0, 2.0, 0.25, osqp.INFTY])


def batch(B=3):
    rng = np.random.default_rng(3)
    Q = rng.standard_normal((N_, B))
    shift = 0.05 * rng.standard_normal((M_, B))
    L = np.where(np.abs(KL)[:, None] < 1e26, KL[:, None] + shift, KL[:, None])
    U = np.where(np.abs(KU)[:, None] < 1e26, KU[:, None] + shift, KU[:, None])
    return Q, L, U


def check(Q, L=None, U=None):
    return osqp._check_batch(Q, L, U, N_, M_, E, KL, KU)


def test_problem_has_solve_batch():
    assert callable(getattr(osqp.Problem, "solve_batch", None))
    assert "solve_batch" in osqp.__doc__


def test_accepted_batch_comes_back_unchanged():
    Q, L, U = batch()
    q, l, u = check(Q, L, U)
    assert np.array_equal(q, Q) and np.array_equal(l, L) and np.array_equal(u, U)
    assert all(v.flags.f_contiguous and v.dtype == np.float64 for v in (q, l, u))
    L1 = L.copy()
    L1[2] = KL[2]                                     # the equality row stays where the kept u has it
    q, l, u = check(matrix(Q), matrix(L1), None)      # dense 'd' matrices; U None: the kept u for every member
    assert np.array_equal(q, Q) and np.array_equal(l, L1) and u is None
    q, l, u = check(Q)
    assert np.array_equal(q, Q) and l is None and u is None
    q, l, u = check(np.ascontiguousarray(Q), np.ascontiguousarray(L), np.ascontiguousarray(U))      # row-major input
    assert np.array_equal(q, Q) and np.array_equal(l, L) and np.array_equal(u, U)


def test_types_and_shapes_have_the_texts_of_solve():
    Q, L, U = batch()
    for bad in (Q.astype(np.float32), Q.astype(np.int64), matrix(np.ones((N_, 2), dtype=np.int64), tc="i"), [[1.0] * 3] * N_, Q[:, 0], None):
        with pytest.raises(TypeError, match="Q must be a matrix with typecode 'd'"):
            check(bad, L, U)
    with pytest.raises(TypeError, match="L must be a matrix with typecode 'd'"):
        check(Q, L.astype(np.float32), U)
    with pytest.raises(TypeError, match="U must be a matrix with typecode 'd'"):
        check(Q, L, np.ones((M_, 3), dtype=np.int64))
    with pytest.raises(ValueError, match="incompatible dimensions"):
        check(Q[:2], L, U)                            # n - 1 rows
    with pytest.raises(ValueError, match="incompatible dimensions"):
        check(Q, L[:3], U)                            # m - 1 rows
    with pytest.raises(ValueError, match="incompatible dimensions"):
        check(Q, L, U[:, :2])                         # another B
    with pytest.raises(ValueError, match="incompatible dimensions"):
        check(Q[:, :0])                               # no member


def test_crossed_bounds_in_one_member():
    Q, L, U = batch()
    L[1, 2] = U[1, 2] + 1.0
    with pytest.raises(ValueError, match=r"l <= u does not hold in member 2, row 1"):
        check(Q, L, U)
    Q, L, U = batch()
    U[2] = KU[2]
    U[0, 1] = KL[0] - 1.0                             # against the kept l
    with pytest.raises(ValueError, match=r"l <= u does not hold in member 1, row 0"):
        check(Q, None, U)


def test_a_member_that_changes_a_rho_class():
    Q, L, U = batch()
    L[1, 1] = U[1, 1]                                 # two-sided -> equality
    with pytest.raises(ValueError, match=r"member 1, row 1 "):
        check(Q, L, U)
    Q, L, U = batch()
    L[0, 2], U[0, 2] = -osqp.INFTY, osqp.INFTY        # two-sided -> free
    with pytest.raises(ValueError, match=r"member 2, row 0 "):
        check(Q, L, U)
    Q, L, U = batch()
    U[2, 0] = L[2, 0] + 1.0                           # equality -> two-sided; also a later member: the first is named
    L[1, 2] = U[1, 2]
    with pytest.raises(ValueError, match=r"member 0, row 2 "):
        check(Q, L, U)
    Q, L, U = batch()
    L[3, 1] = 0.0                                     # free -> one-sided
    with pytest.raises(ValueError, match=r"member 1, row 3 "):
        check(Q, L, U)
    Q, L, U = batch()
    L[0, :] = -osqp.INFTY                             # two-sided -> one-sided: the same class, accepted
    check(Q, L, U)
    # the class is decided on the scaled bounds: row 0 has E = 0.5, so a gap of 1.5e-4 is an equality there
    Q, L, U = batch()
    U[0, 0] = L[0, 0] + 1.5e-4
    with pytest.raises(ValueError, match=r"member 0, row 0 "):
        check(Q, L, U)
