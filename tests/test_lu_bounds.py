"""The reference of test_lu_classes_gpu.py holds itself to the bounds it sets (no GPU): the factors and solutions of the CPU oracle
(oracle/klu_oracle.c), and the solutions of LAPACK, on the dense blocks of the listed orders up to 1056 and the three value patterns,
against the entrywise factor and solve bounds of lu_class_child.py; and the helpers notice a lost rank-1 update and a lost interchange."""
import numpy as np
import pytest

from oracle.kvx_oracle import OracleKLU

import lu_class_child as child

ORDERS = [1, 2, 15, 16, 17, 32, 33, 48, 49, 64, 65, 88, 89, 111, 112, 113, 128, 129, 384, 385, 416, 513, 1024, 1025, 1056]


@pytest.mark.parametrize("n", ORDERS)
def test_oracle_and_lapack_meet_the_bounds(n):
    for pattern in "abc":
        if n == 1 and pattern == "b":
            continue                                                   # the zero matrix of order 1 is singular
        name = "d%d%s" % (n, pattern)
        _, cp, ri, v = child.case_matrix(name)
        A = child.to_csc(n, cp, ri, v)
        fa = child.factors_from_oracle(n, OracleKLU(n, cp, ri, v))
        max_l = child.check_structure(fa)
        assert max_l <= (1.0 + 4 * child.U_ROUND) / child.STOL, (name, max_l)
        if pattern == "c":
            assert max_l <= 1.0 and np.array_equal(fa.p, fa.q), name
        if pattern == "b":
            assert np.any(fa.p != fa.q), name
        assert child.factor_ratio(A, fa) <= 1.0, name
        D = A.toarray()
        O = OracleKLU(n, cp, ri, v)
        for nrhs in (1, 3):
            b = child.rhs(n, nrhs)
            for trans in "NT":
                assert child.solve_ratio(fa, b, O.solve(b, trans), trans) <= 1.0, (name, trans, nrhs)
                assert child.solve_ratio(fa, b, np.linalg.solve(D if trans == "N" else D.T, b), trans) <= 1.0, (name, trans, nrhs, "lapack")


def test_bounds_notice_a_lost_update_and_a_lost_interchange():
    n = 129
    _, cp, ri, v = child.case_matrix("d129a")
    A = child.to_csc(n, cp, ri, v)
    fa = child.factors_from_oracle(n, OracleKLU(n, cp, ri, v))
    assert child.factor_ratio(A, fa) <= 1.0
    U2 = fa.U.tolil(copy=True)
    U2[40, 100] += fa.L[40, 7] * fa.U[7, 100]                          # one term of one rank-1 update left out
    lost = child.Factors(n, fa.L, U2.tocsc(), fa.F, fa.p, fa.q, fa.rs)
    assert child.factor_ratio(A, lost) > 1.0
    p2 = fa.p.copy(); p2[[5, 77]] = p2[[77, 5]]                        # one interchange not recorded
    assert child.factor_ratio(A, child.Factors(n, fa.L, fa.U, fa.F, p2, fa.q, fa.rs)) > 1.0
    b = child.rhs(n, 1)
    x = OracleKLU(n, cp, ri, v).solve(b)
    x[3] *= 1.0 + 1e-9
    assert child.solve_ratio(fa, b, x, "N") > 1.0
    # values that are not numbers miss every bound (a NaN compares false: it must not count as a zero error)
    import pytest
    for bad in (np.nan, np.inf):
        Un = fa.U.copy(); Un.data = Un.data.copy(); Un.data[Un.data.size // 2] = bad
        nan_u = child.Factors(n, fa.L, Un, fa.F, fa.p, fa.q, fa.rs)
        assert child.factor_ratio(A, nan_u) > 1.0 and child.solve_ratio(nan_u, b, OracleKLU(n, cp, ri, v).solve(b), "N") > 1.0
        with pytest.raises(AssertionError):
            child.check_structure(nan_u)
        Ua = fa.U.copy(); Ua.data = np.full_like(Ua.data, bad)
        assert child.factor_ratio(A, child.Factors(n, fa.L, Ua, fa.F, fa.p, fa.q, fa.rs)) > 1.0
        for trans in "NT":
            xn = OracleKLU(n, cp, ri, v).solve(b, trans); xn[11] = bad
            assert child.solve_ratio(fa, b, xn, trans) > 1.0
            assert child.solve_ratio(fa, b, np.full_like(xn, bad), trans) > 1.0
    assert child.worst_ratio(np.array([0.0, np.nan]), np.array([1.0, 1.0])) == np.inf
    assert child.worst_ratio(np.array([0.0, 1.0]), np.array([0.0, np.nan])) == np.inf
    assert child.worst_ratio(np.array([0.0, 0.5]), np.array([0.0, 1.0])) == 0.5


def test_pattern_e_interchanges_once_in_the_oracle_too():
    """the one-interchange matrix does what its name says under plain partial pivoting with the same threshold"""
    for n in (129, 1056):
        _, cp, ri, v = child.case_matrix("d%de" % n)
        fa = child.factors_from_oracle(n, OracleKLU(n, cp, ri, v))
        assert child.check_structure(fa) <= 1.0
        assert np.flatnonzero(fa.p != fa.q).tolist() == [child.ONE_SWAP[0], n + child.ONE_SWAP[1]]
        assert child.factor_ratio(child.to_csc(n, cp, ri, v), fa) <= 1.0


def test_panel_width_schedule():
    assert child.panel_steps(1024, 1024) == {"panel_reg32": 32, "panel_reg16": 0, "panel_reg8": 0, "panel_lds": 0}
    assert child.panel_steps(1025, 1025) == {"panel_reg32": 32, "panel_reg16": 1, "panel_reg8": 0, "panel_lds": 0}      # 16, then 1009 rows
    assert child.panel_steps(1056, 1056) == {"panel_reg32": 32, "panel_reg16": 2, "panel_reg8": 0, "panel_lds": 0}
    assert child.panel_steps(2080, 2080) == {"panel_reg32": 32, "panel_reg16": 64, "panel_reg8": 4, "panel_lds": 0}
    assert child.panel_steps(4100, 4100)["panel_lds"] == 1
    assert [child.lds_T(m) for m in (1, 16, 17, 32, 33, 48, 49, 64, 65, 88, 89, 112)] == [1, 1, 2, 2, 3, 3, 4, 4, 6, 6, 7, 7]
