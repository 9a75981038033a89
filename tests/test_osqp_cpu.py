"""kvxopt_amd.osqp without a GPU: the argument checks of osqp.c, the options, resize_problem, the host plan of kvx_admm_plan
(scaling, pattern of S, rho classes) against tests/osqp_numpy.py, the status codes of the device entry points, and the
restatement itself on the known answers of the reference's tests/test_osqp.py (golden G25)."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import osqp_numpy as R  # noqa: E402

from kvxopt_amd import _lib, osqp, solvers  # noqa: E402
from kvxopt_amd.base import matrix, spmatrix  # noqa: E402

G25 = R.golden()


def sp(M):
    return spmatrix.from_ccs(*R.to_ccs(np.asarray(M, dtype=np.float64)))


def vec(v):
    return matrix(np.asarray(v, dtype=np.float64))


def plan(p, scaling=10):
    Pcc = None if p["P"] is None else R.to_ccs(np.tril(p["P"]))[2:]
    return osqp._Solver(p["q"], R.to_ccs(p["A"]), p["l"], p["u"], Pcc, scaling)


CASES = {"basic": R.case_basic, "qp_grid_3_2": lambda: R.case_qp_grid(3, 2), "lp_grid_eq_6_5_3": lambda: R.case_lp_grid_eq(6, 5, 3),
         "generated_noP": lambda: R.case_generated(False), "generated_P": lambda: R.case_generated(True)}


def test_solve_argument_errors():
    """osqp.c:386-422, in its order, with its exception types and texts."""
    A, q, l, u = sp([[1.0, 2.0], [0.0, 1.0], [1.0, 0.0]]), vec([1.0, 1.0]), vec([0.0] * 3), vec([1.0] * 3)
    with pytest.raises(TypeError, match="A must be a sparse 'd' matrix"):
        osqp.solve(q, matrix(np.ones((3, 2))), l, u)
    with pytest.raises(ValueError, match="m must be a positive integer"):
        osqp.solve(q, spmatrix([], [], [], (0, 2)), vec([]), vec([]))
    with pytest.raises(ValueError, match="n must be a positive integer"):
        osqp.solve(vec([]), spmatrix([], [], [], (3, 0)), l, u)
    with pytest.raises(TypeError, match="q must be a matrix with typecode 'd'"):
        osqp.solve(matrix([1, 1]), A, l, u)
    with pytest.raises(TypeError, match="q must be a matrix with typecode 'd'"):
        osqp.solve([1.0, 1.0], A, l, u)
    with pytest.raises(ValueError, match="incompatible dimensions"):
        osqp.solve(vec([1.0] * 3), A, l, u)
    with pytest.raises(TypeError, match="u must be a matrix with typecode 'd'"):
        osqp.solve(q, A, l, matrix([1, 1, 1]))
    with pytest.raises(ValueError, match="incompatible dimensions"):
        osqp.solve(q, A, l, vec([1.0] * 2))
    with pytest.raises(TypeError, match="l must be a matrix with typecode 'd'"):
        osqp.solve(q, A, None, u)
    with pytest.raises(ValueError, match="incompatible dimensions"):
        osqp.solve(q, A, matrix(np.zeros((3, 2))), u)
    with pytest.raises(ValueError, match="P must be a sparse 'd' matrix"):
        osqp.solve(q, A, l, u, matrix(np.eye(2)))
    with pytest.raises(ValueError, match="incompatible dimensions"):
        osqp.solve(q, A, l, u, sp(np.eye(3)))


def test_qp_argument_errors():
    """osqp.c:455-508."""
    G, h, q = sp([[1.0, 2.0], [0.0, 1.0], [1.0, 0.0]]), vec([1.0] * 3), vec([1.0, 1.0])
    with pytest.raises(TypeError, match="G must be a sparse 'd' matrix"):
        osqp.qp(q, np.ones((3, 2)), h)
    with pytest.raises(ValueError, match="m must be a positive integer"):
        osqp.qp(q, spmatrix([], [], [], (0, 2)), vec([]))
    with pytest.raises(TypeError, match="h must be a matrix with typecode 'd'"):
        osqp.qp(q, G, matrix([1, 1, 1]))
    with pytest.raises(ValueError, match="incompatible dimensions"):
        osqp.qp(q, G, vec([1.0] * 4))
    with pytest.raises(TypeError, match="q must be a matrix with typecode 'd'"):
        osqp.qp(matrix([1, 1]), G, h)
    with pytest.raises(ValueError, match="incompatible dimensions"):
        osqp.qp(vec([1.0]), G, h)
    with pytest.raises(ValueError, match="A must be a sparse 'd' matrix"):
        osqp.qp(q, G, h, matrix(np.ones((1, 2))), vec([1.0]))
    with pytest.raises(ValueError, match="incompatible dimensions"):
        osqp.qp(q, G, h, sp(np.ones((1, 3))), vec([1.0]))
    with pytest.raises(TypeError, match="b must be a matrix with typecode 'd'"):
        osqp.qp(q, G, h, sp(np.ones((1, 2))), matrix([1]))
    with pytest.raises(ValueError, match="incompatible dimensions"):
        osqp.qp(q, G, h, sp(np.ones((1, 2))), vec([1.0, 2.0]))
    with pytest.raises(ValueError, match="P must be a sparse 'd' matrix"):
        osqp.qp(q, G, h, P=matrix(np.eye(2)))
    with pytest.raises(ValueError, match="P must be square matrix of n x n"):
        osqp.qp(q, G, h, P=sp(np.eye(3)))


def test_options():
    """An unknown key warns and is ignored (osqp.c:263-266); options=None reads osqp.options; polish raises."""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        o = osqp._settings({"max_iter": 7, "eps_abs": 1, "bogus": 3, "linsys_solver": 1, "time_limit": 2.0, "warm_start": True})
    assert [str(x.message) for x in w] == ["Invalid parameter name: bogus"]
    assert o["max_iter"] == 7 and o["eps_abs"] == 1.0 and "bogus" not in o and o["rho"] == 0.1 and o["alpha"] == 1.6
    assert o["sigma"] == 1e-6 and o["check_termination"] == 25 and o["eps_prim_inf"] == o["eps_dual_inf"] == 1e-4 and o["scaling"] == 10
    saved = dict(osqp.options)
    try:
        osqp.options["max_iter"] = 11
        assert osqp._settings(None)["max_iter"] == 11
    finally:
        osqp.options.clear()
        osqp.options.update(saved)
    with pytest.raises(NotImplementedError, match="polish"):
        osqp._settings({"polish": 1})
    with pytest.raises(NotImplementedError, match="polish"):
        osqp.solve(vec([1.0]), sp([[1.0]]), vec([0.0]), vec([1.0]), options={"polish": True})
    assert osqp._settings({"polish": False})["polish"] == 0


def test_resize_problem():
    rng = np.random.default_rng(3)
    G = rng.standard_normal((5, 4)) * (rng.random((5, 4)) < 0.6)
    A = rng.standard_normal((2, 4)) * (rng.random((2, 4)) < 0.7)
    h, b = rng.standard_normal(5), rng.standard_normal(2)
    (m, n, cp, ri, vx), l, u = osqp.resize_problem(R.to_ccs(G), h, R.to_ccs(A), b)
    As, ls, us = R.stack_qp(G, h, A, b)
    assert (m, n) == As.shape and np.array_equal(R.dense(m, n, cp, ri, vx), As) and np.array_equal(l, ls) and np.array_equal(u, us)
    assert all(np.all(np.diff(ri[cp[j]:cp[j + 1]]) > 0) for j in range(n))
    (m, n, cp, ri, vx), l, u = osqp.resize_problem(R.to_ccs(G), h, None, None)
    assert np.array_equal(R.dense(m, n, cp, ri, vx), G) and np.all(l == -1e30) and np.array_equal(u, h)


@pytest.mark.parametrize("scaling", [0, 1, 10])
@pytest.mark.parametrize("name", list(CASES))
def test_plan_scaling(name, scaling):
    """D, E, c of kvx_admm_plan against the restatement: the same arithmetic in the same order."""
    p = CASES[name]()
    S = plan(p, scaling)
    D, E, c = R.ruiz(np.zeros((S.n, S.n)) if p["P"] is None else p["P"], p["q"], p["A"], scaling)[:3]
    assert np.abs(S.D / D - 1).max() <= 1e-14 and np.abs(S.E / E - 1).max() <= 1e-14 and abs(S.c / c - 1) <= 1e-14
    if scaling == 0:
        assert np.all(S.D == 1) and np.all(S.E == 1) and S.c == 1
    S.close()


@pytest.mark.parametrize("name", list(CASES))
def test_plan_pattern(name):
    p = CASES[name]()
    S = plan(p)
    n = S.n
    Sp, Si = S.pattern()
    got = np.zeros((n, n), dtype=bool)
    got[Si, np.repeat(np.arange(n), np.diff(Sp))] = True
    nzA = (p["A"] != 0).astype(np.int64)
    want = np.eye(n, dtype=bool) | (nzA.T @ nzA > 0)
    if p["P"] is not None:
        want |= p["P"] != 0
    assert np.array_equal(got, np.tril(want)) and S.snz == Si.size == np.tril(want).sum()
    assert all(np.all(np.diff(Si[Sp[j]:Sp[j + 1]]) > 0) for j in range(n))
    S.close()


def test_rho_classes():
    p = {"P": None, "q": np.ones(2), "A": np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [1.0, -1.0], [2.0, 1.0]]),
         "l": np.array([1.0, -1.0, -1e30, -2e26, 3.0]), "u": np.array([1.0, 1.0, 4.0, 1e30, 1e27])}
    S = plan(p, 0)
    assert np.array_equal(S.rho_vector(0.1), [100.0, 0.1, 0.1, 1e-6, 0.1])      # equality, two-sided, one-sided, free, one-sided
    assert np.array_equal(S.rho_vector(1e9), [1e9, 1e6, 1e6, 1e-6, 1e6])        # rho clipped to [1e-6, 1e6]
    S.close()
    for name in ("generated_noP", "lp_grid_eq_6_5_3"):
        q = CASES[name]()
        S = plan(q)
        ref = R.Admm(q["P"], q["q"], q["A"], q["l"], q["u"])
        assert np.array_equal(S.rho_vector(0.1), R.rho_vector(ref.lb64, ref.ub64, 0.1))
        S.close()
    q = CASES["generated_noP"]()
    S = plan(q)
    assert sorted(np.unique(S.rho_vector(0.1))) == [1e-6, 0.1, 100.0]
    assert (S.info()["short_rows"], S.info()["long_rows"]) == (256, 1)          # the row of 64 entries is summed by a wavefront
    S.close()


def test_abi_status_codes():
    L = _lib.lib()
    p = R.case_basic()
    m, n, Ap, Ai, Ax = R.to_ccs(p["A"])
    h = ctypes.c_void_p()
    pi, pd = _lib.pi, _lib.pd
    args = (pi(Ap), pi(Ai), pd(Ax), None, None, None, pd(p["q"]), pd(p["l"]), pd(p["u"]), 10, None, None, None, None)
    assert L.kvx_admm_plan(m, n, *args, None) == _lib.KVX_EINVAL
    assert L.kvx_admm_plan(0, n, *args, ctypes.byref(h)) == _lib.KVX_EINVAL
    assert L.kvx_admm_plan(m, n, None, *args[1:], ctypes.byref(h)) == _lib.KVX_EINVAL
    assert L.kvx_admm_plan(m, n, *args[:9], -1, None, None, None, None, ctypes.byref(h)) == _lib.KVX_EINVAL
    assert L.kvx_admm_plan(m - 1, n, *args, ctypes.byref(h)) == _lib.KVX_EINVAL  # row index out of range
    bad = np.array([0, 3, 2], dtype=np.int64)
    assert L.kvx_admm_plan(m, n, pi(bad), *args[1:], ctypes.byref(h)) == _lib.KVX_EINVAL
    assert L.kvx_admm_plan(m, n, *args[:7], pd(p["u"]), pd(p["l"]), *args[9:], ctypes.byref(h)) == _lib.KVX_EINVAL   # l > u
    assert L.kvx_admm_plan(m, n, *args, ctypes.byref(h)) == _lib.KVX_OK
    out = np.zeros(24)
    assert L.kvx_admm_iterate(None, 1, pd(out)) == _lib.KVX_EINVAL
    assert L.kvx_admm_iterate(h, -1, pd(out)) == _lib.KVX_EINVAL
    assert L.kvx_admm_iterate(h, 1, None) == _lib.KVX_EINVAL
    assert L.kvx_admm_setup_dev(None, 1e-6, 0.1, 1.6) == _lib.KVX_EINVAL
    assert L.kvx_admm_setup_dev(h, 0.0, 0.1, 1.6) == _lib.KVX_EINVAL
    assert L.kvx_admm_setup_dev(h, 1e-6, 0.1, 2.0) == _lib.KVX_EINVAL
    assert L.kvx_admm_set_rho(h, -1.0) == _lib.KVX_EINVAL
    assert L.kvx_admm_state(None, None, None, None, None, None) == _lib.KVX_EINVAL
    assert L.kvx_admm_solution(h, 3, pd(out), pd(out)) == _lib.KVX_EINVAL
    assert L.kvx_admm_solution(h, 0, None, pd(out)) == _lib.KVX_EINVAL
    assert L.kvx_admm_info(h, None) == _lib.KVX_EINVAL
    assert L.kvx_admm_rho_vector(h, 0.1, None) == _lib.KVX_EINVAL
    if L.kvx_device_count() == 0:                                               # no CPU fallback
        assert L.kvx_admm_setup_dev(h, 1e-6, 0.1, 1.6) == _lib.KVX_EDEVICE
        assert b"no CPU fallback" in L.kvx_last_error()
        assert L.kvx_admm_iterate(h, 1, pd(out)) == _lib.KVX_EDEVICE
        assert L.kvx_admm_set_rho(h, 0.2) == _lib.KVX_EDEVICE
        assert L.kvx_admm_state(h, None, None, None, None, None) == _lib.KVX_EDEVICE
        assert L.kvx_admm_solution(h, 0, pd(out), pd(out)) == _lib.KVX_EDEVICE
        with pytest.raises(RuntimeError):
            osqp.solve(vec(p["q"]), sp(p["A"]), vec(p["l"]), vec(p["u"]), options={"verbose": 0})
    L.kvx_admm_free(h)
    L.kvx_admm_free(None)


def test_other_solvers_still_raise():
    L = G25["lp"]
    c, G, h = vec(L["c"]), sp(L["G"]), vec(L["h"])
    P = sp(np.eye(2))
    with pytest.raises(NotImplementedError):
        solvers.qp(P, c, G, h, solver="mosek")
    with pytest.raises(NotImplementedError):
        solvers.lp(c, G, h, solver="glpk")
    for call in (lambda: solvers.conelp(c, G, h, solver="osqp"), lambda: solvers.coneqp(P, c, G, h, solver="osqp"),
                 lambda: solvers.socp(c, G, h, solver="osqp"), lambda: solvers.sdp(c, G, h, solver="osqp")):
        with pytest.raises(NotImplementedError):
            call()


def test_restatement_reaches_the_known_answers():
    """The five solves of the reference's tests/test_osqp.py at its options, by the restatement: solved, errors below 1e-8, and
    the iteration counts of the sketch the issue was written with."""
    o, want = G25["options"], G25["sketch_iterations"]
    L, Q, Q2, B = G25["lp"], G25["qp"], G25["qp2"], G25["basic"]
    runs = {"lp": (R.from_qp(None, L["c"], L["G"], L["h"]), L["x"], L["z"] + L["y"]),
            "lp_eq": (R.from_qp(None, L["c"], L["G"], L["h"], L["A"], L["b"]), L["x_eq"], L["z_eq"] + L["y_eq"]),
            "qp": (R.from_qp(Q["P"], Q["q"], Q["G"], Q["h"]), Q["x"], Q["z"] + Q["y"]),
            "qp2": (R.from_qp(Q2["P"], Q2["q"], Q2["G"], Q2["h"], Q2["A"], Q2["b"]), Q2["x"], Q2["z"] + Q2["y"]),
            "basic": (R.case_basic(), B["x"], None)}
    for name, (p, x, y) in runs.items():
        status, xs, ys, it, nf = R.solve(p["P"], p["q"], p["A"], p["l"], p["u"], o)
        assert (status, it, nf) == ("solved", want[name], 1), name
        assert np.abs(xs - x).max() < 1e-8
        if y is not None:
            assert np.abs(ys - y).max() < 1e-7
        else:
            assert np.abs(ys - B["y"]).max() < 1e-8 + 5e-9                       # the golden multipliers carry eight decimals


@pytest.mark.parametrize("name,want", [("qp_grid_6_5", (75, 1)), ("lp_grid_6_5", (325, 1)), ("lp_grid_std_6_5", (200, 1)),
                                       ("lp_grid_eq_6_5_3", (200, 1)), ("qp_grid_40_30", (150, 2))])
def test_restatement_decides_with_a_margin(name, want):
    """The cases of the GPU termination test at default options: the restatement's status, iterations and factorisations, and
    no decision (termination test, adoption of a new rho) within 1e-6 relative of its threshold -- so the device, whose numbers
    differ in the last digits, must take the same decisions.  (qp_grid(40, 30) at eps 1e-8, 1125 iterations, is checked the same
    way inside the GPU test, which needs that run anyway.)"""
    p = {"qp_grid_6_5": lambda: R.case_qp_grid(6, 5), "lp_grid_6_5": lambda: R.case_lp_grid(6, 5),
         "lp_grid_std_6_5": lambda: R.case_lp_grid_std(6, 5), "lp_grid_eq_6_5_3": lambda: R.case_lp_grid_eq(6, 5, 3),
         "qp_grid_40_30": lambda: R.case_qp_grid(40, 30)}[name]()
    margins = []
    status, x, y, it, nf = R.solve(p["P"], p["q"], p["A"], p["l"], p["u"], None, margins=margins)
    assert status == "solved" and (it, nf) == want and min(margins) >= 1e-6


def test_restatement_certificates():
    I = R.INFTY
    cases = [(None, [0.0], [[1.0], [1.0]], [-I, 1.0], [-1.0, I], "primal infeasible"),
             (None, [0.0, 0.0], [[1.0, 1.0], [1.0, 0.0], [0.0, 1.0]], [-I, 0.0, 0.0], [-1.0, I, I], "primal infeasible"),
             (None, [-1.0], [[1.0]], [0.0], [I], "dual infeasible"),
             ([[1.0, 0.0], [0.0, 0.0]], [-1.0, -1.0], [[1.0, -1.0], [1.0, 0.0], [0.0, 1.0]], [-I, 0.0, 0.0], [1.0, I, I], "dual infeasible")]
    for P, q, A, l, u, want in cases:
        for o in ({"check_termination": 1}, None):
            status, x, y, it, nf = R.solve(P, np.array(q), np.array(A), np.array(l), np.array(u), o)
            assert status == want and it <= 100
