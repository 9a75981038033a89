"""A kept osqp problem without a GPU: the restatement tests/osqp_session_numpy.py itself (polish decisions and active counts on
the cases of DESIGN section 11, the polished point against exact optima, the algebra of update / warm start / cold start), the
argument checks of the new kvx_admm_* entry points, and the argument checks of osqp.Problem."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import osqp_numpy as R  # noqa: E402
import osqp_session_numpy as N  # noqa: E402

from kvxopt_amd import _lib, osqp  # noqa: E402
from kvxopt_amd.base import matrix, spmatrix  # noqa: E402

CASES = {"basic": R.case_basic, "qp_grid_6_5": lambda: R.case_qp_grid(6, 5), "lp_grid_std_6_5": lambda: R.case_lp_grid_std(6, 5),
         "generated_P": lambda: R.case_generated(True), "lp_grid_6_5": lambda: R.case_lp_grid(6, 5),
         "lp_grid_eq_6_5_3": lambda: R.case_lp_grid_eq(6, 5, 3), "generated_noP": lambda: R.case_generated(False)}
POLISH = {"polish": 1}


def sp(M):
    return spmatrix.from_ccs(*R.to_ccs(np.asarray(M, dtype=np.float64)))


def vec(v):
    return matrix(np.asarray(v, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def polished(name, dtype):
    """(status, x, y, info, smallest margin of the loop's decisions, margin of the polish decision) of a default run with polish."""
    S = N.new_session(CASES[name](), POLISH, dtype)
    margins, pm = [], []
    status, x, y, info = N.session_solve(S, POLISH, margins, pm)
    return status, x, y, info, min(margins), pm


# the decisions of the CPU sketch the feature was specified with: status_polish and the number of active rows
WANT = {"basic": (1, 2), "qp_grid_6_5": (1, 19), "lp_grid_std_6_5": (1, 120), "generated_P": (1, 46), "lp_grid_6_5": (-1, 29),
        "lp_grid_eq_6_5_3": (1, None)}


@pytest.mark.parametrize("name", list(WANT))
def test_restatement_polish_decisions(name):
    status, x, y, info, margin, pm = polished(name, np.float64)
    print("%s: %s, polish %d, active %d + %d, residuals %.3e %.3e -> %.3e %.3e; loop margin %.2e, decision margin %.2e"
          % (name, status, info["status_polish"], info["active_lower"], info["active_upper"], info["pri_res"], info["dua_res"],
             info["pri_res_polish"], info["dua_res_polish"], margin, pm[0]))
    assert status == "solved" and info["factorisations"] == 2          # the setup and the polish; no rho update in these runs
    assert margin >= 1e-6 and len(pm) == 1 and pm[0] >= 1e-6           # no decision within rounding of its threshold
    want, active = WANT[name]
    assert info["status_polish"] == want
    if active is not None:
        assert info["active_lower"] + info["active_upper"] == active
    ld = polished(name, np.longdouble)[3]
    assert (ld["status_polish"], ld["active_lower"], ld["active_upper"]) == (want, info["active_lower"], info["active_upper"])


def test_restatement_polish_ill_posed_cases():
    """lp_grid(6, 5): 29 active rows for 30 unknowns, the polished point is far from feasible and is rejected.
    lp_grid_eq(6, 5, 3): accepted on an inconsistent active set -- the refinement cannot bring |e2| down and yh grows."""
    info = polished("lp_grid_6_5", np.float64)[3]
    print("lp_grid: polished primal residual %.3e" % info["pri_res_polish"])
    assert info["pri_res_polish"] > 1e3 * info["pri_res"] and info["status_polish"] == -1
    S = N.new_session(CASES["lp_grid_eq_6_5_3"](), POLISH)
    R.run(S, N.settings(POLISH))
    out = S.polish(1e-6, 3)
    print("lp_grid_eq: |e2| %.3e, |yh| %.3e" % (out[10], np.abs(S.yh).max()))
    assert 1e-4 < out[10] < 1e-2 and np.abs(S.yh).max() > 1e3


def test_restatement_does_not_polish_an_infeasible_problem():
    status, x, y, info = polished("generated_noP", np.float64)[:4]
    assert status == "dual infeasible" and info["status_polish"] == 0 and info["factorisations"] == 1 and info["active_lower"] is None
    p = CASES["generated_noP"]()
    ref = R.solve(p["P"], p["q"], p["A"], p["l"], p["u"])
    assert ref[0] == status and np.array_equal(ref[1], x) and np.array_equal(ref[2], y)


@pytest.mark.parametrize("name", ["basic", "qp_grid_6_5", "lp_grid_std_6_5", "generated_P"])
def test_polished_point_is_closer_to_the_optimum(name):
    """On the well-posed accepted cases the polished x, y are closer than the ADMM x, y (default eps = 1e-3) to the exact
    optimum: golden G25 for `basic`, the polished longdouble run for the others."""
    p = CASES[name]()
    status, x, y, info = polished(name, np.float64)[:4]
    assert info["status_polish"] == 1
    _, xa, ya, _, _ = R.solve(p["P"], p["q"], p["A"], p["l"], p["u"])
    if name == "basic":
        B = R.golden()["basic"]
        xr, yr = np.array(B["x"]), np.array(B["y"])
    else:
        xr, yr = polished(name, np.longdouble)[1:3]
    ex, ey, eax, eay = np.abs(x - xr).max(), np.abs(y - yr).max(), np.abs(xa - xr).max(), np.abs(ya - yr).max()
    print("%s: |x - x*| %.3e (ADMM %.3e), |y - y*| %.3e (ADMM %.3e)" % (name, ex, eax, ey, eay))
    assert ex < eax and ey < eay
    if name == "basic":
        assert ex < 1e-8 and ey < 1e-8 + 5e-9               # the golden multipliers carry eight decimals


def test_restatement_update_algebra():
    p = CASES["generated_P"]()
    S = N.new_session(p)
    S.iterate(10)
    rng = np.random.default_rng(11)
    q2 = p["q"] + 0.1 * rng.standard_normal(S.n)
    assert S.update(q=q2) is False and S.nfact == 1
    assert np.array_equal(S.qb, (S.c * S.D) * q2)
    u2 = p["u"].copy()
    u2[60:70] += 0.5                                        # one-sided rows stay one-sided
    assert S.update(u=u2) is False and S.nfact == 1 and np.array_equal(S.ub[60:70], S.E[60:70] * u2[60:70])
    assert np.all(S.ub[40:50] == R.INFTY) and np.all(S.lb[40:50] == -R.INFTY)
    l2 = p["l"].copy()
    l2[60] = u2[60]                                         # a one-sided row becomes an equality: one factorisation, same rho
    rho = S.rho
    assert S.update(l=l2) is True and S.nfact == 2 and S.rho == rho and S.rv[60] == 1e3 * rho
    l2[41] = -1.0                                           # a free row gains a bound
    assert S.update(l=l2) is True and S.nfact == 3 and S.rv[41] == rho and S.rv[42] == 1e-6
    l2[12] = u2[12] + 1.0
    before = (S.lb.copy(), S.ub.copy(), S.nfact)
    with pytest.raises(ValueError):
        S.update(l=l2)
    assert np.array_equal(before[0], S.lb) and np.array_equal(before[1], S.ub) and before[2] == S.nfact


def test_restatement_warm_and_cold_start():
    p = CASES["qp_grid_6_5"]()
    S = N.new_session(p)
    S.iterate(30)
    x, y = S.solution(0)
    T = N.new_session(p)
    T.warm_start(x, y)
    # out through the scaling and back: a handful of roundings
    assert np.abs(T.x - S.x).max() <= 1e-15 * np.abs(S.x).max() and np.abs(T.y - S.y).max() <= 1e-15 * np.abs(S.y).max()
    assert np.array_equal(T.z, T.A_(T.x)) and not T.dx.any() and not T.dy.any()
    T.warm_start(y=2.0 * y)
    assert np.abs(T.y - 2.0 * S.y).max() <= 2e-15 * np.abs(S.y).max() and np.abs(T.x - S.x).max() <= 1e-15 * np.abs(S.x).max()
    S.set_rho(0.7)
    nf = S.nfact
    S.cold_start()
    assert not any(v.any() for v in S.state()) and S.rho == 0.7 and S.nfact == nf
    fresh = N.Session(p["P"], p["q"], p["A"], p["l"], p["u"], rho=0.7)
    S.iterate(5)
    fresh.iterate(5)
    assert all(np.array_equal(a, b) for a, b in zip(S.state(), fresh.state()))


def test_restatement_factor_comes_back():
    p = CASES["generated_P"]()
    S, T = N.new_session(p), N.new_session(p)
    S.iterate(125)
    T.iterate(125)
    S.polish()
    assert S.stale and S.nfact == T.nfact + 1
    S.iterate(0)
    assert S.stale and S.nfact == T.nfact + 1               # nothing to solve: nothing restored
    S.iterate(25)
    T.iterate(25)
    assert not S.stale and S.nfact == T.nfact + 2
    assert all(np.array_equal(a, b) for a, b in zip(S.state(), T.state()))


def test_abi_status_codes_of_the_kept_problem():
    L = _lib.lib()
    p = R.case_generated(True)
    m, n, Ap, Ai, Ax = R.to_ccs(p["A"])
    h = ctypes.c_void_p()
    pi, pd = _lib.pi, _lib.pd
    assert L.kvx_admm_plan(m, n, pi(Ap), pi(Ai), pd(Ax), None, None, None, pd(p["q"]), pd(p["l"]), pd(p["u"]), 10, None, None, None, None,
                           ctypes.byref(h)) == _lib.KVX_OK
    out, x, y, act = np.zeros(16), np.zeros(n), np.zeros(m), np.zeros(m, dtype=np.int64)
    assert L.kvx_admm_update(None, None, None, None) == _lib.KVX_EINVAL
    assert L.kvx_admm_warm_start(None, None, None) == _lib.KVX_EINVAL
    assert L.kvx_admm_cold_start(None) == _lib.KVX_EINVAL
    assert L.kvx_admm_polish(None, 1e-6, 3, pd(out)) == _lib.KVX_EINVAL
    assert L.kvx_admm_polish(h, 0.0, 3, pd(out)) == _lib.KVX_EINVAL
    assert L.kvx_admm_polish(h, 1e-6, -1, pd(out)) == _lib.KVX_EINVAL
    assert L.kvx_admm_polish(h, 1e-6, 3, None) == _lib.KVX_EINVAL
    assert L.kvx_admm_polish_state(None, None, None, None, None) == _lib.KVX_EINVAL
    assert L.kvx_admm_polish_accept(None) == _lib.KVX_EINVAL
    assert L.kvx_admm_solution(h, 3, pd(x), pd(y)) == _lib.KVX_EINVAL           # no polished solution is held
    assert L.kvx_admm_solution(h, 4, pd(x), pd(y)) == _lib.KVX_EINVAL
    # l > u is refused before a device is asked for, in either argument and against the kept other bound; nothing changes
    rho = np.zeros(m)
    assert L.kvx_admm_rho_vector(h, 0.1, pd(rho)) == _lib.KVX_OK
    bad = p["u"].copy()
    bad[25] = p["l"][25] - 1.0                                                  # row 25 is two-sided
    assert L.kvx_admm_update(h, None, None, pd(bad)) == _lib.KVX_EINVAL
    assert b"l <= u" in L.kvx_last_error()
    assert L.kvx_admm_update(h, None, pd(p["u"] + 1.0), None) == _lib.KVX_EINVAL
    assert L.kvx_admm_update(h, pd(p["q"]), pd(p["u"]), pd(p["l"])) == _lib.KVX_EINVAL
    rho2 = np.zeros(m)
    assert L.kvx_admm_rho_vector(h, 0.1, pd(rho2)) == _lib.KVX_OK and np.array_equal(rho, rho2)
    # the device entry points: without a GPU KVX_EDEVICE, with one KVX_EINVAL because kvx_admm_setup_dev has not run
    want = _lib.KVX_EDEVICE if L.kvx_device_count() == 0 else _lib.KVX_EINVAL
    assert L.kvx_admm_update(h, pd(p["q"]), None, None) == want
    assert L.kvx_admm_update(h, None, None, None) == want                       # every pointer may be NULL
    assert L.kvx_admm_update(h, None, pd(p["l"]), pd(p["u"])) == want
    assert L.kvx_admm_warm_start(h, None, None) == want
    assert L.kvx_admm_warm_start(h, pd(x), None) == want
    assert L.kvx_admm_cold_start(h) == want
    assert L.kvx_admm_polish(h, 1e-6, 3, pd(out)) == want
    assert L.kvx_admm_polish(h, 1e-6, 0, pd(out)) == want
    assert L.kvx_admm_polish_state(h, None, None, None, None) == want
    assert L.kvx_admm_polish_state(h, pd(x), pd(y), pd(y), pi(act)) == want
    assert L.kvx_admm_polish_accept(h) == want
    if L.kvx_device_count() == 0:
        assert b"no CPU fallback" in L.kvx_last_error()
    L.kvx_admm_free(h)


def test_problem_argument_errors():
    """osqp.Problem checks what osqp.solve checks (osqp.c:386-422), in its order, with its exception types and texts."""
    A, q, l, u = sp([[1.0, 2.0], [0.0, 1.0], [1.0, 0.0]]), vec([1.0, 1.0]), vec([0.0] * 3), vec([1.0] * 3)
    with pytest.raises(TypeError, match="A must be a sparse 'd' matrix"):
        osqp.Problem(q, matrix(np.ones((3, 2))), l, u)
    with pytest.raises(ValueError, match="m must be a positive integer"):
        osqp.Problem(q, spmatrix([], [], [], (0, 2)), vec([]), vec([]))
    with pytest.raises(ValueError, match="n must be a positive integer"):
        osqp.Problem(vec([]), spmatrix([], [], [], (3, 0)), l, u)
    with pytest.raises(TypeError, match="q must be a matrix with typecode 'd'"):
        osqp.Problem(matrix([1, 1]), A, l, u)
    with pytest.raises(ValueError, match="incompatible dimensions"):
        osqp.Problem(vec([1.0] * 3), A, l, u)
    with pytest.raises(TypeError, match="u must be a matrix with typecode 'd'"):
        osqp.Problem(q, A, l, matrix([1, 1, 1]))
    with pytest.raises(ValueError, match="incompatible dimensions"):
        osqp.Problem(q, A, l, vec([1.0] * 2))
    with pytest.raises(TypeError, match="l must be a matrix with typecode 'd'"):
        osqp.Problem(q, A, None, u)
    with pytest.raises(ValueError, match="P must be a sparse 'd' matrix"):
        osqp.Problem(q, A, l, u, matrix(np.eye(2)))
    with pytest.raises(ValueError, match="incompatible dimensions"):
        osqp.Problem(q, A, l, u, sp(np.eye(3)))
    with pytest.warns(RuntimeWarning, match="Invalid parameter name: bogus"):
        o = osqp._read_options({"polish": True, "delta": 1e-5, "polish_refine_iter": 5, "warm_start": 0, "bogus": 1}, 2)
    assert (o["polish"], o["delta"], o["polish_refine_iter"], o["warm_start"]) == (1, 1e-5, 5, 0)
    with pytest.raises(NotImplementedError, match="polish"):                     # the module-level functions still do not polish
        osqp._settings({"polish": 1})
    if _lib.lib().kvx_device_count() == 0:                                       # no CPU fallback
        with pytest.raises(RuntimeError):
            osqp.Problem(q, A, l, u, options={"polish": True, "verbose": 0})
