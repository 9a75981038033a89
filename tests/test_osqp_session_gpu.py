"""A kept osqp problem on the device (kvx_admm_update / warm_start / cold_start / polish, osqp.Problem) against
tests/osqp_session_numpy.py, the numpy restatement of DESIGN section 11, "A kept problem".

Bounds.  Parity (tests 2, 6): the device's distance to the longdouble restatement is at most 4 x the float64 restatement's own
distance to it, with a floor of 1e-13 of the vector's infinity norm -- the rule of test_osqp_gpu.test_iterate_parity, whose
`compare` is used as it is where a whole ADMM state is compared.  The polished residuals of `out` are compared at the point the
device holds, each with a floor of 1e-13 of the largest infinity norm among the vectors it is the (cancelling) sum of, the two
objective terms with 1e-13 of the sum of the absolute values of their terms.  Active set (test 1), rejected answers, restored
factors and repeated runs: exact.  Decisions (tests 3, 6): those of the float64 restatement, which takes none within 1e-6 of a
threshold.  Every measured figure is printed before its assertion; DESIGN section 11 records them.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import osqp_numpy as R  # noqa: E402
import osqp_session_numpy as N  # noqa: E402
import test_osqp_gpu as G0  # noqa: E402  (compare, device, sp, vec: the helpers of the iteration's own tests)

from kvxopt_amd import _lib, osqp  # noqa: E402

pytestmark = pytest.mark.gpu

QUIET = {"verbose": 0}
POLISH = {"verbose": 0, "polish": 1}
CASES = {"basic": R.case_basic, "qp_grid_6_5": lambda: R.case_qp_grid(6, 5), "lp_grid_std_6_5": lambda: R.case_lp_grid_std(6, 5),
         "generated_P": lambda: R.case_generated(True), "lp_grid_6_5": lambda: R.case_lp_grid(6, 5),
         "lp_grid_eq_6_5_3": lambda: R.case_lp_grid_eq(6, 5, 3), "generated_noP": lambda: R.case_generated(False)}
WELL_POSED = ["basic", "qp_grid_6_5", "lp_grid_std_6_5", "generated_P"]
ACCEPTED = WELL_POSED + ["lp_grid_eq_6_5_3"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def problem(p, opts):
    P = None if p["P"] is None else G0.sp(np.tril(p["P"]))
    return osqp.Problem(G0.vec(p["q"]), G0.sp(p["A"]), G0.vec(p["l"]), G0.vec(p["u"]), P, options=opts)


def plain_solve(p, opts):
    P = None if p["P"] is None else G0.sp(np.tril(p["P"]))
    return osqp.solve(G0.vec(p["q"]), G0.sp(p["A"]), G0.vec(p["l"]), G0.vec(p["u"]), P, options=opts)


@functools.lru_cache(maxsize=None)
def device_polished(name):
    """One default run with polish on the device: (status, x, y, info)."""
    with problem(case(name), POLISH) as Q:
        status, x, y = Q.solve()
        return status, x, y, dict(Q.info)


@functools.lru_cache(maxsize=None)
def restated_polished(name):
    S = N.new_session(case(name), POLISH)
    margins, pm = [], []
    return N.session_solve(S, POLISH, margins, pm) + (min(margins + pm),)


def parity(tag, name, dev, own, ref, scale):
    """One line of the 4 x rule: dev, own (float64 restatement), ref (longdouble) are vectors or numbers."""
    ref = np.atleast_1d(np.asarray(ref, dtype=np.longdouble))
    err = float(np.abs(np.atleast_1d(np.asarray(dev, dtype=np.longdouble)) - ref).max())
    mine = float(np.abs(np.atleast_1d(np.asarray(own, dtype=np.longdouble)) - ref).max())
    bound = max(4.0 * mine, 1e-13 * scale)
    print("%s %-8s device-vs-longdouble %.3e  float64-vs-longdouble %.3e  bound %.3e  ratio %.3f" % (tag, name, err, mine, bound, err / bound if bound else 0.0))
    assert err <= bound, (tag, name, err, mine, bound)


# ---- 1, 2. active set and polish parity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WELL_POSED)
def test_polish_parity(name):
    """The loop at default options on the device, then one polish (delta 1e-6, 3 refinement passes).  The flags equal those
    numpy computes from the device's own state and scaled bounds (two subtractions and a comparison: exact).  Both restatements
    polish from the device's ADMM state; xh, zh, yh by the 4 x rule, the residual numbers of `out` at the point the device holds."""
    p = case(name)
    S = G0.device(p, 10)
    try:
        o = osqp._read_options(QUIET, 2)
        status, it = osqp._run(S, o)
        assert status == "solved"
        x, z, y, dx, dy = S.state()
        nf = S.info()["factorisations"]
        out = S.polish(1e-6, 3)
        xh, zh, yh, act = S.polish_state()
        assert out[0] == 1 and S.info()["factorisations"] == nf + 1
        lb = np.where(p["l"] <= -1e26, -1e30, S.E * p["l"])
        ub = np.where(p["u"] >= 1e26, 1e30, S.E * p["u"])
        lo, up = z - lb < -y, ub - z < y
        assert not (lo & up).any()
        assert np.array_equal(act, np.where(lo, -1, np.where(up, 1, 0)))
        assert (out[1], out[2]) == (lo.sum(), up.sum())
        assert all(np.array_equal(a, b) for a, b in zip(S.state(), (x, z, y, dx, dy)))          # the ADMM state is untouched
        r64, rld = N.new_session(p, QUIET, np.float64), N.new_session(p, QUIET, np.longdouble)
        outs = []
        for T in (r64, rld):
            T.x, T.z, T.y = (np.asarray(v, dtype=T.dtype) for v in (x, z, y))
            outs.append(T.polish(1e-6, 3))
            assert np.array_equal(T.act, act)
        print("%s: %d iterations, active %d + %d, |e1| %.3e |e2| %.3e (restatement %.3e %.3e)"
              % (name, it, out[1], out[2], out[9], out[10], outs[0][9], outs[0][10]))
        for key, g, a, b in (("xh", xh, r64.xh, rld.xh), ("zh", zh, r64.zh, rld.zh), ("yh", yh, r64.yh, rld.yh)):
            parity(name, key, g, a, b, float(np.abs(b).max()))
        v64, vld = r64.polish_numbers(xh, yh)[0], rld.polish_numbers(xh, yh)
        for k, key in enumerate(("pri", "dua", "pri unsc", "dua unsc", "x'Px", "q'x")):
            parity(name, key, out[3 + k], v64[k], vld[0][k], vld[1][k])
    finally:
        S.close()


# ---- 3. decisions -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_polish_decisions(name):
    p = case(name)
    status, x, y, info = device_polished(name)
    rstatus, rx, ry, rinfo, margin = restated_polished(name)
    print("%s: device %s polish %d after %d iterations, %d factorisations, active %s + %s; restatement %s %d %d %d; smallest margin %.2e"
          % (name, status, info["status_polish"], info["iterations"], info["factorisations"], info["active_lower"], info["active_upper"],
             rstatus, rinfo["status_polish"], rinfo["iterations"], rinfo["factorisations"], margin))
    assert margin >= 1e-6
    assert (status, info["status_polish"], info["iterations"], info["factorisations"]) == \
        (rstatus, rinfo["status_polish"], rinfo["iterations"], rinfo["factorisations"])
    assert (info["active_lower"], info["active_upper"]) == (rinfo["active_lower"], rinfo["active_upper"])
    if info["status_polish"] != 1:                                      # rejected or not run: what osqp.solve returns, byte for byte
        pstatus, px, py = plain_solve(p, QUIET)
        assert pstatus == status and px.tobytes() == x.tobytes() and py.tobytes() == y.tobytes()
    if name == "generated_noP":
        assert status == "dual infeasible" and info["status_polish"] == 0 and info["pri_res_polish"] is None
    if name == "lp_grid_6_5":
        assert info["status_polish"] == -1


# ---- 4. honest residuals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ACCEPTED)
def test_polished_residuals_are_honest(name):
    """The unscaled residuals recomputed in longdouble from the returned x, y satisfy the acceptance rule against the loop's."""
    p = case(name)
    status, x, y, info = device_polished(name)
    assert info["status_polish"] == 1
    t = lambda v: np.asarray(v, dtype=np.longdouble)
    A, xl, yl = t(p["A"]), t(x), t(y)
    P = t(np.zeros((x.size, x.size)) if p["P"] is None else p["P"])
    ax = A @ xl
    hp = float(np.abs(ax - np.minimum(np.maximum(ax, t(p["l"])), t(p["u"]))).max())
    hd = float(np.abs(P @ xl + t(p["q"]) + A.T @ yl).max())
    print("%s: loop %.3e %.3e, polished (device) %.3e %.3e, recomputed %.3e %.3e"
          % (name, info["pri_res"], info["dua_res"], info["pri_res_polish"], info["dua_res_polish"], hp, hd))
    assert N.accept(info["pri_res"], info["dua_res"], hp, hd)


# ---- 5. the factor comes back ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["qp_grid_6_5", "generated_P"])
def test_factor_comes_back(name):
    p = case(name)
    S, T = G0.device(p, 10), G0.device(p, 10)
    try:
        S.iterate(100)
        T.iterate(100)
        out = S.polish(1e-6, 3)
        assert out[0] == 1 and S.info()["factorisations"] == T.info()["factorisations"] + 1
        S.iterate(25)
        T.iterate(25)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(S.state(), T.state()))
        assert S.info()["factorisations"] == T.info()["factorisations"] + 2          # the polish and the restore
        S.polish(1e-6, 3)
        S.set_rho(0.7)                                                  # a new rho rebuilds the factor anyway: no restore on top
        T.set_rho(0.7)
        S.iterate(5)
        T.iterate(5)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(S.state(), T.state()))
        assert S.info()["factorisations"] == T.info()["factorisations"] + 3
    finally:
        S.close()
        T.close()


# ---- 6. session -------------------------------------------------------------------------------------------------------------------------
def noisy_q(p):
    return p["q"] + 0.1 * np.random.default_rng(6).standard_normal(p["q"].size)


@pytest.mark.parametrize("warm", [1, 0])
def test_session_follows_the_restatement(warm):
    """qp_grid(6, 5): solve, update(q + 0.1 noise), solve -- status, iterations and factorisations of both solves."""
    p = case("qp_grid_6_5")
    opts = {"verbose": 0, "warm_start": warm}
    T = N.new_session(p, opts)
    margins = []
    with problem(p, opts) as Q:
        for step in range(2):
            if step:
                Q.update(q=G0.vec(noisy_q(p)))
                T.update(q=noisy_q(p))
            status, x, y = Q.solve()
            rstatus, rx, ry, rinfo = N.session_solve(T, opts, margins)
            print("warm_start=%d solve %d: device %s %d iterations %d factorisations; restatement %s %d %d; |x - x_r| %.2e"
                  % (warm, step, status, Q.info["iterations"], Q.info["factorisations"], rstatus, rinfo["iterations"],
                     rinfo["factorisations"], np.abs(x - rx).max()))
            assert (status, Q.info["iterations"], Q.info["factorisations"]) == (rstatus, rinfo["iterations"], rinfo["factorisations"])
            assert Q.info["status_polish"] == 0
    print("smallest margin %.2e" % min(margins))
    assert min(margins) >= 1e-6


def test_cold_session_equals_a_fresh_problem():
    """With adaptive_rho = 0 and warm_start = 0 the second solve equals, byte for byte, a fresh Problem on the updated data.
    The scaling is kept across an update and a fresh plan computes its own from the new q (the cost scaling reads |q|), so
    the two scaled problems coincide only where the scaling does not depend on q: the check runs with scaling = 0."""
    p = case("qp_grid_6_5")
    opts = {"verbose": 0, "warm_start": 0, "adaptive_rho": 0, "scaling": 0}
    q2 = noisy_q(p)
    with problem(p, opts) as Q:
        first = Q.solve()
        Q.update(q=G0.vec(q2))
        second = Q.solve()
        info = dict(Q.info)
    with problem(dict(p, q=q2), opts) as F:
        fresh = F.solve()
        finfo = dict(F.info)
    print(first[0], second[0], info["iterations"], finfo["iterations"])
    assert second[0] == fresh[0] == "solved" and second[1].tobytes() == fresh[1].tobytes() and second[2].tobytes() == fresh[2].tobytes()
    assert (info["iterations"], info["factorisations"]) == (finfo["iterations"], finfo["factorisations"])
    assert first[1].tobytes() != second[1].tobytes()


def test_update_that_changes_a_class():
    """An inequality row becomes an equality (l_i = u_i): one more factorisation, then iterate(25) parity by the 4 x rule."""
    p = case("qp_grid_6_5")
    l2 = p["l"].copy()
    l2[[3, 40]] = p["u"][[3, 40]]
    S = G0.device(p, 10)
    try:
        r64, rld = N.new_session(p, QUIET, np.float64), N.new_session(p, QUIET, np.longdouble)
        for T in (S, r64, rld):
            T.iterate(10)
        S.update(u=p["u"] + 0.25)                                       # every row keeps its class: nothing is factored
        assert S.info()["factorisations"] == 1
        S.update(l=l2, u=p["u"])
        assert S.info()["factorisations"] == 2
        for T in (r64, rld):
            assert T.update(l=l2) is True and T.nfact == 2
        res = S.iterate(25)
        r64.iterate(25)
        rld.iterate(25)
        assert S.info()["factorisations"] == 2
        G0.compare("class change", S.state(), res, r64, rld)
        before = S.state()
        with pytest.raises(ValueError, match="l <= u"):
            S.update(l=p["u"] + 1.0)                                    # refused: the problem is unchanged
        S.iterate(1)
        r64.iterate(1)
        rld.iterate(1)
        assert S.info()["factorisations"] == 2 and S.state()[0].tobytes() != before[0].tobytes()
        G0.compare("after a refused update", S.state(), S.iterate(0), r64, rld)
    finally:
        S.close()


@pytest.mark.parametrize("name", ["qp_grid_6_5", "generated_P"])
def test_warm_start_state_parity(name):
    p = case(name)
    rng = np.random.default_rng(8)
    x0, y0 = rng.standard_normal(p["q"].size), rng.standard_normal(p["l"].size)
    S = G0.device(p, 10)
    try:
        r64, rld = N.new_session(p, QUIET, np.float64), N.new_session(p, QUIET, np.longdouble)
        for T in (S, r64, rld):
            T.iterate(3)                                                # dx, dy are not zero before the warm start
            T.warm_start(x0, y0)
        res = S.iterate(0)
        assert not S.state()[3].any() and not S.state()[4].any()
        G0.compare("%s warm start" % name, S.state(), res, r64, rld)
        xs, ys = S.solution(0)                                          # back through the scaling: a handful of roundings
        assert np.abs(xs - x0).max() <= 1e-15 * np.abs(x0).max() and np.abs(ys - y0).max() <= 1e-15 * np.abs(y0).max()
        kept = S.state()
        for T in (S, r64, rld):
            T.warm_start(y=2.0 * y0)                                    # x, z kept
        assert S.state()[0].tobytes() == kept[0].tobytes() and S.state()[1].tobytes() == kept[1].tobytes()
        G0.compare("%s warm start, y alone" % name, S.state(), S.iterate(0), r64, rld)
        for T in (S, r64, rld):
            T.cold_start()
        assert not any(v.any() for v in S.state())
        res = S.iterate(2)
        r64.iterate(2)
        rld.iterate(2)
        G0.compare("%s cold start" % name, S.state(), res, r64, rld)
    finally:
        S.close()


@pytest.mark.parametrize("name", ["qp_grid_6_5", "generated_P", "generated_noP"])
def test_first_solve_is_osqp_solve(name):
    p = case(name)
    with problem(p, QUIET) as Q:
        status, x, y = Q.solve()
        assert Q.info["status_polish"] == 0
    pstatus, px, py = plain_solve(p, QUIET)
    assert status == pstatus and x.tobytes() == px.tobytes() and y.tobytes() == py.tobytes()


# ---- 7. two runs ------------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes():
    p = case("generated_P")
    runs = []
    for _ in range(2):
        with problem(p, POLISH) as Q:
            a = Q.solve()
            ia = dict(Q.info)
            Q.update(q=G0.vec(noisy_q(p)))
            b = Q.solve()
            ib = dict(Q.info)
        runs.append((a[0], a[1].tobytes(), a[2].tobytes(), sorted(ia.items(), key=str), b[0], b[1].tobytes(), b[2].tobytes(),
                     sorted(ib.items(), key=str)))
    print(runs[0][0], runs[0][3], runs[0][4], runs[0][7])
    assert runs[0] == runs[1]
    assert dict(runs[0][3])["status_polish"] == 1
