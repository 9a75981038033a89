"""kvxopt_amd.osqp on the device against tests/osqp_numpy.py, the numpy restatement of DESIGN section 11.

Bounds.  Parity (tests 1, 7): the device's distance to the longdouble restatement is at most 4 x the float64 restatement's own
distance to it, with a floor of 1e-13 of the vector's infinity norm (the rule of test_gp_eval_against_reference).  Known answers
(test 2): the reference's own places.  Termination (test 3): the two inequalities recomputed in numpy, the restatement's
iteration and factorisation counts.  Interior point (test 4): 4 x the restatement's own distance, floor 1e-6 |x|.
Dictionaries (test 6): 1e-12 relative.  The measured figures are printed before every assertion and recorded in DESIGN 11.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import osqp_numpy as R  # noqa: E402

from kvxopt_amd import _lib, osqp, solvers, workloads  # noqa: E402
from kvxopt_amd.base import matrix, spmatrix  # noqa: E402

pytestmark = pytest.mark.gpu

G25 = R.golden()
OPTS = G25["options"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


def sp(M):
    return spmatrix.from_ccs(*R.to_ccs(np.asarray(M, dtype=np.float64)))


def vec(v):
    return matrix(np.asarray(v, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def case(name):
    return {"basic": R.case_basic, "qp_grid_3_2": lambda: R.case_qp_grid(3, 2), "lp_grid_eq_6_5_3": lambda: R.case_lp_grid_eq(6, 5, 3),
            "generated_noP": lambda: R.case_generated(False), "generated_P": lambda: R.case_generated(True),
            "qp_grid_6_5": lambda: R.case_qp_grid(6, 5), "lp_grid_6_5": lambda: R.case_lp_grid(6, 5),
            "lp_grid_std_6_5": lambda: R.case_lp_grid_std(6, 5), "qp_grid_40_30": lambda: R.case_qp_grid(40, 30)}[name]()


def device(p, scaling, sigma=1e-6, rho=0.1, alpha=1.6):
    Pcc = None if p["P"] is None else R.to_ccs(np.tril(p["P"]))[2:]
    return osqp._Solver(p["q"], R.to_ccs(p["A"]), p["l"], p["u"], Pcc, scaling).setup(sigma, rho, alpha)


def restated(p, scaling, dtype):
    return R.Admm(p["P"], p["q"], p["A"], p["l"], p["u"], scaling, dtype=dtype)


def residuals_at(T, state):
    """The residual vector (and the scales of its sums) a restatement object gives at `state` instead of its own."""
    own = T.state()
    T.x, T.z, T.y, T.dx, T.dy = (np.asarray(v, dtype=T.dtype) for v in state)
    out = T.residuals(), T.sum_scales()
    T.x, T.z, T.y, T.dx, T.dy = own
    return out


def compare(tag, dev_state, dev_res, r64, rld):
    """The parity rule.  x, z, y, dx, dy after the iterations: each as one vector, floor 1e-13 of its infinity norm.
    The residual vector pins k_admm_residuals: both restatements evaluate it at the state the device holds, and it is compared
    entry by entry -- its maxima with a floor of 1e-13 of the largest of them (they are infinity norms of vectors formed from the
    same state and data), its four sums (15, 18, 22, 23) with a floor of 1e-13 of the sum of the absolute values of their terms,
    the scale of test_gp_eval_against_reference.  (Evaluated at each side's own state instead, the sums inherit the states'
    difference times sum |u_i| / c, hundreds of times the state's rounding: two float64 orderings of the restatement then differ
    by more than 4 x either one's error, measured: 5.5e-12 against 4 x 1.0e-13 on the generated case.)"""
    checks = list(zip(("x", "z", "y", "dx", "dy"), dev_state, r64.state(), rld.state()))
    checks = [(n, g, a, b, float(np.abs(np.asarray(b, dtype=np.float64)).max())) for n, g, a, b in checks]
    (res64, _), (resld, sums) = residuals_at(r64, dev_state), residuals_at(rld, dev_state)
    sentinel = np.asarray(resld == R.NEG_MAX)
    assert np.array_equal(np.asarray(dev_res) == R.NEG_MAX, sentinel), (tag, dev_res, resld)
    top = max(abs(float(resld[k])) for k in range(24) if not sentinel[k] and k not in sums)
    for k in range(24):
        if not sentinel[k]:
            checks.append(("res[%d]" % k, dev_res[k:k + 1], res64[k:k + 1], resld[k:k + 1], float(sums[k]) if k in sums else top))
    for name, g, a, b, scale in checks:
        b = np.asarray(b, dtype=np.longdouble)
        err = float(np.abs(np.asarray(g, dtype=np.longdouble) - b).max())
        own = float(np.abs(np.asarray(a, dtype=np.longdouble) - b).max())
        bound = max(4.0 * own, 1e-13 * scale)
        print("%s %-7s device-vs-longdouble %.3e  float64-vs-longdouble %.3e  bound %.3e" % (tag, name, err, own, bound))
        assert err <= bound, (tag, name, err, own, bound)


# ---- 1. iterate parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 25])
@pytest.mark.parametrize("scaling", [0, 10])
@pytest.mark.parametrize("name", ["basic", "qp_grid_3_2", "lp_grid_eq_6_5_3", "generated_noP", "generated_P"])
def test_iterate_parity(name, scaling, k):
    """The three kernels against the restatement after k iterations from zero, adaptive rho off.  The generated case has n = 65,
    m = 257, an empty row and an empty column of A, equality, two-sided, one-sided and free rows; its longest row holds 64 entries
    -- with an empty column n = 65 allows no more -- and is summed by a wavefront (rows of 64 entries and more are)."""
    p = case(name)
    S = device(p, scaling)
    try:
        if name.startswith("generated"):
            assert S.info()["long_rows"] == 1 and S.info()["short_rows"] == 256
        res = S.iterate(k)
        r64, rld = restated(p, scaling, np.float64), restated(p, scaling, np.longdouble)
        r64.iterate(k)
        rld.iterate(k)
        compare("%s scaling=%d k=%d" % (name, scaling, k), S.state(), res, r64, rld)
    finally:
        S.close()


# ---- 2. known answers (G25) ---------------------------------------------------------------------------------------------------
def close(a, b, places):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    assert a.size == b.size
    err = float(np.abs(a - b).max()) if a.size else 0.0
    print("   max error %.3e (places %d)" % (err, places))
    assert all(round(abs(u - v), places) == 0 for u, v in zip(a, b)), (a, b, places)      # unittest's assertAlmostEqual


def test_g25_lp():
    L = G25["lp"]
    c, G, h, A, b = vec(L["c"]), sp(L["G"]), vec(L["h"]), sp(L["A"]), vec(L["b"])
    sol = solvers.lp(c, G, h, solver="osqp", options={"osqp": OPTS})
    assert sol["status"] == "optimal"
    for key in "xzy":
        close(sol[key], L[key], L["places"][key])
    ip = solvers.lp(c, G, h, options={"show_progress": False})
    assert ip["status"] == "optimal"
    for key in "xz":
        close(sol[key], ip[key], 2)
    sol = solvers.lp(c, G, h, A, b, solver="osqp", options={"osqp": OPTS})
    assert sol["status"] == "optimal"
    for key in "xzy":
        close(sol[key], L[key + "_eq"], L["places"][key])
    ip = solvers.lp(c, G, h, A, b, options={"show_progress": False})
    for key in "xzy":
        close(sol[key], ip[key], 2)
    assert osqp.qp(c, G, h, options=OPTS)[0] == "solved"
    assert osqp.qp(c, G, h, A, b, options=OPTS)[0] == "solved"
    assert osqp.qp(c, G, h, None, None, options=OPTS)[0] == "solved"


def test_g25_qp():
    Q = G25["qp"]
    sol = solvers.qp(sp(Q["P"]), vec(Q["q"]), sp(Q["G"]), vec(Q["h"]), solver="osqp", options={"osqp": OPTS})
    assert sol["status"] == "optimal"
    for key in "xyz":
        close(sol[key], Q[key], Q["places"][key])
    close([sol["primal objective"]], [Q["objective"]], Q["places"]["objective"])


def test_g25_qp2():
    Q = G25["qp2"]
    sol = solvers.qp(sp(Q["P"]), vec(Q["q"]), sp(Q["G"]), vec(Q["h"]), sp(Q["A"]), vec(Q["b"]), solver="osqp", options={"osqp": OPTS})
    assert sol["status"] == "optimal"
    for key in "xyz":
        close(sol[key], Q[key], Q["places"][key])
    close([sol["primal objective"]], [Q["objective"]], Q["places"]["objective"])


def test_g25_basic():
    B = G25["basic"]
    status, x, y = osqp.solve(vec(B["q"]), sp(B["A"]), vec(B["l"]), vec(B["u"]), sp(B["P"]), options=OPTS)
    assert status == "solved"
    close(x, B["x"], B["places"]["x"])
    close(y, B["y"], B["places"]["y"])


# ---- 3. termination is honest -----------------------------------------------------------------------------------------------------
QUIET = {"verbose": 0}
TIGHT = {"verbose": 0, "eps_abs": 1e-8, "eps_rel": 1e-8}


@functools.lru_cache(maxsize=None)
def restated_solve(name, tight):
    p = case(name)
    margins = []
    out = R.solve(p["P"], p["q"], p["A"], p["l"], p["u"], TIGHT if tight else QUIET, margins=margins)
    return out + (min(margins),)


@functools.lru_cache(maxsize=None)
def device_solve(name, tight):
    p = case(name)
    stats = {}
    P = None if p["P"] is None else sp(np.tril(p["P"]))
    out = osqp.solve(vec(p["q"]), sp(p["A"]), vec(p["l"]), vec(p["u"]), P, options=TIGHT if tight else QUIET, _stats=stats)
    return out + (stats,)


@pytest.mark.parametrize("name,tight", [("qp_grid_6_5", False), ("lp_grid_6_5", False), ("lp_grid_std_6_5", False), ("lp_grid_eq_6_5_3", False),
                                        ("qp_grid_40_30", False), ("qp_grid_40_30", True)])
def test_termination_is_honest(name, tight):
    p = case(name)
    status, x, y, stats = device_solve(name, tight)
    rstatus, rx, ry, rit, rnf, margin = restated_solve(name, tight)
    print("%s: device %s after %d iterations, %d factorisations; restatement %s %d %d, smallest margin %.2e"
          % (name, status, stats["iterations"], stats["factorisations"], rstatus, rit, rnf, margin))
    assert margin >= 1e-6                              # the restatement's decisions are not within rounding of a threshold
    assert status == "solved" and rstatus == "solved"
    eps = 1e-8 if tight else 1e-3
    P = np.zeros((x.size, x.size)) if p["P"] is None else p["P"]
    ax = p["A"] @ x
    z = np.clip(ax, p["l"], p["u"])
    rp, rd = np.abs(ax - z).max(), np.abs(P @ x + p["q"] + p["A"].T @ y).max()
    tp = eps + eps * max(np.abs(ax).max(), np.abs(z).max())
    td = eps + eps * max(np.abs(P @ x).max(), np.abs(p["A"].T @ y).max(), np.abs(p["q"]).max())
    print("   primal %.3e <= %.3e, dual %.3e <= %.3e" % (rp, tp, rd, td))
    assert rp <= tp and rd <= td
    assert (stats["iterations"], stats["factorisations"]) == (rit, rnf)


# ---- 4. against the interior-point path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gx,gy", [(6, 5), (40, 30)])
def test_against_interior_point(gx, gy, golden_dir):
    name = "qp_grid_%d_%d" % (gx, gy)
    W = workloads.qp_grid(gx, gy)
    G = spmatrix.from_ccs(W["ml"], W["n"], W["Gp"], W["Gi"], W["Gx"])
    P = spmatrix.from_ccs(W["n"], W["n"], W["Pp"], W["Pi"], W["Px"])
    ip = solvers.qp(P, W["q"], G, W["h"], options={"show_progress": False})
    assert ip["status"] == "optimal"
    refs = [("solvers.qp", np.asarray(ip["x"]).reshape(-1))]
    if (gx, gy) == (6, 5):
        g5 = np.load(os.path.join(golden_dir, "g5_coneqp.npz"))
        refs.append(("golden G5", np.asarray(g5["qp6x5_x"]).reshape(-1)))
    _, x, _, _ = device_solve(name, True)
    rx = restated_solve(name, True)[1]
    for what, xr in refs:
        err, own = np.abs(x - xr).max(), np.abs(rx - xr).max()
        bound = max(4.0 * own, 1e-6 * np.abs(xr).max())
        print("%s vs %s: device %.3e, restatement %.3e, bound %.3e" % (name, what, err, own, bound))
        assert err <= bound


# ---- 5. certificates -----------------------------------------------------------------------------------------------------------------
I = R.INFTY
CERTS = {
    "x<=-1,x>=1": (None, [0.0], [[1.0], [1.0]], [-I, 1.0], [-1.0, I], "primal infeasible"),
    "x0+x1<=-1,x>=0": (None, [0.0, 0.0], [[1.0, 1.0], [1.0, 0.0], [0.0, 1.0]], [-I, 0.0, 0.0], [-1.0, I, I], "primal infeasible"),
    "min -x,x>=0": (None, [-1.0], [[1.0]], [0.0], [I], "dual infeasible"),
    "min x0^2/2-x0-x1": ([[1.0, 0.0], [0.0, 0.0]], [-1.0, -1.0], [[1.0, -1.0], [1.0, 0.0], [0.0, 1.0]], [-I, 0.0, 0.0], [1.0, I, I],
                         "dual infeasible"),
}


@pytest.mark.parametrize("name", list(CERTS))
def test_certificates(name):
    P, q, A, l, u, want = CERTS[name]
    q, A, l, u = np.array(q), np.array(A), np.array(l), np.array(u)
    Pd = np.zeros((q.size, q.size)) if P is None else np.array(P)
    stats = {}
    status, x, y = osqp.solve(vec(q), sp(A), vec(l), vec(u), None if P is None else sp(P), options={"verbose": 0, "check_termination": 1},
                              _stats=stats)
    print(name, status, stats["iterations"], x, y)
    assert status == want and stats["iterations"] <= 100
    eps = 1e-4
    if want == "primal infeasible":
        nrm = np.abs(y).max()
        assert nrm > eps
        assert not ((y > 0) & (u >= 1e26)).any() and not ((y < 0) & (l <= -1e26)).any()
        lhs = np.where(u < 1e26, u * np.maximum(y, 0), 0).sum() + np.where(l > -1e26, l * np.minimum(y, 0), 0).sum()
        assert lhs < -eps * nrm and np.abs(A.T @ y).max() < eps * nrm
    else:
        nrm = np.abs(x).max()
        assert nrm > eps and q @ x < -eps * nrm and np.abs(Pd @ x).max() < eps * nrm
        ax = A @ x
        assert (ax[u < 1e26] <= eps * nrm).all() and (ax[l > -1e26] >= -eps * nrm).all()
    status2 = osqp.solve(vec(q), sp(A), vec(l), vec(u), None if P is None else sp(P), options={"verbose": 0})[0]
    assert status2 == want                              # default check_termination = 25: still within 100 iterations


def test_lp_passes_the_status_through():
    """x0 + x1 <= -1, x >= 0 as an LP: solvers.lp hands the status on, with x, z, y and None elsewhere (coneprog.py:2892-2906)."""
    G = sp([[1.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
    sol = solvers.lp(vec([0.0, 0.0]), G, vec([-1.0, 0.0, 0.0]), solver="osqp", options={"osqp": {"verbose": 0}})
    assert sol["status"] == "primal infeasible"
    assert sol["z"].size == 3 and sol["x"].size == 2 and sol["y"].size == 0
    assert all(sol[k] is None for k in ("s", "primal objective", "dual objective", "gap", "relative gap", "primal infeasibility",
                                        "dual infeasibility", "primal slack", "dual slack"))
    P = sp([[1.0, 0.0], [0.0, 1.0]])
    sol = solvers.qp(P, vec([0.0, 0.0]), G, vec([-1.0, 0.0, 0.0]), solver="osqp", options={"osqp": {"verbose": 0}})
    assert sol["status"] == "unknown" and all(v is None for k, v in sol.items() if k != "status")
    with pytest.raises(NotImplementedError):
        solvers.qp(P, vec([0.0, 0.0]), G, vec([-1.0, 0.0, 0.0]), solver="mosek")


# ---- 6. dictionaries -----------------------------------------------------------------------------------------------------------------
KEYS = ("status", "x", "s", "y", "z", "primal objective", "dual objective", "gap", "relative gap", "primal infeasibility",
        "dual infeasibility", "primal slack", "dual slack", "residual as primal infeasibility certificate",
        "residual as dual infeasibility certificate")


def check_dict(sol, P, q, G, h, A, b, is_qp):
    assert tuple(sol) == KEYS and sol["status"] == "optimal"
    x, z, y = sol["x"], sol["z"], sol["y"]
    q, G, h = np.asarray(q, dtype=np.float64), np.asarray(G, dtype=np.float64), np.asarray(h, dtype=np.float64)
    A = np.zeros((0, q.size)) if A is None else np.asarray(A, dtype=np.float64)
    b = np.zeros(0) if b is None else np.asarray(b, dtype=np.float64)
    assert y.size == b.size
    nrm = lambda v: float(np.sqrt(v @ v))
    s = h - G @ x
    gap = s @ z
    if is_qp:
        P = np.asarray(P, dtype=np.float64)
        rx = q + P @ x
        pcost = 0.5 * (x @ rx + x @ q)
        rx = rx + A.T @ y + G.T @ z
        ry, rz = A @ x - b, G @ x + s - h
        dcost = pcost + y @ ry + z @ rz - gap
    else:
        pcost, dcost = q @ x, -(h @ z) - b @ y
        rx, ry, rz = q + G.T @ z + A.T @ y, b - A @ x, G @ x + s - h
    want = {"s": s, "primal objective": pcost, "dual objective": dcost, "gap": gap,
            "relative gap": gap / -pcost if pcost < 0 else (gap / dcost if dcost > 0 else None),
            "primal infeasibility": max(nrm(ry) / max(1.0, nrm(b)), nrm(rz) / max(1.0, nrm(h))),
            "dual infeasibility": nrm(rx) / max(1.0, nrm(q)), "primal slack": s.min(), "dual slack": z.min()}
    scale = max(1.0, np.abs(h).max(), np.abs(q).max())
    for k, v in want.items():
        if v is None:
            assert sol[k] is None
            continue
        err = float(np.abs(np.asarray(sol[k]) - v).max())
        size = max(float(np.abs(v).max()), scale if k in ("s", "primal infeasibility", "dual infeasibility", "gap", "primal slack") else 0.0)
        print("   %-22s error %.3e of %.3e" % (k, err, size))
        assert err <= 1e-12 * size, (k, sol[k], v)
    assert sol["residual as primal infeasibility certificate"] is None and sol["residual as dual infeasibility certificate"] is None


def test_dictionaries():
    """Every key against a numpy recomputation from the returned x, z, y to 1e-12: relative to the value, and for the keys that
    are differences of products of the data (s, the residual norms, the gap, the slack) to the size of the data they cancel from."""
    L = G25["lp"]
    sol = solvers.lp(vec(L["c"]), sp(L["G"]), vec(L["h"]), solver="osqp", options={"osqp": OPTS})
    check_dict(sol, None, L["c"], L["G"], L["h"], None, None, False)
    sol = solvers.lp(vec(L["c"]), matrix(np.array(L["G"])), vec(L["h"]), matrix(np.array(L["A"])), vec(L["b"]), solver="osqp",
                     options={"osqp": OPTS})                                              # dense G, A: converted to sparse
    check_dict(sol, None, L["c"], L["G"], L["h"], L["A"], L["b"], False)
    Q = G25["qp"]
    sol = solvers.qp(matrix(np.array(Q["P"])), vec(Q["q"]), sp(Q["G"]), vec(Q["h"]), solver="osqp", options={"osqp": OPTS})
    check_dict(sol, Q["P"], Q["q"], Q["G"], Q["h"], None, None, True)
    Q = G25["qp2"]
    sol = solvers.qp(sp(Q["P"]), vec(Q["q"]), sp(Q["G"]), vec(Q["h"]), sp(Q["A"]), vec(Q["b"]), solver="osqp", options={"osqp": OPTS})
    check_dict(sol, Q["P"], Q["q"], Q["G"], Q["h"], Q["A"], Q["b"], True)
    W = workloads.qp_grid(6, 5)
    p = case("qp_grid_6_5")
    G = spmatrix.from_ccs(W["ml"], W["n"], W["Gp"], W["Gi"], W["Gx"])
    P = spmatrix.from_ccs(W["n"], W["n"], W["Pp"], W["Pi"], W["Px"])
    sol = solvers.qp(P, W["q"], G, W["h"], solver="osqp", options={"osqp": {"verbose": 0}})
    check_dict(sol, p["P"], W["q"], p["A"], W["h"], None, None, True)


# ---- 7. reproducibility and rho updates ------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes():
    p = case("qp_grid_40_30")
    P = sp(np.tril(p["P"]))
    runs = []
    for _ in range(2):
        stats = {}
        status, x, y = osqp.solve(vec(p["q"]), sp(p["A"]), vec(p["l"]), vec(p["u"]), P, options={"verbose": 0, "adaptive_rho": 1}, _stats=stats)
        runs.append((status, x.tobytes(), y.tobytes(), stats["iterations"], stats["factorisations"]))
    print(runs[0][0], runs[0][3], runs[0][4])
    assert runs[0] == runs[1] and runs[0][4] >= 2        # rho did adapt: the factor was rebuilt on the same pattern


@pytest.mark.parametrize("name", ["qp_grid_3_2", "generated_P"])
def test_iterate_after_set_rho(name):
    p = case(name)
    S = device(p, 10)
    try:
        r64, rld = restated(p, 10, np.float64), restated(p, 10, np.longdouble)
        for T in (S, r64, rld):
            T.iterate(2)
            T.set_rho(0.7)
        res = S.iterate(1)
        r64.iterate(1)
        rld.iterate(1)
        assert S.info()["factorisations"] == 2
        compare("%s after set_rho" % name, S.state(), res, r64, rld)
    finally:
        S.close()
