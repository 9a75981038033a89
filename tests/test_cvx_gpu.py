"""GPU checks of the nonlinear convex drivers: kvx_gp_eval_dev against the reference's Fgp closure (G23), the refreshed values
inside the KKT object, solvers.gp / cp / cpl against the reference's solves (G24: tests/golden/make_goldens_cvx.py, dense
matrices, kktsolver='ldl'), the callback path against the device path, and a pattern rebuild."""
import json
import os

import numpy as np
import pytest

from kvxopt_amd import base, cone, cvx, solvers
from kvxopt_amd.coneops import Dims, WDev
from kvxopt_amd.devvec import DVec

from gp_eval_numpy import as_ccs, numpy_eval as _numpy_eval

pytestmark = pytest.mark.gpu

_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G23 = np.load(os.path.join(_GOLD, "g23_gp_eval.npz"))
G23_CASES = [str(c) for c in G23["cases"]]
G24 = np.load(os.path.join(_GOLD, "g24_cvx_programs.npz"))
G24_META = json.load(open(os.path.join(_GOLD, "g24_cvx_programs.json")))["cases"]
QUIET = {"show_progress": False}
POISON = -7.25e300


def _ccs(name):
    n, Fp, Fi, Fx = as_ccs(G23[name + "__F"], bool(G23[name + "__sparse"]))
    return G23[name + "__K"], n, Fp, Fi, Fx


def _evaluate(ev, x, z):
    """(f, Df, tril H) as dense numpy arrays from one kvx_gp_eval_dev call, and the raw value buffers."""
    n, m = ev.n, ev.nrows
    xd, f = DVec(n, x), DVec(m)
    Dfx, Hx = DVec(ev.Dfi.size), DVec(max(ev.Hi.size, 1)).fill(POISON)
    zd = None if z is None else DVec(m, z)
    ev.eval_ptr(xd.ptr, None if z is None else zd.ptr, f.ptr, Dfx.ptr, None if z is None else Hx.ptr)
    Df, H = np.zeros((m, n)), np.zeros((n, n))
    Df[ev.df_pattern] = Dfx.get()
    raw_h = Hx.get()
    if z is not None:
        H[ev.h_pattern] = raw_h[:ev.Hi.size]
    return f.get(), Df, H, Dfx.get(), raw_h


@pytest.mark.parametrize("name", G23_CASES)
def test_gp_eval_against_reference(name):
    """|err| <= 1e-13 x (sum of absolute contributions), the project's bound for assembled values.  Where an output misses it the
    bound is not loosened: the case is evaluated in numpy.longdouble and the GPU's error against that may be at most 4 x the
    reference's own (summation order, exp rounding)."""
    K, n, Fp, Fi, Fx = _ccs(name)
    g, x, z = G23[name + "__g"], G23[name + "__x"], G23[name + "__z"]
    ev = cvx.GPEval(K, n, Fp, Fi, Fx, g)
    f, Df, H, raw_df, raw_h = _evaluate(ev, x, z)
    _, _, _, sf, sDf, sH = _numpy_eval(K, G23[name + "__F"], g, x, z, np.float64)
    tf, tDf, tH, _, _, _ = _numpy_eval(K, G23[name + "__F"], g, x, z, np.longdouble)
    for what, got, ref, sc, true in (("f", f, G23[name + "__f"], sf, tf), ("Df", Df, G23[name + "__Df"], sDf, tDf),
                                     ("H", H, G23[name + "__H"], sH, tH)):
        err = np.abs(got - ref)
        worst = float((err / np.maximum(sc, 1e-300)).max())
        print("G23 %s %s: max |err| / scale = %.3e" % (name, what, worst))
        if np.all(err <= 1e-13 * sc):
            continue
        gpu_err = float(np.abs(got - true).max())
        ref_err = float(np.abs(ref - true).max())
        print("   against longdouble: GPU %.3e, reference %.3e, ratio %.2f" % (gpu_err, ref_err, gpu_err / ref_err if ref_err else np.inf))
        assert gpu_err <= 4.0 * ref_err, (name, what, worst, gpu_err, ref_err)
    # the line-search form: same f and Df, the poisoned H buffer untouched
    f2, Df2, _, raw_df2, raw_h2 = _evaluate(ev, x, None)
    assert f2.tobytes() == f.tobytes() and raw_df2.tobytes() == raw_df.tobytes()
    assert np.all(raw_h2 == POISON)
    # one-term blocks: Df_i = F_i exactly, and H is what the other blocks give, exactly
    ones = np.flatnonzero(K == 1)
    off = np.concatenate([[0], np.cumsum(K)])
    for i in ones:
        assert np.array_equal(Df[i], G23[name + "__F"][off[i]])
    if ones.size:
        z0 = z.copy()
        z0[ones] = 0.0
        assert _evaluate(ev, x, z0)[2].tobytes() == H.tobytes()
        if ones.size == K.size:
            assert not H.any()
    # a second call: the same bytes
    f3, _, _, raw_df3, raw_h3 = _evaluate(ev, x, z)
    assert f3.tobytes() == f.tobytes() and raw_df3.tobytes() == raw_df.tobytes() and raw_h3.tobytes() == raw_h.tobytes()


@pytest.mark.parametrize("name", ["k312", "sparse"])
def test_refreshed_kkt_values_give_S(name):
    """The values of the Df rows of J = [Df; G] and of H, scattered into the KKT object from the evaluator's buffers, assemble to
    S = H + J' diag(dnli, di)^2 J (formed in numpy from the reference's Df and H)."""
    K, n, Fp, Fi, Fx = _ccs(name)
    ev = cvx.GPEval(K, n, Fp, Fi, Fx, G23[name + "__g"])
    rng = np.random.default_rng(7)
    ml, mnl = 3, K.size
    G = rng.standard_normal((ml, n)) * (rng.random((ml, n)) < 0.7)
    _, _, Gp, Gi, Gx = base.ccs(base.spmatrix(G[np.nonzero(G)], *np.nonzero(G), G.shape))
    empty = (np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
    k = cvx._plan(ev, n, ml, (Gp, Gi, Gx), 0, empty)
    x, z = DVec(n, G23[name + "__x"]), DVec(mnl, G23[name + "__z"])
    assert ev.eval(x, z, DVec(mnl), k.Dfx, k.Hx)
    cvx._refresh(k)
    D = Dims({"l": mnl + ml, "q": [], "s": []})
    W = WDev(D)
    di = rng.uniform(0.5, 2.0, mnl + ml)
    W.d.set(1.0 / di); W.di.set(di)
    k.kkt.assemble(W)
    plan = k.kkt.plan
    S = np.zeros((n, n))
    S[plan.Si, np.repeat(np.arange(n), np.diff(plan.Sp))] = k.kkt.Sx.get()[:plan.Si.size]
    J = np.vstack([G23[name + "__Df"], G])
    ref = np.tril(G23[name + "__H"] + J.T @ (J * (di ** 2)[:, None]))
    sc = np.tril(np.abs(G23[name + "__H"]) + np.abs(J).T @ (np.abs(J) * (di ** 2)[:, None]))
    err = np.abs(S - ref)
    print("S from refreshed values (%s): max |err| / scale = %.3e" % (name, (err / np.maximum(sc, 1e-300)).max()))
    assert np.all(err <= 1e-13 * sc)
    # J v with the refreshed transposed copy as well
    v = rng.standard_normal(n)
    out = DVec(mnl + ml)
    k.J.gemv(DVec(n, v), out, trans="N")
    assert np.abs(out.get() - J @ v).max() <= 1e-13 * (np.abs(J) @ np.abs(v)).max()


# ---- G24 -------------------------------------------------------------------------------------------------------------------------
def _lse(K, F, g, x):
    off = np.concatenate([[0], np.cumsum(K)])
    f, Df, Y = np.zeros(len(K)), np.zeros((len(K), F.shape[1])), []
    for i in range(len(K)):
        u = F[off[i]:off[i + 1]] @ x + g[off[i]:off[i + 1]]
        e = np.exp(u - u.max())
        f[i] = u.max() + np.log(e.sum())
        Y.append(e / e.sum())
        Df[i] = Y[-1] @ F[off[i]:off[i + 1]]
    return f, Df, Y


def gp_callback(K, F, g):
    """The blocks of a gp as a cp callback evaluated in numpy (dense Df and H)."""
    off = np.concatenate([[0], np.cumsum(K)])

    def cb(x=None, z=None):
        if x is None:
            return len(K) - 1, base.matrix(np.zeros(F.shape[1]))
        f, Df, Y = _lse(K, F, g, base.flat(x))
        if z is None:
            return f, Df
        H = np.zeros((F.shape[1],) * 2)
        for i, zi in enumerate(base.flat(z)):
            C = F[off[i]:off[i + 1]] - Df[i][None, :]
            H += zi * (C.T @ (C * Y[i][:, None]))
        return f, Df, H
    return cb


def _case(name):
    """(solve, functions) of a G24 case: solve(options) runs the driver; functions(x) -> (c, f, Df) of the cpl form that the
    optimality conditions are checked in (for cp / gp: the objective as row 0 of f and Df, c = 0)."""
    m = G24_META[name]
    d = {k[len(name) + 2:]: G24[k] for k in G24.files if k.startswith(name + "__")}
    kind = m["kind"]
    kw = {}
    if "G" in d:
        kw.update(G=base.matrix(d["G"]), h=base.matrix(d["h"]))
    if "A" in d:
        kw.update(A=base.matrix(d["A"]), b=base.matrix(d["b"]))
    if kind == "gp":
        K = [int(k) for k in m["K"]]
        fn = lambda x: _lse(K, d["F"], d["g"], x)[:2]
        return d, kw, (lambda o: solvers.gp(K, base.matrix(d["F"]), base.matrix(d["g"]), options=o, **kw)), fn, np.zeros(d["F"].shape[1]), True
    if kind == "acent":
        n = d["A"].shape[1]

        def F(x=None, z=None):
            if x is None:
                return 0, base.matrix(np.ones(n))
            xv = base.flat(x)
            if xv.min() <= 0.0:
                return None
            f, Df = -np.log(xv).sum(), (-1.0 / xv)[None, :]
            return (f, Df) if z is None else (f, Df, base.spdiag(base.flat(z)[0] / xv ** 2))
        fn = lambda x: (np.array([-np.log(x).sum()]), (-1.0 / x)[None, :])
        return d, kw, (lambda o: solvers.cp(F, options=o, **kw)), fn, np.ones(n), True
    if kind == "robls":
        A, b, rho = d["A"], d["b"], float(m["rho"])

        def F(x=None, z=None):
            if x is None:
                return 0, base.matrix(np.zeros(A.shape[1]))
            y = A @ base.flat(x) - b
            w = np.sqrt(rho + y ** 2)
            f, Df = w.sum(), ((y / w) @ A)[None, :]
            return (f, Df) if z is None else (f, Df, A.T @ (A * (base.flat(z)[0] * rho / w ** 3)[:, None]))

        def fn(x):
            y = A @ x - b
            w = np.sqrt(rho + y ** 2)
            return np.array([w.sum()]), ((y / w) @ A)[None, :]
        d = {k: v for k, v in d.items() if k not in ("A", "b")}      # the data of the objective, not equality constraints
        return d, {}, (lambda o: solvers.cp(F, options=o)), fn, np.zeros(A.shape[1]), True
    if kind == "floorplan":
        Amin = d["Amin"]
        r5 = np.arange(5)

        def fn(x):
            Df = np.zeros((5, 22))
            Df[r5, 12 + r5] = -1.0
            Df[r5, 17 + r5] = -Amin / x[17:] ** 2
            return -x[12:17] + Amin / x[17:], Df

        def F(x=None, z=None):
            if x is None:
                return 5, base.matrix(np.array(17 * [0.0] + 5 * [1.0]))
            xv = base.flat(x)
            if xv[17:].min() <= 0.0:
                return None
            f, Df = fn(xv)
            Dfs = base.spmatrix(Df[np.nonzero(Df)], *np.nonzero(Df), Df.shape)
            if z is None:
                return f, Dfs
            return f, Dfs, base.spmatrix(2.0 * base.flat(z) * Amin / xv[17:] ** 3, 17 + r5, 17 + r5, (22, 22))
        x0 = np.array(17 * [0.0] + 5 * [1.0])
        return d, kw, (lambda o: solvers.cpl(base.matrix(d["c"]), F, options=o, **kw)), fn, x0, False
    raise ValueError(kind)


def _check_optimal(sol, d, fn, x0, epigraph, opt):
    """The optimality conditions of cpl at the tolerances of the options, in numpy from the returned vectors.  The driver stops at
    residuals relative to those of its starting point (x0, s = z = 1, y = 0: cvxprog.py:709-722); with the epigraph form the
    multiplier of f_0 - t <= 0 is not returned, it is 1 up to the same dual residual."""
    feastol, abstol, reltol = opt.get("feastol", 1e-7), opt.get("abstol", 1e-7), opt.get("reltol", 1e-6)
    n = x0.size
    G, h = d.get("G", np.zeros((0, n))), d.get("h", np.zeros(0))
    A, b = d.get("A", np.zeros((0, n))), d.get("b", np.zeros(0))
    c = np.zeros(n) if epigraph else d["c"]
    f0, Df0 = fn(x0)
    dres0 = max(1.0, np.linalg.norm(c + Df0.T @ np.ones(len(f0)) + G.T @ np.ones(len(h))))
    pres0 = max(1.0, np.sqrt(np.linalg.norm(A @ x0 - b) ** 2 + np.linalg.norm(1.0 + f0) ** 2 + np.linalg.norm(1.0 + G @ x0 - h) ** 2))
    x = sol["x"]
    f, Df = fn(x)
    if epigraph:
        znl, snl_res = np.concatenate([[1.0], sol["znl"]]), f[1:] + sol["snl"]
        slack = 1.0 + np.linalg.norm(Df[0])
    else:
        znl, snl_res, slack = sol["znl"], f + sol["snl"], 1.0
    rx = c + Df.T @ znl + G.T @ sol["zl"] + (A.T @ sol["y"] if A.shape[0] else 0.0)
    print("   |rx| = %.2e (dres0 %.2e), |f + snl| = %.2e, |Gx + sl - h| = %.2e, |Ax - b| = %.2e (pres0 %.2e)" % (
        np.linalg.norm(rx), dres0, np.linalg.norm(snl_res), np.linalg.norm(G @ x + sol["sl"] - h), np.linalg.norm(A @ x - b), pres0))
    assert np.linalg.norm(rx) <= feastol * dres0 * slack
    assert np.linalg.norm(snl_res) <= feastol * pres0
    assert np.linalg.norm(G @ x + sol["sl"] - h) <= feastol * pres0
    assert np.linalg.norm(A @ x - b) <= feastol * pres0
    for v in ("snl", "sl", "znl", "zl"):
        if sol[v].size:
            assert sol[v].min() >= -1e-7 * max(1.0, np.abs(sol[v]).max())
    gap = sol["snl"] @ sol["znl"] + sol["sl"] @ sol["zl"]
    assert gap <= sol["gap"] * (1 + 1e-9) + 1e-15
    assert sol["gap"] <= abstol or (sol["relative gap"] is not None and sol["relative gap"] <= reltol)


@pytest.mark.parametrize("name", sorted(G24_META))
def test_g24_solves_against_reference(name):
    m = G24_META[name]
    d, kw, solve, fn, x0, epigraph = _case(name)
    opt = dict(QUIET)
    opt.update(m["options"])
    sol = solve(opt)
    print("G24 %s: %s in %d iterations (reference: %s in %d)" % (name, sol["status"], sol["iterations"], m["status"], m["iterations"]))
    assert sol["status"] == m["status"]
    ref = d["sol_x"]
    assert np.linalg.norm(sol["x"] - ref) <= 1e-6 * max(np.linalg.norm(ref), 1.0)
    for key in ("primal objective", "dual objective", "gap", "relative gap", "primal infeasibility", "dual infeasibility"):
        if m[key] is None:
            assert sol[key] is None
        else:
            print("   %s: %.10e (reference %.10e)" % (key, sol[key], m[key]))
            assert abs(sol[key] - m[key]) <= 1e-7 * max(abs(m[key]), 1.0), key
    for key in ("y", "znl", "zl", "snl", "sl"):
        assert sol[key].shape == d["sol_" + key].shape, key
    assert set(sol) == {"status", "x", "y", "znl", "zl", "snl", "sl", "gap", "relative gap", "primal objective", "dual objective",
                        "primal infeasibility", "dual infeasibility", "primal slack", "dual slack", "iterations", "factorizations"}
    if m["status"] == "optimal":
        _check_optimal(sol, d, fn, x0, epigraph, opt)


@pytest.mark.parametrize("name", ["gp_random", "gp_edges"])
def test_gp_device_path_and_callback_path_agree(name):
    """The same gp through kvx_gp_eval_dev and through cp with a callback that evaluates the blocks in numpy."""
    m = G24_META[name]
    d, kw, solve, fn, x0, _ = _case(name)
    K = [int(k) for k in m["K"]]
    dev = solve(QUIET)
    cb = solvers.cp(gp_callback(K, d["F"], d["g"]), options=QUIET, **kw)
    print("device: %d iterations, callback: %d" % (dev["iterations"], cb["iterations"]))
    assert dev["status"] == cb["status"] == "optimal"
    assert np.linalg.norm(dev["x"] - cb["x"]) <= 1e-6 * max(np.linalg.norm(dev["x"]), 1.0)
    for key in ("primal objective", "dual objective", "gap"):
        assert abs(dev[key] - cb[key]) <= 1e-7 * max(abs(dev[key]), 1.0), key


def test_sparse_callback_pattern_rebuild():
    """minimize (x0 + x1)^4 / 4 + x0^2 + x1^2 + x0 - 2 x1: the sparse H of the callback has no (1, 0) entry at x0 = 0 (it is
    3 (x0 + x1)^2 there: zero, dropped), and gains it at the second evaluation.  The plan is rebuilt on the wider pattern -- the
    entry is not dropped: the evaluator's pattern has three entries afterwards and the run takes the iterations of the same
    program with a dense H."""
    seen = []

    def parts(x, z):
        a, b = base.flat(x)
        f = 0.25 * (a + b) ** 4 + a * a + b * b + a - 2 * b
        Df = np.array([[(a + b) ** 3 + 2 * a + 1, (a + b) ** 3 + 2 * b - 2]])
        return f, Df, None if z is None else base.flat(z)[0] * (3 * (a + b) ** 2 * np.ones((2, 2)) + 2 * np.eye(2))

    def F(x=None, z=None):
        if x is None:
            return 0, base.matrix(np.zeros(2))
        f, Df, H = parts(x, z)
        if z is None:
            return f, Df
        I, J = np.nonzero(np.tril(H))
        seen.append(len(I))
        return f, Df, base.spmatrix(H[I, J], I, J, (2, 2))

    def Fdense(x=None, z=None):
        if x is None:
            return 0, base.matrix(np.zeros(2))
        f, Df, H = parts(x, z)
        return (f, Df) if z is None else (f, Df, H)
    ev = cvx._CpCallback(F)
    assert ev.h_pattern[0].size == 2                                  # the diagonal only, fixed at the first evaluation
    sol = cvx.cp(ev, options=QUIET)
    assert seen[0] == 2 and max(seen) == 3
    assert ev.h_pattern[0].size == 3 and (1, 0) in zip(*ev.h_pattern)  # the plan was rebuilt with the new entry
    dense = solvers.cp(Fdense, options=QUIET)
    print("sparse H with a rebuild: %d iterations, %d factorisations; dense H: %d, %d" % (
        sol["iterations"], sol["factorizations"], dense["iterations"], dense["factorizations"]))
    assert sol["status"] == dense["status"] == "optimal"
    assert sol["iterations"] == dense["iterations"] and sol["factorizations"] == dense["factorizations"]
    assert np.linalg.norm(sol["x"] - dense["x"]) <= 1e-9
    a, b = sol["x"]
    grad = np.array([(a + b) ** 3 + 2 * a + 1, (a + b) ** 3 + 2 * b - 2])
    assert np.linalg.norm(grad) <= 1e-6


def test_existing_drivers_keep_their_bits():
    """A determinism check only: solvers.lp and solvers.socp share SpMatDev and KKTConeDev with the new drivers, and two runs of
    each give the same bytes.  That they compute what they computed before rests on the change to those classes being additive
    (new methods that the existing drivers never call) and on the earlier GPU tests of those drivers, which stay as they are."""
    c = np.array([-4.0, -5.0])
    G = base.matrix(np.array([[2.0, 1.0], [1.0, 2.0], [-1.0, 0.0], [0.0, -1.0]]))
    h = np.array([3.0, 3.0, 0.0, 0.0])
    a, b = (solvers.lp(c, G, h, options=QUIET) for _ in range(2))
    assert a["status"] == "optimal" and a["x"].tobytes() == b["x"].tobytes() and a["z"].tobytes() == b["z"].tobytes()
    assert np.allclose(a["x"], [1.0, 1.0], atol=1e-6)
    G1 = np.array([[12., 13., 12.], [6., -3., -12.], [-5., -5., 6.]]).T
    G2 = np.array([[3., 3., -1., 1.], [-6., -6., -9., 19.], [10., -2., -2., -3.]]).T
    args = (np.array([-2., 1., 5.]), None, None, [base.matrix(G1), base.matrix(G2)], [np.array([-12., -3., -2.]), np.array([27., 0., 3., -42.])])
    a, b = (solvers.socp(*args, options=QUIET) for _ in range(2))
    assert a["status"] == "optimal" and a["x"].tobytes() == b["x"].tobytes()
