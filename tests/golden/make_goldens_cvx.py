"""Generates G23 (the log-sum-exp evaluation of solvers.gp) and G24 (gp, cp and cpl programs) from the REFERENCE itself, staged
by make_goldens.stage() (build container only; the fixtures travel).  Every solve is the pure reference: dense matrices and
kktsolver='ldl' (misc.kkt_ldl, LAPACK only), tagged "via": "reference".

G23 holds what the reference's own Fgp closure returns: solvers.gp hands that closure to cvxprog.cp, so cp is replaced for the
call by a function that evaluates the closure it is given at the fixed x, z and solves nothing.

    python tests/golden/make_goldens_cvx.py
"""
import contextlib
import io
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens  # noqa: E402


# ---- G23 ------------------------------------------------------------------------------------------------------------------------
def gp_eval_cases():
    out = {}

    def dense(name, K, n, seed, scale=1.0, g=None):
        rng = np.random.default_rng(seed)
        l = sum(K)
        out[name] = dict(K=K, F=rng.standard_normal((l, n)) * scale, g=rng.standard_normal(l) if g is None else g,
                         x=rng.standard_normal(n), z=rng.uniform(0.5, 2.0, len(K)))
    dense("k1", [1], 3, 2301)
    dense("k111", [1, 1, 1], 3, 2302)
    dense("k312", [3, 1, 2], 4, 2303)
    dense("k63_64_65_1", [63, 64, 65, 1], 6, 2304)
    dense("k300_2", [300, 2], 5, 2305)
    dense("spread700", [5, 1, 3], 3, 2306, scale=0.5, g=np.array([700.0, -700.0, 650.0, 0.0, -300.0, 720.0, -710.0, 705.0, 0.5]))
    dense("k5_40_1_n20", [5, 40, 1], 20, 2308)                  # blocks that meet 20 columns: more than one 16 x 16 Gram tile
    # sparse F: column 2 is empty, block 1 meets column 0 only, block 2 is one term
    rng = np.random.default_rng(2307)
    K = [3, 2, 1, 4]
    F = np.zeros((10, 5))
    F[0, [0, 1]] = rng.standard_normal(2); F[1, [1, 3]] = rng.standard_normal(2); F[2, 4] = rng.standard_normal()
    F[3, 0] = rng.standard_normal(); F[4, 0] = rng.standard_normal()
    F[5, [1, 4]] = rng.standard_normal(2)
    F[6, 3] = rng.standard_normal(); F[7, [0, 3]] = rng.standard_normal(2); F[9, [3, 4]] = rng.standard_normal(2)   # row 8: no entry
    out["sparse"] = dict(K=K, F=F, g=rng.standard_normal(10), x=rng.standard_normal(5), z=rng.uniform(0.5, 2.0, 4), sparse=True)
    return out


def g23_gp_eval():
    from kvxopt import cvxprog, matrix, sparse
    npz, names = {}, []
    keep = cvxprog.cp
    for name, cs in gp_eval_cases().items():
        got = {}

        def record(F, *args, **kw):
            got["f"], got["Df"], got["H"] = F(matrix(cs["x"]), matrix(cs["z"]))
            got["f2"], got["Df2"] = F(matrix(cs["x"]))
            return {}
        Fm = matrix(np.asfortranarray(cs["F"]))
        cvxprog.cp = record
        try:
            cvxprog.gp([int(k) for k in cs["K"]], sparse(Fm) if cs.get("sparse") else Fm, matrix(cs["g"]))
        finally:
            cvxprog.cp = keep
        assert np.array_equal(np.array(got["f"]), np.array(got["f2"])) and np.array_equal(np.array(got["Df"]), np.array(got["Df2"]))
        for k in ("K", "F", "g", "x", "z"):
            npz["%s__%s" % (name, k)] = np.asarray(cs[k], dtype=np.int64 if k == "K" else float)
        npz[name + "__f"] = np.array(got["f"]).reshape(-1)
        npz[name + "__Df"] = np.array(got["Df"])
        npz[name + "__H"] = np.tril(np.array(got["H"]))               # syrk writes the lower triangle
        npz[name + "__sparse"] = np.array(bool(cs.get("sparse")))
        names.append(name)
        print("G23", name, np.array(got["f"]).reshape(-1)[:4])
    npz["via"] = np.array("reference (the Fgp closure of cvxprog.gp)")
    npz["cases"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "g23_gp_eval.npz"), **npz)


# ---- G24 ------------------------------------------------------------------------------------------------------------------------
def floorplan_data(Amin):
    """The floor-planning example of the documentation (doc/source/solvers.rst:605-685): rho = 1, gamma = 5."""
    rho, gamma = 1.0, 5.0
    c = np.array(2 * [1.0] + 20 * [0.0])
    G, h = np.zeros((26, 22)), np.zeros(26)
    G[0, 2] = -1.0; G[1, 3] = -1.0; G[2, 5] = -1.0
    for r, cols in ((3, [2, 4, 12]), (4, [3, 4, 13]), (5, [4, 6, 14]), (6, [5, 6, 15])):
        G[r, cols], h[r] = [1.0, -1.0, 1.0], -rho
    G[7, [0, 6, 16]] = -1.0, 1.0, 1.0
    G[8, 8] = -1.0; G[9, 9] = -1.0; G[10, 11] = -1.0
    G[11, [7, 8, 18]], h[11] = [-1.0, 1.0, 1.0], -rho
    G[12, [7, 10, 17]], h[12] = [1.0, -1.0, 1.0], -rho
    G[13, [9, 10, 19]], h[13] = [1.0, -1.0, 1.0], -rho
    G[14, [1, 10, 20]] = -1.0, 1.0, 1.0
    G[15, [1, 11, 21]] = -1.0, 1.0, 1.0
    for k in range(5):
        G[16 + 2 * k, [12 + k, 17 + k]] = -1.0, 1.0 / gamma
        G[17 + 2 * k, [12 + k, 17 + k]] = 1.0, -gamma
    return dict(c=c, G=G, h=h, Amin=np.asarray(Amin, dtype=float))


def programs():
    out = {}
    Aflr, Awall, alpha, beta, gamma, delta = 1000.0, 100.0, 0.5, 2.0, 0.5, 2.0
    doc = dict(kind="gp", K=[1, 2, 1, 1, 1, 1, 1],
               F=np.array([[-1., 1., 1., 0., -1., 1., 0., 0.], [-1., 1., 0., 1., 1., -1., 1., -1.], [-1., 0., 1., 1., 0., 0., -1., 1.]]).T,
               g=np.log(np.array([1.0, 2 / Awall, 2 / Awall, 1 / Aflr, alpha, 1 / beta, gamma, 1 / delta])))
    out["gp_doc"] = doc
    rng = np.random.default_rng(2401)
    A = rng.standard_normal((3, 8))
    A[0] = 1.0                                                  # sum x = const: the feasible set is bounded, the centre exists
    out["cp_acent"] = dict(kind="acent", A=A, b=A @ rng.uniform(0.5, 2.0, 8))
    rng = np.random.default_rng(2402)
    out["cp_robls"] = dict(kind="robls", A=rng.standard_normal((12, 4)), b=rng.standard_normal(12), rho=0.1)
    out["cpl_floorplan"] = dict(kind="floorplan", **floorplan_data([100.0] * 5))
    # seeded gp with G, h and A, b: x0 strictly feasible for every constraint
    rng = np.random.default_rng(2403)
    K, n = [4, 3, 1, 5, 2], 6
    l = sum(K)
    F = rng.standard_normal((l, n)) * (rng.random((l, n)) < 0.6)
    x0 = 0.3 * rng.standard_normal(n)
    g = rng.standard_normal(l)
    off = np.concatenate([[0], np.cumsum(K)])
    for i in range(1, len(K)):                                  # f_i(x0) = -0.5
        u = F[off[i]:off[i + 1]] @ x0 + g[off[i]:off[i + 1]]
        g[off[i]:off[i + 1]] -= np.log(np.exp(u).sum()) + 0.5
    G = np.vstack([np.eye(n), -np.eye(n), rng.standard_normal((3, n))])
    A = rng.standard_normal((2, n))
    out["gp_random"] = dict(kind="gp", K=K, F=F, g=g, G=G, h=G @ x0 + rng.uniform(0.5, 1.5, G.shape[0]), A=A, b=A @ x0)
    # the reference stops at its iteration limit: status 'unknown'
    out["gp_doc_maxiters"] = dict(doc, options={"maxiters": 4})
    # a gp on the edges of the evaluator's size classes: K = 257 (workgroup), 17 (wavefront), 16 (16-lane group), and 17 columns
    # (two Gram tile rows).  g_i = -1 - log K_i on the constraint blocks: f_i(0) = -1, x = 0 is strictly feasible; the objective
    # has 257 Gaussian rows in 17 dimensions: it grows in every direction
    rng = np.random.default_rng(2404)
    K, n = [257, 17, 16], 17
    F = rng.standard_normal((sum(K), n))
    g = np.concatenate([rng.standard_normal(K[0])] + [np.full(k, -1.0 - np.log(k)) for k in K[1:]])
    out["gp_edges"] = dict(kind="gp", K=K, F=F, g=g)
    return out


def _solve(cs):
    """The callbacks evaluate in numpy and hand the reference its own matrix type; the solves are the reference's."""
    from kvxopt import matrix, solvers
    opts = {"show_progress": True}
    opts.update(cs.get("options", {}))
    M = lambda a: matrix(np.asfortranarray(np.asarray(a, dtype=float)))
    vec = lambda v: np.array(v, dtype=float).reshape(-1)
    kind = cs["kind"]
    if kind == "gp":
        kw = {}
        if "G" in cs:
            kw.update(G=M(cs["G"]), h=matrix(cs["h"]))
        if "A" in cs:
            kw.update(A=M(cs["A"]), b=matrix(cs["b"]))
        return solvers.gp([int(k) for k in cs["K"]], M(cs["F"]), matrix(cs["g"]), kktsolver="ldl", options=opts, **kw)
    if kind == "acent":                                          # minimize -sum log x_i  s.t.  A x = b
        n = cs["A"].shape[1]

        def F(x=None, z=None):
            if x is None:
                return 0, matrix(1.0, (n, 1))
            xv = vec(x)
            if xv.min() <= 0.0:
                return None
            f, Df = -np.log(xv).sum(), M((-1.0 / xv)[None, :])
            return (f, Df) if z is None else (f, Df, M(np.diag(z[0] / xv ** 2)))
        return solvers.cp(F, A=M(cs["A"]), b=matrix(cs["b"]), kktsolver="ldl", options=opts)
    if kind == "robls":                                          # minimize sum_k sqrt(rho + (A x - b)_k^2)
        A, b, rho = cs["A"], cs["b"], float(cs["rho"])
        n = A.shape[1]

        def F(x=None, z=None):
            if x is None:
                return 0, matrix(0.0, (n, 1))
            y = A @ vec(x) - b
            w = np.sqrt(rho + y ** 2)
            f, Df = w.sum(), M(((y / w) @ A)[None, :])
            return (f, Df) if z is None else (f, Df, M(A.T @ (A * (z[0] * rho / w ** 3)[:, None])))
        return solvers.cp(F, kktsolver="ldl", options=opts)
    if kind == "floorplan":                                      # f_k = -w_k + Amin_k / h_k, w = x[12:17], h = x[17:22]
        Amin = cs["Amin"]

        def F(x=None, z=None):
            if x is None:
                return 5, matrix(17 * [0.0] + 5 * [1.0])
            xv = vec(x)
            hh = xv[17:]
            if hh.min() <= 0.0:
                return None
            Df = np.zeros((5, 22))
            Df[np.arange(5), 12 + np.arange(5)] = -1.0
            Df[np.arange(5), 17 + np.arange(5)] = -Amin / hh ** 2
            f = M(-xv[12:17] + Amin / hh)
            if z is None:
                return f, M(Df)
            H = np.zeros((22, 22))
            H[17 + np.arange(5), 17 + np.arange(5)] = 2.0 * vec(z) * Amin / hh ** 3
            return f, M(Df), M(H)
        return solvers.cpl(matrix(cs["c"]), F, M(cs["G"]), matrix(cs["h"]), kktsolver="ldl", options=opts)
    raise ValueError(kind)


STATS = ("gap", "relative gap", "primal objective", "dual objective", "primal infeasibility", "dual infeasibility", "primal slack",
         "dual slack")


def g24_cvx_programs():
    npz, meta = {}, {"via": "reference (dense matrices, kktsolver='ldl': misc.kkt_ldl)", "cases": {}}
    for name, cs in programs().items():
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            sol = _solve(cs)
        iters = len(re.findall(r"^\s*\d+: ", buf.getvalue(), flags=re.M)) - 1
        for k, v in cs.items():
            if k not in ("kind", "options", "K", "rho"):
                npz["%s__%s" % (name, k)] = np.asarray(v, dtype=float)
        for k in ("x", "y", "znl", "zl", "snl", "sl"):
            npz["%s__sol_%s" % (name, k)] = np.array(sol[k], dtype=float).reshape(-1)
        m = {"kind": cs["kind"], "options": cs.get("options", {}), "status": sol["status"], "iterations": iters}
        if "K" in cs:
            m["K"] = [int(k) for k in cs["K"]]
        if "rho" in cs:
            m["rho"] = cs["rho"]
        m.update({k: sol[k] for k in STATS})
        meta["cases"][name] = m
        print("G24", name, sol["status"], iters)
    np.savez_compressed(os.path.join(HERE, "g24_cvx_programs.npz"), **npz)
    json.dump(meta, open(os.path.join(HERE, "g24_cvx_programs.json"), "w"), indent=1)


if __name__ == "__main__":
    make_goldens.stage()
    g23_gp_eval()
    g24_cvx_programs()
    print("goldens written to", HERE)
