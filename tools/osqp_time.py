"""Time of one osqp solve on workloads.qp_grid(gx, gy): iterations, factorisations, milliseconds per iteration and the split of an
iteration between the triangular solve and the two ADMM kernels.  Every timed part ends with a device synchronisation.  The
solve alone is timed on a second factor of the same pattern (a diagonally dominant matrix on the pattern of S: the time of a
sweep depends on the pattern only).  Then a kept osqp.Problem: default eps plus polish against a plain run at eps = 1e-8, and a
sequence of 20 update(q) + solve() steps, warm against cold, each next to osqp.qp called on the same data (plan, analysis and
setup every time).  No thresholds: the numbers are printed as JSON.

    python tools/osqp_time.py [--gx GX] [--gy GY] [--eps EPS] [--reps R]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from kvxopt_amd import _lib, osqp, solvers, workloads  # noqa: E402
from kvxopt_amd.base import spmatrix  # noqa: E402
from kvxopt_amd.chol import Factor  # noqa: E402


def _sync():
    _lib.raise_for(_lib.lib().kvx_dev_sync())


def _timed(f):
    _sync()
    t = time.perf_counter()
    r = f()
    _sync()
    return time.perf_counter() - t, r


def _residuals(W, G, P, x, z):
    """Unscaled primal and dual residual of the QP min 1/2 x'Px + q'x, Gx <= h at (x, z)."""
    Gd = np.zeros((W["ml"], W["n"]))
    Gd[W["Gi"], np.repeat(np.arange(W["n"]), np.diff(W["Gp"]))] = W["Gx"]
    L = np.zeros((W["n"], W["n"]))
    L[W["Pi"], np.repeat(np.arange(W["n"]), np.diff(W["Pp"]))] = W["Px"]
    Pd = L + np.tril(L, -1).T
    gx = Gd @ x
    return float(np.maximum(gx - W["h"], 0.0).max()), float(np.abs(Pd @ x + W["q"] + Gd.T @ z).max())


def kept_problem(W, G, P, out, steps=20):
    """The measurements of a kept problem on the workload W (osqp.Problem; DESIGN 11, "A kept problem")."""
    n, m = W["n"], W["ml"]
    l, u = np.full(m, -osqp.INFTY), np.asarray(W["h"], dtype=np.float64)
    q = np.asarray(W["q"], dtype=np.float64)
    tight = {"verbose": 0, "eps_abs": 1e-8, "eps_rel": 1e-8}
    # default eps + polish against eps = 1e-8, both as one call from nothing and as a solve of a problem that is set up
    t, (status, x, z, y) = _timed(lambda: osqp.qp(q, G, W["h"], P=P, options=tight))
    out["osqp.qp eps 1e-8 seconds"] = t
    out["osqp.qp eps 1e-8 residuals"] = _residuals(W, G, P, x, z)
    def whole():
        with osqp.Problem(q, G, l, u, P, options={"verbose": 0, "polish": 1}) as Q:
            return Q.solve(), dict(Q.info)
    t, ((status, x, z), info) = _timed(whole)
    out["Problem + solve, default eps + polish, seconds"] = t
    out["polish"] = {k: info[k] for k in ("status", "status_polish", "iterations", "factorisations", "active_lower", "active_upper",
                                          "pri_res", "dua_res", "pri_res_polish", "dua_res_polish")}
    out["polished residuals recomputed"] = _residuals(W, G, P, x, z)
    for name, opts in (("default eps + polish", {"verbose": 0, "polish": 1, "warm_start": 0}), ("eps 1e-8", dict(tight, warm_start=0))):
        with osqp.Problem(q, G, l, u, P, options=opts) as Q:
            Q.solve()
            t, _ = _timed(Q.solve)                                      # from zero again on the kept plan, analysis and buffers
            out["kept problem, solve() alone, %s, seconds" % name] = t
            out["kept problem, solve() alone, %s, iterations / factorisations" % name] = [Q.info["iterations"], Q.info["factorisations"]]
    # a parametric sequence: q_k = q + 0.1 noise_k
    rng = np.random.default_rng(40)
    qs = [q + 0.1 * rng.standard_normal(n) for _ in range(steps)]
    for name, warm in (("warm", 1), ("cold", 0)):
        with osqp.Problem(q, G, l, u, P, options={"verbose": 0, "warm_start": warm}) as Q:
            Q.solve()
            its = []
            def sequence():
                for qk in qs:
                    Q.update(q=qk)
                    Q.solve()
                    its.append(Q.info["iterations"])
            t, _ = _timed(sequence)
            out["%d x update(q) + solve(), %s, seconds" % (steps, name)] = t
            out["%d x update(q) + solve(), %s, iterations" % (steps, name)] = int(sum(its))
            out["%d x update(q) + solve(), %s, factorisations" % (steps, name)] = Q.info["factorisations"]
    t, _ = _timed(lambda: [osqp.qp(qk, G, W["h"], P=P, options={"verbose": 0}) for qk in qs])
    out["%d x osqp.qp on the same data, seconds" % steps] = t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gx", type=int, default=40)
    ap.add_argument("--gy", type=int, default=30)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    _lib.require_device()
    W = workloads.qp_grid(a.gx, a.gy)
    n, m = W["n"], W["ml"]
    G = spmatrix.from_ccs(m, n, W["Gp"], W["Gi"], W["Gx"])
    P = spmatrix.from_ccs(n, n, W["Pp"], W["Pi"], W["Px"])
    opts = {"verbose": 0, "eps_abs": a.eps, "eps_rel": a.eps}
    out = {"problem": "qp_grid(%d, %d)" % (a.gx, a.gy), "n": n, "m": m, "eps": a.eps}
    for name in ("first solve seconds", "solve seconds"):               # the first call also pays for the library's start-up
        stats = {}
        _sync()
        t = time.perf_counter()
        status, x, z, y = osqp.qp(W["q"], G, W["h"], P=P, options=opts, _stats=stats)
        _sync()
        out[name] = time.perf_counter() - t
    out.update({"status": status, "iterations": stats["iterations"], "factorisations": stats["factorisations"], "nnz(S)": stats["snz"]})
    # one iteration: k iterations per call, one host read at the end
    Acc, l, u = osqp.resize_problem((m, n, W["Gp"], W["Gi"], W["Gx"]), W["h"], None, None)
    S = osqp._Solver(W["q"], Acc, l, u, (W["Pp"], W["Pi"], W["Px"]), 10).setup()
    S.iterate(a.reps)
    _sync()
    t = time.perf_counter()
    S.iterate(a.reps)
    _sync()
    out["ms per iteration"] = 1e3 * (time.perf_counter() - t) / a.reps
    t = time.perf_counter()
    for _ in range(20):
        S.iterate(0)
    out["ms per check (residuals + host read)"] = 1e3 * (time.perf_counter() - t) / 20
    Sp, Si = S.pattern()
    S.close()
    F = Factor(n, Sp, Si, "L")
    vals = np.where(Si == np.repeat(np.arange(n), np.diff(Sp)), 64.0, -0.5)
    F.factorize(vals)
    b = _lib.DeviceBuffer.from_array(np.ones(n))
    F.solve_dev(b.ptr)
    t = time.perf_counter()
    for _ in range(a.reps):
        F.solve_dev(b.ptr, sync=False)
    _sync()
    out["ms per solve"] = 1e3 * (time.perf_counter() - t) / a.reps
    out["ms per iteration in the two kernels"] = out["ms per iteration"] - out["ms per solve"]
    t = time.perf_counter()
    sol = solvers.qp(P, W["q"], G, W["h"], options={"show_progress": False})
    _sync()
    out["solvers.qp (interior point) seconds"] = time.perf_counter() - t
    out["solvers.qp iterations"] = sol["iterations"]
    out["|x - x_ip|_inf"] = float(np.abs(x - np.asarray(sol["x"]).reshape(-1)).max())
    kept_problem(W, G, P, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
