"""Time of one osqp solve on workloads.qp_grid(gx, gy): iterations, factorisations, milliseconds per iteration and the split of an
iteration between the triangular solve and the two ADMM kernels.  Every timed part ends with a device synchronisation.  The
solve alone is timed on a second factor of the same pattern (a diagonally dominant matrix on the pattern of S: the time of a
sweep depends on the pattern only).  No thresholds: the numbers are printed as JSON.

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
    print(json.dumps(out))


if __name__ == "__main__":
    main()
