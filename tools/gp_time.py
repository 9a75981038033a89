"""Time of one geometric program (solvers.gp) and of one evaluation of its log-sum-exp blocks (kvx_gp_eval_dev), with and
without the Hessian.  Every timed part ends with a device synchronisation.  No thresholds: the numbers are printed as JSON.

    python tools/gp_time.py [--blocks M] [--terms K] [--n N] [--density D] [--reps R]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from kvxopt_amd import _lib, cvx, solvers  # noqa: E402
from kvxopt_amd.base import ccs, matrix, spmatrix  # noqa: E402
from kvxopt_amd.devvec import DVec  # noqa: E402


def _sync():
    _lib.raise_for(_lib.lib().kvx_dev_sync())


def problem(m, kterms, n, density, seed=0):
    """m constraints of kterms terms each and an objective, strictly feasible at x = 0 (f_i(0) = -1), boxed by |x| <= 10."""
    rng = np.random.default_rng(seed)
    K = [kterms] * (m + 1)
    l = sum(K)
    mask = rng.random((l, n)) < density
    mask[np.arange(l), rng.integers(0, n, l)] = True
    I, J = np.nonzero(mask)
    F = spmatrix(rng.standard_normal(I.size), I, J, (l, n))
    g = rng.standard_normal(l)
    for i in range(1, m + 1):
        blk = slice(i * kterms, (i + 1) * kterms)
        g[blk] -= np.log(np.exp(g[blk]).sum()) + 1.0
    G = spmatrix(np.concatenate([np.ones(n), -np.ones(n)]), np.arange(2 * n), np.tile(np.arange(n), 2), (2 * n, n))
    return K, F, matrix(g), G, matrix(np.full(2 * n, 10.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2000)
    ap.add_argument("--terms", type=int, default=8)
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    _lib.require_device()
    K, F, g, G, h = problem(a.blocks, a.terms, a.n, a.density)
    _, n, Fp, Fi, Fx = ccs(F)
    ev = cvx.GPEval(K, n, Fp, Fi, Fx, g._a)
    x, z, f = DVec(n).fill(0.0), DVec(len(K)).fill(1.0), DVec(len(K))
    Dfx, Hx = DVec(ev.Dfi.size), DVec(max(ev.Hi.size, 1))
    out = {"blocks": len(K), "terms": a.terms, "n": n, "nnz(F)": int(Fx.size), "nnz(Df)": int(ev.Dfi.size), "nnz(tril H)": int(ev.Hi.size)}
    for name, zz in (("eval f, Df seconds", None), ("eval f, Df, H seconds", z)):
        ev.eval(x, zz, f, Dfx, Hx)
        _sync()
        t = time.perf_counter()
        for _ in range(a.reps):
            ev.eval(x, zz, f, Dfx, Hx)
        _sync()
        out[name] = (time.perf_counter() - t) / a.reps
    solve = lambda: solvers.gp(K, F, g, G, h, options={"show_progress": False})
    solve()
    _sync()
    t = time.perf_counter()
    sol = solve()
    _sync()
    out.update({"solve seconds": time.perf_counter() - t, "status": sol["status"], "iterations": sol["iterations"]})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
