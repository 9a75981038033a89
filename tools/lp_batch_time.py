"""Time solvers.lp_batch against the only way to do the same work without it, a loop of solvers.lp.

    python tools/lp_batch_time.py [--B 4096] [--n 32 --ml 64 --p 8] [--loop 32] [--reps 5]

B members with matrices of their own, generated from a seed as the tests generate their feasible ones: h = G x0 + U(0.1, 1),
b = A x0, c = -G'z0 - A'y0 with z0 ~ U(0.5, 1.5).  Three things are timed by the host clock around calls that end in a device
synchronise, alternating, after one untimed pass of each:

    batch       solvers.lp_batch(c, G, h, A, b): the upload of all data, the launch, the download of all results
    launch      kvx_lp_batch_solve_dev on buffers already on the device: the one launch alone
    one by one  solvers.lp on each of the first --loop members

Printed: the median and the spread (min - max) of each, the launch time per member, the time of one solvers.lp call, the
members' iteration counts, and how far the two ways are apart in x.  The last line is the result as JSON.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvxopt_amd import _lib, lpbatch, solvers  # noqa: E402


def members(n, ml, p, B, seed):
    rng = np.random.default_rng(seed)
    G, A, x0 = rng.standard_normal((B, ml, n)), rng.standard_normal((B, p, n)), rng.standard_normal((B, n, 1))
    h = (G @ x0)[:, :, 0] + rng.uniform(0.1, 1.0, (B, ml))
    z0, y0 = rng.uniform(0.5, 1.5, (B, ml, 1)), rng.standard_normal((B, p, 1))
    c = -(G.transpose(0, 2, 1) @ z0 + A.transpose(0, 2, 1) @ y0)[:, :, 0]
    return np.asfortranarray(c.T), G, np.asfortranarray(h.T), A, np.asfortranarray((A @ x0)[:, :, 0].T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--ml", type=int, default=64)
    ap.add_argument("--p", type=int, default=8)
    ap.add_argument("--loop", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=41)
    a = ap.parse_args()
    _lib.require_device()
    B, n, ml, p = a.B, a.n, a.ml, a.p
    c, G, h, A, b = members(n, ml, p, B, a.seed)
    if not p:
        A = b = None
    quiet = {"show_progress": False}

    def batch():
        t0 = time.perf_counter()
        sol = solvers.lp_batch(c, G, h, A, b)
        return time.perf_counter() - t0, sol

    # the launch alone: the arrays of lp_batch, uploaded once
    opt, _, data = lpbatch._prepare(c, G, h, A, b, None)
    dev = [(None if v is None else _lib.DeviceBuffer.from_array(v), s) for v, s in data]
    out = [_lib.DeviceBuffer(8 * max(1, rows * B)) for rows in (n, p, ml, ml, 10, 1, 1)]
    args = [B, n, ml, p]
    for d, s in dev:
        args += [None if d is None else d.ptr, s]
    args += [opt.maxiters, opt.abstol, opt.reltol, opt.feastol] + [o.ptr for o in out]

    def launch():
        t0 = time.perf_counter()
        _lib.raise_for(_lib.lib().kvx_lp_batch_solve_dev(*args), "kvx_lp_batch_solve_dev")
        return time.perf_counter() - t0

    def one_by_one():
        t0 = time.perf_counter()
        sols = [solvers.lp(c[:, k], G[k], h[:, k], None if A is None else A[k], None if b is None else b[:, k], options=quiet)
                for k in range(a.loop)]
        return time.perf_counter() - t0, sols

    _, sol = batch()                                       # untimed: code objects, the pool's buffers, the symbolic caches
    launch()
    _, sols = one_by_one()
    x_dev = out[0].download(np.float64, n * B).reshape(B, n).T
    same = bool(np.array_equal(x_dev, sol["x"], equal_nan=True))
    diff = max(float(np.linalg.norm(s["x"] - sol["x"][:, k]) / max(1.0, np.linalg.norm(s["x"]))) for k, s in enumerate(sols)
               if s["x"] is not None)
    agree = all(s["status"] == sol["status"][k] and s["iterations"] == sol["iterations"][k] for k, s in enumerate(sols))
    tb, tl, to = [], [], []
    for _ in range(a.reps):
        tb.append(batch()[0] * 1e3)
        tl.append(launch() * 1e3)
        to.append(one_by_one()[0] * 1e3)
    mb, mlch, mo = statistics.median(tb), statistics.median(tl), statistics.median(to)
    its = sol["iterations"]
    print("B = %d members at (n, ml, p) = (%d, %d, %d): %d optimal, iterations %d - %d (mean %.2f)"
          % (B, n, ml, p, sol["status"].count("optimal"), its.min(), its.max(), its.mean()))
    print("batch       %10.2f ms (%.2f - %.2f)   %8.2f us per member" % (mb, min(tb), max(tb), 1e3 * mb / B))
    print("launch      %10.2f ms (%.2f - %.2f)   %8.2f us per member" % (mlch, min(tl), max(tl), 1e3 * mlch / B))
    print("one by one  %10.2f ms (%.2f - %.2f) for %d members: %.2f ms per solvers.lp call" % (mo, min(to), max(to), a.loop, mo / a.loop))
    print("the launch gives the bytes of the batch: %s; solvers.lp and the batch agree on status and count: %s; max |x - x_lp| / max(1, |x_lp|) = %.2e"
          % (same, agree, diff))
    print(json.dumps({"B": B, "n": n, "ml": ml, "p": p, "reps": a.reps, "optimal": sol["status"].count("optimal"),
                      "iterations_min": int(its.min()), "iterations_max": int(its.max()), "iterations_mean": float(its.mean()),
                      "batch_ms": mb, "batch_ms_min": min(tb), "batch_ms_max": max(tb),
                      "launch_ms": mlch, "launch_ms_min": min(tl), "launch_ms_max": max(tl), "launch_us_per_member": 1e3 * mlch / B,
                      "loop_members": a.loop, "one_by_one_ms": mo, "one_by_one_ms_min": min(to), "one_by_one_ms_max": max(to),
                      "lp_ms_per_call": mo / a.loop, "launch_bytes_equal_batch": same, "status_and_count_agree": agree, "max_rel_diff_x": diff}))


if __name__ == "__main__":
    main()
