"""Time solvers.socp_batch against the only way to do the same work without it, a loop of solvers.socp, and its launch against the
launch of lp_batch at the same number of rows.

    python tools/socp_batch_time.py [--B 4096] [--n 32 --ml 16 --q 4 --nq 12 --p 8] [--loop 32] [--reps 5]

B feasible members with matrices of their own, generated from a seed as the tests generate theirs (dense G with 1 added to its
diagonal, h = G x0 + s0, b = A x0, c = -G'z0 - A'y0 with s0, z0 interior to the cone).  Four things are timed by the host clock
around calls that end in a device synchronise, alternating, after one untimed pass of each:

    batch       solvers.socp_batch(c, G, h, dims, A, b): the upload of all data, the launch, the download of all results
    launch      kvx_socp_batch_solve_dev on buffers already on the device: the one launch alone
    lp launch   kvx_lp_batch_solve_dev on resident buffers at (n, N, p), the members of tools/lp_batch_time.py: the same number of
                rows without cones, which states the cost of the cone algebra
    one by one  solvers.socp (refinement 0) on each of the first --loop members

Printed: the median and the spread (min - max) of each, the times per member and per iteration, the members' iteration counts, and
how far the batch and the loop are apart in x.  The last line is the result as JSON.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvxopt_amd import _lib, lpbatch, socpbatch, solvers  # noqa: E402
from tools.lp_batch_time import members as lp_members  # noqa: E402


def interior(ml, q, B, rng):
    parts = [rng.uniform(0.5, 1.5, (B, ml))]
    for m in q:
        u = rng.standard_normal((B, m - 1))
        parts.append(np.concatenate([np.linalg.norm(u, axis=1, keepdims=True) + 0.5 + rng.random((B, 1)), u], axis=1))
    return np.concatenate(parts, axis=1)[:, :, None]


def members(n, ml, q, p, B, seed):
    rng = np.random.default_rng(seed)
    N = ml + sum(q)
    G, A, x0 = rng.standard_normal((B, N, n)), rng.standard_normal((B, p, n)), rng.standard_normal((B, n, 1))
    k = np.arange(min(N, n))
    G[:, k, k] += 1.0
    s0, z0, y0 = interior(ml, q, B, rng), interior(ml, q, B, rng), rng.standard_normal((B, p, 1))
    h = (G @ x0 + s0)[:, :, 0]
    c = -(G.transpose(0, 2, 1) @ z0 + A.transpose(0, 2, 1) @ y0)[:, :, 0]
    return np.asfortranarray(c.T), G, np.asfortranarray(h.T), A, np.asfortranarray((A @ x0)[:, :, 0].T)


def resident(prepared, B, rows):
    """The arrays of a _prepare on the device and result buffers of the given row counts."""
    dev = [(None if v is None else _lib.DeviceBuffer.from_array(v), s) for v, s in prepared]
    out = [_lib.DeviceBuffer(8 * max(1, r * B)) for r in rows]
    args = []
    for d, s in dev:
        args += [None if d is None else d.ptr, s]
    return dev, out, args


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--ml", type=int, default=16)
    ap.add_argument("--q", type=int, default=4)
    ap.add_argument("--nq", type=int, default=12)
    ap.add_argument("--p", type=int, default=8)
    ap.add_argument("--loop", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=41)
    a = ap.parse_args()
    _lib.require_device()
    B, n, ml, p, q = a.B, a.n, a.ml, a.p, [a.q] * a.nq
    N = ml + sum(q)
    dims = {"l": ml, "q": q, "s": []}
    c, G, h, A, b = members(n, ml, q, p, B, a.seed)
    if not p:
        A = b = None
    quiet = {"show_progress": False, "refinement": 0}
    off = [ml + a.q * k for k in range(a.nq + 1)]

    def batch():
        t0 = time.perf_counter()
        sol = solvers.socp_batch(c, G, h, dims, A, b)
        return time.perf_counter() - t0, sol

    opt, _, data = socpbatch._prepare(c, G, h, dims, A, b, None)
    keep, out, dargs = resident(data, B, (n, p, N, N, 10, 1, 1))
    qv = np.asarray(q, dtype=np.int64)
    args = [B, n, ml, len(q), _lib.pi(qv) if q else None, p] + dargs + [opt.maxiters, opt.abstol, opt.reltol, opt.feastol] + [o.ptr for o in out]

    def launch():
        t0 = time.perf_counter()
        _lib.raise_for(_lib.lib().kvx_socp_batch_solve_dev(*args), "kvx_socp_batch_solve_dev")
        return time.perf_counter() - t0

    lc, lG, lh, lA, lb = lp_members(n, N, p, B, a.seed)
    lopt, _, ldata = lpbatch._prepare(lc, lG, lh, lA if p else None, lb if p else None, None)
    lkeep, lout, ldargs = resident(ldata, B, (n, p, N, N, 10, 1, 1))
    largs = [B, n, N, p] + ldargs + [lopt.maxiters, lopt.abstol, lopt.reltol, lopt.feastol] + [o.ptr for o in lout]

    def lp_launch():
        t0 = time.perf_counter()
        _lib.raise_for(_lib.lib().kvx_lp_batch_solve_dev(*largs), "kvx_lp_batch_solve_dev")
        return time.perf_counter() - t0

    def one_by_one():
        t0 = time.perf_counter()
        sols = [solvers.socp(c[:, k], G[k, :ml] if ml else None, h[:ml, k] if ml else None,
                             [G[k, off[j]:off[j + 1]] for j in range(a.nq)], [h[off[j]:off[j + 1], k] for j in range(a.nq)],
                             None if A is None else A[k], None if b is None else b[:, k], options=quiet) for k in range(a.loop)]
        return time.perf_counter() - t0, sols

    _, sol = batch()                                       # untimed: code objects, the pool's buffers, the symbolic caches
    launch()
    lp_launch()
    _, sols = one_by_one()
    x_dev = out[0].download(np.float64, n * B).reshape(B, n).T
    same = bool(np.array_equal(x_dev, sol["x"], equal_nan=True))
    lp_its = lout[5].download(np.int64, B)
    diff = max(float(np.linalg.norm(s["x"] - sol["x"][:, k]) / max(1.0, np.linalg.norm(s["x"]))) for k, s in enumerate(sols)
               if s["x"] is not None)
    apart = [(k, s["status"], s["iterations"], sol["status"][k], int(sol["iterations"][k])) for k, s in enumerate(sols)
             if s["status"] != sol["status"][k] or s["iterations"] != sol["iterations"][k]]
    agree = not apart
    tb, tl, tp, to = [], [], [], []
    for _ in range(a.reps):
        tb.append(batch()[0] * 1e3)
        tl.append(launch() * 1e3)
        tp.append(lp_launch() * 1e3)
        to.append(one_by_one()[0] * 1e3)
    mb, mlch, mlp, mo = (statistics.median(t) for t in (tb, tl, tp, to))
    its = sol["iterations"]
    print("B = %d members at (n, ml, q, p) = (%d, %d, [%d] x %d, %d), N = %d: %d optimal, iterations %d - %d (mean %.2f)"
          % (B, n, ml, a.q, a.nq, p, N, sol["status"].count("optimal"), its.min(), its.max(), its.mean()))
    print("batch       %10.2f ms (%.2f - %.2f)   %8.2f us per member" % (mb, min(tb), max(tb), 1e3 * mb / B))
    print("launch      %10.2f ms (%.2f - %.2f)   %8.2f us per member, %.3f us per member and iteration"
          % (mlch, min(tl), max(tl), 1e3 * mlch / B, 1e3 * mlch / its.sum()))
    print("lp launch   %10.2f ms (%.2f - %.2f)   %8.2f us per member, %.3f us per member and iteration at (n, ml, p) = (%d, %d, %d), iterations mean %.2f"
          % (mlp, min(tp), max(tp), 1e3 * mlp / B, 1e3 * mlp / lp_its.sum(), n, N, p, lp_its.mean()))
    print("one by one  %10.2f ms (%.2f - %.2f) for %d members: %.2f ms per solvers.socp call" % (mo, min(to), max(to), a.loop, mo / a.loop))
    print("the launch gives the bytes of the batch: %s; solvers.socp and the batch agree on status and count: %s; max |x - x_socp| / max(1, |x_socp|) = %.2e"
          % (same, agree, diff))
    for k, st, it, bst, bit in apart:
        print("member %d: solvers.socp %s after %d, the batch %s after %d" % (k, st, it, bst, bit))
    print(json.dumps({"B": B, "n": n, "ml": ml, "q": q, "p": p, "N": N, "reps": a.reps, "optimal": sol["status"].count("optimal"),
                      "iterations_min": int(its.min()), "iterations_max": int(its.max()), "iterations_mean": float(its.mean()),
                      "batch_ms": mb, "batch_ms_min": min(tb), "batch_ms_max": max(tb),
                      "launch_ms": mlch, "launch_ms_min": min(tl), "launch_ms_max": max(tl), "launch_us_per_member": 1e3 * mlch / B,
                      "launch_us_per_member_iteration": 1e3 * mlch / float(its.sum()),
                      "lp_launch_ms": mlp, "lp_launch_ms_min": min(tp), "lp_launch_ms_max": max(tp), "lp_iterations_mean": float(lp_its.mean()),
                      "lp_launch_us_per_member_iteration": 1e3 * mlp / float(lp_its.sum()),
                      "loop_members": a.loop, "one_by_one_ms": mo, "one_by_one_ms_min": min(to), "one_by_one_ms_max": max(to),
                      "socp_ms_per_call": mo / a.loop, "launch_bytes_equal_batch": same, "status_and_count_agree": agree, "max_rel_diff_x": diff}))


if __name__ == "__main__":
    main()
