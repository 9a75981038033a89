"""Time solvers.coneqp_batch against the only way to do the same work without it, a loop of this package's one-problem driver
(solvers.coneqp, refinement 0) over some of the same members on the same device, scaled to the batch, and its launch alone beside
the launch of conelp_batch on the members' linear parts.

    python tools/coneqp_batch_time.py [--B 4096] [--n 24 --ml 8 --q 4 --nq 4 --m 5 --ns 1 --p 4] [--loop 64] [--reps 5]

B feasible members with matrices of their own: those of tools/conelp_batch_time.py (dense G with symmetric 's' blocks and 1 added to
its diagonal, h = G x0 + s0, b = A x0 with s0 interior to the whole cone) with P = F F' + 1e-2 I and the linear term moved by -P x1,
x1 random, so that (x0, s0) stays strictly feasible for the primal and (y0, z0) for the dual.  Timed by the host clock around
calls that end in a device synchronise, alternating, after one untimed pass of each (the clocks are left as the machine has them;
the spread shows their state):

    batch         solvers.coneqp_batch(P, q, G, h, dims, A, b): the upload of all data, the launch, the download of all results
    launch        kvx_coneqp_batch_solve_dev on buffers already on the device: the one launch alone
    one by one    solvers.coneqp (refinement 0) on each of the first --loop members
    conelp        kvx_conelp_batch_solve_dev on the same G, h, A, b with the linear term of tools/conelp_batch_time.py

Printed: the median and the spread (min - max) of each, the times per member and per iteration, the members' iteration counts, the
ratio of the loop, scaled to B members, to the batch, and how far the batch and the loop are apart in x.  The last line is the
result as JSON.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvxopt_amd import _lib, conelpbatch, coneqpbatch, solvers  # noqa: E402
from tools import conelp_batch_time  # noqa: E402
from tools.socp_batch_time import resident  # noqa: E402


def members(n, ml, q, s, p, B, seed):
    """(P, q, G, h, A, b) and the linear term c of the cone LP on the same G, h, A, b."""
    c, G, h, A, b = conelp_batch_time.members(n, ml, q, s, p, B, seed)
    rng = np.random.default_rng(seed + 1000003)
    F = rng.standard_normal((B, n, n))
    P = F @ F.transpose(0, 2, 1) + 1e-2 * np.eye(n)
    # the LP's primal point stays feasible, and with q = c - P x1 its dual point (y0, z0) is feasible for the QP at any x1:
    # P x1 + q + G'z0 + A'y0 = c + G'z0 + A'y0 = 0
    x1 = rng.standard_normal((B, n, 1))
    qv = c - np.asfortranarray((P @ x1)[:, :, 0].T)
    return P, np.asfortranarray(qv), G, h, A, b, c


def dev_launch(entry, prepared, dims, nstat, cone, tail):
    """A function that times one launch of `entry` on resident copies of the prepared members, and its result buffers."""
    opt, sizes, data = prepared
    B, n, N, p = sizes[0], sizes[1], sizes[-2], sizes[-1]
    keep, out, dargs = resident(data, B, (n, p, N, N, nstat, 1, 1))
    arrays = [np.asarray(v, dtype=np.int64) for v in cone]
    head = [B, n, int(dims["l"])]
    for v in arrays:
        head += [len(v), _lib.pi(v) if len(v) else None]
    args = head + [p] + dargs + [opt.maxiters, opt.abstol, opt.reltol, opt.feastol] + tail + [o.ptr for o in out]

    def launch():
        t0 = time.perf_counter()
        _lib.raise_for(getattr(_lib.lib(), entry)(*args), entry)
        return time.perf_counter() - t0
    launch.keep = (keep, arrays)
    return launch, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--n", type=int, default=24)
    ap.add_argument("--ml", type=int, default=8)
    ap.add_argument("--q", type=int, default=4)
    ap.add_argument("--nq", type=int, default=4)
    ap.add_argument("--m", type=int, default=5)
    ap.add_argument("--ns", type=int, default=1)
    ap.add_argument("--p", type=int, default=4)
    ap.add_argument("--loop", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=41)
    a = ap.parse_args()
    _lib.require_device()
    B, n, ml, p, q, s = a.B, a.n, a.ml, a.p, [a.q] * a.nq, [a.m] * a.ns
    N = ml + sum(q) + sum(m * m for m in s)
    dims = {"l": ml, "q": q, "s": s}
    P, qv, G, h, A, b, c = members(n, ml, q, s, p, B, a.seed)
    if not p:
        A = b = None
    quiet = {"show_progress": False, "refinement": 0}

    def batch():
        t0 = time.perf_counter()
        sol = solvers.coneqp_batch(P, qv, G, h, dims, A, b)
        return time.perf_counter() - t0, sol

    launch, out = dev_launch("kvx_coneqp_batch_solve_dev", coneqpbatch._prepare(P, qv, G, h, dims, A, b, None), dims, 8, [q, s], [1])
    lp_launch, lp_out = dev_launch("kvx_conelp_batch_solve_dev", conelpbatch._prepare(c, G, h, dims, A, b, None), dims, 10, [q, s], [])

    def one_by_one():
        t0 = time.perf_counter()
        sols = [solvers.coneqp(P[k], qv[:, k], G[k], h[:, k], dims, None if A is None else A[k], None if b is None else b[:, k],
                               options=quiet) for k in range(a.loop)]
        return time.perf_counter() - t0, sols

    _, sol = batch()                                       # untimed: code objects, the pool's buffers, the symbolic caches
    launch()
    lp_launch()
    _, sols = one_by_one()
    x_dev = out[0].download(np.float64, n * B).reshape(B, n).T
    same = bool(np.array_equal(x_dev, sol["x"], equal_nan=True))
    lp_its = lp_out[5].download(np.int64, B)
    diff = max(float(np.linalg.norm(np.asarray(o["x"]).reshape(-1) - sol["x"][:, k]) / max(1.0, np.linalg.norm(o["x"]))) for k, o in enumerate(sols))
    apart = [(k, o["status"], o["iterations"], sol["status"][k], int(sol["iterations"][k])) for k, o in enumerate(sols)
             if o["status"] != sol["status"][k] or o["iterations"] != sol["iterations"][k]]
    tb, tl, tc, to = [], [], [], []
    for _ in range(a.reps):
        tb.append(batch()[0] * 1e3)
        tl.append(launch() * 1e3)
        tc.append(lp_launch() * 1e3)
        to.append(one_by_one()[0] * 1e3)
    mb, mlch, mc, mo = (statistics.median(t) for t in (tb, tl, tc, to))
    its = sol["iterations"]
    ratio = (mo / a.loop) / (mb / B)
    print("B = %d members at (n, ml, q, s, p) = (%d, %d, [%d] x %d, [%d] x %d, %d), N = %d: %d optimal, iterations %d - %d (mean %.2f)"
          % (B, n, ml, a.q, a.nq, a.m, a.ns, p, N, sol["status"].count("optimal"), its.min(), its.max(), its.mean()))
    print("batch       %10.2f ms (%.2f - %.2f)   %8.2f us per member" % (mb, min(tb), max(tb), 1e3 * mb / B))
    print("launch      %10.2f ms (%.2f - %.2f)   %8.2f us per member, %.3f us per member and iteration"
          % (mlch, min(tl), max(tl), 1e3 * mlch / B, 1e3 * mlch / its.sum()))
    print("conelp      %10.2f ms (%.2f - %.2f)   %8.2f us per member, %.3f us per member and iteration (mean %.2f iterations)"
          % (mc, min(tc), max(tc), 1e3 * mc / B, 1e3 * mc / lp_its.sum(), lp_its.mean()))
    print("one by one  %10.2f ms (%.2f - %.2f) for %d members: %.2f ms per solvers.coneqp call; scaled to B members / batch = %.0f"
          % (mo, min(to), max(to), a.loop, mo / a.loop, ratio))
    print("the launch gives the bytes of the batch: %s; solvers.coneqp and the batch agree on status and count: %s; max |x - x_coneqp| / max(1, |x_coneqp|) = %.2e"
          % (same, not apart, diff))
    for k, st, it, bst, bit in apart:
        print("member %d: solvers.coneqp %s after %d, the batch %s after %d" % (k, st, it, bst, bit))
    print(json.dumps({"B": B, "n": n, "ml": ml, "q": q, "s": s, "p": p, "N": N, "reps": a.reps, "optimal": sol["status"].count("optimal"),
                      "iterations_min": int(its.min()), "iterations_max": int(its.max()), "iterations_mean": float(its.mean()),
                      "batch_ms": mb, "batch_ms_min": min(tb), "batch_ms_max": max(tb), "batch_us_per_member": 1e3 * mb / B,
                      "launch_ms": mlch, "launch_ms_min": min(tl), "launch_ms_max": max(tl), "launch_us_per_member": 1e3 * mlch / B,
                      "launch_us_per_member_iteration": 1e3 * mlch / float(its.sum()),
                      "conelp_launch_ms": mc, "conelp_launch_ms_min": min(tc), "conelp_launch_ms_max": max(tc),
                      "conelp_us_per_member_iteration": 1e3 * mc / float(lp_its.sum()), "conelp_iterations_mean": float(lp_its.mean()),
                      "loop_members": a.loop, "one_by_one_ms": mo, "one_by_one_ms_min": min(to), "one_by_one_ms_max": max(to),
                      "coneqp_ms_per_call": mo / a.loop, "ratio_loop_scaled_to_batch": ratio, "launch_bytes_equal_batch": same,
                      "status_and_count_agree": not apart, "max_rel_diff_x": diff}))


if __name__ == "__main__":
    main()
