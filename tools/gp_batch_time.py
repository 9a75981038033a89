"""Time solvers.gp_batch against the only way to do the same work without it, a loop of this package's one-problem driver
(solvers.gp, refinement 0) over some of the same members on the same device, scaled to the batch.

    python tools/gp_batch_time.py [--B 4096] [--n 12 --K 6,4,4,3,3,2 --ml 24 --p 2] [--loop 64] [--reps 5]

B feasible members with matrices of their own from tests/gp_batch_numpy.members: a point strictly feasible for every row, box rows
at the head of G, orthonormal rows in A.  Timed by the host clock around calls that end in a device synchronise, alternating, after
one untimed pass of each (the clocks are left as the machine has them; the spread shows their state):

    batch         solvers.gp_batch(K, F, g, G, h, A, b): the upload of all data, the launch, the download of all results
    launch        kvx_gp_batch_solve_dev on buffers already on the device: the one launch alone
    one by one    solvers.gp (refinement 0) on each of the first --loop members

Printed: the median and the spread (min - max) of each, the times per member and per iteration, the members' iteration counts, the
ratio of the loop, scaled to B members, to the batch, and how many of the loop's members agree with the batch in status and count.
The last line is the result as JSON.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gp_batch_numpy as R  # noqa: E402
from kvxopt_amd import _lib, gpbatch, solvers  # noqa: E402
from tools.socp_batch_time import resident  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--n", type=int, default=R.TIMING[0])
    ap.add_argument("--K", type=str, default=",".join(str(k) for k in R.TIMING[1]))
    ap.add_argument("--ml", type=int, default=R.TIMING[2])
    ap.add_argument("--p", type=int, default=R.TIMING[3])
    ap.add_argument("--loop", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=41)
    a = ap.parse_args()
    _lib.require_device()
    K = [int(k) for k in a.K.split(",")]
    B, n, ml, p, m = a.B, a.n, a.ml, a.p, len(K)
    N = m + ml
    M = R.members(n, K, ml, p, B, a.seed)
    args = R.batch_args(M)
    quiet = {"show_progress": False, "refinement": 0}

    def batch():
        t0 = time.perf_counter()
        sol = solvers.gp_batch(*args)
        return time.perf_counter() - t0, sol

    opt, _, data = gpbatch._prepare(*args, None)
    keep, out, dargs = resident(data, B, (n, p, N, N, 8, 1, 1))
    scratch = _lib.DeviceBuffer(8 * B * _lib.lib().kvx_gp_batch_scratch_doubles(n, m - 1, ml, p))
    Kv = np.asarray(K, dtype=np.int64)
    cargs = [B, n, m - 1, _lib.pi(Kv), ml, p] + dargs + [opt.maxiters, opt.abstol, opt.reltol, opt.feastol] + [o.ptr for o in out] + [scratch.ptr]

    def launch():
        t0 = time.perf_counter()
        _lib.raise_for(_lib.lib().kvx_gp_batch_solve_dev(*cargs), "kvx_gp_batch_solve_dev")
        return time.perf_counter() - t0

    def one_by_one():
        t0 = time.perf_counter()
        sols = [solvers.gp(*R.member_args(M, k), options=quiet) for k in range(a.loop)]
        return time.perf_counter() - t0, sols

    _, sol = batch()                                       # untimed: code objects, the pool's buffers, the symbolic caches
    launch()
    _, sols = one_by_one()
    x_dev = out[0].download(np.float64, n * B).reshape(B, n).T
    same = bool(np.array_equal(x_dev, sol["x"], equal_nan=True))
    diff = max(float(np.linalg.norm(np.asarray(o["x"]).reshape(-1) - sol["x"][:, k]) / max(1.0, np.linalg.norm(o["x"]))) for k, o in enumerate(sols))
    apart = [(k, o["status"], o["iterations"], sol["status"][k], int(sol["iterations"][k])) for k, o in enumerate(sols)
             if o["status"] != sol["status"][k] or o["iterations"] != sol["iterations"][k]]
    tb, tl, to = [], [], []
    for _ in range(a.reps):
        tb.append(batch()[0] * 1e3)
        tl.append(launch() * 1e3)
        to.append(one_by_one()[0] * 1e3)
    mb, mlch, mo = (statistics.median(t) for t in (tb, tl, to))
    its = sol["iterations"]
    ratio = (mo / a.loop) / (mb / B)
    print("B = %d members at (n, K, ml, p) = (%d, %s, %d, %d), N = %d, l = %d: %d optimal, iterations %d - %d (mean %.2f), exits %s"
          % (B, n, K, ml, p, N, sum(K), sol["status"].count("optimal"), its.min(), its.max(), its.mean(), sorted(set(sol["exit"].tolist()))))
    print("batch       %10.2f ms (%.2f - %.2f)   %8.2f us per member" % (mb, min(tb), max(tb), 1e3 * mb / B))
    print("launch      %10.2f ms (%.2f - %.2f)   %8.2f us per member, %.3f us per member and iteration"
          % (mlch, min(tl), max(tl), 1e3 * mlch / B, 1e3 * mlch / its.sum()))
    print("one by one  %10.2f ms (%.2f - %.2f) for %d members: %.2f ms per solvers.gp call; scaled to B members / batch = %.0f"
          % (mo, min(to), max(to), a.loop, mo / a.loop, ratio))
    print("the launch gives the bytes of the batch: %s; solvers.gp and the batch agree on status and count in %d of %d members; "
          "max |x - x_gp| / max(1, |x_gp|) = %.2e" % (same, a.loop - len(apart), a.loop, diff))
    for k, st, it, bst, bit in apart:
        print("member %d: solvers.gp %s after %d, the batch %s after %d" % (k, st, it, bst, bit))
    print(json.dumps({"B": B, "n": n, "K": K, "ml": ml, "p": p, "N": N, "reps": a.reps, "optimal": sol["status"].count("optimal"),
                      "iterations_min": int(its.min()), "iterations_max": int(its.max()), "iterations_mean": float(its.mean()),
                      "batch_ms": mb, "batch_ms_min": min(tb), "batch_ms_max": max(tb), "batch_us_per_member": 1e3 * mb / B,
                      "launch_ms": mlch, "launch_ms_min": min(tl), "launch_ms_max": max(tl), "launch_us_per_member": 1e3 * mlch / B,
                      "launch_us_per_member_iteration": 1e3 * mlch / float(its.sum()),
                      "loop_members": a.loop, "one_by_one_ms": mo, "one_by_one_ms_min": min(to), "one_by_one_ms_max": max(to),
                      "gp_ms_per_call": mo / a.loop, "ratio_loop_scaled_to_batch": ratio, "launch_bytes_equal_batch": same,
                      "status_and_count_agree": a.loop - len(apart), "max_rel_diff_x": diff}))
    for d, _ in keep:
        if d is not None:
            d.free()
    for o in out + [scratch]:
        o.free()


if __name__ == "__main__":
    main()
