"""Time osqp.Problem.solve_batch against the same work done one member at a time ("A batch on the kept factor").

    python tools/osqp_batch_time.py [--gx 40 --gy 30] [--sizes 1,8,64,256] [--reps 5]

The problem is workloads.qp_grid(gx, gy) as osqp.qp stacks it, at the default tolerances (eps = 1e-3).  One default solve()
settles rho; member b is q + 0.1 max(1, |q|_inf) N(0, 1) and h + 0.05 N(0, 1) (seed 31).  Per batch size B two ways are timed,
alternating, after one untimed pass of each, by the host clock around calls that end in a device-to-host copy:

    batch        Problem.solve_batch(Q, None, U)
    one by one   B x (update(q_b, u=u_b) + solve()) on a kept problem with adaptive_rho = 0, warm_start = 0 at the same rho

Printed per B: the median and the spread (min - max) of both, the ADMM iterations the batch loop ran (those of its slowest member)
and the time per such iteration, the sum of the members' own iterations and the time per iteration of the one-by-one way, and the
ratio of the two wall clocks.  The last line is the table as JSON.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvxopt_amd import _lib, osqp, workloads  # noqa: E402
from kvxopt_amd.base import matrix, spmatrix  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gx", type=int, default=40)
    ap.add_argument("--gy", type=int, default=30)
    ap.add_argument("--sizes", default="1,8,64,256")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    _lib.require_device()
    W = workloads.qp_grid(args.gx, args.gy)
    n, m = W["n"], W["ml"]
    A = spmatrix.from_ccs(m, n, W["Gp"], W["Gi"], W["Gx"])
    P = spmatrix.from_ccs(n, n, W["Pp"], W["Pi"], W["Px"])
    q, h = np.asarray(W["q"], dtype=np.float64), np.asarray(W["h"], dtype=np.float64)
    l = np.full(m, -osqp.INFTY)
    rng = np.random.default_rng(31)
    Bmax = max(sizes)
    Q, U = np.empty((n, Bmax), order="F"), np.empty((m, Bmax), order="F")
    for b in range(Bmax):
        Q[:, b] = q + 0.1 * max(1.0, np.abs(q).max()) * rng.standard_normal(n)
        U[:, b] = h + 0.05 * rng.standard_normal(m)
    rows = []
    with osqp.Problem(matrix(q), A, matrix(l), matrix(h), P, options={"verbose": 0}) as K:
        status, _, _ = K.solve()
        rho = K.info["rho"]
        print("qp_grid(%d, %d): n = %d, m = %d; base solve %s in %d iterations, rho = %.4g" % (args.gx, args.gy, n, m, status, K.info["iterations"], rho))
        one = {"verbose": 0, "rho": rho, "adaptive_rho": 0, "warm_start": 0}
        with osqp.Problem(matrix(q), A, matrix(l), matrix(h), P, options=one) as S:
            def batch(B):
                t0 = time.perf_counter()
                st, X, _ = K.solve_batch(Q[:, :B], None, U[:, :B])
                return time.perf_counter() - t0, st, X, K.batch_info["iterations"].copy()

            def one_by_one(B):
                t0 = time.perf_counter()
                st, its = [], []
                X = np.empty((n, B), order="F")
                for b in range(B):
                    S.update(q=Q[:, b], u=U[:, b])
                    s, X[:, b], _ = S.solve()
                    st.append(s)
                    its.append(S.info["iterations"])
                return time.perf_counter() - t0, st, X, np.array(its)

            print("%5s %22s %10s %12s %24s %12s %12s %8s" % ("B", "batch ms (min-max)", "loop its", "ms / loop it", "one by one ms (min-max)", "member its",
                                                          "ms / it", "ratio"))
            for B in sizes:
                _, sb, Xb, ib = batch(B)                                # untimed: code objects, graphs, workspaces
                _, so, Xo, io = one_by_one(B)
                if sb != so or not np.array_equal(ib, io):
                    print("B = %d: the two ways disagree on a status or an iteration count" % B)
                diff = float(np.abs(Xb - Xo).max() / max(1.0, np.abs(Xo).max()))
                tb, to = [], []
                for _ in range(args.reps):
                    tb.append(batch(B)[0] * 1e3)
                    to.append(one_by_one(B)[0] * 1e3)
                mb, mo = statistics.median(tb), statistics.median(to)
                loop, total = int(ib.max()), int(io.sum())
                rows.append({"B": B, "batch_ms": mb, "batch_ms_min": min(tb), "batch_ms_max": max(tb), "loop_iterations": loop,
                             "batch_ms_per_iteration": mb / loop, "one_by_one_ms": mo, "one_by_one_ms_min": min(to), "one_by_one_ms_max": max(to),
                             "member_iterations": total, "one_by_one_ms_per_iteration": mo / total, "ratio": mo / mb, "max_rel_diff_x": diff,
                             "frozen_member_iterations": int((loop - ib).sum())})
                print("%5d %10.2f (%.2f-%.2f) %10d %12.4f %12.2f (%.2f-%.2f) %12d %12.4f %8.2f" % (B, mb, min(tb), max(tb), loop, mb / loop, mo, min(to), max(to),
                                                                                                 total, mo / total, mo / mb))
    print(json.dumps({"workload": "qp_grid(%d,%d)" % (args.gx, args.gy), "n": n, "m": m, "rho": rho, "reps": args.reps, "rows": rows}))


if __name__ == "__main__":
    main()
