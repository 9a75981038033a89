"""Time solvers.gp_batch_vjp / gp_batch_jvp against the solve they differentiate and against the only way to a derivative
without them, central differences through solvers.gp_batch.

    python tools/gp_batch_diff_time.py [--B 4096] [--n 12 --K 6,4,4,3,3,2 --ml 24 --p 2] [--reps 5]

B members with matrices of their own from tests/gp_batch_numpy.members, at its TIMING shape by default.  Timed by the host clock
around calls that end in a device synchronise, alternating, after one untimed pass of each:

    vjp all       solvers.gp_batch_vjp with all six gradients: upload, launch, download of B matrices per gradient
    vjp g h b     solvers.gp_batch_vjp(wrt=("g", "h", "b")): no matrix gradient is formed
    jvp           solvers.gp_batch_jvp with perturbations of all six data
    dev vjp all   kvx_gp_batch_vjp_dev on resident buffers, per-member matrix gradients: the launch alone
    dev vjp       kvx_gp_batch_vjp_dev without matrix gradients
    dev vjp sum   kvx_gp_batch_vjp_dev with one F for all members and its summed gradient: the second launch, k_batch_outer_sum,
                  is the difference to `dev vjp`
    dev jvp       kvx_gp_batch_jvp_dev
    dev solve     kvx_gp_batch_solve_dev on the same resident batch: the launch a derivative is to be compared with
    forward       solvers.gp_batch, for scale
    differences   the two solvers.gp_batch calls of one central difference along one direction

Printed: the median and the spread (min - max) of each in ms, the iterations of the solve and the ratio of `dev solve` to the
derivative launches; the last line is the result as JSON.  Needs a GPU.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--n", type=int, default=R.TIMING[0])
    ap.add_argument("--K", type=str, default=",".join(str(k) for k in R.TIMING[1]))
    ap.add_argument("--ml", type=int, default=R.TIMING[2])
    ap.add_argument("--p", type=int, default=R.TIMING[3])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=41)
    a = ap.parse_args()
    _lib.require_device()
    B, n, ml, p, K = a.B, a.n, a.ml, a.p, [int(k) for k in a.K.split(",")]
    m, l = len(K), sum(K)
    N = m + ml
    M = R.members(n, K, ml, p, B, a.seed)
    args = R.batch_args(M)
    rng = np.random.default_rng(a.seed + 1)
    gx = np.asfortranarray(rng.standard_normal((n, B)))
    col = lambda r: np.asfortranarray(rng.standard_normal((r, B))) if r else None                               # noqa: E731
    mat = lambda r: rng.standard_normal((B, r, n)) if r else None                                               # noqa: E731
    d = {"dF": mat(l), "dg": col(l), "dG": mat(ml), "dh": col(ml), "dA": mat(p), "db": col(p)}
    eps = 1e-6
    sol = solvers.gp_batch(*args)

    # the launches alone: everything uploaded once, as the C entries take it
    _, _, data = gpbatch._prepare(*args, None)
    up = lambda v: None if v is None else _lib.DeviceBuffer.from_array(v)                                       # noqa: E731
    cols = lambda v: None if v is None else np.ascontiguousarray(v.T).reshape(-1)                               # noqa: E731
    cm = lambda v: None if v is None else np.ascontiguousarray(v.transpose(0, 2, 1)).reshape(-1)                # noqa: E731
    ptr = lambda buf: None if buf is None else buf.ptr                                                          # noqa: E731
    new = lambda count: _lib.DeviceBuffer(8 * max(count, 1))                                                    # noqa: E731
    (Fd, sF), (gd, sg), (Gd, sG), (hd, sh), (Ad, sA), (bd, sb) = [(up(v), s) for v, s in data]
    x, y, s, z, stats, iters, code = new(n * B), new(p * B), new(N * B), new(N * B), new(8 * B), new(B), new(B)
    L = _lib.lib()
    scratch = new(L.kvx_gp_batch_scratch_doubles(n, m - 1, ml, p) * B)
    Kp = _lib.pi(np.asarray(K, dtype=np.int64))

    def dev_solve():
        rc = L.kvx_gp_batch_solve_dev(B, n, m - 1, Kp, ml, p, Fd.ptr, sF, gd.ptr, sg, ptr(Gd), sG, ptr(hd), sh, ptr(Ad), sA, ptr(bd), sb,
                                      100, 1e-7, 1e-6, 1e-7, x.ptr, ptr(y) if p else None, s.ptr, z.ptr, stats.ptr, iters.ptr, code.ptr, scratch.ptr)
        _lib.raise_for(rc, "kvx_gp_batch_solve_dev")

    dev_solve()                                             # the derivative entries below read its x, y, s, z and exit
    gxd = up(cols(gx))
    ux, uy, uz, us, gg, work = new(n * B), new(p * B), new(N * B), new(N * B), new(l * B), new(l * B)
    gF, gG, gA, gexit = new(B * l * n), new(B * ml * n), new(B * p * n), new(B)
    pert = [(up(cm(d["dF"])), l * n), (up(cols(d["dg"])), l), (up(cm(d["dG"])), ml * n), (up(cols(d["dh"])), ml),
            (up(cm(d["dA"])), p * n), (up(cols(d["db"])), p)]

    def head(sF_):
        return [B, n, m - 1, Kp, ml, p, Fd.ptr, sF_, gd.ptr, sg, ptr(Gd), sG, ptr(Ad), sA, x.ptr, ptr(y) if p else None, s.ptr, z.ptr, code.ptr, 1]

    def dev_vjp(sF_, mats, ws=None):
        rest = [gxd.ptr, ux.ptr, uy.ptr if p else None, uz.ptr, gg.ptr] + mats + [ws, gexit.ptr]
        _lib.raise_for(L.kvx_gp_batch_vjp_dev(*(head(sF_) + rest)), "kvx_gp_batch_vjp_dev")

    def dev_jvp():
        rest = []
        for buf, stride in pert:
            rest += [ptr(buf), stride]
        rest += [ux.ptr, uy.ptr if p else None, uz.ptr, us.ptr, gexit.ptr]
        _lib.raise_for(L.kvx_gp_batch_jvp_dev(*(head(sF) + rest)), "kvx_gp_batch_jvp_dev")

    def moved(t):
        return [args[0]] + [v if dv is None else v + t * dv for v, dv in zip(args[1:], (d["dF"], d["dg"], d["dG"], d["dh"], d["dA"], d["db"]))]

    what = {
        "vjp all": lambda: solvers.gp_batch_vjp(*args, sol=sol, gx=gx),
        "vjp g h b": lambda: solvers.gp_batch_vjp(*args, sol=sol, gx=gx, wrt=("g", "h", "b")),
        "jvp": lambda: solvers.gp_batch_jvp(*args, sol=sol, **d),
        "dev vjp all": lambda: dev_vjp(sF, [gF.ptr, ptr(gG) if ml else None, gA.ptr if p else None]),
        "dev vjp": lambda: dev_vjp(sF, [None, None, None]),
        "dev vjp sum": lambda: dev_vjp(0, [gF.ptr, None, None], work.ptr),
        "dev jvp": dev_jvp,
        "dev solve": dev_solve,
        "forward": lambda: solvers.gp_batch(*args),
        "differences": lambda: [solvers.gp_batch(*moved(eps)), solvers.gp_batch(*moved(-eps))],
    }
    times = {k: [] for k in what}
    for rep in range(a.reps + 1):                           # the first pass is not timed: code objects, the pool's buffers
        for k, fn in what.items():
            t0 = time.perf_counter()
            fn()
            if rep:
                times[k].append((time.perf_counter() - t0) * 1e3)
    V = what["vjp all"]()
    its = sol["iterations"][sol["exit"] == 0]
    print("B = %d members at (n, K, ml, p) = (%d, %s, %d, %d): %d optimal after %.1f iterations on average (%d - %d), %d differentiated"
          % (B, n, K, ml, p, len(its), its.mean(), its.min(), its.max(), int((V["exit"] == 0).sum())))
    out = {"B": B, "n": n, "K": K, "ml": ml, "p": p, "reps": a.reps, "iterations_mean": float(its.mean())}
    for k, t in times.items():
        med = statistics.median(t)
        print("%-12s %10.3f ms (%.3f - %.3f)   %8.3f us per member" % (k, med, min(t), max(t), 1e3 * med / B))
        out[k.replace(" ", "_") + "_ms"] = [med, min(t), max(t)]
    for k in ("dev vjp", "dev vjp all", "dev jvp"):
        ratio = statistics.median(times["dev solve"]) / statistics.median(times[k])
        print("dev solve / %-12s %6.2f   (the solve has %.1f iterations)" % (k, ratio, its.mean()))
        out["solve_over_" + k.replace(" ", "_")] = ratio
    print(json.dumps(out))


if __name__ == "__main__":
    main()
