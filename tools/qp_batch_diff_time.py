"""Time solvers.qp_batch_vjp / qp_batch_jvp against the solve they differentiate and against the only way to a derivative
without them, central differences through solvers.qp_batch.

    python tools/qp_batch_diff_time.py [--B 4096] [--n 32 --ml 64 --p 8] [--reps 5]

B members with matrices of their own, generated as tools/qp_batch_time.py generates them.  Timed by the host clock around calls
that end in a device synchronise, alternating, after one untimed pass of each:

    vjp all       solvers.qp_batch_vjp with all six gradients: upload, launch, download of B matrices per gradient
    vjp q h b     solvers.qp_batch_vjp(wrt=("q", "h", "b")): no matrix gradient is formed
    jvp           solvers.qp_batch_jvp with perturbations of all six data
    dev vjp all   kvx_qp_batch_vjp_dev on resident buffers, per-member matrix gradients: the launch alone
    dev vjp       kvx_qp_batch_vjp_dev without matrix gradients
    dev vjp sum   kvx_qp_batch_vjp_dev with one G for all members and its summed gradient: the second launch, k_batch_outer_sum,
                  is the difference to `dev vjp`
    dev jvp       kvx_qp_batch_jvp_dev
    forward       solvers.qp_batch, for scale
    differences   the 1 + 2 solvers.qp_batch calls of one central difference along one direction

Printed: the median and the spread (min - max) of each in ms; the last line is the result as JSON.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvxopt_amd import _lib, qpbatch, solvers  # noqa: E402
from qp_batch_time import members  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--ml", type=int, default=64)
    ap.add_argument("--p", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=41)
    a = ap.parse_args()
    _lib.require_device()
    B, n, ml, p = a.B, a.n, a.ml, a.p
    P, q, G, h, A, b = members(n, ml, p, B, a.seed)
    if not p:
        A = b = None
    rng = np.random.default_rng(a.seed + 1)
    gx = np.asfortranarray(rng.standard_normal((n, B)))
    dP = rng.standard_normal((B, n, n))
    d = {"dP": 0.5 * (dP + dP.transpose(0, 2, 1)), "dq": np.asfortranarray(rng.standard_normal((n, B))),
         "dG": rng.standard_normal((B, ml, n)), "dh": np.asfortranarray(rng.standard_normal((ml, B))),
         "dA": rng.standard_normal((B, p, n)) if p else None, "db": np.asfortranarray(rng.standard_normal((p, B))) if p else None}
    eps = 1e-5
    sol = solvers.qp_batch(P, q, G, h, A, b)

    # the launches alone: everything uploaded once, as the C entries take it
    _, _, data = qpbatch._prepare(P, q, G, h, A, b, None)
    up = lambda v: None if v is None else _lib.DeviceBuffer.from_array(v)                                       # noqa: E731
    cols = lambda v: np.ascontiguousarray(v.T).reshape(-1)                                                      # noqa: E731
    cm = lambda v: None if v is None else np.ascontiguousarray(v.transpose(0, 2, 1)).reshape(-1)                # noqa: E731
    (Pd, sP), _, (Gd, sG), _, (Ad, sA), _ = [(up(v), s) for v, s in data]
    x, y, s, z = (up(cols(sol[k])) for k in ("x", "y", "s", "z"))
    code, gxd = up(sol["exit"].astype(np.int64)), up(cols(gx))
    new = lambda count: _lib.DeviceBuffer(8 * max(count, 1))                                                    # noqa: E731
    ux, uy, uz, us, gP, gG, gA, gexit = new(n * B), new(p * B), new(ml * B), new(ml * B), new(B * n * n), new(B * ml * n), new(B * p * n), new(B)
    pert = [(up(cm(d["dP"])), n * n), (up(cols(d["dq"])), n), (up(cm(d["dG"])), ml * n), (up(cols(d["dh"])), ml),
            (up(cm(d["dA"])), p * n), (up(None if d["db"] is None else cols(d["db"])), p)]
    ptr = lambda buf: None if buf is None else buf.ptr                                                          # noqa: E731

    def head(sG_):
        return [B, n, ml, p, Pd.ptr, sP, Gd.ptr, sG_, ptr(Ad), sA, x.ptr, ptr(y) if p else None, s.ptr, z.ptr, code.ptr, 1]

    L = _lib.lib()

    def dev_vjp(sG_, mats):
        args = head(sG_) + [gxd.ptr, ux.ptr, uy.ptr if p else None, uz.ptr] + mats + [gexit.ptr]
        _lib.raise_for(L.kvx_qp_batch_vjp_dev(*args), "kvx_qp_batch_vjp_dev")

    def dev_jvp():
        args = head(sG)
        for buf, stride in pert:
            args += [ptr(buf), stride]
        _lib.raise_for(L.kvx_qp_batch_jvp_dev(*args, ux.ptr, uy.ptr if p else None, uz.ptr, us.ptr, gexit.ptr), "kvx_qp_batch_jvp_dev")

    moved = lambda t: [v if dv is None else v + t * dv for v, dv in zip((P, q, G, h, A, b), (d["dP"], d["dq"], d["dG"], d["dh"], d["dA"], d["db"]))]   # noqa: E731
    what = {
        "vjp all": lambda: solvers.qp_batch_vjp(P, q, G, h, A, b, sol=sol, gx=gx),
        "vjp q h b": lambda: solvers.qp_batch_vjp(P, q, G, h, A, b, sol=sol, gx=gx, wrt=("q", "h", "b")),
        "jvp": lambda: solvers.qp_batch_jvp(P, q, G, h, A, b, sol=sol, **d),
        "dev vjp all": lambda: dev_vjp(sG, [gP.ptr, gG.ptr, gA.ptr if p else None]),
        "dev vjp": lambda: dev_vjp(sG, [None, None, None]),
        "dev vjp sum": lambda: dev_vjp(0, [None, gG.ptr, None]),
        "dev jvp": dev_jvp,
        "forward": lambda: solvers.qp_batch(P, q, G, h, A, b),
        "differences": lambda: [solvers.qp_batch(P, q, G, h, A, b), solvers.qp_batch(*moved(eps)), solvers.qp_batch(*moved(-eps))],
    }
    times = {k: [] for k in what}
    for rep in range(a.reps + 1):                           # the first pass is not timed: code objects, the pool's buffers
        for k, fn in what.items():
            t0 = time.perf_counter()
            fn()
            if rep:
                times[k].append((time.perf_counter() - t0) * 1e3)
    V = what["vjp all"]()
    print("B = %d members at (n, ml, p) = (%d, %d, %d): %d optimal, %d differentiated" % (B, n, ml, p, int((sol["exit"] == 0).sum()), int((V["exit"] == 0).sum())))
    out = {"B": B, "n": n, "ml": ml, "p": p, "reps": a.reps}
    for k, t in times.items():
        med = statistics.median(t)
        print("%-12s %10.3f ms (%.3f - %.3f)   %8.3f us per member" % (k, med, min(t), max(t), 1e3 * med / B))
        out[k.replace(" ", "_") + "_ms"] = [med, min(t), max(t)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
