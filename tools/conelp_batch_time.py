"""Time solvers.conelp_batch against the only way to do the same work without it, a loop of this package's one-problem driver
(solvers.conelp, refinement 0), its launch alone, and the cost of its generality: the same kernel on the shapes of
tools/socp_batch_time.py and tools/sdp_batch_time.py beside the launches of socp_batch and sdp_batch.

    python tools/conelp_batch_time.py [--B 4096] [--n 24 --ml 8 --q 4 --nq 4 --m 5 --ns 1 --p 4] [--loop 32] [--reps 5]

B feasible members with matrices of their own, generated from a seed as the tests generate theirs (dense G with symmetric 's'
blocks and 1 added to its diagonal, h = G x0 + s0, b = A x0, c = -G'z0 - A'y0 with s0, z0 interior to the whole cone).  Timed by
the host clock around calls that end in a device synchronise, alternating, after one untimed pass of each:

    batch         solvers.conelp_batch(c, G, h, dims, A, b): the upload of all data, the launch, the download of all results
    launch        kvx_conelp_batch_solve_dev on buffers already on the device: the one launch alone
    one by one    solvers.conelp (refinement 0) on each of the first --loop members
    socp shape    kvx_conelp_batch_solve_dev and kvx_socp_batch_solve_dev on the members of tools/socp_batch_time.py
    sdp shape     kvx_conelp_batch_solve_dev and kvx_sdp_batch_solve_dev on the members of tools/sdp_batch_time.py

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
from kvxopt_amd import _lib, conelpbatch, sdpbatch, socpbatch, solvers  # noqa: E402
from tools import sdp_batch_time, socp_batch_time  # noqa: E402
from tools.socp_batch_time import resident  # noqa: E402


def members(n, ml, q, s, p, B, seed):
    rng = np.random.default_rng(seed)
    Ms = ml + sum(q)
    N = Ms + sum(m * m for m in s)
    G, A, x0 = rng.standard_normal((B, N, n)), rng.standard_normal((B, p, n)), rng.standard_normal((B, n, 1))
    k = np.arange(min(N, n))
    G[:, k, k] += 1.0
    for o, m in sdp_batch_time.blocks(Ms, s):              # symmetric coefficient blocks, from their lower triangles
        X = G[:, o:o + m * m].reshape(B, m, m, n)          # [b, column, row, j]
        iu = np.triu_indices(m, 1)
        X[:, iu[1], iu[0]] = X[:, iu[0], iu[1]]
        G[:, o:o + m * m] = X.reshape(B, m * m, n)

    def interior():
        lq, sb = socp_batch_time.interior(ml, q, B, rng), sdp_batch_time.interior(0, s, B, rng)
        return np.concatenate([lq, sb], axis=1)
    s0, z0, y0 = interior(), interior(), rng.standard_normal((B, p, 1))
    h = (G @ x0 + s0)[:, :, 0]
    c = -(G.transpose(0, 2, 1) @ z0 + A.transpose(0, 2, 1) @ y0)[:, :, 0]
    return np.asfortranarray(c.T), G, np.asfortranarray(h.T), A, np.asfortranarray((A @ x0)[:, :, 0].T)


def dev_launch(entry, prepare, c, G, h, dims, A, b, cone):
    """A function that times one launch of `entry` on resident copies of the members, and its result buffers."""
    opt, sizes, data = prepare(c, G, h, dims, A, b, None)
    B, n, N, p = sizes[0], sizes[1], sizes[-2], sizes[-1]
    keep, out, dargs = resident(data, B, (n, p, N, N, 10, 1, 1))
    arrays = [np.asarray(v, dtype=np.int64) for v in cone]
    head = [B, n, int(dims["l"])]
    for v in arrays:
        head += [len(v), _lib.pi(v) if len(v) else None]
    args = head + [p] + dargs + [opt.maxiters, opt.abstol, opt.reltol, opt.feastol] + [o.ptr for o in out]

    def launch():
        t0 = time.perf_counter()
        _lib.raise_for(getattr(_lib.lib(), entry)(*args), entry)
        return time.perf_counter() - t0
    launch.keep = (keep, arrays)
    return launch, out


def generality(name, theirs, prepare, c, G, h, dims, A, b, reps):
    """The new kernel and the specialised one on the same resident members: medians, spreads, iteration counts."""
    B = c.shape[1]
    cone = [dims["q"]] if name == "socp" else [dims["s"]]
    mine, mout = dev_launch("kvx_conelp_batch_solve_dev", conelpbatch._prepare, c, G, h, dims, A, b, [dims["q"], dims["s"]])
    other, oout = dev_launch(theirs, prepare, c, G, h, dims, A, b, cone)
    mine(); other()
    mi, oi = mout[5].download(np.int64, B), oout[5].download(np.int64, B)
    tm, to = [], []
    for _ in range(reps):
        tm.append(mine() * 1e3)
        to.append(other() * 1e3)
    mm, mo = statistics.median(tm), statistics.median(to)
    print("%s shape: conelp launch %8.2f ms (%.2f - %.2f), %.3f us per member and iteration; %s %8.2f ms (%.2f - %.2f), %.3f us; "
          "ratio %.2f; counts equal: %s" % (name, mm, min(tm), max(tm), 1e3 * mm / mi.sum(), theirs, mo, min(to), max(to),
                                            1e3 * mo / oi.sum(), mm / mo, bool(np.array_equal(mi, oi))))
    return {"conelp_launch_ms": mm, "conelp_launch_ms_min": min(tm), "conelp_launch_ms_max": max(tm),
            "conelp_us_per_member_iteration": 1e3 * mm / float(mi.sum()), "own_launch_ms": mo, "own_launch_ms_min": min(to),
            "own_launch_ms_max": max(to), "own_us_per_member_iteration": 1e3 * mo / float(oi.sum()), "ratio": mm / mo,
            "counts_equal": bool(np.array_equal(mi, oi))}


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
    ap.add_argument("--loop", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=41)
    a = ap.parse_args()
    _lib.require_device()
    B, n, ml, p, q, s = a.B, a.n, a.ml, a.p, [a.q] * a.nq, [a.m] * a.ns
    N = ml + sum(q) + sum(m * m for m in s)
    dims = {"l": ml, "q": q, "s": s}
    c, G, h, A, b = members(n, ml, q, s, p, B, a.seed)
    if not p:
        A = b = None
    quiet = {"show_progress": False, "refinement": 0}

    def batch():
        t0 = time.perf_counter()
        sol = solvers.conelp_batch(c, G, h, dims, A, b)
        return time.perf_counter() - t0, sol

    launch, out = dev_launch("kvx_conelp_batch_solve_dev", conelpbatch._prepare, c, G, h, dims, A, b, [q, s])

    def one_by_one():
        t0 = time.perf_counter()
        sols = [solvers.conelp(c[:, k], G[k], h[:, k], dims, None if A is None else A[k], None if b is None else b[:, k], options=quiet)
                for k in range(a.loop)]
        return time.perf_counter() - t0, sols

    _, sol = batch()                                       # untimed: code objects, the pool's buffers, the symbolic caches
    launch()
    _, sols = one_by_one()
    x_dev = out[0].download(np.float64, n * B).reshape(B, n).T
    same = bool(np.array_equal(x_dev, sol["x"], equal_nan=True))
    diff = max(float(np.linalg.norm(np.asarray(o["x"]).reshape(-1) - sol["x"][:, k]) / max(1.0, np.linalg.norm(o["x"]))) for k, o in enumerate(sols)
               if o["x"] is not None)
    apart = [(k, o["status"], o["iterations"], sol["status"][k], int(sol["iterations"][k])) for k, o in enumerate(sols)
             if o["status"] != sol["status"][k] or o["iterations"] != sol["iterations"][k]]
    agree = not apart
    tb, tl, to = [], [], []
    for _ in range(a.reps):
        tb.append(batch()[0] * 1e3)
        tl.append(launch() * 1e3)
        to.append(one_by_one()[0] * 1e3)
    mb, mlch, mo = (statistics.median(t) for t in (tb, tl, to))
    its = sol["iterations"]
    print("B = %d members at (n, ml, q, s, p) = (%d, %d, [%d] x %d, [%d] x %d, %d), N = %d: %d optimal, iterations %d - %d (mean %.2f)"
          % (B, n, ml, a.q, a.nq, a.m, a.ns, p, N, sol["status"].count("optimal"), its.min(), its.max(), its.mean()))
    print("batch       %10.2f ms (%.2f - %.2f)   %8.2f us per member" % (mb, min(tb), max(tb), 1e3 * mb / B))
    print("launch      %10.2f ms (%.2f - %.2f)   %8.2f us per member, %.3f us per member and iteration"
          % (mlch, min(tl), max(tl), 1e3 * mlch / B, 1e3 * mlch / its.sum()))
    print("one by one  %10.2f ms (%.2f - %.2f) for %d members: %.2f ms per solvers.conelp call" % (mo, min(to), max(to), a.loop, mo / a.loop))
    print("the launch gives the bytes of the batch: %s; solvers.conelp and the batch agree on status and count: %s; max |x - x_conelp| / max(1, |x_conelp|) = %.2e"
          % (same, agree, diff))
    for k, st, it, bst, bit in apart:
        print("member %d: solvers.conelp %s after %d, the batch %s after %d" % (k, st, it, bst, bit))

    # ---- the cost of generality, on the default shapes of the two specialised tools
    sq = [4] * 12
    sc, sG, sh, sA, sb = socp_batch_time.members(32, 16, sq, 8, B, a.seed)
    socp = generality("socp", "kvx_socp_batch_solve_dev", socpbatch._prepare, sc, sG, sh, {"l": 16, "q": sq, "s": []}, sA, sb, a.reps)
    ss = [6] * 2
    dc, dG, dh, dA, db = sdp_batch_time.members(16, 4, ss, 4, B, a.seed)
    sdp = generality("sdp", "kvx_sdp_batch_solve_dev", sdpbatch._prepare, dc, dG, dh, {"l": 4, "q": [], "s": ss}, dA, db, a.reps)

    print(json.dumps({"B": B, "n": n, "ml": ml, "q": q, "s": s, "p": p, "N": N, "reps": a.reps, "optimal": sol["status"].count("optimal"),
                      "iterations_min": int(its.min()), "iterations_max": int(its.max()), "iterations_mean": float(its.mean()),
                      "batch_ms": mb, "batch_ms_min": min(tb), "batch_ms_max": max(tb),
                      "launch_ms": mlch, "launch_ms_min": min(tl), "launch_ms_max": max(tl), "launch_us_per_member": 1e3 * mlch / B,
                      "launch_us_per_member_iteration": 1e3 * mlch / float(its.sum()),
                      "loop_members": a.loop, "one_by_one_ms": mo, "one_by_one_ms_min": min(to), "one_by_one_ms_max": max(to),
                      "conelp_ms_per_call": mo / a.loop, "launch_bytes_equal_batch": same, "status_and_count_agree": agree, "max_rel_diff_x": diff,
                      "socp_shape": socp, "sdp_shape": sdp}))


if __name__ == "__main__":
    main()
