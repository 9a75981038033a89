"""One SHA-256 per named batch of the batch solvers and of their derivatives: what a change that must not move a
bit is held to.

    python tools/batch_bytes.py [--only qp,lp,socp,sdp,conelp,coneqp,gp,qpdiff,coneqpdiff]
    KVX_LIB_PATH=/path/to/other/libkvxhip.so python tools/batch_bytes.py

For solvers.qp_batch, lp_batch, socp_batch, sdp_batch, conelp_batch and coneqp_batch it runs every named batch of
tests/{qp,lp,socp,sdp,conelp,coneqp}_batch_numpy.py --
all of SHAPES, every key of BATCHES (qp: INDEPENDENCE and MIXED; coneqp: each with its options), the spoiled "mixed" variants as
tests/test_*_batch_gpu.py spoil them, and the golden cases as those tests batch them (member 0 of a batch of three with shared
matrices and perturbed linear terms; the tiny LPs in batches of their own; coneqp's with the options recorded with the case) --
and prints, for each (solver, batch), the SHA-256 over the bytes of x, y, s, z,
every stat, `iterations`, `exit` and the statuses.  `gp`: every named batch of tests/gp_batch_numpy.py (the edges with their
options, "spread700", "independence", "mixed", "branches", "restore", "restore2"), the vectors being x, y, znl, snl, zl, sl.  `qpdiff`
and `coneqpdiff`: every shape of qp_batch_diff_numpy.SHAPES and every batch of coneqp_batch_diff_numpy.SMALL_BATCHES, solved and
differentiated as tests/test_{qp,coneqp}_batch_diff_gpu.py do it, once with matrices per member and once with member 0's P, G, A
shared by all; the digest covers ux, uy, uz, exit and every `wrt` gradient of the vjp and x, y, z, s, exit of the jvp, for coneqp also
'centrality' and 'centering steps' of both.  The last line is the whole as JSON.  The library is loaded through
kvxopt_amd._lib, so KVX_LIB_PATH selects the build; run two builds in two processes and compare the two last lines.  The digests
belong to one compiler and one device: none is kept in the repository.

The maxiters of a spoiled "mixed" batch is the median of the members' iteration counts, as in the tests; here the counts are
those of the device's own run of the unspoiled batch, which the tests hold equal to the restatement's.  Needs a GPU.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conelp_batch_numpy as CONE  # noqa: E402
import coneqp_batch_diff_numpy as CONEQPDIFF  # noqa: E402
import coneqp_batch_numpy as CONEQP  # noqa: E402
import gp_batch_numpy as GP  # noqa: E402
import lp_batch_numpy as LP  # noqa: E402
import qp_batch_diff_numpy as QPDIFF  # noqa: E402
import qp_batch_numpy as QP  # noqa: E402
import sdp_batch_numpy as SDP  # noqa: E402
import socp_batch_numpy as SOCP  # noqa: E402
from kvxopt_amd import _lib, solvers  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
VECTORS = ("x", "y", "s", "z")
QP_STATS = ("gap", "relative gap", "primal objective", "dual objective", "primal infeasibility", "dual infeasibility",
            "primal slack", "dual slack")
LP_STATS = QP_STATS + ("residual as primal infeasibility certificate", "residual as dual infeasibility certificate")


def digest(sol, stats, vectors=VECTORS):
    h = hashlib.sha256()
    for v in vectors:
        h.update(np.ascontiguousarray(sol[v], dtype=np.float64).tobytes())
    for f in stats:
        h.update(np.ascontiguousarray(sol[f], dtype=np.float64).tobytes())
    for f in ("iterations", "exit"):
        h.update(np.ascontiguousarray(sol[f], dtype=np.int64).tobytes())
    h.update("\n".join(sol["status"]).encode())
    return h.hexdigest()


def perturbed(c):
    """The three linear terms of test_golden_member_of_a_batch."""
    rng = np.random.default_rng(5)
    return np.asfortranarray(np.stack([c, c * (1.0 + 0.01 * rng.standard_normal(c.size)), c * (1.0 + 0.01 * rng.standard_normal(c.size))],
                                      axis=1))


def median_iterations(sol):
    return {"maxiters": int(np.median(sol["iterations"]))}


def qp_batches():
    def call(M, options=None, **replace):
        a = {"P": M.P, "q": M.q, "G": M.G, "h": M.h, "A": M.A, "b": M.b}
        a.update(replace)
        return solvers.qp_batch(a["P"], a["q"], a["G"], a["h"], a["A"], a["b"], options=options)

    for shape in QP.SHAPES:
        yield "shape-%d-%d-%d" % shape, call(QP.batch(shape))
    yield "independence", call(QP.batch(*QP.INDEPENDENCE))
    M = QP.batch(*QP.MIXED)
    plain = call(M)
    yield "mixed", plain
    P, G, q = M.P.copy(), M.G.copy(), M.q.copy()
    ZERO, NAN = 2, 5                                       # test_qp_batch_gpu.py::test_mixed_outcomes_in_one_batch
    P[ZERO, :, 3] = 0.0; P[ZERO, 3, :] = 0.0; G[ZERO, :, 3] = 0.0
    q[1, NAN] = np.nan
    yield "mixed-spoiled", call(M, median_iterations(plain), P=P, G=G, q=q)
    for name, p in (("qp6x5", 0), ("qpeq6x5p4", 4)):
        P, q, G, h, A, b = QP.grid_dense(p)
        yield "golden-" + name, solvers.qp_batch(P, perturbed(q), G, h, A, b)


def cone_batches(R, solve, spoil):
    """The batches of a conelp solver: solve(M, options, **replace) on a batch of R.members, spoil(M) the replaced arrays of "mixed"."""
    for name in R.BATCHES:
        M = R.batch(name)
        sol = solve(M, None)
        yield name, sol
        if name == "mixed":
            yield "mixed-spoiled", solve(M, median_iterations(sol), **spoil(M))


def spoil_lp(M, R=LP):
    c, G, A = M.c.copy(), M.G.copy(), M.A.copy()
    ZERO, NAN = R.MIXED_CHANGED[-2:]
    G[ZERO, :, 3] = 0.0; A[ZERO, :, 3] = 0.0
    c[1, NAN] = np.nan
    return {"c": c, "G": G, "A": A}


def spoil_sdp(M):
    r = spoil_lp(M, SDP)
    h = M.h.copy()
    o = SDP.blocks(M.ml, M.s)[2][1]
    h[o:o + 9, SDP.MIXED_CHANGED[0]] = 1e200 * np.diag([1.0, -1.0, 1.0]).reshape(-1)
    r["h"] = h
    return r


def spoil_conelp(M):
    r = spoil_lp(M, CONE)
    h = M.h.copy()
    o = SDP.blocks(M.Ms, M.s)[0][1]
    h[o:o + 9, CONE.MIXED_CHANGED[0]] = 1e200 * np.diag([1.0, -1.0, 1.0]).reshape(-1)
    r["h"] = h
    return r


def lp_batches():
    def solve(M, options, **replace):
        a = {"c": M.c, "G": M.G, "h": M.h, "A": M.A, "b": M.b}
        a.update(replace)
        return solvers.lp_batch(a["c"], a["G"], a["h"], a["A"], a["b"], options=options)

    yield from cone_batches(LP, solve, spoil_lp)
    for name, p in (("grid6x5", 0), ("eq6x5p4", 4)):
        c, G, h, A, b = LP.grid_dense(p)
        yield "golden-" + name, solvers.lp_batch(perturbed(c), G, h, A, b)
    for name in sorted(LP.TINY):
        c, G, h = LP.TINY[name][:3]
        yield "golden-" + name, solvers.lp_batch(np.array(c), np.array(G), np.array(h))


def dims_batches(R, fn, spoil, gfile, cases):
    def solve(M, options, **replace):
        a = {"c": M.c, "G": M.G, "h": M.h, "A": M.A, "b": M.b}
        a.update(replace)
        return fn(a["c"], a["G"], a["h"], M.dims, a["A"], a["b"], options=options)

    yield from cone_batches(R, solve, spoil)
    meta = json.load(open(os.path.join(GOLDEN, gfile + ".json")))["cases"]
    g = np.load(os.path.join(GOLDEN, gfile + ".npz"))
    for name in cases:
        get = lambda k: g["%s__%s" % (name, k)] if "%s__%s" % (name, k) in g else None         # noqa: E731
        yield "golden-" + name, fn(perturbed(get("c")), get("G"), get("h"), meta[name]["dims"], get("A"), get("b"))


def coneqp_batches():
    def call(M, options, **replace):
        a = {"P": M.P, "q": M.q, "G": M.G, "h": M.h, "A": M.A, "b": M.b}
        a.update(replace)
        return solvers.coneqp_batch(a["P"], a["q"], a["G"], a["h"], M.dims, a["A"], a["b"], options=options)

    for name in CONEQP.BATCHES:
        M, options = CONEQP.batch(name), CONEQP.BATCHES[name][4]
        yield name, call(M, options)
        if name == "mixed":                                # test_coneqp_batch_gpu.py::test_mixed_outcomes_in_one_batch
            h = M.h.copy()
            h[1, CONEQP.MIXED_NAN] = np.nan
            yield "mixed-spoiled", call(M, options, h=h)
    meta = json.load(open(os.path.join(GOLDEN, "g29_coneqp_batch.json")))["cases"]
    g = np.load(os.path.join(GOLDEN, "g29_coneqp_batch.npz"))
    for name in ("doc_coneqp", "doc_coneqp_garbage", "mixed_eq", "mixed_eq_garbage", "p_rank_deficient", "mixed_eq_cut"):
        get = lambda k: g["%s__%s" % (name, k)] if "%s__%s" % (name, k) in g else None         # noqa: E731
        yield "golden-" + name, solvers.coneqp_batch(get("P"), perturbed(get("q")), get("G"), get("h"), meta[name]["dims"], get("A"),
                                                     get("b"), options=meta[name]["options"])


def gp_batches():
    for name in list(GP.EDGES) + ["spread700", "independence", "mixed", "branches", "restore", "restore2"]:
        sol = solvers.gp_batch(*GP.batch_args(GP.named(name)), options=GP.EDGE_OPTIONS.get(name))
        yield name, digest(sol, QP_STATS, ("x", "y", "znl", "snl", "zl", "sl"))


def derivative_digest(V, J, extra=()):
    h = hashlib.sha256()
    for r, vectors in ((V, ("ux", "uy", "uz")), (J, ("x", "y", "z", "s"))):
        for v in vectors:
            h.update(np.ascontiguousarray(r[v], dtype=np.float64).tobytes())
        h.update(np.ascontiguousarray(r["exit"], dtype=np.int64).tobytes())
        for k in extra:
            h.update(np.ascontiguousarray(r[k]).tobytes())
    for name in QPDIFF.NAMES:
        h.update(b"none" if V[name] is None else np.ascontiguousarray(V[name], dtype=np.float64).tobytes())
    return h.hexdigest()


def derivative_batches(batches, solve, vjp, jvp, extra=()):
    """batches: (name, M, gx, d); solve / vjp / jvp(P, G, A) take the three matrices, per member or shared."""
    for name, M, gx, d in batches:
        pert = {"d" + k: v for k, v in d.items()}
        for kind, (P, G, A) in (("members", (M.P, M.G, M.A)), ("shared", (M.P[0], M.G[0], None if M.A is None else M.A[0]))):
            sol = solve(M, P, G, A)
            yield "%s-%s" % (name, kind), derivative_digest(vjp(M, P, G, A, sol, gx), jvp(M, P, G, A, sol, pert), extra)


def qpdiff_batches():
    def batches():
        for shape in QPDIFF.SHAPES:                        # tests/test_qp_batch_diff_gpu.py::case
            seed = QPDIFF.SEEDS[shape]
            M = QP.batch(shape, QP.SHAPE_B, seed)
            gx = np.asfortranarray(np.random.default_rng(seed + 1).standard_normal((M.n, QP.SHAPE_B)))
            yield "shape-%d-%d-%d" % shape, M, gx, QPDIFF.direction(M, seed + 2)

    return derivative_batches(batches(), lambda M, P, G, A: solvers.qp_batch(P, M.q, G, M.h, A, M.b),
                              lambda M, P, G, A, sol, gx: solvers.qp_batch_vjp(P, M.q, G, M.h, A, M.b, sol=sol, gx=gx),
                              lambda M, P, G, A, sol, pert: solvers.qp_batch_jvp(P, M.q, G, M.h, A, M.b, sol=sol, **pert))


def coneqpdiff_batches():
    def batches():
        for name in CONEQPDIFF.SMALL_BATCHES:              # tests/test_coneqp_batch_diff_gpu.py::case
            M = CONEQPDIFF.batch(name)
            yield name, M, CONEQPDIFF.cotangent(M, 5), CONEQPDIFF.direction(M, 6)

    return derivative_batches(batches(),
                              lambda M, P, G, A: solvers.coneqp_batch(P, M.q, G, M.h, M.dims, A, M.b, options=CONEQPDIFF.SOLVE_TOL),
                              lambda M, P, G, A, sol, gx: solvers.coneqp_batch_vjp(P, M.q, G, M.h, M.dims, A, M.b, sol=sol, gx=gx),
                              lambda M, P, G, A, sol, pert: solvers.coneqp_batch_jvp(P, M.q, G, M.h, M.dims, A, M.b, sol=sol, **pert),
                              ("centrality", "centering steps"))


SOLVERS = {
    "qp": (qp_batches, QP_STATS),
    "lp": (lp_batches, LP_STATS),
    "socp": (lambda: dims_batches(SOCP, solvers.socp_batch, lambda M: spoil_lp(M, SOCP), "g26_socp_batch",
                                  ("doc_socp", "mixed_eq", "socp_pinf", "socp_dinf")), LP_STATS),
    "sdp": (lambda: dims_batches(SDP, solvers.sdp_batch, spoil_sdp, "g27_sdp_batch",
                                 ("doc_sdp", "doc_sdp_lower", "mixed_eq", "sdp_pinf", "sdp_dinf")), LP_STATS),
    "conelp": (lambda: dims_batches(CONE, solvers.conelp_batch, spoil_conelp, "g28_conelp_batch",
                                    ("doc_conelp", "doc_conelp_lower", "mixed_eq", "conelp_pinf", "conelp_dinf")), LP_STATS),
    "coneqp": (coneqp_batches, QP_STATS),
    "gp": (gp_batches, None),                              # these three yield digests
    "qpdiff": (qpdiff_batches, None),
    "coneqpdiff": (coneqpdiff_batches, None),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(SOLVERS))
    a = ap.parse_args()
    _lib.require_device()
    print("library: %s" % _lib.LIB_PATH)
    out = {}
    for solver in a.only.split(","):
        batches, stats = SOLVERS[solver]
        out[solver] = {}
        for name, sol in batches():
            out[solver][name] = sol if stats is None else digest(sol, stats)
            print("%-10s %-36s %s" % (solver, name, out[solver][name]), flush=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
