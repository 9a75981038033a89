"""Generates G29 (the cases kvxopt_amd.coneqpbatch is pinned on) from the REFERENCE itself, staged by make_goldens.stage() (build
container only; the fixtures travel).  Every solve is the pure reference: solvers.coneqp with dense P and G, kktsolver='chol'
(misc.kkt_chol with H = P) and options['refinement'] = 0, which is what coneqp_batch carries -- solvers.coneqp defaults to 1 with
'q' or 's' rows -- tagged "via": "reference".  Data only: inputs, x, y, s, z, status, iterations, objectives.

    python tests/golden/make_goldens_coneqp_batch.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens  # noqa: E402
from make_goldens_conelp_batch import garbage_upper  # noqa: E402
from make_goldens_cones import _feasible  # noqa: E402
from make_goldens_coneqp import _doc_coneqp  # noqa: E402

sys.path.insert(0, make_goldens.ROOT)
from kvxopt_amd import workloads  # noqa: E402


def garbage(cs, seed):
    """Arbitrary numbers above the diagonal of P and in the strict upper triangles of the 's' blocks of G and h: nothing may read them."""
    out = garbage_upper(cs)
    P = np.tril(cs["P"])
    iu = np.triu_indices(P.shape[0], 1)
    P[iu] = 1e3 * np.random.default_rng(seed).standard_normal(iu[0].size)
    return dict(out, P=P)


def cases():
    out = {"doc_coneqp": _doc_coneqp()}
    out["doc_coneqp_garbage"] = garbage(out["doc_coneqp"], 71)
    # 2: l + q + s with two equality rows
    st, _ = _feasible({"l": 4, "q": [3, 4], "s": [3, 2]}, 8, 2, 0.5, 72)
    rng = np.random.default_rng(73)
    B = rng.standard_normal((8, 8)) * (rng.random((8, 8)) < 0.4)
    out["mixed_eq"] = dict(P=B @ B.T + 0.1 * np.eye(8), q=st["c"], G=st["G"], h=st["h"], dims=st["dims"], A=st["A"], b=st["b"])
    out["mixed_eq_garbage"] = garbage(out["mixed_eq"], 74)
    # 3: P of rank 2 < n = 10; the box rows of G give Rank([P; G]) = n
    c, G, h, dims = workloads.sdp_box(10, [4], density=0.4, seed=75)
    U = np.random.default_rng(76).standard_normal((10, 2))
    assert np.linalg.matrix_rank(U @ U.T) == 2 and np.linalg.matrix_rank(G) == 10
    out["p_rank_deficient"] = dict(P=U @ U.T, q=c, G=G, h=h, dims=dims)
    # 4: case 2 cut at maxiters = 3
    out["mixed_eq_cut"] = dict(out["mixed_eq"], options={"maxiters": 3})
    return out


def g29_coneqp_batch():
    from kvxopt import matrix, solvers
    npz, meta = {}, {"via": "reference (dense P and G, kktsolver='chol': misc.kkt_chol with H = P, refinement 0)", "cases": {}}
    sols = {}
    for name, cs in cases().items():
        kw = {}
        if "A" in cs:
            kw["A"], kw["b"] = matrix(np.asfortranarray(cs["A"])), matrix(cs["b"])
        opts = {"show_progress": False, "refinement": 0}
        opts.update(cs.get("options", {}))
        sol = solvers.coneqp(matrix(np.asfortranarray(cs["P"])), matrix(cs["q"]), matrix(np.asfortranarray(cs["G"])), matrix(cs["h"]),
                             cs["dims"], kktsolver="chol", options=opts, **kw)
        sols[name] = sol
        for k in ("P", "q", "G", "h", "A", "b"):
            if k in cs:
                npz["%s__%s" % (name, k)] = np.asarray(cs[k], dtype=float)
        for k in ("x", "y", "s", "z"):
            npz["%s__sol_%s" % (name, k)] = np.array(sol[k], dtype=float).reshape(-1)
        meta["cases"][name] = {"dims": cs["dims"], "options": cs.get("options", {}), "status": sol["status"],
                               "iterations": sol["iterations"], "primal objective": sol["primal objective"],
                               "dual objective": sol["dual objective"], "gap": sol["gap"]}
        print(name, sol["status"], sol["iterations"])
    # what lies above the diagonals is never read: the results of the garbage cases are those of the clean ones, to the bit
    for name in ("doc_coneqp", "mixed_eq"):
        for k in ("x", "y", "s", "z"):
            assert np.array_equal(np.array(sols[name + "_garbage"][k]), np.array(sols[name][k])), (name, k)
    np.savez_compressed(os.path.join(HERE, "g29_coneqp_batch.npz"), **npz)
    json.dump(meta, open(os.path.join(HERE, "g29_coneqp_batch.json"), "w"), indent=1)


if __name__ == "__main__":
    make_goldens.stage()
    g29_coneqp_batch()
    print("goldens written to", HERE)
