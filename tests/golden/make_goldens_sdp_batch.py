"""Generates G27 (the cases kvxopt_amd.sdpbatch is pinned on) from the REFERENCE itself, staged by make_goldens.stage() (build
container only; the fixtures travel).  Every solve is the pure reference: solvers.conelp with dense G, kktsolver='chol'
(misc.kkt_chol) and options['refinement'] = 0, which is what sdp_batch carries -- solvers.sdp defaults to 1 -- tagged
"via": "reference".  Data only: inputs, x, y, s, z, status, iterations, objectives.

    python tests/golden/make_goldens_sdp_batch.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens  # noqa: E402
from make_goldens_cones import _doc_sdp, _feasible  # noqa: E402


def garbage_upper(cs):
    """The strict upper triangles of every 's' block of G and h overwritten: nothing may read them (coneprog.rst:357-367)."""
    G, h, o = cs["G"].copy(), cs["h"].copy(), cs["dims"]["l"]
    for m in cs["dims"]["s"]:
        for j in range(m):
            for i in range(j):
                G[o + i + j * m, :] = 1e3 + 7.0 * (i + j * m) - np.arange(G.shape[1])
                h[o + i + j * m] = -1e3 - 3.0 * (i + j * m)
        o += m * m
    return dict(cs, G=G, h=h)


def cases():
    out = {"doc_sdp": _doc_sdp(False), "doc_sdp_lower": garbage_upper(_doc_sdp(True))}
    out["mixed_eq"], _ = _feasible({"l": 2, "q": [], "s": [1, 3, 4]}, 6, 2, 0.7, 271)
    # X = [[x0, x1], [x1, x2]] with X - I >= 0 and -X >= 0: primal infeasible
    E = np.array([[1., 0., 0.], [0., 1., 0.], [0., 1., 0.], [0., 0., 1.]])
    out["sdp_pinf"] = dict(c=np.array([1., 0., 1.]), G=np.vstack([-E, E]), h=np.array([-1., 0., 0., -1., 0., 0., 0., 0.]),
                           dims={"l": 0, "q": [], "s": [2, 2]})
    # minimize -x0 s.t. [[x0, x1], [x1, x0]] >= 0, x1 <= 1: dual infeasible (unbounded below)
    out["sdp_dinf"] = dict(c=np.array([-1., 0.]), G=np.array([[0., 1.], [-1., 0.], [0., -1.], [0., -1.], [-1., 0.]]),
                           h=np.array([1., 0., 0., 0., 0.]), dims={"l": 1, "q": [], "s": [2]})
    return out


def g27_sdp_batch():
    from kvxopt import matrix, solvers
    npz, meta = {}, {"via": "reference (dense G, kktsolver='chol': misc.kkt_chol, refinement 0)", "cases": {}}
    for name, cs in cases().items():
        kw = {}
        if "A" in cs:
            kw["A"], kw["b"] = matrix(np.asfortranarray(cs["A"])), matrix(cs["b"])
        sol = solvers.conelp(matrix(cs["c"]), matrix(np.asfortranarray(cs["G"])), matrix(cs["h"]), cs["dims"], kktsolver="chol",
                             options={"show_progress": False, "refinement": 0}, **kw)
        for k in ("c", "G", "h", "A", "b"):
            if k in cs:
                npz["%s__%s" % (name, k)] = np.asarray(cs[k], dtype=float)
        for k in ("x", "y", "s", "z"):
            if sol[k] is not None:
                npz["%s__sol_%s" % (name, k)] = np.array(sol[k], dtype=float).reshape(-1)
        meta["cases"][name] = {"dims": cs["dims"], "status": sol["status"], "iterations": sol["iterations"],
                               "primal objective": sol["primal objective"], "dual objective": sol["dual objective"],
                               "gap": sol["gap"]}
        print(name, sol["status"], sol["iterations"])
    np.savez_compressed(os.path.join(HERE, "g27_sdp_batch.npz"), **npz)
    json.dump(meta, open(os.path.join(HERE, "g27_sdp_batch.json"), "w"), indent=1)


if __name__ == "__main__":
    make_goldens.stage()
    g27_sdp_batch()
    print("goldens written to", HERE)
