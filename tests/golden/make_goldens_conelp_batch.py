"""Generates G28 (the cases kvxopt_amd.conelpbatch is pinned on) from the REFERENCE itself, staged by make_goldens.stage() (build
container only; the fixtures travel).  Every solve is the pure reference: solvers.conelp with dense G, kktsolver='chol'
(misc.kkt_chol) and options['refinement'] = 0, which is what conelp_batch carries -- solvers.conelp defaults to 1 with 'q' or 's'
rows -- tagged "via": "reference".  Data only: inputs, x, y, s, z, status, iterations, objectives.

    python tests/golden/make_goldens_conelp_batch.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens  # noqa: E402
from make_goldens_cones import _doc_conelp, _feasible  # noqa: E402


def garbage_upper(cs):
    """The strict upper triangles of every 's' block of G and h overwritten: nothing may read them (coneprog.rst:357-367)."""
    G, h, o = cs["G"].copy(), cs["h"].copy(), cs["dims"]["l"] + sum(cs["dims"]["q"])
    for m in cs["dims"]["s"]:
        for j in range(m):
            for i in range(j):
                G[o + i + j * m, :] = 1e3 + 7.0 * (i + j * m) - np.arange(G.shape[1])
                h[o + i + j * m] = -1e3 - 3.0 * (i + j * m)
        o += m * m
    return dict(cs, G=G, h=h)


def cases():
    out = {"doc_conelp": _doc_conelp(False), "doc_conelp_lower": garbage_upper(_doc_conelp(True))}
    out["mixed_eq"], _ = _feasible({"l": 4, "q": [3, 4], "s": [3, 2]}, 8, 2, 0.5, 43)
    # x0 >= 2, |(x0, x1)| <= 1 and [[1, x1], [x1, 1]] >= 0: primal infeasible, by the 'l' row and the cone together
    out["conelp_pinf"] = dict(c=np.array([1., 1.]),
                              G=np.array([[-1., 0.], [0., 0.], [-1., 0.], [0., -1.], [0., 0.], [0., -1.], [0., -1.], [0., 0.]]),
                              h=np.array([-2., 1., 0., 0., 1., 0., 0., 1.]), dims={"l": 1, "q": [3], "s": [2]})
    # minimize -x0 s.t. x1 <= 1, |x1| <= x0 and [[x0, x1], [x1, x0]] >= 0: dual infeasible (unbounded below)
    out["conelp_dinf"] = dict(c=np.array([-1., 0.]),
                              G=np.array([[0., 1.], [-1., 0.], [0., -1.], [-1., 0.], [0., -1.], [0., -1.], [-1., 0.]]),
                              h=np.array([1., 0., 0., 0., 0., 0., 0.]), dims={"l": 1, "q": [2], "s": [2]})
    return out


def g28_conelp_batch():
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
    np.savez_compressed(os.path.join(HERE, "g28_conelp_batch.npz"), **npz)
    json.dump(meta, open(os.path.join(HERE, "g28_conelp_batch.json"), "w"), indent=1)


if __name__ == "__main__":
    make_goldens.stage()
    g28_conelp_batch()
    print("goldens written to", HERE)
