"""Generates G26 (the cases kvxopt_amd.socpbatch is pinned on) from the REFERENCE itself, staged by make_goldens.stage() (build
container only; the fixtures travel).  Every solve is the pure reference: solvers.conelp with dense G, kktsolver='chol'
(misc.kkt_chol) and options['refinement'] = 0, which is what socp_batch carries -- solvers.socp defaults to 1 -- tagged
"via": "reference".  Data only: inputs, x, y, s, z, status, iterations, objectives.

    python tests/golden/make_goldens_socp_batch.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens  # noqa: E402
from make_goldens_cones import _doc_socp, _feasible  # noqa: E402


def cases():
    out = {"doc_socp": _doc_socp()}
    out["mixed_eq"], _ = _feasible({"l": 3, "q": [4, 1, 5], "s": []}, 6, 2, 0.7, 261)
    # ||(x0, x1)|| <= 1 and x0 >= 2: primal infeasible
    out["socp_pinf"] = dict(c=np.array([1., 1.]), G=np.array([[-1., 0.], [0., 0.], [-1., 0.], [0., -1.]]),
                            h=np.array([-2., 1., 0., 0.]), dims={"l": 1, "q": [3], "s": []})
    # minimize -x0 s.t. |x1| <= x0, x1 <= 1: dual infeasible (unbounded below)
    out["socp_dinf"] = dict(c=np.array([-1., 0.]), G=np.array([[0., 1.], [-1., 0.], [0., -1.]]), h=np.array([1., 0., 0.]),
                            dims={"l": 1, "q": [2], "s": []})
    return out


def g26_socp_batch():
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
    # G19 holds doc_socp at the reference's default refinement 1
    g19 = json.load(open(os.path.join(HERE, "g19_cone_programs.json")))["cases"]["doc_socp"]["iterations"]
    meta["doc_socp iterations at refinement 1 (G19)"] = g19
    np.savez_compressed(os.path.join(HERE, "g26_socp_batch.npz"), **npz)
    json.dump(meta, open(os.path.join(HERE, "g26_socp_batch.json"), "w"), indent=1)


if __name__ == "__main__":
    make_goldens.stage()
    g26_socp_batch()
    print("goldens written to", HERE)
