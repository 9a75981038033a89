"""Generates G30 (the cases kvxopt_amd.gpbatch is pinned on) from the REFERENCE itself, staged by make_goldens.stage() (build
container only; the fixtures travel).  Every solve is the pure reference: solvers.gp with dense matrices, kktsolver='ldl'
(misc.kkt_ldl, LAPACK only, as G24) and options['refinement'] = 0, which is what gp_batch carries -- solvers.gp defaults to 1 --
tagged "via": "reference".  Data only: inputs, x, y, znl, zl, snl, sl, status, iterations, objectives.

    python tests/golden/make_goldens_gp_batch.py
"""
import contextlib
import io
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens  # noqa: E402
from make_goldens_cvx import STATS, programs  # noqa: E402

sys.path.insert(0, os.path.join(make_goldens.ROOT, "tests"))
import gp_batch_numpy as R  # noqa: E402


def cases():
    P = programs()
    out = {name: {k: v for k, v in P[name].items() if k != "kind"} for name in ("gp_doc", "gp_random", "gp_doc_maxiters")}

    def one(M):
        cs = dict(K=M.K, F=M.F[0], g=M.g[:, 0])
        if M.A is not None:
            cs.update(A=M.A[0], b=M.b[:, 0])
        return cs
    out["gp_objective_only"] = one(R.members(3, [8], 0, 0, 1, 3051))          # ml = 0, mnl = 0: centred rows, the minimum exists
    out["gp_eq_no_linear"] = one(R.members(4, [7, 3, 2], 0, 1, 1, 3052))      # p = 1, ml = 0
    return out


def g30_gp_batch():
    from kvxopt import matrix, solvers
    M = lambda a: matrix(np.asfortranarray(np.asarray(a, dtype=float)))        # noqa: E731
    npz, meta = {}, {"via": "reference (dense matrices, kktsolver='ldl': misc.kkt_ldl, refinement 0)", "cases": {}}
    for name, cs in cases().items():
        kw = {}
        if "G" in cs:
            kw.update(G=M(cs["G"]), h=matrix(np.asarray(cs["h"], dtype=float)))
        if "A" in cs:
            kw.update(A=M(cs["A"]), b=matrix(np.asarray(cs["b"], dtype=float)))
        opts = {"show_progress": True, "refinement": 0}
        opts.update(cs.get("options", {}))
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            sol = solvers.gp([int(k) for k in cs["K"]], M(cs["F"]), matrix(np.asarray(cs["g"], dtype=float)), kktsolver="ldl",
                             options=opts, **kw)
        iters = len(re.findall(r"^\s*\d+: ", buf.getvalue(), flags=re.M)) - 1
        for k in ("F", "g", "G", "h", "A", "b"):
            if k in cs:
                npz["%s__%s" % (name, k)] = np.asarray(cs[k], dtype=float)
        for k in ("x", "y", "znl", "zl", "snl", "sl"):
            npz["%s__sol_%s" % (name, k)] = np.array(sol[k], dtype=float).reshape(-1)
        m = {"K": [int(k) for k in cs["K"]], "options": cs.get("options", {}), "status": sol["status"], "iterations": iters}
        m.update({k: sol[k] for k in STATS})
        meta["cases"][name] = m
        print("G30", name, sol["status"], iters)
    np.savez_compressed(os.path.join(HERE, "g30_gp_batch.npz"), **npz)
    json.dump(meta, open(os.path.join(HERE, "g30_gp_batch.json"), "w"), indent=1)


if __name__ == "__main__":
    make_goldens.stage()
    g30_gp_batch()
    print("goldens written to", HERE)
