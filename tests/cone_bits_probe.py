"""Bit-for-bit probe of the general-cone drivers and the host-array cone operations: prints SHA-256 digests of x, y, s, z, the
status and the iteration count of every case of the goldens G19 (cone.conelp) and G21 (cone.coneqp) -- which hold both
infeasibility certificates, both starting points given, a dualstart alone, initvals, use_correction False and refinement 0, 1, 2 --
of G19's 'starts' with either starting point alone and of both doc problems stopped by maxiters = 2, and of every output of each
`misc` operation on the inputs stored in G1, G15 and G16.  Two builds of the package compute the same thing exactly when their
outputs are equal; run it in each and compare."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from kvxopt_amd import cone, misc                       # noqa: E402
from kvxopt_amd.base import matrix                      # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
QUIET = {"show_progress": False}


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes())
    return h.hexdigest()


def sol_digest(sol):
    out = {"status": sol["status"], "iterations": sol["iterations"]}
    for k in ("x", "y", "s", "z"):
        out[k] = None if sol.get(k) is None else sha(sol[k])
    return out


def cases(stem):
    meta = json.load(open(os.path.join(GOLD, stem + ".json")))["cases"]
    Z = np.load(os.path.join(GOLD, stem + ".npz"))
    for name in sorted(meta):
        yield name, {k.split("__", 1)[1]: Z[k] for k in Z.files if k.startswith(name + "__")}, meta[name]


def dense(a):
    return matrix(np.asfortranarray(a))


res = {}
for name, d, meta in cases("g19_cone_programs"):
    kw = {}
    if "A" in d:
        kw["A"], kw["b"] = dense(d["A"]), matrix(d["b"])
    if "primalstart_x" in d:
        kw["primalstart"] = {"x": matrix(d["primalstart_x"]), "s": matrix(d["primalstart_s"])}
    if "dualstart_z" in d:
        kw["dualstart"] = {k: matrix(d["dualstart_" + k]) for k in ("y", "z") if "dualstart_" + k in d}
    res["g19." + name] = sol_digest(cone.conelp(matrix(d["c"]), dense(d["G"]), matrix(d["h"]), meta["dims"], options=QUIET, **kw))
    if name == "starts":                                # either starting point alone: the other half comes from the W = I system
        for half in ("primalstart", "dualstart"):
            one = {k: v for k, v in kw.items() if k in ("A", "b", half)}
            res["g19.starts." + half] = sol_digest(cone.conelp(matrix(d["c"]), dense(d["G"]), matrix(d["h"]), meta["dims"], options=QUIET, **one))
    if name == "doc_conelp":
        res["g19.doc_conelp.maxiters2"] = sol_digest(cone.conelp(matrix(d["c"]), dense(d["G"]), matrix(d["h"]), meta["dims"],
                                                                 options=dict(QUIET, maxiters=2)))
for name, d, meta in cases("g21_coneqp_cones"):
    kw = {}
    if "A" in d:
        kw["A"], kw["b"] = dense(d["A"]), matrix(d["b"])
    if "init_x" in d:
        kw["initvals"] = {k: matrix(d["init_" + k]) for k in ("x", "y", "s", "z")}
    opts = dict(QUIET)
    opts.update(meta["options"])
    res["g21." + name] = sol_digest(cone.coneqp(dense(d["P"]), matrix(d["q"]), dense(d["G"]), matrix(d["h"]), meta["dims"],
                                                options=opts, **kw))
    if name == "doc_coneqp":
        res["g21.doc_coneqp.maxiters2"] = sol_digest(cone.coneqp(dense(d["P"]), matrix(d["q"]), dense(d["G"]), matrix(d["h"]), meta["dims"],
                                                                 options=dict(QUIET, maxiters=2)))


def w_digest(W):
    return sha(*([W[k]._a for k in ("dnl", "dnli", "d", "di") if k in W] + [v._a for v in W["v"]] + [W["beta"]] +
                 [r._a for r in W["r"]] + [r._a for r in W["rti"]]))


def misc_ops(tag, g, key, dims, mnl, diag_key=None, helpers=False):
    """Every operation of misc on the stored inputs; `key(name)` reads the fixture."""
    k = mnl or 0
    nlq = k + dims["l"] + sum(dims["q"])
    N, Nd = nlq + sum(m * m for m in dims["s"]), nlq + sum(dims["s"])
    out = {}
    lm = matrix(0.0, (Nd, 1))
    W = misc.compute_scaling(matrix(key("s").copy()), matrix(key("z").copy()), lm, dims, mnl)
    out["compute_scaling"] = [w_digest(W), sha(lm._a)]
    for tr in "NT":
        for inv in "NI":
            x = matrix(key("X").copy(order="F"))
            misc.scale(x, W, trans=tr, inverse=inv)
            out["scale_" + tr + inv] = sha(x._a)
    x1, y1 = key("x1"), key("y1")
    yd = key(diag_key) if diag_key else y1
    for name, fn in (("scale2_N", lambda a: misc.scale2(lm, a, dims, k)), ("scale2_I", lambda a: misc.scale2(lm, a, dims, k, inverse="I")),
                     ("sprod_D", lambda a: misc.sprod(a, matrix(yd.copy()), dims, k, diag="D")),
                     ("sinv", lambda a: misc.sinv(a, matrix(yd.copy()), dims, k))):
        a = matrix(x1.copy()); fn(a); out[name] = sha(a._a)
    a, b = matrix(x1.copy()), matrix(y1.copy())
    misc.sprod(a, b, dims, k)
    out["sprod"] = sha(a._a, b._a)
    a = matrix(0.0, (Nd, 1)); misc.ssqr(a, matrix(yd[:Nd].copy()), dims, k); out["ssqr"] = sha(a._a)
    out["sdot"] = float(misc.sdot(matrix(x1), matrix(y1), dims, k)).hex()
    out["max_step"] = float(misc.max_step(matrix(x1.copy()), dims, k)).hex()
    xs, sg = matrix(x1.copy()), matrix(0.0, (max(sum(dims["s"]), 1), 1))
    out["max_step_sigma"] = [float(misc.max_step(xs, dims, k, sg)).hex(), sha(xs._a, sg._a)]
    if helpers:
        npk = nlq + sum(m * (m + 1) // 2 for m in dims["s"])
        yp = matrix(0.0, (npk + 3, 1)); misc.pack(matrix(x1), yp, dims, k, 0, 2)
        yu = matrix(7.0, (N + 1, 1)); misc.unpack(yp, yu, dims, k, 2, 1)
        x2 = matrix(np.column_stack([x1, y1]).copy(order="F")); misc.pack2(x2, dims, k)
        out["pack"] = sha(yp._a, yu._a, x2._a)
        if not k:
            a, b, c = matrix(x1.copy()), matrix(x1.copy()), matrix(x1.copy())
            misc.trisc(a, dims); misc.triusc(b, dims); misc.symm(c, dims["s"][-1], N - dims["s"][-1] ** 2)
            out["tri"] = sha(a._a, b._a, c._a)
    lm2, ms, mz = matrix(key("lmbda").copy()), matrix(key("us_s_in").copy()), matrix(key("us_z_in").copy())
    misc.update_scaling(W, lm2, ms, mz)
    out["update_scaling"] = [w_digest(W), sha(lm2._a, ms._a, mz._a)]
    res[tag] = out


g1 = np.load(os.path.join(GOLD, "g1_nt_scaling.npz"))
for ml in (1, 7, 1000):
    def key(name, ml=ml):
        return g1["ml%d_%s" % (ml, {"us_s_in": "us_ds", "us_z_in": "us_dz"}.get(name, name))]
    misc_ops("g1.ml%d" % ml, g1, key, {"l": ml, "q": [], "s": []}, None)
g15, g16 = np.load(os.path.join(GOLD, "g15_q_cone_scaling.npz")), np.load(os.path.join(GOLD, "g16_s_cone_scaling.npz"))
for tag, mnl in (("a", None), ("b", 3)):
    misc_ops("g15." + tag, g15, lambda name, tag=tag: g15[tag + "_" + name], {"l": 4, "q": [5, 1, 9], "s": []}, mnl)
for tag, mnl in (("a", None), ("b", 2)):
    misc_ops("g16." + tag, g16, lambda name, tag=tag: g16[tag + "_" + name], {"l": 3, "q": [4], "s": [3, 1, 6]}, mnl, "yd", helpers=True)
print(json.dumps(res, sort_keys=True))
