"""Generates G19 (cone programs with 'q' / 's' blocks) and G20 (misc.kkt_chol) from the REFERENCE itself, staged by
make_goldens.stage() (build container only; the fixtures travel).  Every solve is the pure reference: dense G, kktsolver='chol'
(misc.kkt_chol, the same reduced system kvxopt_amd.cone factors), tagged "via": "reference".

    python tests/golden/make_goldens_cones.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens  # noqa: E402

sys.path.insert(0, make_goldens.ROOT)
from kvxopt_amd import workloads  # noqa: E402


def _interior(dims, rng):
    parts = [rng.uniform(0.5, 1.5, dims["l"])]
    for k in dims["q"]:
        u = rng.standard_normal(k - 1)
        parts.append(np.concatenate([[np.linalg.norm(u) + 0.5 + rng.random()], u]))
    for m in dims["s"]:
        B = rng.standard_normal((m, m))
        parts.append((B @ B.T + m * np.eye(m)).reshape(-1, order="F"))
    return np.concatenate(parts)


def _doc_conelp(lower_only):
    G = np.array([[16., 7., 24., -8., 8., -1., 0., -1., 0., 0., 7., -5., 1., -5., 1., -7., 1., -7., -4.],
                  [-14., 2., 7., -13., -18., 3., 0., 0., -1., 0., 3., 13., -6., 13., 12., -10., -6., -10., -28.],
                  [5., 0., -15., 12., -6., 17., 0., 0., 0., -1., 9., 6., -6., 6., -7., -7., -6., -7., -11.]]).T
    h = np.array([-3., 5., 12., -2., -14., -13., 10., 0., 0., 0., 68., -30., -19., -30., 99., 23., -19., 23., 10.])
    if lower_only:                                     # coneprog.rst:357-367: only the lower triangles are read
        G[[13, 16, 17], :] = 0.0
        h[[13, 16, 17]] = 0.0
    return dict(c=np.array([-6., -4., -5.]), G=G, h=h, dims={"l": 2, "q": [4, 4], "s": [3]})


def _doc_socp():
    G1 = np.array([[12., 13., 12.], [6., -3., -12.], [-5., -5., 6.]]).T
    G2 = np.array([[3., 3., -1., 1.], [-6., -6., -9., 19.], [10., -2., -2., -3.]]).T
    return dict(c=np.array([-2., 1., 5.]), G=np.vstack([G1, G2]), h=np.array([-12., -3., -2., 27., 0., 3., -42.]),
                dims={"l": 0, "q": [3, 4], "s": []})


def _doc_sdp(lower_only):
    if lower_only:
        G1 = np.array([[-7., -11., 0., 3.], [7., -18., 0., 8.], [-2., -8., 0., 1.]]).T
        G2 = np.array([[-21., -11., 0., 0., 10., 8., 0., 0., 5.], [0., 10., 16., 0., -10., -10., 0., 0., 3.],
                       [-5., 2., -17., 0., -6., 8., 0., 0., 6.]]).T
        h = [33., -9., 0., 26., 14., 9., 40., 0., 91., 10., 0., 0., 15.]
    else:
        G1 = np.array([[-7., -11., -11., 3.], [7., -18., -18., 8.], [-2., -8., -8., 1.]]).T
        G2 = np.array([[-21., -11., 0., -11., 10., 8., 0., 8., 5.], [0., 10., 16., 10., -10., -10., 16., -10., 3.],
                       [-5., 2., -17., 2., -6., 8., -17., 8., 6.]]).T
        h = [33., -9., -9., 26., 14., 9., 40., 9., 91., 10., 40., 10., 15.]
    return dict(c=np.array([1., -1., 1.]), G=np.vstack([G1, G2]), h=np.array(h), dims={"l": 0, "q": [], "s": [2, 3]})


def _feasible(dims, n, p, dens, seed):
    """G x0 + s0 = h, A x0 = b, c = -G'z0 - A'y0 with s0, z0 interior: primal and dual strictly feasible."""
    rng = np.random.default_rng(seed)
    N = dims["l"] + sum(dims["q"]) + sum(m * m for m in dims["s"])
    G = rng.standard_normal((N, n)) * (rng.random((N, n)) < dens)
    G[np.arange(min(N, n)), np.arange(min(N, n))] += 1.0
    r = dims["l"] + sum(dims["q"])
    for m in dims["s"]:                                # symmetric coefficient blocks
        B = G[r:r + m * m, :].reshape(m, m, n, order="F")
        G[r:r + m * m, :] = (B + B.transpose(1, 0, 2)).reshape(m * m, n, order="F")
        r += m * m
    A = rng.standard_normal((p, n))
    x0, y0 = rng.standard_normal(n), rng.standard_normal(p)
    s0, z0 = _interior(dims, rng), _interior(dims, rng)
    out = dict(c=-G.T @ z0 - A.T @ y0, G=G, h=G @ x0 + s0, dims=dims)
    if p:
        out.update(A=A, b=A @ x0)
    return out, (x0, y0, s0, z0)


def cases():
    out = {"doc_conelp": _doc_conelp(False), "doc_conelp_lower": _doc_conelp(True), "doc_socp": _doc_socp(),
           "doc_sdp": _doc_sdp(False), "doc_sdp_lower": _doc_sdp(True)}
    c, (N, n, cp, ri, v), h, dims = workloads.socp_sum_of_norms(200, 100, seed=41)
    G = np.zeros((N, n))
    G[ri, np.repeat(np.arange(n), np.diff(cp))] = v
    out["socp_sparse"] = dict(c=c, G=G, h=h, dims=dims)
    c, G, h, dims = workloads.sdp_box(30, [5, 20, 40], density=0.3, seed=42)
    out["sdp_blocks"] = dict(c=c, G=G, h=h, dims=dims)
    out["mixed_eq"], _ = _feasible({"l": 4, "q": [3, 4], "s": [3, 2]}, 8, 2, 0.5, 43)
    # ||(x0, x1)|| <= 1 and x0 >= 2: primal infeasible
    out["socp_pinf"] = dict(c=np.array([1., 1.]), G=np.array([[-1., 0.], [0., 0.], [-1., 0.], [0., -1.]]),
                            h=np.array([-2., 1., 0., 0.]), dims={"l": 1, "q": [3], "s": []})
    # minimize -x0 s.t. |x1| <= x0, x1 <= 1: dual infeasible (unbounded below)
    out["socp_dinf"] = dict(c=np.array([-1., 0.]), G=np.array([[0., 1.], [-1., 0.], [0., -1.]]), h=np.array([1., 0., 0.]),
                            dims={"l": 1, "q": [2], "s": []})
    st, (x0, y0, s0, z0) = _feasible({"l": 3, "q": [4], "s": [3]}, 6, 1, 0.6, 44)
    st.update(primalstart_x=x0, primalstart_s=s0, dualstart_y=y0, dualstart_z=z0)
    out["starts"] = st
    # dualstart without 'y' (p > 0): y starts at 0 (coneprog.py:655-656, 731-733)
    ny = dict(out["mixed_eq"])
    ny["dualstart_z"] = np.concatenate([np.ones(4), [2.0, 0.5, 0.5], [2.0, 0.5, 0.5, 0.5], np.eye(3).reshape(-1), np.eye(2).reshape(-1)])
    out["dualstart_no_y"] = ny
    return out


def g19_cone_programs():
    from kvxopt import matrix, solvers
    npz, meta = {}, {"via": "reference (dense G, kktsolver='chol': misc.kkt_chol)", "cases": {}}
    for name, cs in cases().items():
        kw = {}
        if "A" in cs:
            kw["A"], kw["b"] = matrix(np.asfortranarray(cs["A"])), matrix(cs["b"])
        if "primalstart_x" in cs:
            kw["primalstart"] = {"x": matrix(cs["primalstart_x"]), "s": matrix(cs["primalstart_s"])}
        if "dualstart_z" in cs:
            kw["dualstart"] = {"z": matrix(cs["dualstart_z"])}
            if "dualstart_y" in cs:
                kw["dualstart"]["y"] = matrix(cs["dualstart_y"])
        sol = solvers.conelp(matrix(cs["c"]), matrix(np.asfortranarray(cs["G"])), matrix(cs["h"]), cs["dims"],
                             kktsolver="chol", options={"show_progress": False}, **kw)
        for k in ("c", "G", "h", "A", "b", "primalstart_x", "primalstart_s", "dualstart_y", "dualstart_z"):
            if k in cs:
                npz["%s__%s" % (name, k)] = np.asarray(cs[k], dtype=float)
        for k in ("x", "y", "s", "z"):
            if sol[k] is not None:
                npz["%s__sol_%s" % (name, k)] = np.array(sol[k], dtype=float).reshape(-1)
        meta["cases"][name] = {"dims": cs["dims"], "status": sol["status"], "iterations": sol["iterations"],
                               "primal objective": sol["primal objective"], "dual objective": sol["dual objective"],
                               "gap": sol["gap"]}
        print(name, sol["status"], sol["iterations"])
    np.savez_compressed(os.path.join(HERE, "g19_cone_programs.npz"), **npz)
    json.dump(meta, open(os.path.join(HERE, "g19_cone_programs.json"), "w"), indent=1)


def g20_kkt_chol_cones():
    from kvxopt import matrix, misc
    out = {}
    dims = {"l": 4, "q": [3, 4], "s": [3, 2]}
    N = 4 + 7 + 9 + 4
    n = 10
    for p in (0, 3):
        rng = np.random.default_rng(200 + p)
        G = rng.standard_normal((N, n)) * (rng.random((N, n)) < 0.6)
        A = rng.standard_normal((p, n))
        s, z = _interior(dims, rng), _interior(dims, rng)
        lm = matrix(0.0, (4 + 7 + 5, 1))
        W = misc.compute_scaling(matrix(s), matrix(z), lm, dims)
        f = misc.kkt_chol(matrix(np.asfortranarray(G)), dims, matrix(np.asfortranarray(A)) if p else matrix(0.0, (0, n)))
        solve = f(W)
        bx, by, bz = rng.standard_normal(n), rng.standard_normal(p), rng.standard_normal(N)
        x, y, zz = matrix(bx.copy()), matrix(by.copy()), matrix(bz.copy())
        solve(x, y, zz)
        pre = "p%d_" % p
        # W itself: the 's' part of an NT scaling is defined up to the signs of singular vectors, and W uz depends on that choice
        out.update({pre + "W_d": np.array(W["d"]).reshape(-1), pre + "W_di": np.array(W["di"]).reshape(-1),
                    pre + "W_v": np.concatenate([np.array(v).reshape(-1) for v in W["v"]]), pre + "W_beta": np.array(W["beta"]),
                    pre + "W_r": np.concatenate([np.array(r).reshape(-1, order="F") for r in W["r"]]),
                    pre + "W_rti": np.concatenate([np.array(r).reshape(-1, order="F") for r in W["rti"]])})
        out.update({pre + "G": G, pre + "A": A, pre + "s": s, pre + "z": z, pre + "bx": bx, pre + "by": by, pre + "bz": bz,
                    pre + "ux": np.array(x).reshape(-1), pre + "uy": np.array(y).reshape(-1), pre + "uz": np.array(zz).reshape(-1)})
    out["dims_l"], out["dims_q"], out["dims_s"] = np.array([4]), np.array([3, 4]), np.array([3, 2])
    np.savez_compressed(os.path.join(HERE, "g20_kkt_chol_cones.npz"), **out)


if __name__ == "__main__":
    make_goldens.stage()
    g19_cone_programs()
    g20_kkt_chol_cones()
    print("goldens written to", HERE)
