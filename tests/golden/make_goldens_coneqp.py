"""Generates G21 (cone QPs with 'q' / 's' blocks) and G22 (misc.kkt_chol with H) from the REFERENCE itself, staged by
make_goldens.stage() (build container only; the fixtures travel).  Every solve is the pure reference: dense G and P,
kktsolver='chol' (misc.kkt_chol with H = P, the same reduced system kvxopt_amd.cone factors), tagged "via": "reference".

    python tests/golden/make_goldens_coneqp.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens  # noqa: E402
from make_goldens_cones import _feasible, _interior  # noqa: E402

sys.path.insert(0, make_goldens.ROOT)
from kvxopt_amd import workloads  # noqa: E402


def _dense_sym(n, lower):
    """Full symmetric n x n array of a lower CCS (colptr, rowind, values)."""
    cp, ri, vx = lower
    M = np.zeros((n, n))
    M[ri, np.repeat(np.arange(n), np.diff(cp))] = vx
    return M + np.tril(M, -1).T


def _dense_ccs(N, n, cp, ri, v):
    G = np.zeros((N, n))
    G[ri, np.repeat(np.arange(n), np.diff(cp))] = v
    return G


def _doc_coneqp():
    # coneprog.rst:584-599: minimize ||Ax - b||_2^2 s.t. x >= 0, ||x||_2 <= 1 (the factor 2 of the objective dropped, as there)
    A = np.array([[.3, -.4, -.2, -.4, 1.3], [.6, 1.2, -1.7, .3, -.3], [-.3, .0, .6, -1.2, -2.0]]).T
    b = np.array([1.5, .0, -1.2, -.7, .0])
    n = 3
    G = np.vstack([-np.eye(n), np.zeros((1, n)), np.eye(n)])
    h = np.array(n * [0.0] + [1.0] + n * [0.0])
    return dict(P=A.T @ A, q=-A.T @ b, G=G, h=h, dims={"l": n, "q": [n + 1], "s": []})


def cases():
    out = {"doc_coneqp": _doc_coneqp()}
    # 2: sparse SOCP with a path-graph Laplacian (its pattern is not inside the cliques of G)
    Pl, q, (N, n, cp, ri, v), h, dims = workloads.socp_qp_sum_of_norms(200, 100, seed=51)
    out["socp_qp_sparse"] = dict(P=_dense_sym(n, Pl), q=q, G=_dense_ccs(N, n, cp, ri, v), h=h, dims=dims)
    # 3: 's' blocks of orders 5 and 20, P = diagonal plus a rank-two term
    c, G, h, dims = workloads.sdp_box(30, [5, 20], density=0.3, seed=52)
    rng = np.random.default_rng(53)
    U = rng.standard_normal((30, 2))
    out["sdp_qp"] = dict(P=np.diag(rng.uniform(0.5, 1.5, 30)) + U @ U.T, q=c, G=G, h=h, dims=dims)
    # 4: l + q + s with three equality rows
    st, (x0, y0, s0, z0) = _feasible({"l": 4, "q": [3, 4], "s": [3, 2]}, 8, 3, 0.5, 54)
    rng = np.random.default_rng(55)
    B = rng.standard_normal((8, 8)) * (rng.random((8, 8)) < 0.4)
    mixed = dict(P=B @ B.T + 0.1 * np.eye(8), q=st["c"], G=st["G"], h=st["h"], dims=st["dims"], A=st["A"], b=st["b"])
    out["mixed_eq"] = mixed
    # 5: P with an empty pattern (a cone LP solved by coneqp)
    c, (N, n, cp, ri, v), h, dims = workloads.socp_sum_of_norms(20, 10, seed=56)
    out["p_zero"] = dict(P=np.zeros((n, n)), q=c, G=_dense_ccs(N, n, cp, ri, v), h=h, dims=dims)
    # 6: rank-deficient PSD P (rank 2 of 10); the box rows of G give Rank([P; G]) = n
    c, G, h, dims = workloads.sdp_box(10, [4], density=0.4, seed=57)
    U = np.random.default_rng(58).standard_normal((10, 2))
    out["p_singular"] = dict(P=U @ U.T, q=c, G=G, h=h, dims=dims)
    # 6b: Rank(G) = 4 < n = 6 (G does not touch x4, x5: a box and a norm ball on x0..x3); only P makes S definite
    rng = np.random.default_rng(63)
    G4 = np.vstack([np.eye(4), -np.eye(4), np.zeros((1, 4)), -rng.standard_normal((3, 4))])
    B = rng.standard_normal((6, 3))
    B[:4, 2] = 0.0
    Pr = B @ B.T                                        # rank 3; its null space meets that of G in 0 only
    Gr = np.hstack([G4, np.zeros((12, 2))])
    assert np.linalg.matrix_rank(Gr) == 4 and np.linalg.matrix_rank(Pr) == 3 and np.linalg.matrix_rank(np.vstack([Pr, Gr])) == 6
    out["g_rank_deficient"] = dict(P=Pr, q=rng.standard_normal(6), G=Gr, h=np.concatenate([np.ones(8), [2.0, 0.0, 0.0, 0.0]]),
                                   dims={"l": 8, "q": [4], "s": []})
    # 7: P couples variables that no row, cone or block of G couples: the path plus far off-diagonal entries
    Pl, q, (N, n, cp, ri, v), h, dims = workloads.socp_qp_sum_of_norms(40, 20, seed=59)
    P = _dense_sym(n, Pl)
    far = np.arange(0, 20)
    P[far + 30, far] = P[far, far + 30] = -0.05
    P[np.arange(n), np.arange(n)] += 0.1
    out["p_widens_pattern"] = dict(P=P, q=q, G=_dense_ccs(N, n, cp, ri, v), h=h, dims=dims)
    # 8: case 2 with arbitrary numbers above the diagonal of P (only the lower triangle is read)
    g = dict(out["socp_qp_sparse"])
    Pg = np.tril(g["P"])
    iu = np.triu_indices(Pg.shape[0], 1)
    Pg[iu] = np.random.default_rng(60).standard_normal(iu[0].size) * (np.random.default_rng(61).random(iu[0].size) < 0.05)
    g["P"] = Pg
    out["p_upper_garbage"] = g
    # 9: a start for x, s, z and y
    iv = dict(mixed)
    rng = np.random.default_rng(62)
    iv.update(init_x=x0 + 0.1 * rng.standard_normal(8), init_y=y0, init_s=_interior(st["dims"], rng), init_z=_interior(st["dims"], rng))
    out["initvals"] = iv
    # 10, 11: options
    out["no_correction"] = dict(mixed, options={"use_correction": False})
    out["refine0"] = dict(mixed, options={"refinement": 0})
    out["refine2"] = dict(mixed, options={"refinement": 2})
    return out


def g21_coneqp_cones():
    from kvxopt import matrix, solvers
    npz, meta = {}, {"via": "reference (dense P and G, kktsolver='chol': misc.kkt_chol with H = P)", "cases": {}}
    sols = {}
    for name, cs in cases().items():
        kw = {}
        if "A" in cs:
            kw["A"], kw["b"] = matrix(np.asfortranarray(cs["A"])), matrix(cs["b"])
        if "init_x" in cs:
            kw["initvals"] = {k: matrix(cs["init_" + k]) for k in ("x", "y", "s", "z")}
        opts = {"show_progress": False}
        opts.update(cs.get("options", {}))
        sol = solvers.coneqp(matrix(np.asfortranarray(cs["P"])), matrix(cs["q"]), matrix(np.asfortranarray(cs["G"])), matrix(cs["h"]),
                             cs["dims"], kktsolver="chol", options=opts, **kw)
        sols[name] = sol
        for k in ("P", "q", "G", "h", "A", "b", "init_x", "init_y", "init_s", "init_z"):
            if k in cs:
                npz["%s__%s" % (name, k)] = np.asarray(cs[k], dtype=float)
        for k in ("x", "y", "s", "z"):
            npz["%s__sol_%s" % (name, k)] = np.array(sol[k], dtype=float).reshape(-1)
        meta["cases"][name] = {"dims": cs["dims"], "options": cs.get("options", {}), "status": sol["status"],
                               "iterations": sol["iterations"], "primal objective": sol["primal objective"],
                               "dual objective": sol["dual objective"], "gap": sol["gap"]}
        print(name, sol["status"], sol["iterations"])
    # what lies above the diagonal of P is never read: the results of case 8 are those of case 2, to the bit
    for k in ("x", "y", "s", "z"):
        assert np.array_equal(np.array(sols["p_upper_garbage"][k]), np.array(sols["socp_qp_sparse"][k])), k
    np.savez_compressed(os.path.join(HERE, "g21_coneqp_cones.npz"), **npz)
    json.dump(meta, open(os.path.join(HERE, "g21_coneqp_cones.json"), "w"), indent=1)


def g22_kkt_chol_h():
    from kvxopt import matrix, misc
    out = {}
    dims = {"l": 4, "q": [3, 4], "s": [3, 2]}
    N = 4 + 7 + 9 + 4
    n = 10
    for p in (0, 3):
        rng = np.random.default_rng(300 + p)
        G = rng.standard_normal((N, n)) * (rng.random((N, n)) < 0.6)
        A = rng.standard_normal((p, n))
        B = rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.3)
        H = B @ B.T + np.diag(rng.uniform(0.0, 1.0, n))
        s, z = _interior(dims, rng), _interior(dims, rng)
        lm = matrix(0.0, (4 + 7 + 5, 1))
        W = misc.compute_scaling(matrix(s), matrix(z), lm, dims)
        f = misc.kkt_chol(matrix(np.asfortranarray(G)), dims, matrix(np.asfortranarray(A)) if p else matrix(0.0, (0, n)))
        solve = f(W, matrix(np.asfortranarray(H)))
        bx, by, bz = rng.standard_normal(n), rng.standard_normal(p), rng.standard_normal(N)
        x, y, zz = matrix(bx.copy()), matrix(by.copy()), matrix(bz.copy())
        solve(x, y, zz)
        pre = "p%d_" % p
        out.update({pre + "W_d": np.array(W["d"]).reshape(-1), pre + "W_di": np.array(W["di"]).reshape(-1),
                    pre + "W_v": np.concatenate([np.array(v).reshape(-1) for v in W["v"]]), pre + "W_beta": np.array(W["beta"]),
                    pre + "W_r": np.concatenate([np.array(r).reshape(-1, order="F") for r in W["r"]]),
                    pre + "W_rti": np.concatenate([np.array(r).reshape(-1, order="F") for r in W["rti"]])})
        out.update({pre + "G": G, pre + "A": A, pre + "H": H, pre + "bx": bx, pre + "by": by, pre + "bz": bz,
                    pre + "ux": np.array(x).reshape(-1), pre + "uy": np.array(y).reshape(-1), pre + "uz": np.array(zz).reshape(-1)})
    out["dims_l"], out["dims_q"], out["dims_s"] = np.array([4]), np.array([3, 4]), np.array([3, 2])
    np.savez_compressed(os.path.join(HERE, "g22_kkt_chol_h.npz"), **out)


if __name__ == "__main__":
    make_goldens.stage()
    g21_coneqp_cones()
    g22_kkt_chol_h()
    print("goldens written to", HERE)
