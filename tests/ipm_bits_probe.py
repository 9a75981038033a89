"""Helper of test_kkt_gpu.py::test_fused_iteration_is_bitwise: solves a few problems with the device-resident interior-point
drivers and prints a digest of every returned array (run once with KVX_LP_UNFUSED=1, once without).  Two builds of the package
compute the same thing exactly when their outputs are equal under every switch."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from kvxopt_amd import lp as kvx_lp, workloads          # noqa: E402
from kvxopt_amd.base import spmatrix                    # noqa: E402


def digest(sol):
    out = {"status": sol["status"], "iterations": sol["iterations"]}
    for k in ("x", "s", "z", "y"):
        v = sol.get(k)
        if v is not None:
            out[k] = hashlib.sha256(np.ascontiguousarray(v, dtype=np.float64).tobytes()).hexdigest()
    for k in ("gap", "primal objective", "dual objective", "primal infeasibility", "dual infeasibility"):
        out[k] = None if sol.get(k) is None else float(sol[k]).hex()
    return out


res = {}
for name, (gx, gy) in (("grid30x20", (30, 20)), ("grid61x47", (61, 47))):
    P = workloads.lp_grid(gx, gy)
    G = spmatrix.from_ccs(P["ml"], P["n"], P["Gp"], P["Gi"], P["Gx"])
    res[name] = digest(kvx_lp.conelp(P["c"], G, P["h"]))
# long rows and columns (the 16-lane forms of the fused kernels): random rows with up to 12 entries over a box
rng = np.random.default_rng(11)
n, mr = 60, 240
rows, cols, vals = [], [], []
for i in range(mr):
    js = rng.choice(n, size=int(rng.integers(1, 13)), replace=False)
    rows += [i] * len(js); cols += list(js); vals += list(rng.standard_normal(len(js)))
for j in range(n):                                      # -1 <= x_j <= 1
    rows += [mr + 2 * j, mr + 2 * j + 1]; cols += [j, j]; vals += [1.0, -1.0]
ml = mr + 2 * n
import scipy.sparse as sp                               # noqa: E402
Gs = sp.csc_matrix((vals, (rows, cols)), shape=(ml, n)); Gs.sort_indices()
x0 = rng.uniform(-0.5, 0.5, n)
h = Gs @ x0 + rng.uniform(0.1, 1.0, ml)
h[mr:] = 1.0
G = spmatrix.from_ccs(ml, n, Gs.indptr.astype(np.int64), Gs.indices.astype(np.int64), Gs.data)
res["random_long_rows"] = digest(kvx_lp.conelp(rng.standard_normal(n), G, h))
assert np.diff(Gs.indptr).max() > 8 and np.bincount(Gs.indices).max() > 8

# a QP on the same constraints (coneqp uses KKTChol2Dev.solve / factor with H = P)
P = workloads.lp_grid(25, 18)
n = P["n"]
G = spmatrix.from_ccs(P["ml"], n, P["Gp"], P["Gi"], P["Gx"])
H = spmatrix.from_ccs(n, n, np.arange(n + 1), np.arange(n), np.full(n, 0.5))
res["qp25x18"] = digest(kvx_lp.coneqp(H, P["c"], G, P["h"]))

# the schedules that have no fused form -- equality constraints (general G: KKTGenEqDev; standard form: KKTDiagEqDev) and iterative
# refinement -- under the same switches: the library reads KVX_LP_UNFUSED too
L = workloads.lp_grid_eq(6, 5, 4)
G = spmatrix.from_ccs(L["ml"], L["n"], L["Gp"], L["Gi"], L["Gx"])
A = spmatrix.from_ccs(L["p"], L["n"], L["Ap"], L["Ai"], L["Ax"])
res["eq6x5p4"] = digest(kvx_lp.conelp(L["c"], G, L["h"], A=A, b=L["b"]))
res["eq6x5p4_r1"] = digest(kvx_lp.conelp(L["c"], G, L["h"], A=A, b=L["b"], options={"refinement": 1}))
L = workloads.lp_grid_std(6, 5)
G = spmatrix.from_ccs(L["ml"], L["n"], L["Gp"], L["Gi"], L["Gx"])
A = spmatrix.from_ccs(L["p"], L["n"], L["Ap"], L["Ai"], L["Ax"])
res["std6x5"] = digest(kvx_lp.conelp(L["c"], G, L["h"], A=A, b=L["b"]))
P = workloads.lp_grid(6, 5)
G = spmatrix.from_ccs(P["ml"], P["n"], P["Gp"], P["Gi"], P["Gx"])
for r in (1, 2):
    res["grid6x5_r%d" % r] = digest(kvx_lp.conelp(P["c"], G, P["h"], options={"refinement": r}))

# lp.coneqp on the 6x5 grid past its default path: equality constraints (KKTGenEqDev with H = P), iterative refinement, initvals
# (x, s, z and x, s only), no Mehrotra correction, and a caller's kktsolver (a dense host solve of the whole KKT matrix)
Q = workloads.qp_grid(6, 5)
L = workloads.lp_grid_eq(6, 5, 4)
n, ml = Q["n"], Q["ml"]
G = spmatrix.from_ccs(ml, n, Q["Gp"], Q["Gi"], Q["Gx"])
H = spmatrix.from_ccs(n, n, Q["Pp"], Q["Pi"], Q["Px"])
A = spmatrix.from_ccs(L["p"], n, L["Ap"], L["Ai"], L["Ax"])
K0 = np.zeros((n + ml, n + ml))
K0[Q["Pi"], np.repeat(np.arange(n), np.diff(Q["Pp"]))] = Q["Px"]
K0[n + Q["Gi"], np.repeat(np.arange(n), np.diff(Q["Gp"]))] = Q["Gx"]
K0 = K0 + np.tril(K0, -1).T


def dense_kkt(W):
    d = W["d"]._a.ravel()
    Ki = np.linalg.inv(K0 - np.diag(np.concatenate([np.zeros(n), d * d])))

    def f(x, y, z):
        u = Ki @ np.concatenate([x._a.ravel(), z._a.ravel()])
        x._a[:] = u[:n].reshape(x._a.shape)
        z._a[:] = (d * u[n:]).reshape(z._a.shape)
    return f


res["qpeq6x5p4"] = digest(kvx_lp.coneqp(H, Q["q"], G, Q["h"], A=A, b=L["b"]))
res["qpeq6x5p4_r1"] = digest(kvx_lp.coneqp(H, Q["q"], G, Q["h"], {"refinement": 1}, A=A, b=L["b"]))
res["qp6x5_r1"] = digest(kvx_lp.coneqp(H, Q["q"], G, Q["h"], {"refinement": 1}))
res["qp6x5_init_xsz"] = digest(kvx_lp.coneqp(H, Q["q"], G, Q["h"], initvals={"x": Q["x0"], "s": Q["s0"], "z": Q["z0"]}))
res["qp6x5_init_xs"] = digest(kvx_lp.coneqp(H, Q["q"], G, Q["h"], initvals={"x": Q["x0"], "s": Q["s0"]}))
res["qp6x5_nocorr"] = digest(kvx_lp.coneqp(H, Q["q"], G, Q["h"], {"use_correction": False}))
res["qp6x5_user_kkt"] = digest(kvx_lp.coneqp(H, Q["q"], G, Q["h"], kktsolver=dense_kkt))
print(json.dumps(res))
