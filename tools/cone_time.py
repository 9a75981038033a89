"""Per-iteration time of the general-cone conelp (kvxopt_amd.cone) on the two at-scale workloads of tests/test_cone_gpu.py,
split into S assembly (kvx_cone_assemble_dev), factorisation (S and K), KKT solves and the rest (cone operations, residuals,
host reductions).  Every timed part ends with a device synchronisation, so the parts add up to the wall time of the loop.
With --qp: coneqp on the same two workloads with a quadratic term (workloads.socp_qp_sum_of_norms, sdp_qp_box; the assembly is
kvx_cone_assemble_h_dev), and the assembly alone with and without H on the same G and W.

    python tools/cone_time.py [--qp] [--socp NX NCONES] [--sdp N ORDER]
    python tools/cone_time.py --gram ORDER COLUMNS      (the FP64 rate of the 's' Gram product, by subtraction)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from kvxopt_amd import _lib, cone, solvers, workloads  # noqa: E402
from kvxopt_amd.base import spmatrix  # noqa: E402


def _sync():
    _lib.raise_for(_lib.lib().kvx_dev_sync())


def run(name, c, G, h, dims, P=None):
    """P = None: conelp(c, G, h, dims); else coneqp(P, c, G, h, dims)."""
    if P is None:
        call = lambda: solvers.conelp(c, G, h, dims, options={"show_progress": False})
    else:
        call = lambda: solvers.coneqp(P, c, G, h, dims, options={"show_progress": False})
    acc = {"assembly": 0.0, "factorisation": 0.0, "solves": 0.0}
    orig_asm, orig_factor, orig_solve = cone.KKTConeDev.assemble, cone.KKTConeDev.factor, cone.KKTConeDev.solve

    def asm(self, W):
        _sync(); t = time.perf_counter(); orig_asm(self, W); _sync(); acc["assembly"] += time.perf_counter() - t

    def factor(self, W):
        _sync(); t = time.perf_counter(); orig_factor(self, W); _sync()
        acc["factorisation"] += time.perf_counter() - t

    def solve(self, x, y, z):
        _sync(); t = time.perf_counter(); orig_solve(self, x, y, z); _sync(); acc["solves"] += time.perf_counter() - t

    cone.KKTConeDev.assemble, cone.KKTConeDev.factor, cone.KKTConeDev.solve = asm, factor, solve
    try:
        call()                                                                  # warm-up (plans, pools, code objects)
        for k in acc:
            acc[k] = 0.0
        _sync()
        t0 = time.perf_counter()
        sol = call()
        _sync()
        wall = time.perf_counter() - t0
    finally:
        cone.KKTConeDev.assemble, cone.KKTConeDev.factor, cone.KKTConeDev.solve = orig_asm, orig_factor, orig_solve
    it = max(sol["iterations"], 1)
    acc["factorisation"] -= acc["assembly"]                  # (factor() contains the assembly)
    other = wall - sum(acc.values())
    out = {"workload": name, "solver": "conelp" if P is None else "coneqp", "status": sol["status"], "iterations": sol["iterations"], "ms_total": 1e3 * wall,
           "ms_per_iteration": 1e3 * wall / it}
    for k, v in list(acc.items()) + [("cone ops and rest", other)]:
        out["ms_per_iteration " + k] = 1e3 * v / it
        out["share " + k] = v / wall
    print(json.dumps(out))


def gram_rate(m, c, reps=20):
    """FP64 rate of the 's' Gram product Y'Y (k_cone_gram), by subtraction: the assembly of an 's'-only S (one block of order m,
    c dense clique columns) minus the congruence kvx_nts_scale_dev on the same c columns, both timed over `reps` calls with a
    device synchronisation around them.  What remains is the Gram product plus the densification, pack2 and gathers (memory
    passes over 8 (2 m^2 + m(m+1)/2) c bytes), so the rate is a lower bound on the kernel's own."""
    rng = np.random.default_rng(7)
    D = cone.Dims({"l": 0, "q": [], "s": [m]})
    F = rng.standard_normal((m, m, c))
    G = (F + F.transpose(1, 0, 2)).reshape(m * m, c, order="F")
    Gp = np.arange(c + 1, dtype=np.int64) * (m * m)
    Gi = np.tile(np.arange(m * m, dtype=np.int64), c)
    plan = cone.ConePlan(D, c, Gp, Gi)
    W = cone.WDev(D)
    W.identity()
    Gx = cone.DVec(m * m * c, G.reshape(-1, order="F"))
    Sx = cone.DVec(plan.Si.size)
    X, Wk = cone.DVec(m * m * c, G.reshape(-1, order="F")), cone.DVec(m * m * c)
    plan.assemble(Gx, W, Sx)
    _sync()
    t = time.perf_counter()
    for _ in range(reps):
        plan.assemble(Gx, W, Sx)
    _sync()
    t_asm = (time.perf_counter() - t) / reps
    t = time.perf_counter()
    for _ in range(reps):
        _lib.raise_for(_lib.lib().kvx_nts_scale_dev(1, D.d_off2.ptr, D.d_off1.ptr, W.rti.ptr, X.ptr, m * m, c, 0, Wk.ptr, m * m))
    _sync()
    t_scale = (time.perf_counter() - t) / reps
    mp = m * (m + 1) // 2
    nt = (c + 15) // 16
    flops_useful = mp * c * (c + 1)                      # lower triangle with the diagonal, 2 flops per multiply-add
    flops_tiles = 2 * mp * 256 * nt * (nt + 1) // 2      # what the 16 x 16 tiles execute
    rest = max(t_asm - t_scale, 1e-9)
    print(json.dumps({"gram": "order %d, %d clique columns" % (m, c), "ms_assembly": 1e3 * t_asm, "ms_congruence": 1e3 * t_scale,
                      "ms_rest (Gram + densify + pack2 + gathers)": 1e3 * rest, "gflop_useful": flops_useful / 1e9,
                      "tflops_lower_bound_useful": flops_useful / rest / 1e12, "tflops_lower_bound_tiles": flops_tiles / rest / 1e12,
                      "fraction_of_50_tflops_tiles": flops_tiles / rest / 50e12}))


def assembly_with_and_without_h(name, G, dims, Pl, reps=20):
    """The assembly alone on the pattern of G at W = I: kvx_cone_assemble_dev, and kvx_cone_assemble_h_dev with the lower CCS Pl,
    `reps` calls each between two device synchronisations, three rounds (the spread is printed)."""
    D = cone.Dims(dims)
    _, n, Gp, Gi, Gx = cone._ccs(G)
    W = cone.WDev(D)
    W.identity()
    Gxd = cone.DVec(max(Gx.size, 1), Gx)
    Hxd = cone.DVec(max(Pl[2].size, 1), Pl[2])
    out = {"assembly": name}
    for key, plan, hx in (("without H", cone.ConePlan(D, n, Gp, Gi), None), ("with H", cone.ConePlan(D, n, Gp, Gi, Pl[0], Pl[1]), Hxd)):
        Sx = cone.DVec(max(plan.Si.size, 1))
        plan.assemble(Gxd, W, Sx, hx)
        ms = []
        for _ in range(3):
            _sync()
            t = time.perf_counter()
            for _ in range(reps):
                plan.assemble(Gxd, W, Sx, hx)
            _sync()
            ms.append(1e3 * (time.perf_counter() - t) / reps)
        out["ms " + key] = sorted(ms)
        out["nnz(S) " + key] = int(plan.Si.size)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--socp", nargs=2, type=int, default=[30000, 20000])
    ap.add_argument("--sdp", nargs=2, type=int, default=[2000, 128])
    ap.add_argument("--qp", action="store_true", help="coneqp on the two workloads with a quadratic term, and the assembly with / without H")
    ap.add_argument("--gram", nargs=2, type=int, default=None, metavar=("ORDER", "COLUMNS"),
                    help="only the Gram-rate measurement of one 's' block")
    a = ap.parse_args()
    _lib.require_device()
    if a.gram:
        gram_rate(*a.gram)
        return
    if a.qp:
        Pl, q, (N, n, cp, ri, v), h, dims = workloads.socp_qp_sum_of_norms(*a.socp)
        G = spmatrix.from_ccs(N, n, cp, ri, v)
        run("socp-qp %d x %d cones" % tuple(a.socp), q, G, h, dims, P=spmatrix.from_ccs(n, n, *Pl))
        assembly_with_and_without_h("socp-qp %d x %d cones" % tuple(a.socp), G, dims, Pl)
        Pl, q, G, h, dims = workloads.sdp_qp_box(a.sdp[0], [a.sdp[1]], density=0.02)
        nz = np.nonzero(G)
        G = spmatrix(G[nz], *nz, size=G.shape)
        run("sdp-qp n=%d, one block of order %d" % tuple(a.sdp), q, G, h, dims, P=spmatrix.from_ccs(q.size, q.size, *Pl))
        assembly_with_and_without_h("sdp-qp n=%d, one block of order %d" % tuple(a.sdp), G, dims, Pl)
        return
    c, (N, n, cp, ri, v), h, dims = workloads.socp_sum_of_norms(*a.socp)
    run("socp %d x %d cones" % tuple(a.socp), c, spmatrix.from_ccs(N, n, cp, ri, v), h, dims)
    c, G, h, dims = workloads.sdp_box(a.sdp[0], [a.sdp[1]], density=0.02)
    nz = np.nonzero(G)
    run("sdp n=%d, one block of order %d" % tuple(a.sdp), c, spmatrix(G[nz], *nz, size=G.shape), h, dims)


if __name__ == "__main__":
    main()
