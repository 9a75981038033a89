"""General-cone path on the GPU: kvx_cone_assemble_dev against a dense Gs' Gs, misc.kkt_chol against a dense solve of the
reduced system, and solvers.conelp / socp / sdp on the reference's documented examples and on generated workloads."""
import json
import os

import numpy as np
import pytest

from kvxopt_amd import _lib, base, cone, misc, solvers, workloads
from kvxopt_amd.base import matrix, spmatrix

pytestmark = pytest.mark.gpu


def _interior(dims, rng):
    """A random point in the interior of the cone."""
    parts = [rng.random(dims["l"]) + 0.5]
    for k in dims["q"]:
        u = rng.standard_normal(k - 1)
        parts.append(np.concatenate([[np.linalg.norm(u) + 0.5 + rng.random()], u]))
    for m in dims["s"]:
        B = rng.standard_normal((m, m))
        parts.append((B @ B.T + m * np.eye(m)).reshape(-1, order="F"))
    return np.concatenate(parts)


def _dense_gs(G, W, dims):
    """pack2(W^-T G) with the pinned GPU ops misc.scale / misc.pack2, as a numpy array (cdim_pckd x n)."""
    Gs = matrix(np.asfortranarray(G.copy()))
    misc.scale(Gs, W, trans="T", inverse="I")
    misc.pack2(Gs, dims)
    npk = dims["l"] + sum(dims["q"]) + sum(m * (m + 1) // 2 for m in dims["s"])
    return np.asarray(Gs.a)[:npk, :]


def _setup(dims, n, dens, seed):
    rng = np.random.default_rng(seed)
    D = cone.Dims(dims)
    G = rng.standard_normal((D.N, n)) * (rng.random((D.N, n)) < dens)
    s, z = _interior(dims, rng), _interior(dims, rng)
    lm = matrix(np.zeros(D.Nd))
    W = misc.compute_scaling(matrix(s), matrix(z), lm, dims)
    return rng, D, G, W


@pytest.mark.parametrize("dims,n,dens,ws", [
    ({"l": 0, "q": [5, 3, 7], "s": []}, 14, 0.3, None),
    ({"l": 0, "q": [], "s": [4, 6]}, 12, 0.3, None),
    ({"l": 6, "q": [4, 2], "s": [3, 5]}, 16, 0.25, None),
    ({"l": 2, "q": [], "s": [70]}, 40, 0.05, None),     # order >= 64, 40 clique columns: full and partial 16 x 16 MFMA tiles
    ({"l": 2, "q": [3], "s": [70, 9]}, 40, 0.05, 30000),  # a workspace of 6 columns of order 70: the densification in chunks
])
def test_assembly_matches_dense_gram(dims, n, dens, ws, monkeypatch):
    _lib.require_device()
    if ws is not None:
        monkeypatch.setenv("KVX_CONE_WS_DOUBLES", str(ws))
    rng, D, G, W = _setup(dims, n, dens, 7 + n)
    Gs = _dense_gs(G, W, dims)
    ref = np.tril(Gs.T @ Gs)
    sp = spmatrix(G[np.nonzero(G)], *np.nonzero(G), size=G.shape)
    _, _, Gp, Gi, Gx = cone._ccs(sp)
    plan = cone.ConePlan(D, n, Gp, Gi)
    Wd = cone.WDev(D)
    Wd.set_host(W)
    Gxd = cone.DVec(max(Gx.size, 1), Gx)
    Sx = cone.DVec(max(plan.Si.size, 1))
    plan.assemble(Gxd, Wd, Sx)
    got = np.zeros((n, n))
    vals = Sx.get()[:plan.Si.size]
    for j in range(n):
        got[plan.Si[plan.Sp[j]:plan.Sp[j + 1]], j] = vals[plan.Sp[j]:plan.Sp[j + 1]]
    scale_ = np.abs(ref).max()
    assert np.abs(got - ref).max() <= 1e-13 * scale_, np.abs(got - ref).max() / scale_
    # the dense product vanishes off the pattern
    on = np.zeros((n, n), dtype=bool)
    for j in range(n):
        on[plan.Si[plan.Sp[j]:plan.Sp[j + 1]], j] = True
    assert np.all(ref[~on] == 0.0)
    # two assemblies: the same bits
    Sx2 = cone.DVec(max(plan.Si.size, 1))
    plan.assemble(Gxd, Wd, Sx2)
    assert Sx2.get().tobytes() == Sx.get().tobytes()


@pytest.mark.parametrize("p", [0, 3])
def test_kkt_chol_matches_dense_reduced_system(p):
    _lib.require_device()
    dims = {"l": 4, "q": [3, 4], "s": [3, 2]}
    n = 10
    rng, D, G, W = _setup(dims, n, 0.6, 100 + p)
    A = rng.standard_normal((p, n))
    f = misc.kkt_chol(matrix(np.asfortranarray(G)), dims, matrix(np.asfortranarray(A)) if p else spmatrix([], [], [], (0, n)))
    solve = f(W)
    bx, by, bz = rng.standard_normal(n), rng.standard_normal(p), rng.standard_normal(D.N)
    x, y, z = matrix(bx.copy()), matrix(by.copy()), matrix(bz.copy())
    solve(x, y, z)
    # dense: [Gs'Gs A'; A 0] [ux; uy] = [bx + Gs' bzp; by], W uz (packed) = Gs ux - bzp, bzp = pack(W^-T bz)
    Gs = _dense_gs(G, W, dims)
    t = matrix(bz.copy())
    misc.scale(t, W, trans="T", inverse="I")
    bzp = matrix(np.zeros(D.Np))
    misc.pack(t, bzp, dims)
    bzp = np.asarray(bzp.a).reshape(-1)
    K = np.block([[Gs.T @ Gs, A.T], [A, np.zeros((p, p))]])
    u = np.linalg.solve(K, np.concatenate([bx + Gs.T @ bzp, by]))
    wz = Gs @ u[:n] - bzp
    zp = matrix(np.zeros(D.Np))
    misc.pack(z, zp, dims)
    rel = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1.0)
    assert rel(np.asarray(x.a).reshape(-1), u[:n]) < 1e-10
    if p:
        assert rel(np.asarray(y.a).reshape(-1), u[n:]) < 1e-10
    assert rel(np.asarray(zp.a).reshape(-1), wz) < 1e-10


def _doc_conelp(lower_only=False):
    c = matrix([-6., -4., -5.])
    G = matrix([[16., 7., 24., -8., 8., -1., 0., -1., 0., 0., 7., -5., 1., -5., 1., -7., 1., -7., -4.],
                [-14., 2., 7., -13., -18., 3., 0., 0., -1., 0., 3., 13., -6., 13., 12., -10., -6., -10., -28.],
                [5., 0., -15., 12., -6., 17., 0., 0., 0., -1., 9., 6., -6., 6., -7., -7., -6., -7., -11.]])
    h = matrix([-3., 5., 12., -2., -14., -13., 10., 0., 0., 0., 68., -30., -19., -30., 99., 23., -19., 23., 10.])
    if lower_only:                                   # doc/source/coneprog.rst: only the lower triangles are read
        for r in (13, 16, 17):
            G.a[r, :] = 0.0
            h.a[r, 0] = 0.0
    return c, G, h, {"l": 2, "q": [4, 4], "s": [3]}


@pytest.mark.parametrize("lower_only", [False, True])
def test_conelp_doc_example(lower_only):
    # doc/source/coneprog.rst:317-355; reference (pure, kkt_chol): optimal in 12 iterations,
    # x = [-1.2209152502626, 0.0966332396663, 3.5775015538661]
    c, G, h, dims = _doc_conelp(lower_only)
    sol = solvers.conelp(c, G, h, dims, options={"show_progress": False})
    assert sol["status"] == "optimal"
    np.testing.assert_allclose(sol["x"], [-1.2209152502626, 0.0966332396663, 3.5775015538661], rtol=1e-6)
    assert sol["iterations"] == 12
    zdoc = [9.30e-02, 2.04e-08, 2.35e-01, 1.33e-01, -4.74e-02, 1.88e-01, 2.79e-08, 1.85e-09, -6.32e-10, -7.59e-09,
            1.26e-01, 8.78e-02, -8.67e-02, 8.78e-02, 6.13e-02, -6.06e-02, -8.67e-02, -6.06e-02, 5.98e-02]
    np.testing.assert_allclose(sol["z"], zdoc, rtol=5e-3, atol=1e-6)
    # sparse and dense G: the same answer
    sp = solvers.conelp(c, spmatrix(G.a[np.nonzero(G.a)], *np.nonzero(G.a), size=G.size), h, dims, options={"show_progress": False})
    np.testing.assert_allclose(sp["x"], sol["x"], rtol=1e-10)


def test_socp_doc_example():
    # doc/source/coneprog.rst:945-975; reference: optimal in 9 iterations
    c = matrix([-2., 1., 5.])
    G = [matrix([[12., 13., 12.], [6., -3., -12.], [-5., -5., 6.]])]
    G += [matrix([[3., 3., -1., 1.], [-6., -6., -9., 19.], [10., -2., -2., -3.]])]
    h = [matrix([-12., -3., -2.]), matrix([27., 0., 3., -42.])]
    sol = solvers.socp(c, Gq=G, hq=h, options={"show_progress": False})
    assert sol["status"] == "optimal"
    assert sol["iterations"] == 9
    np.testing.assert_allclose(sol["x"], [-5.02, -5.77, -8.52], rtol=5e-3)
    np.testing.assert_allclose(sol["zq"][0], [1.34, -7.63e-02, -1.34], rtol=5e-3)
    np.testing.assert_allclose(sol["zq"][1], [1.02, 4.02e-01, 7.80e-01, -5.17e-01], rtol=5e-3)


@pytest.mark.parametrize("lower_only", [False, True])
def test_sdp_doc_example(lower_only):
    # doc/source/coneprog.rst:1127-1160; reference: optimal in 7 iterations
    c = matrix([1., -1., 1.])
    if lower_only:
        G = [matrix([[-7., -11., 0., 3.], [7., -18., 0., 8.], [-2., -8., 0., 1.]])]
        G += [matrix([[-21., -11., 0., 0., 10., 8., 0., 0., 5.], [0., 10., 16., 0., -10., -10., 0., 0., 3.],
                      [-5., 2., -17., 0., -6., 8., 0., 0., 6.]])]
        h = [matrix([[33., -9.], [0., 26.]]), matrix([[14., 9., 40.], [0., 91., 10.], [0., 0., 15.]])]
    else:
        G = [matrix([[-7., -11., -11., 3.], [7., -18., -18., 8.], [-2., -8., -8., 1.]])]
        G += [matrix([[-21., -11., 0., -11., 10., 8., 0., 8., 5.], [0., 10., 16., 10., -10., -10., 16., -10., 3.],
                      [-5., 2., -17., 2., -6., 8., -17., 8., 6.]])]
        h = [matrix([[33., -9.], [-9., 26.]]), matrix([[14., 9., 40.], [9., 91., 10.], [40., 10., 15.]])]
    sol = solvers.sdp(c, Gs=G, hs=h, options={"show_progress": False})
    assert sol["status"] == "optimal"
    assert sol["iterations"] == 7
    np.testing.assert_allclose(sol["x"], [-3.68e-01, 1.90, -8.88e-01], rtol=5e-3)
    np.testing.assert_allclose(sol["zs"][0], [[3.96e-03, -4.34e-03], [-4.34e-03, 4.75e-03]], rtol=5e-3)
    np.testing.assert_allclose(sol["zs"][1], [[5.58e-02, -2.41e-03, 2.42e-02], [-2.41e-03, 1.04e-04, -1.05e-03],
                                              [2.42e-02, -1.05e-03, 1.05e-02]], rtol=5e-3, atol=1e-6)


def test_mixed_cones_runs_are_bitwise_reproducible():
    c, G, h, dims = _doc_conelp()
    A = matrix([[1.0], [1.0], [1.0]])
    b = matrix([2.4])
    runs = [solvers.conelp(c, G, h, dims, A=A, b=b, options={"show_progress": False}) for _ in range(2)]
    assert runs[0]["status"] == "optimal"
    assert abs(runs[0]["x"].sum() - 2.4) < 1e-7
    for k in ("x", "y", "s", "z"):
        assert runs[0][k].tobytes() == runs[1][k].tobytes()


def _check_optimal(sol, c, Gmv, Gtmv, h, dims, tol):
    """residuals (against feastol, as the solver's own pres / dres: coneprog.py:861-896), cone membership and gap in numpy"""
    x, s, z = sol["x"], sol["s"], sol["z"]
    assert np.linalg.norm(Gmv(x) + s - h) / max(1.0, np.linalg.norm(h)) <= tol * (1 + 1e-6)
    assert np.linalg.norm(Gtmv(z) + c) / max(1.0, np.linalg.norm(c)) <= tol * (1 + 1e-6)
    r = dims["l"]
    assert s[:r].min() >= -tol and z[:r].min() >= -tol
    for k in dims["q"]:
        for v in (s, z):
            assert v[r] - np.linalg.norm(v[r + 1:r + k]) >= -tol
        r += k
    for m in dims["s"]:
        for v in (s, z):
            assert np.linalg.eigvalsh(v[r:r + m * m].reshape(m, m, order="F")).min() >= -tol * max(1.0, np.abs(v[r:r + m * m]).max())
        r += m * m
    assert sol["gap"] <= max(1e-7, 1e-6 * abs(sol["primal objective"]))


def test_socp_at_scale():
    c, (N, n, cp, ri, v), h, dims = workloads.socp_sum_of_norms(30000, 20000)
    G = spmatrix.from_ccs(N, n, cp, ri, v)
    sol = solvers.conelp(c, G, h, dims, options={"show_progress": False})
    assert sol["status"] == "optimal"
    cols = np.repeat(np.arange(n), np.diff(cp))
    _check_optimal(sol, c, lambda u: np.bincount(ri, v * u[cols], minlength=N), lambda w: np.bincount(cols, v * w[ri], minlength=n),
                   h, dims, 1e-7)


def test_sdp_at_scale():
    c, G, h, dims = workloads.sdp_box(2000, [128], density=0.02)
    nz = np.nonzero(G)
    sol = solvers.conelp(c, spmatrix(G[nz], *nz, size=G.shape), h, dims, options={"show_progress": False})
    assert sol["status"] == "optimal"
    _check_optimal(sol, c, lambda u: G @ u, lambda w: G.T @ w, h, dims, 1e-7)


# ---- G19 / G20: recorded from the pure reference (tests/golden/make_goldens_cones.py: dense G, kktsolver='chol') ---------------
_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_G19 = json.load(open(os.path.join(_GOLD, "g19_cone_programs.json")))


def _g19(name):
    Z = np.load(os.path.join(_GOLD, "g19_cone_programs.npz"))
    return {k.split("__", 1)[1]: Z[k] for k in Z.files if k.startswith(name + "__")}, _G19["cases"][name]


def _g19_solve(d, meta, G=None, **kw):
    dims = meta["dims"]
    A = matrix(np.asfortranarray(d["A"])) if "A" in d else None
    b = matrix(d["b"]) if "b" in d else None
    Gm = G if G is not None else matrix(np.asfortranarray(d["G"]))
    return solvers.conelp(matrix(d["c"]), Gm, matrix(d["h"]), dims, A=A, b=b, options={"show_progress": False}, **kw)


@pytest.mark.parametrize("name", sorted(_G19["cases"]))
def test_conelp_matches_g19(name):
    d, meta = _g19(name)
    kw = {}
    if "primalstart_x" in d:
        kw["primalstart"] = {"x": matrix(d["primalstart_x"]), "s": matrix(d["primalstart_s"])}
    if "dualstart_z" in d:                               # (case dualstart_no_y: no 'y', which must start at 0)
        kw["dualstart"] = {"z": matrix(d["dualstart_z"])}
        if "dualstart_y" in d:
            kw["dualstart"]["y"] = matrix(d["dualstart_y"])
    sol = _g19_solve(d, meta, **kw)
    assert sol["status"] == meta["status"]
    assert sol["iterations"] == meta["iterations"]      # the same Newton system as the reference's kkt_chol
    for k, rel in (("x", True), ("y", True), ("s", False), ("z", False)):
        if "sol_" + k not in d or d["sol_" + k].size == 0:
            continue
        ref = d["sol_" + k]
        err = np.linalg.norm(sol[k] - ref)
        assert err <= 1e-6 * max(np.linalg.norm(ref), 1.0 if rel else 0.0) + (0.0 if rel else 1e-12), (k, err)
    for k in ("primal objective", "dual objective"):
        if meta[k] is not None:
            assert abs(sol[k] - meta[k]) <= 1e-7 * max(abs(meta[k]), 1.0), (k, sol[k], meta[k])


@pytest.mark.parametrize("p", [0, 3])
def test_kkt_chol_matches_g20(p):
    Z = np.load(os.path.join(_GOLD, "g20_kkt_chol_cones.npz"))
    dims = {"l": int(Z["dims_l"][0]), "q": [int(k) for k in Z["dims_q"]], "s": [int(k) for k in Z["dims_s"]]}
    g = lambda k: Z["p%d_%s" % (p, k)]
    D = cone.Dims(dims)
    n = g("G").shape[1]
    # the reference's W (its 's' part is defined up to the signs of singular vectors, and W uz depends on that choice)
    cut = lambda a, sizes: [a[o:o + k] for o, k in zip(np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(int), sizes)]
    W = {"d": matrix(g("W_d")), "di": matrix(g("W_di")), "beta": list(g("W_beta")),
         "v": [matrix(v) for v in cut(g("W_v"), dims["q"])],
         "r": [matrix(r, (m, m)) for r, m in zip(cut(g("W_r"), [m * m for m in dims["s"]]), dims["s"])],
         "rti": [matrix(r, (m, m)) for r, m in zip(cut(g("W_rti"), [m * m for m in dims["s"]]), dims["s"])]}
    A = matrix(np.asfortranarray(g("A"))) if p else spmatrix([], [], [], (0, n))
    solve = misc.kkt_chol(matrix(np.asfortranarray(g("G"))), dims, A)(W)
    x, y, z = matrix(g("bx").copy()), matrix(g("by").copy()), matrix(g("bz").copy())
    solve(x, y, z)
    rel = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    assert rel(np.asarray(x.a).reshape(-1), g("ux")) <= 1e-10
    if p:
        assert rel(np.asarray(y.a).reshape(-1), g("uy")) <= 1e-10
    # uz: the 'l' and 'q' entries and the lower triangles of the 's' blocks (the upper triangles are not part of the result)
    keep = np.ones(D.N, dtype=bool)
    for k, m in enumerate(dims["s"]):
        i, j = np.triu_indices(m, 1)
        keep[D.ind + D.off2[k] + i + m * j] = False
    assert rel(np.asarray(z.a).reshape(-1)[keep], g("uz")[keep]) <= 1e-10
