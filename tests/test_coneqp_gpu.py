"""Cone QPs with 'q' / 's' blocks on the GPU: kvx_cone_assemble_h_dev against a dense H + Gs' Gs, misc.kkt_chol(G, dims, A)(W, H)
against the reference (G22), solvers.coneqp against the reference (G21: tests/golden/make_goldens_coneqp.py, dense P and G,
kktsolver='chol') and on generated workloads at scale."""
import json
import os

import numpy as np
import pytest

from kvxopt_amd import _lib, cone, misc, solvers, workloads
from kvxopt_amd.base import matrix, spmatrix

pytestmark = pytest.mark.gpu

_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_G21 = json.load(open(os.path.join(_GOLD, "g21_coneqp_cones.json")))
QUIET = {"show_progress": False}


def _interior(dims, rng):
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


def _sp(M):
    nz = np.nonzero(M)
    return spmatrix(M[nz], *nz, size=M.shape)


def _unpack(n, plan, Sx):
    got = np.zeros((n, n))
    on = np.zeros((n, n), dtype=bool)
    vals = Sx.get()[:plan.Si.size]
    for j in range(n):
        got[plan.Si[plan.Sp[j]:plan.Sp[j + 1]], j] = vals[plan.Sp[j]:plan.Sp[j + 1]]
        on[plan.Si[plan.Sp[j]:plan.Sp[j + 1]], j] = True
    return got, on


GRID = [
    ({"l": 0, "q": [5, 3, 7], "s": []}, 14, 0.3, None),
    ({"l": 0, "q": [], "s": [4, 6]}, 12, 0.3, None),
    ({"l": 6, "q": [4, 2], "s": [3, 5]}, 16, 0.25, None),
    ({"l": 2, "q": [], "s": [70]}, 40, 0.05, None),
    ({"l": 2, "q": [3], "s": [70, 9]}, 40, 0.05, 30000),
]


@pytest.mark.parametrize("widen", [False, True])
@pytest.mark.parametrize("dims,n,dens,ws", GRID)
def test_assembly_with_h_matches_dense(dims, n, dens, ws, widen, monkeypatch):
    """The parameter grid of test_cone_gpu.test_assembly_matches_dense_gram, with an H inside the clique pattern of G and with
    one that widens it."""
    _lib.require_device()
    if ws is not None:
        monkeypatch.setenv("KVX_CONE_WS_DOUBLES", str(ws))
    rng, D, G, W = _setup(dims, n, dens, 7 + n)
    if widen:
        G[:, n - 3:] = 0.0      # (the cliques of these G cover the whole lower triangle) three columns that no row of G touches
    Gs = _dense_gs(G, W, dims)
    _, _, Gp, Gi, Gx = cone._ccs(_sp(G))
    base = cone.ConePlan(D, n, Gp, Gi)
    _, inside = _unpack(n, base, cone.DVec(max(base.Si.size, 1)).fill(0.0))
    if widen:
        mask = np.tril(rng.random((n, n)) < 0.3)
        mask[n - 1, n - 1] = mask[n - 1, 0] = True
        assert (mask & ~inside).any() and (mask & inside).any()
    else:
        mask = inside & np.tril(rng.random((n, n)) < 0.5)
        assert mask.any()
    H = np.where(mask, rng.standard_normal((n, n)), 0.0)              # lower triangle of a symmetric H
    Hp, Hi, Hx = cone.lower_ccs(_sp(H), n)
    assert Hx.size == mask.sum()
    plan = cone.ConePlan(D, n, Gp, Gi, Hp, Hi)
    Wd = cone.WDev(D)
    Wd.set_host(W)
    Gxd = cone.DVec(max(Gx.size, 1), Gx)
    Hxd = cone.DVec(max(Hx.size, 1), Hx)
    Sx = cone.DVec(max(plan.Si.size, 1))
    plan.assemble(Gxd, Wd, Sx, Hxd)
    got, on = _unpack(n, plan, Sx)
    np.testing.assert_array_equal(on, inside | mask)
    ref = np.tril(Gs.T @ Gs) + H
    scale_ = np.abs(ref).max()
    err = np.abs(got - ref).max()
    print("assembly with H: max error / max|S| = %.3e" % (err / scale_))
    assert err <= 1e-13 * scale_, err / scale_
    # entries that only H reaches hold its value alone
    only = mask & ~inside
    assert np.array_equal(got[only], H[only])
    # two assemblies with a nonzero H: the same bits
    Sx2 = cone.DVec(max(plan.Si.size, 1))
    plan.assemble(Gxd, Wd, Sx2, Hxd)
    assert Sx2.get().tobytes() == Sx.get().tobytes()
    if not widen:
        # an H inside the cliques with all-zero values: the bits of the assembly without H
        assert np.array_equal(plan.Sp, base.Sp) and np.array_equal(plan.Si, base.Si)
        S0, S1 = cone.DVec(max(plan.Si.size, 1)), cone.DVec(max(plan.Si.size, 1))
        base.assemble(Gxd, Wd, S0)
        plan.assemble(Gxd, Wd, S1, cone.DVec(max(Hx.size, 1)).fill(0.0))
        assert S1.get().tobytes() == S0.get().tobytes()


def _g22_W(g, dims):
    cut = lambda a, sizes: [a[o:o + k] for o, k in zip(np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(int), sizes)]
    return {"d": matrix(g("W_d")), "di": matrix(g("W_di")), "beta": list(g("W_beta")),
            "v": [matrix(v) for v in cut(g("W_v"), dims["q"])],
            "r": [matrix(r, (m, m)) for r, m in zip(cut(g("W_r"), [m * m for m in dims["s"]]), dims["s"])],
            "rti": [matrix(r, (m, m)) for r, m in zip(cut(g("W_rti"), [m * m for m in dims["s"]]), dims["s"])]}


@pytest.mark.parametrize("kind", ["dense", "sparse", "numpy"])
@pytest.mark.parametrize("p", [0, 3])
def test_kkt_chol_with_h_matches_g22(p, kind):
    Z = np.load(os.path.join(_GOLD, "g22_kkt_chol_h.npz"))
    dims = {"l": int(Z["dims_l"][0]), "q": [int(k) for k in Z["dims_q"]], "s": [int(k) for k in Z["dims_s"]]}
    g = lambda k: Z["p%d_%s" % (p, k)]
    D = cone.Dims(dims)
    n = g("G").shape[1]
    W = _g22_W(g, dims)
    A = matrix(np.asfortranarray(g("A"))) if p else spmatrix([], [], [], (0, n))
    Hd = g("H")
    H = {"dense": matrix(np.asfortranarray(Hd)), "sparse": _sp(np.tril(Hd)), "numpy": Hd}[kind]
    factor = misc.kkt_chol(matrix(np.asfortranarray(g("G"))), dims, A)
    rel = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    keep = np.ones(D.N, dtype=bool)                      # uz: not the strict upper triangles of the 's' blocks
    for k, m in enumerate(dims["s"]):
        i, j = np.triu_indices(m, 1)
        keep[D.ind + D.off2[k] + i + m * j] = False

    def check(solve):
        x, y, z = matrix(g("bx").copy()), matrix(g("by").copy()), matrix(g("bz").copy())
        solve(x, y, z)
        ex = rel(np.asarray(x.a).reshape(-1), g("ux"))
        ez = rel(np.asarray(z.a).reshape(-1)[keep], g("uz")[keep])
        ey = rel(np.asarray(y.a).reshape(-1), g("uy")) if p else 0.0
        print("G22 p=%d %s: ux %.2e uy %.2e uz %.2e" % (p, kind, ex, ey, ez))
        assert ex <= 1e-10 and ey <= 1e-10 and ez <= 1e-10
        return np.asarray(x.a).reshape(-1).copy()

    x1 = check(factor(W, H))
    # other values on the same pattern (values refreshed, same plan), then the first values again: the same bits as before
    H2 = {"dense": matrix(np.asfortranarray(2.0 * Hd)), "sparse": _sp(np.tril(2.0 * Hd)), "numpy": 2.0 * Hd}[kind]
    x, y, z = matrix(g("bx").copy()), matrix(g("by").copy()), matrix(g("bz").copy())
    factor(W, H2)(x, y, z)
    assert rel(np.asarray(x.a).reshape(-1), g("ux")) > 1e-6
    assert check(factor(W, H)).tobytes() == x1.tobytes()
    # another pattern: a new plan and analysis (here: the diagonal of H only), checked against a dense solve through H = 0 + diag
    if kind == "sparse":
        Hdiag = np.diag(np.diag(Hd))
        xa, ya, za = matrix(g("bx").copy()), matrix(g("by").copy()), matrix(g("bz").copy())
        factor(W, _sp(Hdiag))(xa, ya, za)
        xb, yb, zb = matrix(g("bx").copy()), matrix(g("by").copy()), matrix(g("bz").copy())
        misc.kkt_chol(matrix(np.asfortranarray(g("G"))), dims, A)(W, matrix(np.asfortranarray(Hdiag)))(xb, yb, zb)
        assert rel(np.asarray(xa.a).reshape(-1), np.asarray(xb.a).reshape(-1)) <= 1e-10
        assert check(factor(W, H)).tobytes() == x1.tobytes()


def test_kkt_chol_df_and_mnl_still_raise():
    dims = {"l": 2, "q": [2], "s": []}
    G = matrix(np.asfortranarray(np.ones((4, 2))))
    A = spmatrix([], [], [], (0, 2))
    with pytest.raises(NotImplementedError) as e:
        misc.kkt_chol(G, dims, A, mnl=1)
    assert "H" not in str(e.value).replace("HBM", "")
    W = {"d": matrix([1.0, 1.0]), "di": matrix([1.0, 1.0]), "beta": [1.0], "v": [matrix([1.0, 0.0])], "r": [], "rti": []}
    with pytest.raises(NotImplementedError) as e:
        misc.kkt_chol(G, dims, A)(W, None, matrix(np.ones((1, 2))))
    assert " H " not in str(e.value) and "Df" in str(e.value)


# ---- G21 ------------------------------------------------------------------------------------------------------------------------
def _g21(name):
    Z = np.load(os.path.join(_GOLD, "g21_coneqp_cones.npz"))
    return {k.split("__", 1)[1]: Z[k] for k in Z.files if k.startswith(name + "__")}, _G21["cases"][name]


def _g21_solve(d, meta, dense=False):
    kw = {}
    if "A" in d:
        kw["A"], kw["b"] = matrix(np.asfortranarray(d["A"])), matrix(d["b"])
    if "init_x" in d:
        kw["initvals"] = {k: matrix(d["init_" + k]) for k in ("x", "y", "s", "z")}
    opts = dict(QUIET)
    opts.update(meta["options"])
    if dense:
        P, G = matrix(np.asfortranarray(d["P"])), matrix(np.asfortranarray(d["G"]))
    else:
        P, G = _sp(d["P"]), _sp(d["G"])                  # P with whatever the fixture holds above its diagonal
    return solvers.coneqp(P, matrix(d["q"]), G, matrix(d["h"]), meta["dims"], options=opts, **kw)


G21_CASES = ["doc_coneqp", "socp_qp_sparse", "sdp_qp", "mixed_eq", "p_zero", "p_singular", "g_rank_deficient", "p_widens_pattern",
             "p_upper_garbage", "initvals", "no_correction", "refine0", "refine2"]


def test_g21_holds_every_case():
    assert sorted(_G21["cases"]) == sorted(G21_CASES)
    assert _G21["via"].startswith("reference")
    # case 8: the inputs of case 2 but for the upper triangle of P, and the results of case 2
    a, b = _g21("socp_qp_sparse")[0], _g21("p_upper_garbage")[0]
    assert np.array_equal(np.tril(a["P"]), np.tril(b["P"])) and not np.array_equal(a["P"], b["P"])
    for k in ("q", "G", "h", "sol_x", "sol_s", "sol_z"):
        assert np.array_equal(a[k], b[k])
    # g_rank_deficient: G alone has deficient column rank, S = P + Gs' Gs is definite through P only (Rank([P; G]) = n)
    d = _g21("g_rank_deficient")[0]
    n = d["G"].shape[1]
    assert np.linalg.matrix_rank(d["G"]) < n and np.linalg.matrix_rank(d["P"]) < n
    assert np.linalg.matrix_rank(np.vstack([d["P"], d["G"]])) == n


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("name", G21_CASES)
def test_coneqp_matches_g21(name, dense):
    d, meta = _g21(name)
    sol = _g21_solve(d, meta, dense)
    print("G21 %s: %s in %d iterations (reference: %s in %d)" % (name, sol["status"], sol["iterations"], meta["status"],
                                                                  meta["iterations"]))
    assert sol["status"] == meta["status"]
    assert sol["iterations"] == meta["iterations"]      # the same Newton system as the reference's kkt_chol with H = P
    for k, rel in (("x", True), ("y", True), ("s", False), ("z", False)):
        if d["sol_" + k].size == 0:
            continue
        ref = d["sol_" + k]
        err = np.linalg.norm(sol[k] - ref)
        print("   %s: |diff| = %.3e, |ref| = %.3e" % (k, err, np.linalg.norm(ref)))
        assert err <= 1e-6 * max(np.linalg.norm(ref), 1.0 if rel else 0.0) + (0.0 if rel else 1e-12), (k, err)
    for k in ("primal objective", "dual objective"):
        assert abs(sol[k] - meta[k]) <= 1e-7 * max(abs(meta[k]), 1.0), (k, sol[k], meta[k])
    assert set(sol) == {"x", "y", "s", "z", "status", "gap", "relative gap", "primal objective", "dual objective",
                        "primal infeasibility", "dual infeasibility", "primal slack", "dual slack", "iterations", "factorizations"}
    if name == "doc_coneqp":                             # doc/source/coneprog.rst:596-599
        assert ["%.3f" % v for v in sol["x"]] == ["0.726", "0.618", "0.303"]
    # the 's' blocks come back as full symmetric matrices
    r = meta["dims"]["l"] + sum(meta["dims"]["q"])
    for m in meta["dims"]["s"]:
        for v in (sol["s"], sol["z"]):
            B = v[r:r + m * m].reshape(m, m)
            assert np.array_equal(B, B.T)
        r += m * m


def test_coneqp_doc_example_as_documented():
    # doc/source/coneprog.rst:584-599, the call as it is printed there
    A = matrix([[.3, -.4, -.2, -.4, 1.3], [.6, 1.2, -1.7, .3, -.3], [-.3, .0, .6, -1.2, -2.0]])
    b = matrix([1.5, .0, -1.2, -.7, .0])
    n = 3
    Aa, ba = np.asarray(A.a).reshape(5, 3), np.asarray(b.a).reshape(-1)
    G = matrix(np.asfortranarray(np.vstack([-np.eye(n), np.zeros((1, n)), np.eye(n)])))
    h = matrix(n * [0.0] + [1.0] + n * [0.0])
    dims = {"l": n, "q": [n + 1], "s": []}
    sol = solvers.coneqp(matrix(np.asfortranarray(Aa.T @ Aa)), matrix(-Aa.T @ ba), G, h, dims, options=QUIET)
    assert sol["status"] == "optimal"
    assert ["%.3f" % v for v in sol["x"]] == ["0.726", "0.618", "0.303"]
    assert abs(np.linalg.norm(sol["x"]) - 1.0) < 1e-6    # the norm ball is active
    # two runs: the same bits
    again = solvers.coneqp(matrix(np.asfortranarray(Aa.T @ Aa)), matrix(-Aa.T @ ba), G, h, dims, options=QUIET)
    for k in ("x", "s", "z"):
        assert again[k].tobytes() == sol[k].tobytes()


def test_coneqp_without_l_rows():
    # dims['l'] = 0: minimize (1/2)|x - a|^2 s.t. |x| <= 1 -> x = a / |a|
    a = np.array([3.0, 4.0])
    G = matrix(np.asfortranarray(np.vstack([np.zeros((1, 2)), -np.eye(2)])))
    sol = solvers.coneqp(matrix(np.asfortranarray(np.eye(2))), matrix(-a), G, matrix([1.0, 0.0, 0.0]), {"l": 0, "q": [3], "s": []},
                         options=QUIET)
    assert sol["status"] == "optimal"
    np.testing.assert_allclose(sol["x"], a / 5.0, atol=1e-6)


# ---- at scale -------------------------------------------------------------------------------------------------------------------
def _check_qp_optimal(sol, Pmv, q, Gmv, Gtmv, h, dims, tol, A=None, b=None):
    """Residuals (against feastol, as the solver's own pres / dres: coneprog.py:2169-2204), cone membership and gap, in numpy."""
    x, y, s, z = sol["x"], sol["y"], sol["s"], sol["z"]
    assert sol["status"] == "optimal"
    rx = Pmv(x) + Gtmv(z) + q + (A.T @ y if A is not None else 0.0)
    dres = np.linalg.norm(rx) / max(1.0, np.linalg.norm(q))
    pres = np.linalg.norm(Gmv(x) + s - h) / max(1.0, np.linalg.norm(h))
    print("at scale: dres %.3e pres %.3e gap %.3e s'z %.3e iterations %d" % (dres, pres, sol["gap"], float(s @ z), sol["iterations"]))
    assert dres <= tol * (1 + 1e-6)
    assert pres <= tol * (1 + 1e-6)
    if A is not None:
        assert np.linalg.norm(A @ x - b) / max(1.0, np.linalg.norm(b)) <= tol * (1 + 1e-6)
    r = dims["l"]
    assert s[:r].min() >= -1e-7 * max(1.0, np.abs(s[:r]).max()) and z[:r].min() >= -1e-7 * max(1.0, np.abs(z[:r]).max())
    for k in dims["q"]:
        for v in (s, z):
            assert v[r] - np.linalg.norm(v[r + 1:r + k]) >= -1e-7 * max(1.0, abs(v[r]))
        r += k
    for m in dims["s"]:
        for v in (s, z):
            assert np.linalg.eigvalsh(v[r:r + m * m].reshape(m, m, order="F")).min() >= -1e-7 * max(1.0, np.abs(v[r:r + m * m]).max())
        r += m * m
    # s'z (full symmetric 's' blocks: the plain inner product is the trace inner product) is the reported gap.  The solver
    # reports lmbda'lmbda, equal to s'z in exact arithmetic (s = W'lmbda, z = W^-1 lmbda); near the boundary of a 'q' cone or an
    # 's' block the terms of s'z cancel, so its rounding error is a few ulps of sum |s_i z_i|, not of the gap
    assert abs(float(s @ z) - sol["gap"]) <= 1e-6 * abs(sol["gap"]) + 64 * np.finfo(float).eps * float(np.abs(s) @ np.abs(z))


def _sym_mv(n, Pl):
    cp, ri, vx = Pl
    cols = np.repeat(np.arange(n), np.diff(cp))
    off = ri != cols
    return lambda u: np.bincount(ri, vx * u[cols], minlength=n) + np.bincount(cols[off], vx[off] * u[ri[off]], minlength=n)


def test_socp_qp_at_scale():
    Pl, q, (N, n, cp, ri, v), h, dims = workloads.socp_qp_sum_of_norms(30000, 20000)
    assert n == 50000
    sol = solvers.coneqp(spmatrix.from_ccs(n, n, *Pl), q, spmatrix.from_ccs(N, n, cp, ri, v), h, dims, options=QUIET)
    cols = np.repeat(np.arange(n), np.diff(cp))
    _check_qp_optimal(sol, _sym_mv(n, Pl), q, lambda u: np.bincount(ri, v * u[cols], minlength=N),
                      lambda w: np.bincount(cols, v * w[ri], minlength=n), h, dims, 1e-7)


def test_sdp_qp_at_scale():
    Pl, q, G, h, dims = workloads.sdp_qp_box(2000, [128], density=0.02)
    n = q.size
    sol = solvers.coneqp(spmatrix.from_ccs(n, n, *Pl), q, _sp(G), h, dims, options=QUIET)
    _check_qp_optimal(sol, _sym_mv(n, Pl), q, lambda u: G @ u, lambda w: G.T @ w, h, dims, 1e-7)


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def _small():
    d, meta = _g21("doc_coneqp")
    return matrix(np.asfortranarray(d["P"])), matrix(d["q"]), matrix(np.asfortranarray(d["G"])), matrix(d["h"]), meta["dims"]


def test_coneqp_with_cones_no_longer_raises():
    P, q, G, h, dims = _small()
    sol = solvers.coneqp(P, q, G, h, dims, options=QUIET)
    assert sol["status"] == "optimal" and sol["factorizations"] == sol["iterations"] + 1


def test_kktsolver_on_the_cone_path_raises():
    P, q, G, h, dims = _small()
    with pytest.raises(NotImplementedError):
        solvers.coneqp(P, q, G, h, dims, kktsolver=lambda W: None, options=QUIET)
    with pytest.raises(NotImplementedError):
        solvers.coneqp(P, q, G, h, dims, kktsolver="chol", options=QUIET)


def test_rank_deficient_p_and_g_raise_the_reference_text():
    # P and G both vanish on (1, 0, -1): S = P + G'G = [4 0 4; 0 1 0; 4 0 4] at W = I, whose second pivot is exactly zero
    P = spmatrix([3.0, 3.0, 3.0], [0, 2, 2], [0, 0, 2], (3, 3))
    G = matrix(np.asfortranarray(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 0.0]])))
    with pytest.raises(ValueError, match=r"Rank\(A\) < p or Rank\(\[P; A; G\]\) < n"):
        solvers.coneqp(P, matrix([1.0, 1.0, 0.0]), G, matrix([1.0, 0.0, 0.0]), {"l": 0, "q": [3], "s": []}, options=QUIET)


def test_wrong_sizes_raise_typeerror():
    P, q, G, h, dims = _small()
    with pytest.raises(TypeError):
        solvers.coneqp(matrix(np.asfortranarray(np.eye(4))), q, G, h, dims, options=QUIET)
    with pytest.raises(TypeError):
        solvers.coneqp(P, matrix([1.0, 2.0]), G, h, dims, options=QUIET)
    with pytest.raises(TypeError):
        solvers.coneqp(P, q, G, matrix(np.ones(6)), dims, options=QUIET)
    A = matrix(np.asfortranarray(np.ones((1, 3))))
    with pytest.raises(TypeError):
        solvers.coneqp(P, q, G, h, dims, A=A, b=matrix([1.0, 2.0]), options=QUIET)
    with pytest.raises(TypeError):
        solvers.coneqp(P, q, G, h, dims, A=matrix(np.asfortranarray(np.ones((1, 2)))), b=matrix([1.0]), options=QUIET)


def test_option_checks():
    P, q, G, h, dims = _small()
    for bad, text in (({"maxiters": 0}, "maxiters"), ({"feastol": 0.0}, "feastol"), ({"abstol": -1.0, "reltol": -1.0}, "reltol"),
                      ({"refinement": -1}, "refinement")):
        with pytest.raises(ValueError, match=text):
            solvers.coneqp(P, q, G, h, dims, options=dict(QUIET, **bad))
    sol = solvers.coneqp(P, q, G, h, dims, options=dict(QUIET, maxiters=2))
    assert sol["status"] == "unknown" and sol["iterations"] == 2
    with pytest.raises(ValueError, match="initial s is not positive"):
        solvers.coneqp(P, q, G, h, dims, initvals={"s": matrix(-np.ones(7))}, options=QUIET)
