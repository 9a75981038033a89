"""solvers.lp_batch on the device against the reference's own runs (G4 doc_lp, primal_infeasible,
dual_infeasible, grid6x5; G8 eq6x5p4), against solvers.lp of this package, and against the numpy.longdouble restatement of
tests/lp_batch_numpy.py on generated members: feasible ones at every shape edge of the kernel (n = 1, n not a multiple of anything,
n = 63 / 64, ml = 255 / 256 / 257 around the 256 threads and the 32-row steps of the assembly, ml = 512, p = 0 / 1 / 16 / n),
primal and dual infeasible ones with their certificates recomputed in numpy, and members with free variables that need the A'A
repair.  The rule of test_coneqp_matches_g21: vectors to 1e-6 max(|ref|, 1) in the 2-norm, objectives to 1e-7 max(|ref|, 1),
statuses, iteration counts and exits exactly.  tests/test_lp_batch_cpu.py shows that no expected status or count of these
batches sits on a rounding edge."""
import json
import os

import numpy as np
import pytest

import lp_batch_numpy as R
from kvxopt_amd import solvers

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VECTORS = ("x", "y", "s", "z")
FLOATS = ("gap", "relative gap", "primal objective", "dual objective", "primal infeasibility", "dual infeasibility",
          "primal slack", "dual slack", "residual as primal infeasibility certificate", "residual as dual infeasibility certificate")
FEASTOL = 1e-7
nrm = np.linalg.norm


def call(M, options=None, which=None, **replace):
    """lp_batch on the members `which` (all of them by default) of a batch from lp_batch_numpy.members."""
    w = slice(None) if which is None else list(which)
    args = {"c": M.c, "G": M.G, "h": M.h, "A": M.A, "b": M.b}
    args.update(replace)
    cut = lambda v, cols: None if v is None else (v[:, w] if cols else v[w])          # noqa: E731
    return solvers.lp_batch(cut(args["c"], True), cut(args["G"], False), cut(args["h"], True), cut(args["A"], False),
                            cut(args["b"], True), options=options)


def vec_err(got, ref):
    """|got - ref| in units of the rule's bound 1e-6 max(|ref|, 1): passes when <= 1."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(nrm(got - ref) / (1e-6 * max(nrm(ref), 1.0)))


def obj_err(got, ref):
    return abs(got - float(ref)) / (1e-7 * max(abs(float(ref)), 1.0))


def member_bytes(sol, k):
    return b"".join([np.ascontiguousarray(sol[v][:, k]).tobytes() for v in VECTORS] + [np.float64(sol[f][k]).tobytes() for f in FLOATS]
                    + [np.int64(sol["iterations"][k]).tobytes(), np.int64(sol["exit"][k]).tobytes(), sol["status"][k].encode()])


def all_bytes(sol):
    return b"".join(member_bytes(sol, k) for k in range(len(sol["status"])))


@pytest.mark.parametrize("name,gfile,p", [("grid6x5", "g4_conelp", 0), ("eq6x5p4", "g8_conelp_eq", 4)])
def test_golden_member_of_a_batch(name, gfile, p):
    meta = json.load(open(os.path.join(GOLDEN, gfile + ".json")))["cases"][name]
    g = np.load(os.path.join(GOLDEN, gfile + ".npz"))
    c, G, h, A, b = R.grid_dense(p)
    rng = np.random.default_rng(5)
    C3 = np.asfortranarray(np.stack([c, c * (1.0 + 0.01 * rng.standard_normal(c.size)), c * (1.0 + 0.01 * rng.standard_normal(c.size))], axis=1))
    sol = solvers.lp_batch(C3, G, h, A, b)                            # shared matrices, h and b as one column
    assert sol["status"] == ["optimal"] * 3 and list(sol["exit"]) == [0, 0, 0]
    assert sol["status"][0] == meta["status"] and sol["iterations"][0] == meta["iterations"]
    one = solvers.lp(c, G, h, A, b, options=R.QUIET)                  # this package's one-problem driver on the same data
    assert one["status"] == "optimal" and one["iterations"] == sol["iterations"][0]
    errs = {}
    for k in VECTORS[:1] + (VECTORS[1:2] if p else ()) + VECTORS[2:]:
        errs[k] = vec_err(sol[k][:, 0], g[name + "_" + k])
        errs[k + " vs solvers.lp"] = vec_err(sol[k][:, 0], one[k])
    for k in ("primal objective", "dual objective"):
        errs[k] = obj_err(sol[k][0], meta[k])
        errs[k + " vs solvers.lp"] = obj_err(sol[k][0], one[k])
    print("%s: errors in units of the bound: %s" % (name, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) <= 1.0
    assert np.isnan(sol[FLOATS[8]]).all() and np.isnan(sol[FLOATS[9]]).all()
    assert len(set(C3[:, k].tobytes() for k in range(3))) == 3 and not np.array_equal(sol["x"][:, 0], sol["x"][:, 1])


@pytest.mark.parametrize("name", sorted(R.TINY))
def test_tiny_golden_in_a_batch_of_its_own(name):
    meta = json.load(open(os.path.join(GOLDEN, "g4_conelp.json")))["cases"][name]
    c, G, h, status, iters, key = R.TINY[name]
    sol = solvers.lp_batch(np.array(c), np.array(G), np.array(h))
    assert sol["status"] == [status] and sol["iterations"][0] == iters == meta["iterations"] and sol["exit"][0] == R.EXITS[status]
    err = vec_err(sol[key][:, 0], meta[key])
    one = solvers.lp(np.array(c), np.array(G), np.array(h), options=R.QUIET)
    assert one["status"] == status and one["iterations"] == iters
    err_one = vec_err(sol[key][:, 0], one[key])
    print("%s: %s within %.2e of the bound of the golden, %.2e of solvers.lp" % (name, key, err, err_one))
    assert err <= 1.0 and err_one <= 1.0
    for f in FLOATS:                                                  # None in solvers.lp's dictionary is NaN here, and nowhere else
        assert (one[f] is None) == bool(np.isnan(sol[f][0])), f
    for v in ("x", "s", "z"):
        assert (one[v] is None) == bool(np.isnan(sol[v][:, 0]).all()) == bool(np.isnan(sol[v][:, 0]).any()), v


def check_certificate(sol, k, c, G, h, A, b, label):
    """The certificate of member k recomputed in numpy from the returned vectors (coneprog.py:976-1024)."""
    x, y, s, z = (sol[v][:, k] for v in VECTORS)
    if sol["exit"][k] == 4:
        assert np.isnan(x).all() and np.isnan(s).all() and not np.isnan(y).any() and not np.isnan(z).any()
        assert abs(h @ z + b @ y + 1.0) <= 1e-12, (label, k, h @ z + b @ y)
        assert z.min() >= 0.0 and sol["dual slack"][k] == z.min() and np.isnan(sol["primal slack"][k])
        res = nrm(G.T @ z + A.T @ y) / max(1.0, nrm(c))
        assert res <= FEASTOL, (label, k, res)
        assert sol["dual objective"][k] == 1.0 and abs(sol[FLOATS[8]][k] - res) <= 1e-12
        assert all(np.isnan(sol[f][k]) for f in FLOATS if f not in ("dual objective", "dual slack", FLOATS[8]))
    else:
        assert np.isnan(y).all() and np.isnan(z).all() and not np.isnan(x).any() and not np.isnan(s).any()
        assert abs(c @ x + 1.0) <= 1e-12, (label, k, c @ x)
        assert s.min() >= 0.0 and sol["primal slack"][k] == s.min() and np.isnan(sol["dual slack"][k])
        res = max(nrm(A @ x) / max(1.0, nrm(b)), nrm(G @ x + s) / max(1.0, nrm(h)))
        assert res <= FEASTOL, (label, k, res)
        assert sol["primal objective"][k] == -1.0 and abs(sol[FLOATS[9]][k] - res) <= 1e-12
        assert all(np.isnan(sol[f][k]) for f in FLOATS if f not in ("primal objective", "primal slack", FLOATS[9]))


def check_against(sol, ref, M, label):
    """Statuses, iteration counts and exits equal the restatement's, vectors and objectives obey the rule, the NaN halves are where
    the restatement has them, certificates hold recomputed, and the stopping test recomputed in numpy from the returned x, y, s, z
    holds.  Recomputing moves the last bits of the sums: a residual entry is a sum of at most 600 products of size up to 1e2, so the
    infeasibilities get an absolute slack of 1e-12 and the gap a relative one."""
    worst = 0.0
    for k, r in enumerate(ref):
        got = (sol["status"][k], sol["iterations"][k], sol["exit"][k])
        assert got == (r.status, r.iterations, r.exit), (label, k, got, r.status, r.iterations, r.exit)
        errs = []
        for v in VECTORS:
            want = np.asarray(getattr(r, v), dtype=np.float64)
            assert np.array_equal(np.isnan(sol[v][:, k]), np.isnan(want)), (label, k, v)
            if not np.isnan(want).any():
                errs.append(vec_err(sol[v][:, k], want))
        c, G, h = M.c[:, k], M.G[k], M.h[:, k]
        A, b = (np.zeros((0, M.n)), np.zeros(0)) if M.A is None else (M.A[k], M.b[:, k])
        if r.status == "optimal":
            errs += [obj_err(sol["primal objective"][k], r.stats[2]), obj_err(sol["dual objective"][k], r.stats[3])]
            x, y, s, z = (sol[v][:, k] for v in VECTORS)
            rx, ry, rz = c + A.T @ y + G.T @ z, A @ x - b, s + G @ x - h
            pres = max(nrm(ry) / max(1.0, nrm(b)), nrm(rz) / max(1.0, nrm(h)))
            dres = nrm(rx) / max(1.0, nrm(c))
            gap, pcost, dcost = s @ z, c @ x, -b @ y - h @ z
            relgap = gap / -pcost if pcost < 0 else (gap / dcost if dcost > 0 else np.inf)
            assert pres <= FEASTOL + 1e-12 and dres <= FEASTOL + 1e-12, (label, k, pres, dres)
            assert gap <= 1e-7 * (1 + 1e-9) + 1e-12 or relgap <= 1e-6 * (1 + 1e-9), (label, k, gap, relgap)
            if r.iterations > 0:
                assert s.min() > 0 and z.min() > 0
            else:                                         # returned as computed with W = I: on the boundary is allowed
                assert s.min() >= 0 and z.min() >= 0
            assert sol["primal slack"][k] == s.min() and sol["dual slack"][k] == z.min()
            assert np.isnan(sol[FLOATS[8]][k]) and np.isnan(sol[FLOATS[9]][k])
        else:
            check_certificate(sol, k, c, G, h, A, b, label)
        worst = max(worst, *errs)
        assert max(errs) <= 1.0, (label, k, errs)
    return worst


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "n%d-ml%d-p%d" % s)
def test_shape_edges(shape):
    name = "shape-%d-%d-%d" % shape
    M = R.batch(name)
    sol = call(M)
    assert sol["x"].shape == (shape[0], R.SHAPE_B) and sol["y"].shape == (shape[2], R.SHAPE_B) and sol["s"].shape == sol["z"].shape == (shape[1], R.SHAPE_B)
    worst = check_against(sol, R.restated(name), M, name)
    print("%s: iterations %s, largest error %.2e of the bound" % (shape, sol["iterations"].tolist(), worst))
    assert list(sol["exit"]) == [0] * R.SHAPE_B and sol["status"] == ["optimal"] * R.SHAPE_B


@pytest.mark.parametrize("name", ["certificates-8-17-3", "certificates-33-65-5"])
def test_certificates(name):
    M = R.batch(name)
    sol = call(M)
    worst = check_against(sol, R.restated(name), M, name)
    print("%s: exits %s, iterations %s, largest error %.2e of the bound" % (name, sol["exit"].tolist(), sol["iterations"].tolist(), worst))
    assert list(sol["exit"]) == [0, 4, 5] * (M.B // 3)
    assert sol["status"] == ["optimal", "primal infeasible", "dual infeasible"] * (M.B // 3)


@pytest.mark.parametrize("name", ["free-8-17-3", "free-64-256-16"])
def test_free_variables_take_the_repair(name):
    M = R.batch(name)
    free = R.BATCHES[name][4]
    assert not M.G[:, :, M.n - free:].any() and all(r.singular for r in R.restated(name))
    sol = call(M)
    worst = check_against(sol, R.restated(name), M, name)
    print("%s: iterations %s, largest error %.2e of the bound" % (name, sol["iterations"].tolist(), worst))
    assert sol["status"] == ["optimal"] * M.B


def test_repaired_and_unrepaired_members_in_one_batch():
    F, N = R.batch("free-8-17-3"), R.batch("shape-8-17-3")
    pick = lambda a, b, cols: np.concatenate([a[:, :6], b[:, :6]], axis=1) if cols else np.concatenate([a[:6], b[:6]])    # noqa: E731
    c, G, h, A, b = pick(F.c, N.c, True), pick(F.G, N.G, False), pick(F.h, N.h, True), pick(F.A, N.A, False), pick(F.b, N.b, True)
    order = [0, 6, 1, 7, 2, 8, 3, 9, 4, 10, 5, 11]                     # repaired and unrepaired members take turns
    c, G, h, A, b = np.asfortranarray(c[:, order]), G[order], np.asfortranarray(h[:, order]), A[order], np.asfortranarray(b[:, order])
    sol = solvers.lp_batch(c, G, h, A, b)
    assert sol["status"] == ["optimal"] * 12
    ref = [(R.restated("free-8-17-3") if k < 6 else R.restated("shape-8-17-3"))[k % 6] for k in order]
    assert [r.singular for r in ref] == [True, False] * 6
    for k in range(12):
        assert sol["iterations"][k] == ref[k].iterations and vec_err(sol["x"][:, k], ref[k].x) <= 1.0, k
        solo = solvers.lp_batch(c[:, [k]], G[[k]], h[:, [k]], A[[k]], b[:, [k]])
        assert member_bytes(solo, 0) == member_bytes(sol, k), k


def test_shared_and_per_member_matrices_give_the_same_bytes():
    M = R.batch("shape-33-65-5")
    B = M.B
    shared = solvers.lp_batch(M.c, M.G[0], M.h[:, 0], M.A[0], M.b[:, 0])
    assert len(set(shared["x"][:, k].tobytes() for k in range(B))) == B and shared["status"][0] == "optimal"
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))         # noqa: E731
    col = lambda v: np.asfortranarray(np.tile(v.reshape(-1, 1), (1, B)))              # noqa: E731
    per = solvers.lp_batch(M.c, rep(M.G[0]), col(M.h[:, 0]), rep(M.A[0]), col(M.b[:, 0]))
    assert all_bytes(shared) == all_bytes(per)
    mixed = solvers.lp_batch(M.c, rep(M.G[0]), M.h[:, 0], M.A[0], col(M.b[:, 0]))
    assert all_bytes(shared) == all_bytes(mixed)
    print("shared matrices with the c of twelve members: exits %s" % shared["exit"].tolist())


def test_a_member_does_not_depend_on_its_batch():
    M = R.batch("independence")
    B = M.B
    sol = call(M)
    assert sol["status"] == ["optimal"] * B
    counts = sorted(set(int(v) for v in sol["iterations"]))
    print("B = %d at %s: iteration counts %s" % (B, R.BATCHES["independence"][0], counts))
    assert len(counts) >= 3
    for k in (0, 63, 64, 299):
        solo = call(M, which=[k])
        assert member_bytes(solo, 0) == member_bytes(sol, k), k
    assert all_bytes(call(M)) == all_bytes(sol)


def test_mixed_outcomes_in_one_batch():
    M = R.batch("mixed")
    B = M.B
    full = [r.iterations for r in R.restated("mixed")]
    maxiters = int(np.median(full))
    assert min(full) < maxiters <= max(full)            # a member that needs maxiters iterations ends "unknown" (coneprog.py:925-960)
    opts = {"maxiters": maxiters}
    ref = R.restate(M, opts, np.longdouble)
    c, G, A = M.c.copy(), M.G.copy(), M.A.copy()
    ZERO, NAN = R.MIXED_CHANGED
    G[ZERO, :, 3] = 0.0; A[ZERO, :, 3] = 0.0             # nothing holds x3: an exact zero pivot in G'G and in G'G + A'A
    c[1, NAN] = np.nan
    sol = call(M, opts, c=c, G=G, A=A)
    assert sol["exit"][ZERO] == 3 and sol["status"][ZERO] == "unknown" and sol["iterations"][ZERO] == 0
    assert all(not sol[v][:, ZERO].any() for v in VECTORS) and all(np.isnan(sol[f][ZERO]) for f in FLOATS)
    assert sol["exit"][NAN] in (1, 2, 3) and sol["status"][NAN] == "unknown"
    ended = []
    for k in range(B):
        if k in (ZERO, NAN):
            continue
        got = (sol["status"][k], sol["exit"][k], sol["iterations"][k])
        assert got == (ref[k].status, ref[k].exit, ref[k].iterations), (k, got)
        if got[1] == 1:
            assert got[2] == maxiters and np.isfinite(sol["gap"][k]) and sol["gap"][k] > 0
            assert vec_err(sol["x"][:, k], ref[k].x) <= 1.0
        elif got[1] == 0:
            assert vec_err(sol["x"][:, k], ref[k].x) <= 1.0
        else:
            check_certificate(sol, k, M.c[:, k], M.G[k], M.h[:, k], M.A[k], M.b[:, k], "mixed")
        ended.append(got[1])
        solo = call(M, opts, which=[k])
        assert member_bytes(solo, 0) == member_bytes(sol, k), k
    print("maxiters = %d of %s: exits %s, the NaN member exit %d" % (maxiters, full, sol["exit"].tolist(), sol["exit"][NAN]))
    assert set(ended) == {0, 1, 4, 5}
