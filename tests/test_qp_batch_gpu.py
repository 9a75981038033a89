"""solvers.qp_batch on the device against the reference's own runs (G5 qp6x5, G9 qpeq6x5p4), against
solvers.qp of this package, and against the numpy.longdouble restatement of tests/qp_batch_numpy.py on generated members at
every shape edge of the kernel: n = 1, n not a multiple of anything, n = 63 / 64, ml = 255 / 256 / 257 around the 256 threads and
the 32-row steps of the assembly, ml = 512, p = 0 / 1 / 16 / n.  The rule of test_coneqp_matches_g21: vectors to
1e-6 max(|ref|, 1) in the 2-norm, objectives to 1e-7 max(|ref|, 1).  tests/test_qp_batch_cpu.py shows that no expected iteration
count of these batches sits on a rounding edge."""
import json
import os

import numpy as np
import pytest

import qp_batch_numpy as R
from kvxopt_amd import solvers

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VECTORS = ("x", "y", "s", "z")
FLOATS = ("gap", "relative gap", "primal objective", "dual objective", "primal infeasibility", "dual infeasibility",
          "primal slack", "dual slack")


def call(M, options=None, which=None, **replace):
    """qp_batch on the members `which` (all of them by default) of a batch from qp_batch_numpy.members."""
    w = slice(None) if which is None else list(which)
    args = {"P": M.P[w], "q": M.q[:, w], "G": M.G[w], "h": M.h[:, w], "A": None if M.A is None else M.A[w],
            "b": None if M.b is None else M.b[:, w]}
    args.update(replace)
    return solvers.qp_batch(args["P"], args["q"], args["G"], args["h"], args["A"], args["b"], options=options)


def vec_err(got, ref):
    """|got - ref| in units of the rule's bound 1e-6 max(|ref|, 1): passes when <= 1."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(got - ref) / (1e-6 * max(np.linalg.norm(ref), 1.0)))


def obj_err(got, ref):
    return abs(got - float(ref)) / (1e-7 * max(abs(float(ref)), 1.0))


def member_bytes(sol, k):
    return b"".join([np.ascontiguousarray(sol[v][:, k]).tobytes() for v in VECTORS] + [np.float64(sol[f][k]).tobytes() for f in FLOATS]
                    + [np.int64(sol["iterations"][k]).tobytes(), np.int64(sol["exit"][k]).tobytes(), sol["status"][k].encode()])


def all_bytes(sol):
    return b"".join(member_bytes(sol, k) for k in range(len(sol["status"])))


@pytest.mark.parametrize("name,gfile,p", [("qp6x5", "g5_coneqp", 0), ("qpeq6x5p4", "g9_coneqp_eq", 4)])
def test_golden_member_of_a_batch(name, gfile, p):
    meta = json.load(open(os.path.join(GOLDEN, gfile + ".json")))["cases"][name]
    g = np.load(os.path.join(GOLDEN, gfile + ".npz"))
    P, q, G, h, A, b = R.grid_dense(p)
    rng = np.random.default_rng(5)
    Q3 = np.asfortranarray(np.stack([q, q * (1.0 + 0.01 * rng.standard_normal(q.size)), q * (1.0 + 0.01 * rng.standard_normal(q.size))], axis=1))
    sol = solvers.qp_batch(P, Q3, G, h, A, b)                        # shared matrices, h and b as one column
    assert sol["status"] == ["optimal"] * 3 and list(sol["exit"]) == [0, 0, 0]
    assert sol["status"][0] == meta["status"] and sol["iterations"][0] == meta["iterations"]
    one = solvers.qp(P, q, G, h, A, b, options=R.QUIET)               # this package's one-problem driver on the same data
    assert one["status"] == "optimal" and one["iterations"] == sol["iterations"][0]
    errs = {}
    for k in VECTORS[:1] + (VECTORS[1:2] if p else ()) + VECTORS[2:]:
        errs[k] = vec_err(sol[k][:, 0], g[name + "_" + k])
        errs[k + " vs solvers.qp"] = vec_err(sol[k][:, 0], one[k])
    for k in ("primal objective", "dual objective"):
        errs[k] = obj_err(sol[k][0], meta[k])
        errs[k + " vs solvers.qp"] = obj_err(sol[k][0], one[k])
    print("%s: errors in units of the bound: %s" % (name, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) <= 1.0
    assert len(set(Q3[:, k].tobytes() for k in range(3))) == 3 and not np.array_equal(sol["x"][:, 0], sol["x"][:, 1])


def check_against(sol, ref, M, label):
    """Statuses and iteration counts equal the restatement's, vectors and objectives obey the rule, and the stopping test
    recomputed in numpy from the returned x, y, s, z holds.  Recomputing moves the last bits of the sums: a residual entry is a sum
    of at most 600 products of size up to 1e2, so the infeasibilities get an absolute slack of 1e-12 and the gap a relative one."""
    worst = 0.0
    for k, r in enumerate(ref):
        assert sol["status"][k] == r.status and sol["iterations"][k] == r.iterations, (label, k, sol["status"][k], sol["iterations"][k], r.status, r.iterations)
        errs = [vec_err(sol[v][:, k], getattr(r, v)) for v in VECTORS]
        errs += [obj_err(sol["primal objective"][k], r.stats[2]), obj_err(sol["dual objective"][k], r.stats[3])]
        worst = max(worst, *errs)
        assert max(errs) <= 1.0, (label, k, errs)
        if r.status == "optimal":
            x, y, s, z = (sol[v][:, k] for v in VECTORS)
            P = np.tril(M.P[k]) + np.tril(M.P[k], -1).T
            q, G, h = M.q[:, k], M.G[k], M.h[:, k]
            A, b = (np.zeros((0, M.n)), np.zeros(0)) if M.A is None else (M.A[k], M.b[:, k])
            rx, ry, rz = P @ x + q + A.T @ y + G.T @ z, A @ x - b, s + G @ x - h
            nrm = np.linalg.norm
            pres = max(nrm(ry) / max(1.0, nrm(b)), nrm(rz) / max(1.0, nrm(h)))
            dres = nrm(rx) / max(1.0, nrm(q))
            gap, pcost = s @ z, 0.5 * x @ (P @ x) + q @ x
            dcost = pcost + y @ ry + z @ rz - gap
            relgap = gap / -pcost if pcost < 0 else (gap / dcost if dcost > 0 else np.inf)
            assert pres <= 1e-7 + 1e-12 and dres <= 1e-7 + 1e-12, (label, k, pres, dres)
            assert gap <= 1e-7 * (1 + 1e-9) or relgap <= 1e-6 * (1 + 1e-9), (label, k, gap, relgap)
            assert s.min() > 0 and z.min() > 0
            assert sol["primal slack"][k] == s.min() and sol["dual slack"][k] == z.min()
    return worst


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "n%d-ml%d-p%d" % s)
def test_shape_edges(shape):
    M = R.batch(shape)
    sol = call(M)
    assert sol["x"].shape == (shape[0], R.SHAPE_B) and sol["y"].shape == (shape[2], R.SHAPE_B) and sol["s"].shape == sol["z"].shape == (shape[1], R.SHAPE_B)
    worst = check_against(sol, R.restated(shape), M, str(shape))
    print("%s: iterations %s, largest error %.2e of the bound" % (shape, sol["iterations"].tolist(), worst))
    assert list(sol["exit"]) == [0] * R.SHAPE_B and sol["status"] == ["optimal"] * R.SHAPE_B


def test_shared_and_per_member_matrices_give_the_same_bytes():
    M = R.batch((33, 65, 5))
    B = M.B
    shared = solvers.qp_batch(M.P[0], M.q, M.G[0], M.h[:, 0], M.A[0], M.b[:, 0])
    assert shared["status"] == ["optimal"] * B and len(set(shared["x"][:, k].tobytes() for k in range(B))) == B
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))         # noqa: E731
    col = lambda v: np.asfortranarray(np.tile(v.reshape(-1, 1), (1, B)))              # noqa: E731
    per = solvers.qp_batch(rep(M.P[0]), M.q, rep(M.G[0]), col(M.h[:, 0]), rep(M.A[0]), col(M.b[:, 0]))
    assert all_bytes(shared) == all_bytes(per)
    mixed = solvers.qp_batch(M.P[0], M.q, rep(M.G[0]), M.h[:, 0], M.A[0], col(M.b[:, 0]))
    assert all_bytes(shared) == all_bytes(mixed)


def test_a_member_does_not_depend_on_its_batch():
    shape, B, seed = R.INDEPENDENCE
    M = R.batch(shape, B, seed)
    sol = call(M)
    assert sol["status"] == ["optimal"] * B
    counts = sorted(set(int(v) for v in sol["iterations"]))
    print("B = %d at %s: iteration counts %s" % (B, shape, counts))
    assert len(counts) >= 3
    for k in (0, 63, 64, 299):
        solo = call(M, which=[k])
        assert member_bytes(solo, 0) == member_bytes(sol, k), k
    assert all_bytes(call(M)) == all_bytes(sol)


def test_mixed_outcomes_in_one_batch():
    shape, B, seed = R.MIXED
    M = R.batch(shape, B, seed)
    ref = R.restated(shape, B, seed)
    full = [r.iterations for r in ref]
    maxiters = int(np.median(full))
    assert min(full) < maxiters <= max(full)            # a member that needs maxiters iterations ends "unknown" (coneprog.py:2210-2224)
    P, G, q = M.P.copy(), M.G.copy(), M.q.copy()
    ZERO, NAN = 2, 5
    P[ZERO, :, 3] = 0.0; P[ZERO, 3, :] = 0.0; G[ZERO, :, 3] = 0.0       # an exact zero pivot in S = P + G'G
    q[1, NAN] = np.nan
    opts = {"maxiters": maxiters}
    sol = call(M, opts, P=P, G=G, q=q)
    assert sol["exit"][ZERO] == 3 and sol["status"][ZERO] == "unknown" and sol["iterations"][ZERO] == 0
    assert all(not sol[v][:, ZERO].any() for v in VECTORS)
    assert sol["exit"][NAN] in (1, 2, 3) and sol["status"][NAN] == "unknown"
    ended = []
    for k in range(B):
        if k in (ZERO, NAN):
            continue
        if full[k] < maxiters:
            assert (sol["status"][k], sol["exit"][k], sol["iterations"][k]) == ("optimal", 0, full[k]), k
            assert vec_err(sol["x"][:, k], ref[k].x) <= 1.0
        else:
            assert (sol["status"][k], sol["exit"][k], sol["iterations"][k]) == ("unknown", 1, maxiters), k
            assert np.isfinite(sol["gap"][k]) and sol["gap"][k] > 0
        ended.append(sol["exit"][k])
        solo = call(M, opts, which=[k])
        assert member_bytes(solo, 0) == member_bytes(sol, k), k
    print("maxiters = %d of %s: exits %s, the NaN member exit %d" % (maxiters, full, sol["exit"].tolist(), sol["exit"][NAN]))
    assert 0 in ended and 1 in ended


def test_without_correction():
    shape = (8, 17, 3)
    M = R.batch(shape)
    sol = call(M, {"use_correction": False})
    assert sol["status"] == ["optimal"] * M.B
    worst = check_against(sol, R.restated(shape, correction=False), M, "use_correction False")
    with_correction = [r.iterations for r in R.restated(shape)]
    print("use_correction False: iterations %s (with: %s), largest error %.2e of the bound" % (sol["iterations"].tolist(), with_correction, worst))
    assert list(sol["iterations"]) != with_correction
