"""solvers.conelp_batch on the device against the reference's own runs at refinement 0 (G28), against
solvers.conelp of this package, and against the numpy.longdouble restatement of tests/conelp_batch_numpy.py on generated members
whose cone has all three kinds: feasible ones at every edge of the kernel's tile sequence (the smallest member, no 'l' rows, a cone
across the first tile boundary with a block begun mid-tile, more cones than wavefronts, a cone of two wavefront passes beside an
order-16 block, 64 cones and 16 blocks, the LDS corner), primal and dual infeasible ones with their certificates recomputed in numpy,
members with one kind absent against lp_batch, socp_batch and sdp_batch, and members with free variables that need the A'A repair.
The rule of tests/test_lp_batch_gpu.py: vectors to 1e-6 max(|ref|, 1) in the 2-norm, objectives to 1e-7 max(|ref|, 1), statuses,
iteration counts and exits exactly.  tests/test_conelp_batch_cpu.py shows that float64 and longdouble agree on every member of these
batches.

Measured on an MI355X (this file's prints), largest error in units of the rule's bound: G28 cases 9.0e-5 (mixed_eq) against the
reference and 7.3e-2 against solvers.conelp; cone edges 2.1e-8 (2, 0, [1], [1], 0), 4.7e-2 (8, 0, [3, 4], [2, 3], 2), 1.8e-3
(16, 30, [5], [3], 2), 1.1e-3 (12, 3, [2] x 6, [1, 2, 3], 2), 1.2e-1 (20, 3, [65], [16], 3), 8.1e-1 (24, 0, [2] x 64, [3] x 16, 4) (an
objective; the vectors of that batch within 5.9e-3), 3.6e-6 at the LDS corner (64, 28, [100], [16], 64); one kind absent 3.8e-8 of
lp_batch, 0.0 of socp_batch, 0.0 of sdp_batch; certificates 1.3e-4; free variables 3.6e-3."""
import json
import os

import numpy as np
import pytest

import conelp_batch_numpy as R
import sdp_batch_numpy as SDN
import socp_batch_numpy as SON
from kvxopt_amd import _lib, solvers

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VECTORS = ("x", "y", "s", "z")
FLOATS = ("gap", "relative gap", "primal objective", "dual objective", "primal infeasibility", "dual infeasibility",
          "primal slack", "dual slack", "residual as primal infeasibility certificate", "residual as dual infeasibility certificate")
FEASTOL = 1e-7
nrm = np.linalg.norm


def call(M, options=None, which=None, **replace):
    """conelp_batch on the members `which` (all of them by default) of a batch from conelp_batch_numpy.members."""
    w = slice(None) if which is None else list(which)
    args = {"c": M.c, "G": M.G, "h": M.h, "A": M.A, "b": M.b}
    args.update(replace)
    cut = lambda v, cols: None if v is None else (v[:, w] if cols else v[w])          # noqa: E731
    return solvers.conelp_batch(cut(args["c"], True), cut(args["G"], False), cut(args["h"], True), M.dims, cut(args["A"], False),
                                cut(args["b"], True), options=options)


def vec_err(got, ref):
    """|got - ref| in units of the rule's bound 1e-6 max(|ref|, 1): passes when <= 1."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(nrm(got - ref) / (1e-6 * max(nrm(ref), 1.0)))


def obj_err(got, ref):
    return abs(got - float(ref)) / (1e-7 * max(abs(float(ref)), 1.0))


def cone_slack(u, dims):
    """-max_step(u) (misc_solvers.c:1052-1160) by numpy: the smallest 'l' entry, u_0 - |u_1| of every cone, the smallest eigenvalue
    of every block by numpy.linalg.eigvalsh.  Positive inside the cone."""
    ml, t = dims["l"], []
    if ml:
        t.append(u[:ml].min())
    off = SON.offsets(ml, dims["q"])
    for o, e in zip(off[:-1], off[1:]):
        t.append(u[o] - nrm(u[o + 1:e]))
    for _, o, _, m in SDN.blocks(off[-1], dims["s"]):
        X = SDN.mat(u, o, m)
        assert np.array_equal(X, X.T)                    # the blocks are returned as full symmetric matrices, to the bit
        t.append(np.linalg.eigvalsh(X).min())
    return min(t)


def same_slack(got, u, dims):
    """The kernel's smallest eigenvalue is a singular value of x + 1.5 |x|_F I less the shift: its error is a few m eps |x|_F, with
    m <= 16 below 1e-13 |x|_F; eigvalsh's is of the same kind, and |u_1| of a cone is a sum of at most 384 squares."""
    want = cone_slack(u, dims)
    return abs(got - want) <= 1e-12 * max(1.0, nrm(u))


def member_bytes(sol, k):
    return b"".join([np.ascontiguousarray(sol[v][:, k]).tobytes() for v in VECTORS] + [np.float64(sol[f][k]).tobytes() for f in FLOATS]
                    + [np.int64(sol["iterations"][k]).tobytes(), np.int64(sol["exit"][k]).tobytes(), sol["status"][k].encode()])


def all_bytes(sol):
    return b"".join(member_bytes(sol, k) for k in range(len(sol["status"])))


def g28(name):
    meta = json.load(open(os.path.join(GOLDEN, "g28_conelp_batch.json")))["cases"][name]
    g = np.load(os.path.join(GOLDEN, "g28_conelp_batch.npz"))
    get = lambda k: g["%s__%s" % (name, k)] if "%s__%s" % (name, k) in g else None         # noqa: E731
    return meta, get


def g28_batch(name):
    """The golden case as member 0 of a batch of 3 with shared matrices, h and b as one column, and perturbed c."""
    meta, get = g28(name)
    c = get("c")
    rng = np.random.default_rng(5)
    C3 = np.asfortranarray(np.stack([c, c * (1.0 + 0.01 * rng.standard_normal(c.size)), c * (1.0 + 0.01 * rng.standard_normal(c.size))], axis=1))
    return solvers.conelp_batch(C3, get("G"), get("h"), meta["dims"], get("A"), get("b"))


@pytest.mark.parametrize("name", ["doc_conelp", "doc_conelp_lower", "mixed_eq", "conelp_pinf", "conelp_dinf"])
def test_golden_member_of_a_batch(name):
    meta, get = g28(name)
    sol = g28_batch(name)
    status = meta["status"]
    assert sol["status"][0] == status and sol["iterations"][0] == meta["iterations"] and sol["exit"][0] == R.EXITS[status]
    one = solvers.conelp(get("c"), get("G"), get("h"), meta["dims"], get("A"), get("b"), options=dict(R.QUIET, refinement=0))
    assert one["status"] == status and one["iterations"] == sol["iterations"][0]
    errs = {}
    for k in VECTORS:
        want = get("sol_" + k)
        if want is None or not want.size:
            assert np.isnan(sol[k][:, 0]).all() or not sol[k].shape[0]
            assert one[k] is None or not np.asarray(one[k]).size
            continue
        errs[k] = vec_err(sol[k][:, 0], want)
        errs[k + " vs solvers.conelp"] = vec_err(sol[k][:, 0], np.asarray(one[k]).reshape(-1))
    for k in ("primal objective", "dual objective"):
        if meta[k] is not None:
            errs[k] = obj_err(sol[k][0], meta[k])
            errs[k + " vs solvers.conelp"] = obj_err(sol[k][0], one[k])
    print("%s: errors in units of the bound: %s" % (name, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) <= 1.0
    for f in FLOATS:                                                  # None in solvers.conelp's dictionary is NaN here, and nowhere else
        assert (one[f] is None) == bool(np.isnan(sol[f][0])), f


def test_the_upper_triangles_are_not_read():
    assert all_bytes(g28_batch("doc_conelp")) == all_bytes(g28_batch("doc_conelp_lower"))


def check_certificate(sol, k, c, G, h, A, b, dims, label):
    """The certificate of member k recomputed in numpy from the returned vectors (coneprog.py:976-1024)."""
    x, y, s, z = (sol[v][:, k] for v in VECTORS)
    if sol["exit"][k] == 4:
        assert np.isnan(x).all() and np.isnan(s).all() and not np.isnan(y).any() and not np.isnan(z).any()
        assert abs(h @ z + b @ y + 1.0) <= 1e-12, (label, k, h @ z + b @ y)
        assert cone_slack(z, dims) >= 0.0 and same_slack(sol["dual slack"][k], z, dims) and np.isnan(sol["primal slack"][k])
        res = nrm(G.T @ z + A.T @ y) / max(1.0, nrm(c))
        assert res <= FEASTOL, (label, k, res)
        assert sol["dual objective"][k] == 1.0 and abs(sol[FLOATS[8]][k] - res) <= 1e-12
        assert all(np.isnan(sol[f][k]) for f in FLOATS if f not in ("dual objective", "dual slack", FLOATS[8]))
    else:
        assert np.isnan(y).all() and np.isnan(z).all() and not np.isnan(x).any() and not np.isnan(s).any()
        assert abs(c @ x + 1.0) <= 1e-12, (label, k, c @ x)
        assert cone_slack(s, dims) >= 0.0 and same_slack(sol["primal slack"][k], s, dims) and np.isnan(sol["dual slack"][k])
        res = max(nrm(A @ x) / max(1.0, nrm(b)), nrm(G @ x + s) / max(1.0, nrm(h)))
        assert res <= FEASTOL, (label, k, res)
        assert sol["primal objective"][k] == -1.0 and abs(sol[FLOATS[9]][k] - res) <= 1e-12
        assert all(np.isnan(sol[f][k]) for f in FLOATS if f not in ("primal objective", "primal slack", FLOATS[9]))


def check_against(sol, ref, M, label):
    """Statuses, iteration counts and exits equal the restatement's, vectors and objectives obey the rule, the NaN halves are where
    the restatement has them, certificates hold recomputed, and the stopping inequalities and the membership of s and z in each kind
    of cone hold recomputed in numpy from the returned x, y, s, z (the generated G and h have symmetric blocks and s, z come back as
    full symmetric matrices, so plain products are the cone's).  Recomputing moves the last bits of the sums: a residual entry is a
    sum of at most 450 products of size up to 1e2, so the infeasibilities get an absolute slack of 1e-12 and the gap a relative one."""
    worst = 0.0
    for k, r in enumerate(ref):
        got = (sol["status"][k], sol["iterations"][k], sol["exit"][k])
        assert got == (r.status, r.iterations, r.exit), (label, k, got, r.status, r.iterations, r.exit)
        errs = []
        for v in VECTORS:
            want = np.asarray(getattr(r, v), dtype=np.float64)
            assert np.array_equal(np.isnan(sol[v][:, k]), np.isnan(want)), (label, k, v)
            if want.size and not np.isnan(want).any():
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
                assert cone_slack(s, M.dims) > 0 and cone_slack(z, M.dims) > 0
            else:                                         # returned as computed with W = I: on the boundary is allowed, to rounding
                assert cone_slack(s, M.dims) >= -1e-12 * max(1.0, nrm(s)) and cone_slack(z, M.dims) >= -1e-12 * max(1.0, nrm(z))
            assert same_slack(sol["primal slack"][k], s, M.dims) and same_slack(sol["dual slack"][k], z, M.dims)
            assert np.isnan(sol[FLOATS[8]][k]) and np.isnan(sol[FLOATS[9]][k])
        else:
            check_certificate(sol, k, c, G, h, A, b, M.dims, label)
        worst = max(worst, *errs)
        assert max(errs) <= 1.0, (label, k, errs)
    return worst


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_name)
def test_cone_edges(shape):
    name = R.shape_name(shape)
    M = R.batch(name)
    sol = call(M)
    n, ml, q, s, p = shape
    N = ml + sum(q) + sum(m * m for m in s)
    assert sol["x"].shape == (n, R.SHAPE_B) and sol["y"].shape == (p, R.SHAPE_B) and sol["s"].shape == sol["z"].shape == (N, R.SHAPE_B)
    worst = check_against(sol, R.restated(name), M, name)
    print("%s: iterations %s, largest error %.2e of the bound" % (name, sol["iterations"].tolist(), worst))
    assert list(sol["exit"]) == [0] * R.SHAPE_B and sol["status"] == ["optimal"] * R.SHAPE_B


def agrees_with(sol, other, M, label):
    assert sol["status"] == other["status"] and list(sol["iterations"]) == list(other["iterations"]) and list(sol["exit"]) == list(other["exit"])
    both = max(vec_err(sol[v][:, k], other[v][:, k]) for v in VECTORS for k in range(M.B))
    assert both <= 1.0, (label, both)
    return both


def test_without_cones_and_blocks_agrees_with_lp_batch():
    M = R.batch("absent-qs")
    assert M.dims == {"l": 17, "q": [], "s": []}
    sol = call(M)
    worst = check_against(sol, R.restated("absent-qs"), M, "absent-qs")
    both = agrees_with(sol, solvers.lp_batch(M.c, M.G, M.h, M.A, M.b), M, "lp_batch")
    print("absent-qs: iterations %s, largest error %.2e of the bound of the restatement, %.2e of lp_batch" % (sol["iterations"].tolist(), worst, both))


def test_without_blocks_agrees_with_socp_batch():
    M = R.batch("absent-s")
    assert M.dims == {"l": 5, "q": [1, 2, 7], "s": []}
    sol = call(M)
    worst = check_against(sol, R.restated("absent-s"), M, "absent-s")
    both = agrees_with(sol, solvers.socp_batch(M.c, M.G, M.h, M.dims, M.A, M.b), M, "socp_batch")
    print("absent-s: iterations %s, largest error %.2e of the bound of the restatement, %.2e of socp_batch" % (sol["iterations"].tolist(), worst, both))


def test_without_cones_agrees_with_sdp_batch():
    M = R.batch("absent-q")
    assert M.dims == {"l": 2, "q": [], "s": [1, 2, 3]}
    sol = call(M)
    worst = check_against(sol, R.restated("absent-q"), M, "absent-q")
    both = agrees_with(sol, solvers.sdp_batch(M.c, M.G, M.h, M.dims, M.A, M.b), M, "sdp_batch")
    print("absent-q: iterations %s, largest error %.2e of the bound of the restatement, %.2e of sdp_batch" % (sol["iterations"].tolist(), worst, both))


def test_certificates():
    M = R.batch("certificates")
    assert M.dims == {"l": 3, "q": [4], "s": [3]} and (M.n, M.p) == (8, 2)
    sol = call(M)
    worst = check_against(sol, R.restated("certificates"), M, "certificates")
    print("certificates: exits %s, iterations %s, largest error %.2e of the bound" % (sol["exit"].tolist(), sol["iterations"].tolist(), worst))
    assert list(sol["exit"]) == [0, 4, 5] * 4
    assert sol["status"] == ["optimal", "primal infeasible", "dual infeasible"] * 4


def test_free_variables_take_the_repair():
    M = R.batch("free")
    free = R.BATCHES["free"][4]
    assert free == 2 and not M.G[:, :, M.n - free:].any() and all(r.singular for r in R.restated("free"))
    sol = call(M)
    worst = check_against(sol, R.restated("free"), M, "free")
    print("free: iterations %s, largest error %.2e of the bound" % (sol["iterations"].tolist(), worst))
    assert sol["status"] == ["optimal"] * M.B


def test_repaired_and_unrepaired_members_in_one_batch():
    F, N = R.batch("free"), R.batch("certificates")
    un = [0, 3, 6, 9, 0, 3]                                            # the feasible members of "certificates", unrepaired
    pick = lambda a, b, cols: np.concatenate([a[:, :6], b[:, un]], axis=1) if cols else np.concatenate([a[:6], b[un]])    # noqa: E731
    c, G, h, A, b = pick(F.c, N.c, True), pick(F.G, N.G, False), pick(F.h, N.h, True), pick(F.A, N.A, False), pick(F.b, N.b, True)
    order = [0, 6, 1, 7, 2, 8, 3, 9, 4, 10, 5, 11]                     # repaired and unrepaired members take turns
    c, G, h, A, b = np.asfortranarray(c[:, order]), G[order], np.asfortranarray(h[:, order]), A[order], np.asfortranarray(b[:, order])
    sol = solvers.conelp_batch(c, G, h, F.dims, A, b)
    assert sol["status"] == ["optimal"] * 12
    ref = [R.restated("free")[k] if k < 6 else R.restated("certificates")[un[k - 6]] for k in order]
    assert [r.singular for r in ref] == [True, False] * 6
    for k in range(12):
        assert sol["iterations"][k] == ref[k].iterations and vec_err(sol["x"][:, k], ref[k].x) <= 1.0, k
        solo = solvers.conelp_batch(c[:, [k]], G[[k]], h[:, [k]], F.dims, A[[k]], b[:, [k]])
        assert member_bytes(solo, 0) == member_bytes(sol, k), k


def test_shared_and_per_member_matrices_give_the_same_bytes():
    M = R.batch("certificates")
    B = M.B
    shared = solvers.conelp_batch(M.c, M.G[0], M.h[:, 0], M.dims, M.A[0], M.b[:, 0])
    assert len(set(shared["x"][:, k].tobytes() for k in range(B))) >= 2 and shared["status"][0] == "optimal"
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))         # noqa: E731
    col = lambda v: np.asfortranarray(np.tile(v.reshape(-1, 1), (1, B)))              # noqa: E731
    per = solvers.conelp_batch(M.c, rep(M.G[0]), col(M.h[:, 0]), M.dims, rep(M.A[0]), col(M.b[:, 0]))
    assert all_bytes(shared) == all_bytes(per)
    mixed = solvers.conelp_batch(M.c, rep(M.G[0]), M.h[:, 0], M.dims, M.A[0], col(M.b[:, 0]))
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
    c, G, h, A = M.c.copy(), M.G.copy(), M.h.copy(), M.A.copy()
    HUGE, ZERO, NAN = R.MIXED_CHANGED
    # the block of order 3 of h, indefinite and so large that its Frobenius norm overflows: the block is not iterated on, the push
    # into the cone comes from the other rows alone, and the Cholesky factor of s_k in the first scaling meets a negative pivot
    o = SDN.blocks(M.Ms, M.s)[0][1]
    h[o:o + 9, HUGE] = 1e200 * np.diag([1.0, -1.0, 1.0]).reshape(-1)
    G[ZERO, :, 3] = 0.0; A[ZERO, :, 3] = 0.0             # nothing holds x3: an exact zero pivot in Gs'Gs and in Gs'Gs + A'A
    c[1, NAN] = np.nan                                   # z of the starting point is NaN, and so is the pivot of every z_k
    sol = call(M, opts, c=c, G=G, h=h, A=A)
    for k in (HUGE, ZERO, NAN):
        assert sol["exit"][k] == 3 and sol["status"][k] == "unknown" and sol["iterations"][k] == 0, (k, sol["exit"][k])
        assert all(not sol[v][:, k].any() for v in VECTORS) and all(np.isnan(sol[f][k]) for f in FLOATS)
    ended = []
    for k in range(B):
        if k in (HUGE, ZERO, NAN):
            continue
        got = (sol["status"][k], sol["exit"][k], sol["iterations"][k])
        assert got == (ref[k].status, ref[k].exit, ref[k].iterations), (k, got)
        if got[1] == 1:
            assert got[2] == maxiters and np.isfinite(sol["gap"][k]) and sol["gap"][k] > 0
            assert vec_err(sol["x"][:, k], ref[k].x) <= 1.0
        elif got[1] == 0:
            assert vec_err(sol["x"][:, k], ref[k].x) <= 1.0
        else:
            check_certificate(sol, k, M.c[:, k], M.G[k], M.h[:, k], M.A[k], M.b[:, k], M.dims, "mixed")
        ended.append(got[1])
        solo = call(M, opts, which=[k])
        assert member_bytes(solo, 0) == member_bytes(sol, k), k
    print("maxiters = %d of %s: exits %s" % (maxiters, full, sol["exit"].tolist()))
    assert set(ended) == {0, 1, 4, 5} and set(sol["exit"].tolist()) == {0, 1, 3, 4, 5}


def test_the_dev_entry_on_resident_buffers_returns_the_bytes_of_the_host_entry():
    """kvx_conelp_batch_solve_dev takes no workspace: the kernel stages the scaled rows of G in LDS."""
    M = R.batch("certificates")
    host = call(M)
    B, n, N, p = M.B, M.n, M.N, M.p
    up = _lib.DeviceBuffer.from_array
    data = [up(np.ascontiguousarray(M.c.T)), up(M.G.transpose(0, 2, 1)), up(np.ascontiguousarray(M.h.T)), up(M.A.transpose(0, 2, 1)),
            up(np.ascontiguousarray(M.b.T))]
    outs = [_lib.DeviceBuffer(8 * k * B) for k in (n, p, N, N, len(FLOATS), 1, 1)]
    qv, mv = np.asarray(M.q, dtype=np.int64), np.asarray(M.s, dtype=np.int64)
    args = [B, n, M.ml, len(M.q), _lib.pi(qv), len(M.s), _lib.pi(mv), p]
    for buf, stride in zip(data, (n, N * n, N, p * n, p)):
        args += [buf.ptr, stride]
    args += [100, 1e-7, 1e-6, 1e-7] + [o.ptr for o in outs]
    _lib.raise_for(_lib.lib().kvx_conelp_batch_solve_dev(*args), "kvx_conelp_batch_solve_dev")
    for key, buf, rows in zip(VECTORS, outs, (n, p, N, N)):
        assert buf.download(np.float64, rows * B).tobytes() == np.ascontiguousarray(host[key].T).tobytes(), key
    stats = outs[4].download(np.float64, len(FLOATS) * B).reshape(B, len(FLOATS))
    assert stats.tobytes() == np.ascontiguousarray(np.stack([host[f] for f in FLOATS], axis=1)).tobytes()
    assert outs[5].download(np.int64, B).tolist() == host["iterations"].tolist() and outs[6].download(np.int64, B).tolist() == host["exit"].tolist()
    for buf in data + outs:
        buf.free()
