"""solvers.coneqp_batch on the device against the reference's own runs at refinement 0 (G29), against
solvers.coneqp of this package, against solvers.qp_batch on the orthant, and against the numpy.longdouble restatement of
tests/coneqp_batch_numpy.py on generated members whose cone has all three kinds: feasible ones at every edge of the kernel's tile
sequence (the shapes of tests/conelp_batch_numpy.py: the smallest member, no 'l' rows, a cone across the first tile boundary with a
block begun mid-tile, more cones than wavefronts, a cone of two wavefront passes beside an order-16 block, 64 cones and 16 blocks,
the LDS corner), P = 0, a P of rank n - 2, a coordinate nothing holds, both settings of use_correction and a run cut at maxiters.
The rule of tests/test_lp_batch_gpu.py: vectors to 1e-6 max(|ref|, 1) in the 2-norm, objectives to 1e-7 max(|ref|, 1), statuses,
iteration counts and exits exactly.  tests/test_coneqp_batch_cpu.py shows that float64 and longdouble agree on every member of these
batches.

Measured on an MI355X (this file's prints), largest error in units of the rule's bound: G29 cases 2.3e-5 (p_rank_deficient) against the
reference and 2.5e-2 (mixed_eq, z) against solvers.coneqp; cone edges 4.7e-8 (2, 0, [1], [1], 0), 5.4e-6 (8, 0, [3, 4], [2, 3], 2), 1.9e-6
(16, 30, [5], [3], 2), 1.7e-6 (12, 3, [2] x 6, [1, 2, 3], 2), 4.0e-6 (20, 3, [65], [16], 3), 1.0e-5 (24, 0, [2] x 64, [3] x 16, 4), 3.0e-7 at
the LDS corner (64, 28, [100], [16], 64); orthant only 5.2e-6 of qp_batch; P = 0 3.6e-5; P of rank n - 2 2.5e-5; without the
correction 2.4e-5, with it 2.3e-6; maxiters = 3 2.2e-7."""
import json
import os

import numpy as np
import pytest

import coneqp_batch_numpy as R
import qp_batch_numpy as QBN
import sdp_batch_numpy as SDN
import socp_batch_numpy as SON
from kvxopt_amd import _lib, solvers

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VECTORS = ("x", "y", "s", "z")
FLOATS = ("gap", "relative gap", "primal objective", "dual objective", "primal infeasibility", "dual infeasibility",
          "primal slack", "dual slack")
FEASTOL = 1e-7
nrm = np.linalg.norm


def call(M, options=None, which=None, **replace):
    """coneqp_batch on the members `which` (all of them by default) of a batch from coneqp_batch_numpy.members."""
    w = slice(None) if which is None else list(which)
    args = {"P": M.P, "q": M.q, "G": M.G, "h": M.h, "A": M.A, "b": M.b}
    args.update(replace)
    cut = lambda v, cols: None if v is None else (v[:, w] if cols else v[w])          # noqa: E731
    return solvers.coneqp_batch(cut(args["P"], False), cut(args["q"], True), cut(args["G"], False), cut(args["h"], True), M.dims,
                                cut(args["A"], False), cut(args["b"], True), options=options)


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


def failed(sol, k):
    """Member k ended with exit 3: zeros, 0 iterations, NaN statistics."""
    return (sol["exit"][k] == 3 and sol["status"][k] == "unknown" and sol["iterations"][k] == 0
            and all(not sol[v][:, k].any() for v in VECTORS) and all(np.isnan(sol[f][k]) for f in FLOATS))


def g29(name):
    meta = json.load(open(os.path.join(GOLDEN, "g29_coneqp_batch.json")))["cases"][name]
    g = np.load(os.path.join(GOLDEN, "g29_coneqp_batch.npz"))
    get = lambda k: g["%s__%s" % (name, k)] if "%s__%s" % (name, k) in g else None         # noqa: E731
    return meta, get


def g29_batch(name):
    """The golden case as member 0 of a batch of 3 with shared matrices, h and b as one column, and perturbed q."""
    meta, get = g29(name)
    q = get("q")
    rng = np.random.default_rng(5)
    Q3 = np.asfortranarray(np.stack([q, q * (1.0 + 0.01 * rng.standard_normal(q.size)), q * (1.0 + 0.01 * rng.standard_normal(q.size))], axis=1))
    return solvers.coneqp_batch(get("P"), Q3, get("G"), get("h"), meta["dims"], get("A"), get("b"), options=meta["options"])


@pytest.mark.parametrize("name", ["doc_coneqp", "doc_coneqp_garbage", "mixed_eq", "mixed_eq_garbage", "p_rank_deficient", "mixed_eq_cut"])
def test_golden_member_of_a_batch(name):
    meta, get = g29(name)
    sol = g29_batch(name)
    status = meta["status"]
    assert sol["status"][0] == status and sol["iterations"][0] == meta["iterations"] and sol["exit"][0] == (0 if status == "optimal" else 1)
    one = solvers.coneqp(get("P"), get("q"), get("G"), get("h"), meta["dims"], get("A"), get("b"),
                         options=dict(R.QUIET, refinement=0, **meta["options"]))
    assert one["status"] == status and one["iterations"] == sol["iterations"][0]
    errs = {}
    for k in VECTORS:
        want = get("sol_" + k)
        if not want.size:
            assert not sol[k].shape[0]
            continue
        errs[k] = vec_err(sol[k][:, 0], want)
        errs[k + " vs solvers.coneqp"] = vec_err(sol[k][:, 0], np.asarray(one[k]).reshape(-1))
    for k in ("primal objective", "dual objective"):
        errs[k] = obj_err(sol[k][0], meta[k])
        errs[k + " vs solvers.coneqp"] = obj_err(sol[k][0], one[k])
    print("%s: errors in units of the bound: %s" % (name, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) <= 1.0
    for f in FLOATS:                                                  # None in solvers.coneqp's dictionary is NaN here, and nowhere else
        assert (one[f] is None) == bool(np.isnan(sol[f][0])), f


@pytest.mark.parametrize("name", ["doc_coneqp", "mixed_eq"])
def test_the_upper_triangles_are_not_read(name):
    assert all_bytes(g29_batch(name)) == all_bytes(g29_batch(name + "_garbage"))


def check_against(sol, ref, M, label, options=None):
    """Statuses, iteration counts and exits equal the restatement's, vectors and objectives obey the rule, and for an optimal member
    the stopping inequalities, the membership of s and z in each kind of cone and the slacks hold recomputed in numpy from the
    returned x, y, s, z (the generated G and h have symmetric blocks and s, z come back as full symmetric matrices, so plain products
    are the cone's).  Recomputing moves the last bits of the sums: a residual entry is a sum of at most 450 products of size up to
    1e2, so the infeasibilities get an absolute slack of 1e-12 and the gap a relative one."""
    worst = 0.0
    for k, r in enumerate(ref):
        got = (sol["status"][k], sol["iterations"][k], sol["exit"][k])
        assert got == (r.status, r.iterations, r.exit), (label, k, got, r.status, r.iterations, r.exit)
        if r.exit == 3:
            assert failed(sol, k), (label, k)
            continue
        errs = [vec_err(sol[v][:, k], getattr(r, v)) for v in VECTORS if sol[v].shape[0]]
        errs += [obj_err(sol["primal objective"][k], r.stats[2]), obj_err(sol["dual objective"][k], r.stats[3])]
        P, q, G, h = np.tril(M.P[k]) + np.tril(M.P[k], -1).T, M.q[:, k], M.G[k], M.h[:, k]
        A, b = (np.zeros((0, M.n)), np.zeros(0)) if M.A is None else (M.A[k], M.b[:, k])
        x, y, s, z = (sol[v][:, k] for v in VECTORS)
        assert cone_slack(s, M.dims) > 0 and cone_slack(z, M.dims) > 0, (label, k)
        assert same_slack(sol["primal slack"][k], s, M.dims) and same_slack(sol["dual slack"][k], z, M.dims), (label, k)
        if r.status == "optimal":
            rx, ry, rz = P @ x + q + A.T @ y + G.T @ z, A @ x - b, s + G @ x - h
            pres = max(nrm(ry) / max(1.0, nrm(b)), nrm(rz) / max(1.0, nrm(h)))
            dres = nrm(rx) / max(1.0, nrm(q))
            gap, pcost = s @ z, 0.5 * (x @ (P @ x)) + q @ x
            dcost = pcost + y @ ry + z @ rz - gap
            relgap = gap / -pcost if pcost < 0 else (gap / dcost if dcost > 0 else np.inf)
            assert pres <= FEASTOL + 1e-12 and dres <= FEASTOL + 1e-12, (label, k, pres, dres)
            assert gap <= 1e-7 * (1 + 1e-9) + 1e-12 or relgap <= 1e-6 * (1 + 1e-9), (label, k, gap, relgap)
        worst = max(worst, *errs)
        assert max(errs) <= 1.0, (label, k, errs)
    return worst


def run_batch(name):
    M, options = R.batch(name), R.BATCHES[name][4]
    sol = call(M, options)
    worst = check_against(sol, R.restated(name), M, name)
    print("%s: exits %s, iterations %s, largest error %.2e of the bound" % (name, sol["exit"].tolist(), sol["iterations"].tolist(), worst))
    return M, sol


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_name)
def test_cone_edges(shape):
    M, sol = run_batch(R.shape_name(shape))
    n, ml, q, s, p = shape
    N = ml + sum(q) + sum(m * m for m in s)
    assert sol["x"].shape == (n, R.SHAPE_B) and sol["y"].shape == (p, R.SHAPE_B) and sol["s"].shape == sol["z"].shape == (N, R.SHAPE_B)
    assert list(sol["exit"]) == [0] * R.SHAPE_B and sol["status"] == ["optimal"] * R.SHAPE_B


def test_without_cones_and_blocks_agrees_with_qp_batch():
    shape = (8, 17, 3)
    M = QBN.batch(shape)
    dims = {"l": M.ml, "q": [], "s": []}
    sol = solvers.coneqp_batch(M.P, M.q, M.G, M.h, dims, M.A, M.b)
    other = solvers.qp_batch(M.P, M.q, M.G, M.h, M.A, M.b)
    assert sol["status"] == other["status"] and list(sol["iterations"]) == list(other["iterations"]) and list(sol["exit"]) == list(other["exit"])
    both = max(vec_err(sol[v][:, k], other[v][:, k]) for v in VECTORS for k in range(M.B))
    ref = QBN.restated(shape)                              # tests/test_coneqp_batch_cpu.py: the cone restatement's bytes on the orthant
    assert [(r.iterations, r.exit) for r in ref] == list(zip(sol["iterations"], sol["exit"]))
    worst = max(vec_err(sol[v][:, k], getattr(r, v)) for v in VECTORS for k, r in enumerate(ref))
    print("orthant only: iterations %s, largest error %.2e of the bound of the restatement, %.2e of qp_batch" % (sol["iterations"].tolist(), worst, both))
    assert both <= 1.0 and worst <= 1.0


def test_p_zero_is_a_cone_lp():
    M, sol = run_batch("p-zero")
    assert not M.P.any() and all(np.linalg.matrix_rank(M.G[k]) == M.n for k in range(M.B)) and sol["status"] == ["optimal"] * M.B


def test_p_of_rank_n_minus_2_with_g_supplying_the_rest():
    M, sol = run_batch("p-rank")
    assert sol["status"] == ["optimal"] * M.B


def test_a_coordinate_nothing_holds_is_exit_3_and_disturbs_nobody():
    F = R.batch("p-rank")
    M = R.take(F, range(3))
    R.drop_coordinate(M, 1)
    sol = call(M)
    assert failed(sol, 1) and sol["status"][0] == sol["status"][2] == "optimal"
    ref = R.restated("p-rank")
    for k in (0, 2):
        assert sol["iterations"][k] == ref[k].iterations and vec_err(sol["x"][:, k], ref[k].x) <= 1.0
        assert member_bytes(call(M, which=[k]), 0) == member_bytes(sol, k), k
    assert R.solve_member(*R.member(M, 1)).exit == 3


def test_use_correction_false_and_true():
    _, off = run_batch("no-correction")
    _, on = run_batch("correction")
    assert off["status"] == on["status"] == ["optimal"] * R.SHAPE_B
    assert any(a != b for a, b in zip(off["iterations"], on["iterations"]))


def test_maxiters_3_returns_the_iterate():
    M, sol = run_batch("maxiters-3")
    assert list(sol["exit"]) == [1] * M.B and list(sol["iterations"]) == [3] * M.B and sol["status"] == ["unknown"] * M.B
    assert all(np.isfinite(sol["gap"])) and all(sol["gap"] > 0)


def test_shared_and_per_member_matrices_give_the_same_bytes():
    M = R.batch("correction")
    B = M.B
    shared = solvers.coneqp_batch(M.P[0], M.q, M.G[0], M.h[:, 0], M.dims, M.A[0], M.b[:, 0])
    assert len(set(shared["x"][:, k].tobytes() for k in range(B))) >= 2 and shared["status"][0] == "optimal"
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))         # noqa: E731
    col = lambda v: np.asfortranarray(np.tile(v.reshape(-1, 1), (1, B)))              # noqa: E731
    per = solvers.coneqp_batch(rep(M.P[0]), M.q, rep(M.G[0]), col(M.h[:, 0]), M.dims, rep(M.A[0]), col(M.b[:, 0]))
    assert all_bytes(shared) == all_bytes(per)
    mixed = solvers.coneqp_batch(M.P[0], M.q, rep(M.G[0]), M.h[:, 0], M.dims, M.A[0], col(M.b[:, 0]))
    assert all_bytes(shared) == all_bytes(mixed)
    print("shared matrices with the q of twelve members: exits %s" % shared["exit"].tolist())


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
    M, opts = R.batch("mixed"), R.BATCHES["mixed"][4]
    ref = R.restated("mixed")
    h = M.h.copy()
    h[1, R.MIXED_NAN] = np.nan                           # z of the starting point is NaN: no pivot and no comparison passes
    sol = call(M, opts, h=h)
    assert sol["exit"][R.MIXED_NAN] != 0 and sol["status"][R.MIXED_NAN] == "unknown"
    ended = []
    for k in range(M.B):
        if k == R.MIXED_NAN:
            continue
        got = (sol["status"][k], sol["exit"][k], sol["iterations"][k])
        assert got == (ref[k].status, ref[k].exit, ref[k].iterations), (k, got)
        if got[1] == 3:
            assert failed(sol, k) and k in R.MIXED_RANK
        else:
            assert vec_err(sol["x"][:, k], ref[k].x) <= 1.0 and vec_err(sol["z"][:, k], ref[k].z) <= 1.0
            if got[1] == 1:
                assert got[2] == opts["maxiters"] and np.isfinite(sol["gap"][k]) and sol["gap"][k] > 0
        ended.append(got[1])
        solo = call(M, opts, which=[k])
        assert member_bytes(solo, 0) == member_bytes(sol, k), k
    print("maxiters = %d: exits %s" % (opts["maxiters"], sol["exit"].tolist()))
    assert set(ended) == {0, 1, 3}


def test_the_dev_entry_on_resident_buffers_returns_the_bytes_of_the_host_entry():
    """kvx_coneqp_batch_solve_dev takes no workspace: the kernel stages the scaled rows of G in LDS."""
    M = R.batch("correction")
    host = call(M)
    B, n, N, p = M.B, M.n, M.N, M.p
    up = _lib.DeviceBuffer.from_array
    data = [up(M.P.transpose(0, 2, 1)), up(np.ascontiguousarray(M.q.T)), up(M.G.transpose(0, 2, 1)), up(np.ascontiguousarray(M.h.T)),
            up(M.A.transpose(0, 2, 1)), up(np.ascontiguousarray(M.b.T))]
    outs = [_lib.DeviceBuffer(8 * k * B) for k in (n, p, N, N, len(FLOATS), 1, 1)]
    qv, mv = np.asarray(M.qd, dtype=np.int64), np.asarray(M.s, dtype=np.int64)
    args = [B, n, M.ml, len(M.qd), _lib.pi(qv), len(M.s), _lib.pi(mv), p]
    for buf, stride in zip(data, (n * n, n, N * n, N, p * n, p)):
        args += [buf.ptr, stride]
    args += [100, 1e-7, 1e-6, 1e-7, 1] + [o.ptr for o in outs]
    _lib.raise_for(_lib.lib().kvx_coneqp_batch_solve_dev(*args), "kvx_coneqp_batch_solve_dev")
    for key, buf, rows in zip(VECTORS, outs, (n, p, N, N)):
        assert buf.download(np.float64, rows * B).tobytes() == np.ascontiguousarray(host[key].T).tobytes(), key
    stats = outs[4].download(np.float64, len(FLOATS) * B).reshape(B, len(FLOATS))
    assert stats.tobytes() == np.ascontiguousarray(np.stack([host[f] for f in FLOATS], axis=1)).tobytes()
    assert outs[5].download(np.int64, B).tolist() == host["iterations"].tolist() and outs[6].download(np.int64, B).tolist() == host["exit"].tolist()
    for buf in data + outs:
        buf.free()
