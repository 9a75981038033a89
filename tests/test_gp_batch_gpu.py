"""solvers.gp_batch on the device against the reference's own runs at refinement 0 (G30), against solvers.gp of
this package, and against the numpy.longdouble restatement of tests/gp_batch_numpy.py on generated members at every edge of the
kernel: block sizes across the strides of the wavefront reductions, one-term blocks, the limits n = p = 63, N = 192, l = 768, the
edge of the staging tile and the LDS corner; g of about +-700, a column nothing holds, a NaN, a run cut at maxiters, and the batches
whose line searches backtrack, save, count relaxed iterations, resume and restore.  The rule of tests/test_lp_batch_gpu.py: vectors
to 1e-6 max(|ref|, 1) in the 2-norm, objectives to 1e-7 max(|ref|, 1), statuses, iteration counts and exits exactly.
tests/test_gp_batch_cpu.py shows that float64 and longdouble agree on every member of these batches.

Measured on an MI355X (this file's prints), largest error in units of the rule's bound: G30 cases 1.6e-5 (gp_doc, znl) against the
reference and 2.3e-5 against solvers.gp; edges 3.6e-8 (2, [1, 1, 1], 0, 1), 2.2e-7 (5, [63, 64, 65], 3, 0), 1.7e-7 (6, [255, 256, 257], 0, 2),
3.5e-6 with one-term blocks mixed in, 2.0e-6 at n = p = 63, 2.5e-6 and 1.9e-4 at N = 192 through blocks and through ml, 1.1e-7, 9.7e-8,
8.1e-8 at 31, 32, 33 staged factor rows, 3.1e-5 at 33 gradient rows, 6.4e-9 at the LDS corner; g of +-700 3.2e-7; maxiters = 3 4.4e-9;
independence 2.2e-6; mixed outcomes 4.7e-7; the branches batch 9.1e-7, the restore batches 1.7e-7 and 9.4e-7."""
import json
import os

import numpy as np
import pytest

import gp_batch_numpy as R
from kvxopt_amd import _lib, solvers

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOATS = ("gap", "relative gap", "primal objective", "dual objective", "primal infeasibility", "dual infeasibility",
          "primal slack", "dual slack")
VECTORS = ("x", "y", "znl", "snl", "zl", "sl")
G30_CASES = ("gp_doc", "gp_random", "gp_doc_maxiters", "gp_objective_only", "gp_eq_no_linear")
nrm = np.linalg.norm


def call(M, options=None, which=None):
    return solvers.gp_batch(*R.batch_args(M, which), options=options)


def vec_err(got, ref):
    """|got - ref| in units of the rule's bound 1e-6 max(|ref|, 1): passes when <= 1."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(nrm(got - ref) / (1e-6 * max(nrm(ref), 1.0)))


def obj_err(got, ref):
    return abs(got - float(ref)) / (1e-7 * max(abs(float(ref)), 1.0))


def parts(r):
    """The vectors of a restated member under the keys of gp_batch."""
    m = len(r.K)
    return {"x": r.x, "y": r.y, "znl": r.z[1:m], "snl": r.s[1:m], "zl": r.z[m:], "sl": r.s[m:]}


def member_bytes(sol, k):
    return b"".join(np.ascontiguousarray(sol[key][:, k]).tobytes() for key in VECTORS) + \
        b"".join(np.asarray(sol[key][k]).tobytes() for key in FLOATS + ("iterations", "exit"))


def lse(F, g, K, x):
    off = np.concatenate([[0], np.cumsum(K)])
    u = F @ x + g
    return np.array([np.log(np.exp(u[a:b] - u[a:b].max()).sum()) + u[a:b].max() for a, b in zip(off[:-1], off[1:])])


def against(sol, ref, M, label, which=None, options=None):
    """Every member of `sol` against its restated result: status, count and exit equal, vectors and objectives by the rule; for an
    optimal member the stopping inequalities, the signs and the residuals recomputed in numpy.  Returns the largest error."""
    opt = dict({"abstol": 1e-7, "reltol": 1e-6, "feastol": 1e-7}, **(options or {}))
    worst = 0.0
    for j, r in enumerate(ref):
        k = j if which is None else list(which)[j]
        assert (sol["status"][j], int(sol["iterations"][j]), int(sol["exit"][j])) == (r.status, r.iterations, r.exit), (label, k)
        if r.exit == R.EXIT_RANK:
            assert all(not sol[key][:, j].any() for key in VECTORS) and all(np.isnan(sol[f][j]) for f in FLOATS), (label, k)
            continue
        assert all(np.isfinite(sol[key][:, j]).all() for key in VECTORS), (label, k)
        errs = [vec_err(sol[key][:, j], v) for key, v in parts(r).items()]
        errs += [obj_err(sol["primal objective"][j], r.stats[2]), obj_err(sol["dual objective"][j], r.stats[3])]
        worst = max(worst, max(errs))
        assert max(errs) <= 1.0, (label, k, errs)
        if r.exit == R.EXIT_OPTIMAL:
            K, F, g, G, h, A, b = R.member_args(M, k)
            m, x = len(K), sol["x"][:, j]
            assert sol["primal infeasibility"][j] <= opt["feastol"] and sol["dual infeasibility"][j] <= opt["feastol"], (label, k)
            assert sol["gap"][j] <= opt["abstol"] or sol["relative gap"][j] <= opt["reltol"], (label, k)
            assert all((sol[key][:, j] > 0).all() for key in ("snl", "sl", "znl", "zl")), (label, k)
            f0 = lse(F, g, K, np.zeros(M.n))                                  # the residuals at the starting point scale the test
            pres0 = max(1.0, np.sqrt(nrm(1.0 + f0) ** 2 + (nrm(1.0 - h) ** 2 if h is not None else 0.0) + (nrm(b) ** 2 if b is not None else 0.0)))
            assert nrm(lse(F, g, K, x)[1:] + sol["snl"][:, j]) <= opt["feastol"] * pres0 + 1e-12, (label, k)
            if G is not None:
                assert nrm(G @ x + sol["sl"][:, j] - h) <= opt["feastol"] * pres0 + 1e-12, (label, k)
    print("%s: largest error %.2e of the bound" % (label, worst))
    return worst


# ---- the reference's own runs
def g30_case(name):
    meta = json.load(open(os.path.join(GOLDEN, "g30_gp_batch.json")))["cases"][name]
    g = np.load(os.path.join(GOLDEN, "g30_gp_batch.npz"))
    get = lambda k: g["%s__%s" % (name, k)] if "%s__%s" % (name, k) in g else None          # noqa: E731
    return meta, (meta["K"], get("F"), get("g"), get("G"), get("h"), get("A"), get("b")), {k: get("sol_" + k) for k in VECTORS}


@pytest.mark.parametrize("name", G30_CASES)
def test_golden_member_of_a_batch(name):
    """Member 0 of a batch of 3 with a shared F and perturbed g: the reference's status, count and vectors, and the status and
    count of this package's solvers.gp at refinement 0."""
    meta, (K, F, g, G, h, A, b), ref = g30_case(name)
    rng = np.random.default_rng(5)
    g3 = np.asfortranarray(np.stack([g, g + 1e-3 * rng.standard_normal(g.size), g - 1e-3 * rng.standard_normal(g.size)], axis=1))
    sol = solvers.gp_batch(K, F, g3, G, h, A, b, options=meta["options"])
    assert (sol["status"][0], int(sol["iterations"][0])) == (meta["status"], meta["iterations"])
    assert int(sol["exit"][0]) == (0 if meta["status"] == "optimal" else 1)
    errs = {k: vec_err(sol[k][:, 0], ref[k]) for k in VECTORS}
    errs["pcost"] = obj_err(sol["primal objective"][0], meta["primal objective"])
    errs["dcost"] = obj_err(sol["dual objective"][0], meta["dual objective"])
    print("%s against G30: %s" % (name, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) <= 1.0
    one = solvers.gp(K, F, g, G, h, A, b, options=dict(meta["options"], refinement=0, show_progress=False))
    assert (one["status"], one["iterations"]) == (meta["status"], meta["iterations"])
    ours = {k: vec_err(sol[k][:, 0], np.asarray(one[k]).reshape(-1)) for k in VECTORS}
    print("%s against solvers.gp: %s" % (name, ", ".join("%s %.2e" % kv for kv in ours.items())))
    assert max(ours.values()) <= 1.0


# ---- the edges of the kernel
@pytest.mark.parametrize("name", list(R.EDGES))
def test_edges(name):
    M, opts = R.edge(name), R.EDGE_OPTIONS.get(name)
    ref = R.restated(name)
    against(call(M, opts), ref, M, name, options=opts)
    if name == "n1_k1":                                                    # S = dnli^2 [F; -1][F; -1]' has rank 1 of 2
        assert [r.exit for r in ref] == [R.EXIT_RANK] * M.B
    else:
        assert [r.status for r in ref] == ["optimal"] * M.B


def test_g_of_about_700_is_finite():
    """exp(700) is near the largest double and exp(-700) near the smallest normal one: the maximum of a block is taken before exp."""
    M = R.spread_batch()
    assert np.abs(M.g).max() > 600
    against(call(M), R.restated("spread700"), M, "spread700")


def zero_column(M, k, c):
    """Member k of a copy of M with column c of F, G and A zero: nothing holds x_c."""
    F, G, A = M.F.copy(), None if M.G is None else M.G.copy(), None if M.A is None else M.A.copy()
    for X in (F, G, A):
        if X is not None:
            X[k, :, c] = 0.0
    return R.types.SimpleNamespace(**dict(M.__dict__, F=F, G=G, A=A))


def test_a_column_nothing_holds_is_exit_3_and_disturbs_nobody():
    M = zero_column(R.shaped((4, (5, 3), 8, 1), 3, 3020), 1, 2)
    ref = R.restate(M, None, np.longdouble)
    assert [r.exit for r in ref] == [0, R.EXIT_RANK, 0]
    sol = call(M)
    against(sol, ref, M, "zero column")
    for k in (0, 2):
        assert member_bytes(sol, k) == member_bytes(call(M, which=[k]), 0)


def test_a_nan_in_g_is_exit_3_and_disturbs_nobody():
    """The NaN reaches every entry of S through the block's gradient: pivot 0 fails before any line search."""
    M0 = R.shaped((4, (5, 3), 8, 1), 3, 3020)
    g = M0.g.copy()
    g[6, 1] = np.nan
    M = R.types.SimpleNamespace(**dict(M0.__dict__, g=g))
    ref = R.restate(M, None, np.longdouble)
    assert [r.exit for r in ref] == [0, R.EXIT_RANK, 0]
    sol = call(M)
    against(sol, ref, M, "nan")
    for k in (0, 2):
        assert member_bytes(sol, k) == member_bytes(call(M0, which=[k]), 0)


def test_maxiters_3_returns_the_iterate():
    M = R.named("mixed")
    ref = R.restated("mixed", maxiters=3)
    assert [r.exit for r in ref] == [R.EXIT_MAXITERS] * M.B
    against(call(M, {"maxiters": 3}), ref, M, "maxiters 3")


def test_shared_and_per_member_matrices_give_the_same_bytes():
    M = R.shaped((4, (5, 3), 8, 1), 1, 3021)
    B = 5
    g = np.asfortranarray(M.g + 1e-2 * np.random.default_rng(6).standard_normal((M.g.shape[0], B)))
    rep = lambda a: np.ascontiguousarray(np.repeat(a, B, axis=0))         # noqa: E731
    col = lambda v: np.asfortranarray(np.repeat(v, B, axis=1))            # noqa: E731
    shared = solvers.gp_batch(M.K, M.F[0], g, M.G[0], M.h[:, 0], M.A[0], M.b[:, 0])
    per = solvers.gp_batch(M.K, rep(M.F), g, rep(M.G), col(M.h), rep(M.A), col(M.b))
    mixed = solvers.gp_batch(M.K, rep(M.F), g, M.G[0], col(M.h), M.A[0], M.b[:, 0])
    assert shared["status"] == ["optimal"] * B
    for k in range(B):
        assert member_bytes(shared, k) == member_bytes(per, k) == member_bytes(mixed, k)


def test_a_member_does_not_depend_on_its_batch():
    M = R.named("independence")
    assert M.B == 300
    sol, again = call(M), call(M)
    assert all(member_bytes(sol, k) == member_bytes(again, k) for k in range(M.B))
    which = (0, 63, 64, 299)
    for k in which:
        assert member_bytes(sol, k) == member_bytes(call(M, which=[k]), 0), k
    sub = {key: (sol[key][:, list(which)] if key in VECTORS else [sol[key][k] for k in which]) for key in sol}
    against(sub, R.restated("independence", which=which), M, "independence", which=which)


def test_mixed_outcomes_in_one_batch():
    """Exits 0, 1 and 3 in one call: maxiters = 9 cuts the members that need more, and one member has a column nothing holds."""
    M = zero_column(R.named("mixed"), 3, 1)
    ref = R.restate(M, {"maxiters": 9}, np.longdouble)
    assert sorted(set(r.exit for r in ref)) == [0, 1, 3]
    sol = call(M, {"maxiters": 9})
    against(sol, ref, M, "mixed outcomes")
    for k in range(M.B):
        assert member_bytes(sol, k) == member_bytes(call(M, {"maxiters": 9}, which=[k]), 0), k


def test_the_dev_entry_on_resident_buffers_returns_the_bytes_of_the_host_entry():
    M = R.named("mixed")
    host = call(M)
    B, n, m, ml, p, l = M.B, M.n, len(M.K), M.ml, M.p, sum(M.K)
    N = m + ml
    up = _lib.DeviceBuffer.from_array
    data = [up(M.F.transpose(0, 2, 1)), up(np.ascontiguousarray(M.g.T)), up(M.G.transpose(0, 2, 1)), up(np.ascontiguousarray(M.h.T)),
            up(M.A.transpose(0, 2, 1)), up(np.ascontiguousarray(M.b.T))]
    outs = [_lib.DeviceBuffer(8 * k * B) for k in (n, p, N, N, len(FLOATS), 1, 1)]
    per = _lib.lib().kvx_gp_batch_scratch_doubles(n, m - 1, ml, p)
    assert per > 0
    scratch = _lib.DeviceBuffer(8 * per * B)
    Kv = np.asarray(M.K, dtype=np.int64)
    args = [B, n, m - 1, _lib.pi(Kv), ml, p]
    for buf, stride in zip(data, (l * n, l, ml * n, ml, p * n, p)):
        args += [buf.ptr, stride]
    args += [100, 1e-7, 1e-6, 1e-7] + [o.ptr for o in outs] + [scratch.ptr]
    _lib.raise_for(_lib.lib().kvx_gp_batch_solve_dev(*args), "kvx_gp_batch_solve_dev")
    s, z = (outs[k].download(np.float64, N * B).reshape(B, N) for k in (2, 3))
    got = {"x": outs[0].download(np.float64, n * B).reshape(B, n), "y": outs[1].download(np.float64, p * B).reshape(B, p),
           "znl": z[:, 1:m], "snl": s[:, 1:m], "zl": z[:, m:], "sl": s[:, m:]}
    for key in VECTORS:
        assert np.ascontiguousarray(got[key]).tobytes() == np.ascontiguousarray(host[key].T).tobytes(), key
    stats = outs[4].download(np.float64, len(FLOATS) * B).reshape(B, len(FLOATS))
    assert stats.tobytes() == np.ascontiguousarray(np.stack([host[f] for f in FLOATS], axis=1)).tobytes()
    assert outs[5].download(np.int64, B).tolist() == host["iterations"].tolist() and outs[6].download(np.int64, B).tolist() == host["exit"].tolist()
    for buf in data + outs + [scratch]:
        buf.free()


@pytest.mark.parametrize("name", ["branches", "restore", "restore2"])
def test_the_line_search_branches(name):
    """The batches tests/test_gp_batch_cpu.py certifies for the branch counters: backtracking, the saved state, relaxed iterations
    and the resume at MAX_RELAXED_ITERS (branches); the restore after a failed factorisation (restore, restore2)."""
    M = R.named(name)
    against(call(M), R.restated(name), M, name)
