"""The host side of solvers.lp_batch, without a device: the restatement of tests/lp_batch_numpy.py against the
reference's own runs (G4 doc_lp, primal_infeasible, dual_infeasible, grid6x5; G8 eq6x5p4) to the 1e-10 of
tests/test_lp_loop_cpu.py; the A'A repair against an equivalent problem that needs none; that no expected status or iteration
count of a batch of tests/test_lp_batch_gpu.py sits on a rounding edge (float64, numpy.longdouble and float64 with the factors
of numpy.linalg.qr and numpy.linalg.solve in place of the Cholesky ones agree for every member) and that float64 and longdouble differ by at most 1e-2
of the bound the GPU results are held to; the argument checks of lp_batch with their texts; and the KVX_EINVAL of both C entries."""
import json
import os

import numpy as np
import pytest

import lp_batch_numpy as R
from kvxopt_amd import _lib, base, lpbatch, solvers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VECTORS = ("x", "y", "s", "z")


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / np.abs(b).max()


def vec_err(got, ref):
    """|got - ref| in units of the bound 1e-6 max(|ref|, 1) the GPU results are held to."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - ref) / (1e-6 * max(np.linalg.norm(ref), 1.0)))


@pytest.fixture(scope="module")
def g4():
    return json.load(open(os.path.join(GOLDEN, "g4_conelp.json")))["cases"]


@pytest.mark.parametrize("precision", ["float64", "longdouble"])
@pytest.mark.parametrize("name", sorted(R.TINY))
def test_restatement_reproduces_the_tiny_runs(g4, name, precision):
    c, G, h, status, iters, key = R.TINY[name]
    r = R.solve_member(c, G, h, dtype=getattr(np, precision))
    assert r.status == status == g4[name].get("status", status) and r.exit == R.EXITS[status]
    assert r.iterations == iters == g4[name]["iterations"]
    assert rel(getattr(r, key), g4[name][key]) < 1e-10
    gap, rgap, pcost, dcost, pres, dres, pslack, dslack, pinfres, dinfres = r.stats
    if status == "optimal":
        assert np.isnan([pinfres, dinfres]).all() and not np.isnan(r.stats[:8]).any()
        assert abs(pcost - g4[name]["primal objective"]) < 1e-10 * abs(g4[name]["primal objective"])
    elif status == "primal infeasible":                   # the certificate comes without x and s
        assert np.isnan(r.x).all() and np.isnan(r.s).all() and dcost == 1.0 and dslack > 0
        assert np.isnan([gap, rgap, pcost, pres, dres, pslack, dinfres]).all()
        assert abs(pinfres - g4[name]["residual"]) < 1e-13 and pinfres <= 1e-7        # a norm of differences of numbers of size 1
    else:
        assert np.isnan(r.z).all() and pcost == -1.0 and pslack > 0
        assert np.isnan([gap, rgap, dcost, pres, dres, dslack, pinfres]).all()
        assert abs(dinfres - g4[name]["residual"]) < 1e-13 and dinfres <= 1e-7        # a norm of differences of numbers of size 1


@pytest.mark.parametrize("precision", ["float64", "longdouble"])
@pytest.mark.parametrize("name,gfile,p,iters", [("grid6x5", "g4_conelp", 0, 10), ("eq6x5p4", "g8_conelp_eq", 4, 8)])
def test_restatement_reproduces_the_grid_runs(name, gfile, p, iters, precision):
    meta = json.load(open(os.path.join(GOLDEN, gfile + ".json")))["cases"][name]
    g = np.load(os.path.join(GOLDEN, gfile + ".npz"))
    r = R.solve_member(*R.grid_dense(p), dtype=getattr(np, precision))
    assert r.status == meta["status"] == "optimal" and r.exit == 0 and r.iterations == meta["iterations"] == iters
    errs = {k: rel(getattr(r, k), g[name + "_" + k]) for k in (VECTORS if p else ("x",))}
    print("%s in %s: relative distance to the golden: %s" % (name, precision, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) < 1e-10
    assert abs(r.stats[2] - meta["primal objective"]) < 1e-10 * abs(meta["primal objective"])


def test_restatement_reports_a_failed_factorisation_and_maxiters():
    c, G, h, A, b = R.grid_dense(4)
    G0, A0 = G.copy(), A.copy()
    G0[:, 7] = 0.0; A0[:, 7] = 0.0                                    # nothing holds x7: S + A'A is singular too
    r = R.solve_member(c, G0, h, A0, b)
    assert (r.status, r.exit, r.iterations, r.singular) == ("unknown", 3, 0, True) and not r.x.any() and not r.s.any()
    r = R.solve_member(c, G0, h)                                      # p = 0: no repair to try
    assert (r.status, r.exit, r.iterations, r.singular) == ("unknown", 3, 0, False)
    r = R.solve_member(c, G, h, A, b, {"maxiters": 8})                # the reference needs 8: at maxiters it is "unknown"
    assert (r.status, r.exit, r.iterations) == ("unknown", 1, 8) and not np.isnan(r.stats[:8]).any()


@pytest.mark.parametrize("precision", ["float64", "longdouble"])
def test_the_repair_agrees_with_an_equivalent_problem_without_free_variables(precision):
    """A member whose last two variables have no inequality on them (S = G'G has two exact zero pivots; A holds them) against the same
    member with -1e3 <= x_j <= 1e3 added for both: the bounds are a hundred times looser than the solution needs (|x_j| < 10), so both
    problems have the same solution, and the two runs must agree in status and, by the project's vector rule, to 1e-6 max(|x|, 1).
    (Looser bounds still, 1e6, cost the bounded problem its conditioning: it ends "unknown", which says nothing about the repair.)"""
    M = R.batch("free-8-17-3")
    n, k, free = M.n, 0, 2
    c, G, h, A, b = R.member(M, k)
    assert not G[:, n - free:].any() and np.linalg.matrix_rank(A[:, n - free:]) == free
    E = np.zeros((2 * free, n))
    for j in range(free):
        E[2 * j, n - free + j], E[2 * j + 1, n - free + j] = 1.0, -1.0
    dt = getattr(np, precision)
    r = R.solve_member(c, G, h, A, b, None, dt)
    q = R.solve_member(c, np.vstack([G, E]), np.concatenate([h, np.full(2 * free, 1e3)]), A, b, None, dt)
    assert r.singular and not q.singular
    assert r.status == q.status == "optimal" and np.abs(np.asarray(q.x, float)[n - free:]).max() < 10.0
    err = vec_err(r.x, q.x)
    print("%s: x with the repair against x of the bounded problem: %.2e of the bound; iterations %d and %d"
          % (precision, err, r.iterations, q.iterations))
    assert err <= 1.0
    assert vec_err(r.y, q.y) <= 1.0 and vec_err(r.z, np.asarray(q.z)[:len(h)]) <= 1.0


def outcomes(runs):
    return [[(r.status, r.iterations, r.exit) for r in run] for run in runs]


def three_ways(name, which=None):
    if which is None:
        return [R.restated(name), R.restated(name, "float64"), R.restated(name, "float64", True)]
    M = R.batch(name)
    return [R.restate(M, None, dt, ls, which) for dt, ls in ((np.longdouble, False), (np.float64, False), (np.float64, True))]


def float64_against_longdouble(runs):
    """The largest distance of the float64 restatement from the longdouble one in x, y, s, z, in units of the GPU's bound."""
    worst = 0.0
    for a, b in zip(runs[1], runs[0]):
        for v in VECTORS:
            u, w = np.asarray(getattr(a, v), float), np.asarray(getattr(b, v), float)
            assert np.array_equal(np.isnan(u), np.isnan(w))
            if not np.isnan(w).any():
                worst = max(worst, vec_err(u, w))
    return worst


@pytest.mark.parametrize("name", R.SMALL_BATCHES)
def test_no_outcome_of_a_batch_sits_on_a_rounding_edge(name):
    runs = three_ways(name)
    o = outcomes(runs)
    assert o[0] == o[1] == o[2], o
    worst = float64_against_longdouble(runs)
    M = R.batch(name)
    print("%s: (exit, iterations) %s, float64 within %.2e of the GPU's bound of longdouble"
          % (name, [(e, i) for _, i, e in o[0]], worst))
    assert worst <= 1e-2
    want = {R.FEASIBLE: "optimal", R.PRIMAL_INFEASIBLE: "primal infeasible", R.DUAL_INFEASIBLE: "dual infeasible"}
    assert [s for s, _, _ in o[0]] == [want[k] for k in M.kind]
    assert all(i <= 14 for _, i, _ in o[0])
    free = R.BATCHES[name][4]
    assert all(r.singular == bool(free) for r in runs[0]) and all(r.singular == bool(free) for r in runs[1])
    if name == "shape-1-1-0":
        assert all(i == 0 for _, i, _ in o[0])              # a vertex at the start (tests/lp_batch_numpy.py on its seed)
    else:
        assert all(i >= 3 for _, i, _ in o[0])


def test_the_mixed_batch_ends_in_every_way_at_its_median_count():
    runs = three_ways("mixed")
    counts = [r.iterations for r in runs[0]]
    m = int(np.median(counts))
    M = R.batch("mixed")
    limited = [R.restate(M, {"maxiters": m}, dt, ls) for dt, ls in ((np.longdouble, False), (np.float64, False), (np.float64, True))]
    o = outcomes(limited)
    assert o[0] == o[1] == o[2], o
    kept = [e for k, (_, _, e) in enumerate(o[0]) if k not in R.MIXED_CHANGED]
    assert set(kept) == {0, 1, 4, 5}, o[0]
    assert all(i == m for _, i, e in o[0] if e == 1) and all(i < m for _, i, e in o[0] if e != 1)


@pytest.mark.parametrize("part", range(4))
def test_no_outcome_of_the_independence_batch_sits_on_a_rounding_edge(part):
    B = R.BATCHES["independence"][1]
    runs = three_ways("independence", which=range(part * B // 4, (part + 1) * B // 4))
    o = outcomes(runs)
    assert o[0] == o[1] == o[2], o
    assert len(o[0]) == B // 4 and len(set(i for _, i, _ in o[0])) >= 2 and set(s for s, _, _ in o[0]) == {"optimal"}
    assert float64_against_longdouble(runs) <= 1e-2


# ---- argument checks: all of them before a device is asked for (this box has none, or the call would go on to the device)
def data(n=4, ml=6, p=2, B=3, seed=0):
    M = R.members(n, ml, p, B, seed)
    return M.c, M.G, M.h, M.A, M.b


@pytest.mark.parametrize("n,ml,p,text", [(65, 70, 0, r"n = 65 is outside its limit 1 <= n <= 64.*solvers\.lp"),
                                         (4, 513, 0, r"ml = 513 is outside its limit 1 <= ml <= 512.*solvers\.lp"),
                                         (4, 6, 5, r"p = 5 is outside its limit 0 <= p <= n.*solvers\.lp"),
                                         (8, 5, 2, r"p \+ ml = 7 is outside its limit p \+ ml >= n = 8.*solvers\.lp")])
def test_limits(n, ml, p, text):
    c, G, h, A, b = data(n, ml, p)
    with pytest.raises(ValueError, match=text):
        solvers.lp_batch(c, G, h, A, b)
    with pytest.raises(ValueError, match=text):                       # shared matrices run into the same limits
        solvers.lp_batch(c, G[0], h, None if A is None else A[0], b)


def test_limits_at_zero():
    c, G, h, A, b = data()
    with pytest.raises(ValueError, match="ml = 0 is outside its limit 1 <= ml <= 512"):
        solvers.lp_batch(c, np.zeros((0, 4)), np.zeros(0))
    with pytest.raises(ValueError, match="n = 0 is outside its limit 1 <= n <= 64"):
        solvers.lp_batch(np.zeros((0, 3)), np.zeros((6, 0)), h)


def test_sizes_and_types():
    c, G, h, A, b = data()
    bad = [
        ((c, G[:2], h, A, b), "'G' has 2 members, 'c' has 3 columns"),
        ((c, G, h, A[:1], b), "'A' has 1 members, 'c' has 3 columns"),
        ((c, G, h[:, :2], A, b), "'h' must have one column or B = 3 columns"),
        ((c, G, h, A, b[:, :2]), "'b' must have one column or B = 3 columns"),
        ((c, G[:, :, :3], h, A, b), r"'G' must be a 'd' matrix of size \(ml, 4\)"),
        ((c, G, h[:5], A, b), r"'h' must be a 'd' matrix of size \(6,1\)"),
        ((c, G, h, A[:, :, :3], b), "'A' must be a 'd' matrix with 4 columns"),
        ((c, G, h, A, b[:1]), "'b' must have length 2"),
        ((c, G, h, A, None), "'b' must have length 2"),
        ((c, G, h, None, b), "'b' must have length 0"),
        ((c, G.astype(np.float32), h, A, b), r"'G' must be one matrix or a float64 array of shape \(B, rows, 4\)"),
        ((c, G[None], h, A, b), r"'G' must be one matrix or a float64 array of shape \(B, rows, 4\)"),
        ((c[:, :, None], G, h, A, b), "'c' must be a 'd' matrix with one column per member"),
    ]
    for args, text in bad:
        with pytest.raises(TypeError, match=text):
            solvers.lp_batch(*args)


def test_shared_inputs_of_every_kind_pass_the_checks():
    c, G, h, A, b = data()
    sp = base.spmatrix([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 0, 1], (6, 4))
    for Gm in (G[0], base.matrix(np.asfortranarray(G[0])), sp):
        opt, dims, parts = lpbatch._prepare(base.matrix(np.asfortranarray(c)), Gm, h[:, 0], base.matrix(np.asfortranarray(A[0])), b[:, :1], None)
        assert dims == (3, 4, 6, 2) and [s for _, s in parts] == [4, 0, 0, 0, 0]
    D = parts[1][0].reshape(4, 6).T
    assert D[4, 0] == 5.0 and D[5, 1] == 6.0 and D[3, 3] == 4.0 and np.count_nonzero(D) == 6
    opt, dims, parts = lpbatch._prepare(c, G, h, A, b, {"maxiters": 7})
    assert opt.maxiters == 7 and [s for _, s in parts] == [4, 24, 6, 8, 2]
    assert np.array_equal(parts[1][0][24:48].reshape(4, 6).T, G[1]) and np.array_equal(parts[2][0][6:12], h[:, 1])       # column-major members
    opt, dims, parts = lpbatch._prepare(c[:, 0], G[0], h[:, 0], None, None, None)                                          # B = 1, p = 0
    assert dims == (1, 4, 6, 0) and parts[3] == (None, 0) and parts[4] == (None, 0)


def test_options():
    args = data()
    with pytest.raises(NotImplementedError, match=r"options\['refinement'\] = 1 is not carried"):
        solvers.lp_batch(*args, options={"refinement": 1})
    for o, text in (({"maxiters": 0}, r"options\['maxiters'\] must be a positive integer"),
                    ({"maxiters": 2.5}, r"options\['maxiters'\] must be a positive integer"),
                    ({"abstol": "a"}, r"options\['abstol'\] must be a scalar"),
                    ({"reltol": -1.0, "abstol": 0.0}, r"at least one of options\['reltol'\] and options\['abstol'\] must be positive"),
                    ({"feastol": 0.0}, r"options\['feastol'\] must be a positive scalar"),
                    ({"refinement": -1}, r"options\['refinement'\] must be a nonnegative integer")):
        with pytest.raises(ValueError, match=text):
            solvers.lp_batch(*args, options=o)
    for kw in ({"primalstart": {}}, {"dualstart": {}}, {"kktsolver": "chol2"}, {"solver": "glpk"}):
        with pytest.raises(TypeError):
            solvers.lp_batch(*args, **kw)


def test_the_entry_is_public():
    assert hasattr(solvers, "lp_batch") and solvers.lp_batch is lpbatch.lp_batch and "lp_batch" in solvers.__doc__
    for text in ("primal infeasible", "A'A", "_ipm.conelp_start", "does not disturb the others"):
        assert text in lpbatch.__doc__


def test_good_arguments_reach_the_device_or_fail_loudly():
    """No fallback loop: without a device a call that passes every check raises, it does not compute."""
    args, opts = data(), {"refinement": 0, "show_progress": True}
    if _lib.lib().kvx_device_count() > 0:
        assert solvers.lp_batch(*args, options=opts)["status"] == ["optimal"] * 3
    else:
        with pytest.raises(RuntimeError, match="no HIP device"):
            solvers.lp_batch(*args, options=opts)


@pytest.mark.parametrize("entry", ["kvx_lp_batch_solve", "kvx_lp_batch_solve_dev"])
def test_c_entries_answer_einval_without_a_device(entry):
    fn = getattr(_lib.lib(), entry)
    n, ml, p, B = 4, 6, 2, 3
    buf = np.zeros(4096)
    ints = np.zeros(8, dtype=np.int64)
    dev = entry.endswith("_dev")
    D = (lambda a: a.ctypes.data) if dev else _lib.pd
    Di = (lambda a: a.ctypes.data) if dev else _lib.pi

    def call(B=B, n=n, ml=ml, p=p, strides=(4, 24, 6, 8, 2), null=(), maxiters=10, abstol=1e-7, reltol=1e-6, feastol=1e-7):
        data = []
        for k, s in enumerate(strides):
            data += [None if k in null else D(buf), s]
        outs = [None if 5 + k in null else D(buf) for k in range(5)] + [None if 10 + k in null else Di(ints) for k in range(2)]
        return fn(B, n, ml, p, *data, maxiters, abstol, reltol, feastol, *outs)

    for kw, text in (({"B": 0}, "1 <= B"), ({"n": 0}, "1 <= n <= 64"), ({"n": 65}, "1 <= n <= 64"), ({"ml": 0}, "1 <= ml <= 512"),
                     ({"ml": 513}, "1 <= ml <= 512"), ({"p": -1}, "0 <= p <= n"), ({"p": 5}, "0 <= p <= n"),
                     ({"n": 9, "p": 2}, "p + ml >= n"),
                     ({"strides": (3, 24, 6, 8, 2)}, "stride of c"), ({"strides": (4, 23, 6, 8, 2)}, "stride of G"),
                     ({"strides": (4, 24, 6, 8, 1)}, "stride of b"), ({"strides": (4, 24, 6, -8, 2)}, "stride of A"),
                     ({"null": (0,)}, "data pointer"), ({"null": (2,)}, "data pointer"), ({"null": (3,)}, "data pointer"),
                     ({"null": (5,)}, "result pointer"), ({"null": (6,)}, "result pointer"), ({"null": (9,)}, "result pointer"),
                     ({"null": (11,)}, "result pointer"), ({"maxiters": 0}, "maxiters"), ({"feastol": 0.0}, "feastol"),
                     ({"abstol": 0.0, "reltol": -1.0}, "reltol and abstol"), ({"feastol": float("nan")}, "feastol")):
        assert call(**kw) == _lib.KVX_EINVAL, kw
        assert entry in _lib.last_error() and text in _lib.last_error(), (kw, _lib.last_error())
    if _lib.lib().kvx_device_count() == 0:
        assert call() == _lib.KVX_EDEVICE and "no CPU fallback" in _lib.last_error()
        assert call(p=0, null=(3, 4, 6), strides=(0, 0, 0, 0, 0)) == _lib.KVX_EDEVICE        # A, b, y may be NULL when p = 0
