"""The host side of solvers.gp_batch, without a device: the restatement of tests/gp_batch_numpy.py against the
reference's own runs at refinement 0 (G30) in status, iterations and x, y, znl, snl, zl, sl to 1e-8 relative; that float64 and
numpy.longdouble agree in status, count and exit for every member of every batch of tests/test_gp_batch_gpu.py and differ by at
most 1e-2 of the bound the GPU results are held to; that those batches reach the branches of the line search they are to show; the
argument checks of gp_batch with their texts; the KVX_EINVAL of both C entries; and that the corners of the box pass the LDS check.

Measured (this file's prints), largest relative distance of the vectors to G30 in float64 / longdouble: gp_doc 2.5e-11 / 7.4e-15,
gp_random 1.1e-9 / 1.8e-12 (zl), gp_doc_maxiters 1.1e-15 / 2.3e-16, gp_objective_only 5.4e-16 / 5.4e-16, gp_eq_no_linear 2.5e-13 /
5.9e-14.  The reference solves by LAPACK's LDL' (kktsolver='ldl') after eliminating t in closed form; the restatement carries t as
column n and factors S and K by Cholesky: the same iterates, other roundings.

Over the batches of the GPU file the line search halves its step at most 9 times in one loop (BRANCHES); the bound is 64."""
import json
import os

import numpy as np
import pytest

import gp_batch_numpy as R
from kvxopt_amd import _lib, gpbatch, solvers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VECTORS = ("x", "y", "znl", "snl", "zl", "sl")
G30_CASES = ("gp_doc", "gp_random", "gp_doc_maxiters", "gp_objective_only", "gp_eq_no_linear")
BATCHES = list(R.EDGES) + ["spread700", "mixed", "branches", "restore", "restore2"]


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def vec_err(got, ref):
    """|got - ref| in units of the bound 1e-6 max(|ref|, 1) the GPU results are held to."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - ref) / (1e-6 * max(np.linalg.norm(ref), 1.0)))


def parts(r):
    m = len(r.K)
    return {"x": r.x, "y": r.y, "znl": r.z[1:m], "snl": r.s[1:m], "zl": r.z[m:], "sl": r.s[m:]}


def agree(a, b):
    """Status, count and exit equal member by member; the largest distance of the vectors in units of the GPU bound."""
    assert [(r.status, r.iterations, r.exit) for r in a] == [(r.status, r.iterations, r.exit) for r in b]
    return max(vec_err(getattr(u, k), getattr(w, k)) for u, w in zip(a, b) for k in ("x", "y", "s", "z"))


def g30_case(name):
    meta = json.load(open(os.path.join(GOLDEN, "g30_gp_batch.json")))["cases"][name]
    g = np.load(os.path.join(GOLDEN, "g30_gp_batch.npz"))
    get = lambda k: g["%s__%s" % (name, k)] if "%s__%s" % (name, k) in g else None           # noqa: E731
    return meta, (meta["K"], get("F"), get("g"), get("G"), get("h"), get("A"), get("b")), {k: get("sol_" + k) for k in VECTORS}


@pytest.mark.parametrize("precision", ["float64", "longdouble"])
@pytest.mark.parametrize("name", G30_CASES)
def test_restatement_reproduces_the_reference_at_refinement_0(name, precision):
    meta, data, sol = g30_case(name)
    r = R.solve_member(*data, options=meta["options"], dtype=getattr(np, precision))
    assert r.status == meta["status"] and r.iterations == meta["iterations"]
    assert r.exit == (0 if meta["status"] == "optimal" else 1)
    errs = {k: rel(v, sol[k]) for k, v in parts(r).items() if sol[k].size}
    print("%s in %s: relative distance to G30: %s" % (name, precision, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) < 1e-8
    assert abs(r.stats[2] - meta["primal objective"]) < 1e-8 * max(abs(meta["primal objective"]), 1.0)
    assert abs(r.stats[3] - meta["dual objective"]) < 1e-8 * max(abs(meta["dual objective"]), 1.0)


def test_g30_holds_the_cases_it_is_to_hold():
    cases = {name: g30_case(name) for name in G30_CASES}
    assert cases["gp_doc"][0]["K"] == [1, 2, 1, 1, 1, 1, 1] and cases["gp_doc"][0]["status"] == "optimal"
    m, d, _ = cases["gp_random"]
    assert m["K"] == [4, 3, 1, 5, 2] and d[3].shape == (15, 6) and d[5].shape == (2, 6)
    m, _, _ = cases["gp_doc_maxiters"]
    assert (m["status"], m["iterations"], m["options"]) == ("unknown", 4, {"maxiters": 4}) and cases["gp_doc"][0]["iterations"] > 4
    m, d, _ = cases["gp_objective_only"]
    assert len(m["K"]) == 1 and d[3] is None and d[5] is None and m["status"] == "optimal"          # ml = 0, mnl = 0
    m, d, _ = cases["gp_eq_no_linear"]
    assert len(m["K"]) > 1 and d[3] is None and d[5].shape[0] > 0 and m["status"] == "optimal"      # p > 0, ml = 0


# ---- the batches of the GPU file
@pytest.mark.parametrize("name", BATCHES)
def test_float64_and_longdouble_agree_on_every_member(name):
    a, b = R.restated(name, "float64"), R.restated(name, "longdouble")
    err = agree(a, b)
    print("%s: float64 and longdouble %.2e of the GPU bound apart; exits %s" % (name, err, sorted(set(r.exit for r in b))))
    assert err <= 1e-2


def test_the_cut_and_the_mixed_runs_agree_too():
    for maxiters in (3, 9):
        assert agree(R.restated("mixed", "float64", maxiters=maxiters), R.restated("mixed", "longdouble", maxiters=maxiters)) <= 1e-2


@pytest.mark.parametrize("part", range(4))
def test_float64_and_longdouble_agree_on_the_independence_batch(part):
    M, B = R.named("independence"), R.INDEPENDENCE[1]
    which = range(part * B // 4, (part + 1) * B // 4)
    a, b = R.restate(M, None, np.float64, which), R.restate(M, None, np.longdouble, which)
    assert agree(a, b) <= 1e-2
    assert len(set(r.iterations for r in b)) >= 2 and set(r.status for r in b) == {"optimal"}


def test_the_batches_have_the_shapes_they_are_to_show():
    E = R.EDGES
    assert E["n1_k1"][:4] == (1, [1], 0, 0) and E["one_term_blocks"][:4] == (2, [1, 1, 1], 0, 1)
    assert E["k63_64_65"][:4] == (5, [63, 64, 65], 3, 0) and E["l768"][:4] == (6, [255, 256, 257], 0, 2)
    assert 1 in E["mixed_one_term"][1] and max(E["mixed_one_term"][1]) > 1
    assert E["n63_p63"][0] == E["n63_p63"][3] == 63 and sum(E["n63_p63"][1]) <= 8
    n, K, ml, p = E["N192_blocks"][:4]
    assert len(K) + ml == 192 and ml == 0 and set(K[1:]) == {1, 2}
    n, K, ml, p = E["N192_linear"][:4]
    assert len(K) + ml == 192 and ml == 191 - (len(K) - 1)
    assert [sum(E[k][1]) for k in ("tile_minus", "tile_exact", "tile_plus")] == [R.TILE - 1, R.TILE, R.TILE + 1]
    assert len(E["blocks_tile_plus"][1]) == R.TILE + 1
    n, K, ml, p = E["lds_corner"][:4]
    assert (n, p, len(K) + ml, sum(K)) == (63, 63, 192, 768)
    assert all(B in range(8, 13) for _, _, _, _, B, _ in E.values())


def test_the_line_search_branches_are_reached():
    """Over the batches of the GPU file, at least once each: a backtrack with halvings, a saved state, relaxed_iters += 1, the
    resume of a saved line search at MAX_RELAXED_ITERS -- and the restore after a failed factorisation, which feasible data do
    reach.  Runs with other roundings take the same branches in every member."""
    key = lambda r: (r.exit, r.iterations, tuple(r.counters[k] for k in R.COUNTERS))          # noqa: E731
    total = dict.fromkeys(R.COUNTERS, 0)
    for name in BATCHES:
        a, b = R.restated(name, "float64"), R.restated(name, "longdouble")
        if name in ("branches", "restore", "restore2"):
            assert [key(r) for r in a] == [key(r) for r in b], name
        for r in b:
            for k in R.COUNTERS:
                total[k] = max(total[k], r.counters[k]) if k == "max_halvings" else total[k] + r.counters[k]
    print("branches taken over the batches of the GPU file:", total)
    assert total["backtracks"] > 0 and total["saved"] > 0 and total["relaxed_inc"] > 0 and total["resumed"] > 0
    assert total["restored"] > 0
    assert 1 <= total["max_halvings"] < R.MAX_HALVINGS // 2
    b = R.restated("branches", "float64")
    assert [key(r) for r in b] == [key(r) for r in R.restated("branches", "float64", linsolve=True)]
    assert sum(r.counters["resumed"] for r in b) > 0 and sum(r.counters["backtracks"] for r in b) > 0
    for name in ("restore", "restore2"):
        s = R.restated(name, "float64")
        assert [key(r) for r in s] == [key(r) for r in R.restated(name, "float64", reverse=True)]
        assert [key(r) for r in s] == [key(r) for r in R.restated(name, "float64", linsolve=True)]
        assert sum(r.counters["restored"] for r in s) > 0


# ---- argument checks: all of them before a device is asked for
def data(n=4, K=(5, 3), ml=8, p=1, B=3, seed=0):
    M = R.members(n, list(K), ml, p, B, seed)
    return R.batch_args(M)


@pytest.mark.parametrize("n,K,ml,p,text", [
    (64, (70,), 0, 0, r"n = 64 is outside its limit 1 <= n <= 63.*solvers\.gp solves one problem"),
    (4, (5, 3), 191, 0, r"N = 193 is outside its limit 1 <= N <= 192.*solvers\.gp"),
    (2, (3,) + (1,) * 192, 0, 0, r"N = 193 is outside its limit 1 <= N <= 192.*solvers\.gp"),
    (4, (700, 69), 0, 0, r"l = 769 is outside its limit 1 <= l <= 768.*solvers\.gp"),
    (4, (5, 3), 8, 5, r"p = 5 is outside its limit 0 <= p <= n.*solvers\.gp")])
def test_limits(n, K, ml, p, text):
    rng = np.random.default_rng(0)
    l, B = sum(K), 2
    F, g = rng.standard_normal((B, l, n)), rng.standard_normal((l, B))
    G, h = (rng.standard_normal((B, ml, n)), rng.standard_normal((ml, B))) if ml else (None, None)
    A, b = (rng.standard_normal((B, p, n)), rng.standard_normal((p, B))) if p else (None, None)
    with pytest.raises(ValueError, match=text):
        solvers.gp_batch(list(K), F, g, G, h, A, b)
    with pytest.raises(ValueError, match=text):                       # shared matrices run into the same limits
        solvers.gp_batch(list(K), F[0], g, None if G is None else G[0], h, None if A is None else A[0], b)


def test_sizes_and_types():
    K, F, g, G, h, A, b = data()
    bad = [
        (((5, 3), F, g, G, h, A, b), "'K' must be a list of positive integers"),
        (([5, 0, 3], F, g, G, h, A, b), "'K' must be a list of positive integers"),
        (([5, 3.0], F, g, G, h, A, b), "'K' must be a list of positive integers"),
        (([], F, g, G, h, A, b), "'K' must be a list of positive integers"),
        (([5, 4], F, g, G, h, A, b), "'F' must be a dense or sparse 'd' matrix with 9 rows"),
        ((K, F.astype(np.float32), g, G, h, A, b), "'F' must be a dense or sparse 'd' matrix with 8 rows"),
        ((K, F, g[:7], G, h, A, b), "'g' must be a 'd' matrix with 8 rows, one column per member"),
        ((K, F[:2], g, G, h, A, b), "'F' has 2 members, 'g' has 3 columns"),
        ((K, F, g, G[:, :, :3], h, A, b), "'G' must be a dense or sparse 'd' matrix with 4 columns"),
        ((K, F, g, G[:2], h, A, b), "'G' has 2 members, 'g' has 3 columns"),
        ((K, F, g, G, h[:, :2], A, b), "'h' must have one column or B = 3 columns"),
        ((K, F, g, G, h[:5], A, b), r"'h' must be a dense 'd' matrix of size \(8,1\)"),
        ((K, F, g, G, None, A, b), r"'h' must be a dense 'd' matrix of size \(8,1\)"),
        ((K, F, g, None, h, A, b), r"'h' must be a dense 'd' matrix of size \(0,1\)"),
        ((K, F, g, G, h, A[:, :, :3], b), "'A' must be a dense or sparse 'd' matrix with 4 columns"),
        ((K, F, g, G, h, A, None), r"'b' must be a dense 'd' matrix of size \(1,1\)"),
        ((K, F, g, G, h, None, b), r"'b' must be a dense 'd' matrix of size \(0,1\)"),
    ]
    for args, text in bad:
        with pytest.raises(TypeError, match=text):
            solvers.gp_batch(*args)
    opt, sizes, parts_ = gpbatch._prepare(K, F, g, G, h, A, b, None)
    assert sizes == (3, 4, [5, 3], 8, 1) and [s for _, s in parts_] == [32, 8, 32, 8, 4, 1]
    _, sizes, parts_ = gpbatch._prepare(K, F[0], g, None, None, None, None, None)              # ml = 0 and p = 0: G, h, A, b absent
    assert sizes == (3, 4, [5, 3], 0, 0) and [(v is None, s) for v, s in parts_] == [(False, 0), (False, 8)] + [(True, 0)] * 4
    _, sizes, parts_ = gpbatch._prepare(K, F[0], g[:, :1], G[0], h[:, 0], A[0], b[:, 0], None)   # one member, everything shared
    assert sizes[0] == 1 and [s for _, s in parts_] == [0] * 6


def test_options():
    args = data()
    with pytest.raises(NotImplementedError, match=r"options\['refinement'\] = 1 is not carried, only 0 \(the default here\); "
                                                  r"solvers\.gp refines, once by default"):
        solvers.gp_batch(*args, options={"refinement": 1})
    assert gpbatch._prepare(*args, None)[0].refinement == 0                # absent: 0 here, whereas solvers.gp defaults to 1
    assert gpbatch._prepare(*args, {"refinement": 0, "show_progress": True})[0].refinement == 0
    for o, text in (({"maxiters": 0}, r"options\['maxiters'\] must be a positive integer"),
                    ({"abstol": "a"}, r"options\['abstol'\] must be a scalar"),
                    ({"reltol": -1.0, "abstol": 0.0}, r"at least one of options\['reltol'\] and options\['abstol'\] must be positive"),
                    ({"feastol": 0.0}, r"options\['feastol'\] must be a positive scalar"),
                    ({"refinement": -1}, r"options\['refinement'\] must be a nonnegative integer")):
        with pytest.raises(ValueError, match=text):
            solvers.gp_batch(*args, options=o)
    with pytest.raises(TypeError):
        solvers.gp_batch(*args, kktsolver="ldl")
    solvers.options["refinement"] = 2                                  # the module-level dict is not read
    try:
        assert gpbatch._prepare(*args, None)[0].refinement == 0
    finally:
        del solvers.options["refinement"]


def test_the_entry_is_public():
    assert hasattr(solvers, "gp_batch") and solvers.gp_batch is gpbatch.gp_batch and "gp_batch" in solvers.__doc__
    for text in ("solvers.gp defaults to 1", "cvx._cpl", "64 halvings", "no A'A repair", "objective row", "does not disturb"):
        assert text in gpbatch.__doc__, text


def test_good_arguments_reach_the_device_or_fail_loudly():
    """No fallback loop: without a device a call that passes every check raises, it does not compute."""
    args = data()
    if _lib.lib().kvx_device_count() > 0:
        assert solvers.gp_batch(*args)["status"] == ["optimal"] * 3
    else:
        with pytest.raises(RuntimeError, match="no HIP device"):
            solvers.gp_batch(*args)


def c_call(entry, B=3, n=4, K=(5, 3), mnl=None, ml=8, p=1, strides=(32, 8, 32, 8, 4, 1), null=(), maxiters=10, abstol=1e-7,
           reltol=1e-6, feastol=1e-7):
    """null: 0..5 the data F, g, G, h, A, b; 6..10 the results x, y, s, z, stats; 11, 12 iterations and exit; 13 K; 14 the scratch."""
    fn = getattr(_lib.lib(), entry)
    buf = np.zeros(1 << 20)
    ints = np.zeros(8, dtype=np.int64)
    dev = entry.endswith("_dev")
    D = (lambda a: a.ctypes.data) if dev else _lib.pd
    Di = (lambda a: a.ctypes.data) if dev else _lib.pi
    args = []
    for k, s in enumerate(strides):
        args += [None if k in null else D(buf), s]
    outs = [None if 6 + k in null else D(buf) for k in range(5)] + [None if 11 + k in null else Di(ints) for k in range(2)]
    if dev:
        outs.append(None if 14 in null else D(buf))
    Kv = np.asarray(K, dtype=np.int64)
    return fn(B, n, len(K) - 1 if mnl is None else mnl, None if 13 in null else _lib.pi(Kv), ml, p, *args, maxiters, abstol, reltol,
              feastol, *outs)


ENTRIES = ["kvx_gp_batch_solve", "kvx_gp_batch_solve_dev"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_c_entries_answer_einval_without_a_device(entry):
    refusals = [({"B": 0}, "1 <= B"), ({"n": 0}, "1 <= n <= 63"), ({"n": 64}, "1 <= n <= 63"), ({"mnl": -1}, "0 <= mnl"),
                ({"K": (1,) * 193, "ml": 0}, "N = mnl + 1 + ml <= 192"), ({"null": (13,)}, "block sizes K are NULL"),
                ({"K": (5, 0)}, "every block size"), ({"K": (5, -3)}, "every block size"), ({"K": (700, 69)}, "l = sum(K) <= 768"),
                ({"K": (769,)}, "l = sum(K) <= 768"), ({"ml": -1}, "ml >= 0"), ({"ml": 191}, "N = mnl + 1 + ml <= 192"),
                ({"p": -1}, "0 <= p <= n"), ({"p": 5}, "0 <= p <= n"),
                ({"strides": (31, 8, 32, 8, 4, 1)}, "stride of F"), ({"strides": (32, 7, 32, 8, 4, 1)}, "stride of g"),
                ({"strides": (32, 8, 31, 8, 4, 1)}, "stride of G"), ({"strides": (32, 8, 32, 7, 4, 1)}, "stride of h"),
                ({"strides": (32, 8, 32, 8, 3, 1)}, "stride of A"), ({"strides": (32, 8, 32, 8, 4, -1)}, "stride of b"),
                ({"null": (0,)}, "data pointer"), ({"null": (1,)}, "data pointer"), ({"null": (2,)}, "data pointer"),
                ({"null": (3,)}, "data pointer"), ({"null": (4,)}, "data pointer"), ({"null": (5,)}, "data pointer"),
                ({"null": (6,)}, "result pointer"), ({"null": (7,)}, "result pointer"), ({"null": (8,)}, "result pointer"),
                ({"null": (9,)}, "result pointer"), ({"null": (10,)}, "result pointer"), ({"null": (11,)}, "result pointer"),
                ({"null": (12,)}, "result pointer"), ({"maxiters": 0}, "maxiters"), ({"feastol": 0.0}, "feastol"),
                ({"abstol": 0.0, "reltol": -1.0}, "reltol and abstol"), ({"feastol": float("nan")}, "feastol")]
    if entry.endswith("_dev"):
        refusals.append(({"null": (14,)}, "scratch pointer is NULL"))
    for kw, text in refusals:
        assert c_call(entry, **kw) == _lib.KVX_EINVAL, kw
        assert entry in _lib.last_error() and text in _lib.last_error(), (kw, _lib.last_error())
    if _lib.lib().kvx_device_count() == 0:
        assert c_call(entry) == _lib.KVX_EDEVICE and "no CPU fallback" in _lib.last_error()
        assert c_call(entry, p=0, null=(4, 5, 7), strides=(0, 0, 0, 0, 0, 0)) == _lib.KVX_EDEVICE   # A, b, y may be NULL when p = 0
        assert c_call(entry, ml=0, null=(2, 3)) == _lib.KVX_EDEVICE                                # G, h may be NULL when ml = 0
        assert c_call(entry, K=(8,), ml=0, p=0, null=(2, 3, 4, 5, 7)) == _lib.KVX_EDEVICE          # mnl = 0: the objective alone


def test_the_scratch_of_a_member():
    f = _lib.lib().kvx_gp_batch_scratch_doubles
    assert f(64, 0, 0, 0) == f(0, 0, 0, 0) == f(4, -1, 0, 0) == f(4, 1, 191, 0) == f(4, 0, 0, 5) == -1
    assert f(1, 0, 0, 0) == 3 * 2 + 11 * 2 and f(63, 4, 187, 63) == 63 * 64 + 3 * 64 + 3 * 64 + 11 * 192


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_corners_of_the_box_pass_the_lds_check(entry):
    """The members of the box with the most LDS pass every check, the 160 KiB refusal among them: without a device they are refused
    for the missing device alone; with one the host entry runs them (all-zero data: the documented exit 3), and the _dev entry, which
    would take this test's host buffers for device memory, is not called."""
    device = _lib.lib().kvx_device_count() > 0
    if device and entry.endswith("_dev"):
        return
    for K, ml in (((768,), 191), ((577,) + (1,) * 191, 0), ((4,) * 192, 0), ((300, 200, 140, 64, 64), 187), ((1,) * 192, 0), ((384, 384), 190)):
        assert len(K) + ml == 192
        rc = c_call(entry, B=1, n=63, K=K, ml=ml, p=63, strides=(0, 0, 0, 0, 0, 0))
        assert rc == (_lib.KVX_OK if device else _lib.KVX_EDEVICE), (K, ml, _lib.last_error())
