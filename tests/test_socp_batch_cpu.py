"""The host side of solvers.socp_batch, without a device: the restatement of tests/socp_batch_numpy.py against the
reference's own runs at refinement 0 (G26) in status, iterations and x, y, s, z to 1e-8 relative; its 'q' operations against G15;
with dims['q'] = [] against tests/lp_batch_numpy.py on the same member; that float64 and numpy.longdouble agree in status, count
and exit for every member of every batch of tests/test_socp_batch_gpu.py and differ by at most 1e-2 of the bound the GPU results are
held to; the argument checks of socp_batch with their texts; and the KVX_EINVAL of both C entries.

Measured (this file's prints), largest relative distance of x, y, s, z to G26 in float64 / longdouble: doc_socp 4.1e-12 / 2.9e-12,
mixed_eq 4.4e-11 / 6.4e-11, socp_pinf 7.0e-15 / 2.0e-15, socp_dinf 1.1e-15 / 6.7e-16.  The reference eliminates the equality rows
by a QR factorisation (misc.kkt_chol), the restatement through X and K (misc.kkt_chol2): the same solution, other roundings."""
import json
import os

import numpy as np
import pytest

import lp_batch_numpy as LPN
import socp_batch_numpy as R
from kvxopt_amd import _lib, socpbatch, solvers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VECTORS = ("x", "y", "s", "z")
G26_CASES = ("doc_socp", "mixed_eq", "socp_pinf", "socp_dinf")


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def vec_err(got, ref):
    """|got - ref| in units of the bound 1e-6 max(|ref|, 1) the GPU results are held to."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - ref) / (1e-6 * max(np.linalg.norm(ref), 1.0)))


def g26_case(name):
    meta = json.load(open(os.path.join(GOLDEN, "g26_socp_batch.json")))["cases"][name]
    g = np.load(os.path.join(GOLDEN, "g26_socp_batch.npz"))
    get = lambda k: g["%s__%s" % (name, k)] if "%s__%s" % (name, k) in g else None         # noqa: E731
    return meta, (get("c"), get("G"), get("h"), meta["dims"], get("A"), get("b")), {k: get("sol_" + k) for k in VECTORS}


@pytest.mark.parametrize("precision", ["float64", "longdouble"])
@pytest.mark.parametrize("name", G26_CASES)
def test_restatement_reproduces_the_reference_at_refinement_0(name, precision):
    meta, data, sol = g26_case(name)
    r = R.solve_member(*data, dtype=getattr(np, precision))
    assert r.status == meta["status"] and r.iterations == meta["iterations"] and r.exit == R.EXITS[meta["status"]]
    errs = {k: rel(getattr(r, k), sol[k]) for k in VECTORS if sol[k] is not None and sol[k].size}
    print("%s in %s: relative distance to G26: %s" % (name, precision, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) < 1e-8
    if meta["status"] == "optimal":
        assert abs(r.stats[2] - meta["primal objective"]) < 1e-8 * max(abs(meta["primal objective"]), 1.0)
        assert r.stats[6] > 0 and r.stats[7] > 0
    elif meta["status"] == "primal infeasible":
        assert np.isnan(r.x).all() and np.isnan(r.s).all() and r.stats[3] == 1.0 and r.stats[7] > 0
    else:
        assert np.isnan(r.z).all() and r.stats[2] == -1.0 and r.stats[6] > 0


def test_g26_records_the_count_of_doc_socp_at_both_refinements():
    meta = json.load(open(os.path.join(GOLDEN, "g26_socp_batch.json")))
    g19 = json.load(open(os.path.join(GOLDEN, "g19_cone_programs.json")))["cases"]["doc_socp"]["iterations"]
    assert meta["doc_socp iterations at refinement 1 (G19)"] == g19 == 9
    assert meta["cases"]["doc_socp"]["iterations"] == 9                   # the same count as with the reference's default refinement


def test_q_operations_reproduce_g15():
    """dims = {'l': 4, 'q': [5, 1, 9]} without (a) and with (b, 3 more 'l' rows) an offset, as tests/test_oracle.py reads G15."""
    g = np.load(os.path.join(GOLDEN, "g15_q_cone_scaling.npz"))
    for tag, k in (("a", 0), ("b", 3)):
        ind, iv = k + 4, 0
        for bidx, m in enumerate((5, 1, 9)):
            sl = slice(ind, ind + m)
            v, beta, lm = R.compute_scaling_q(g[tag + "_s"][sl].copy(), g[tag + "_z"][sl].copy())
            assert rel(v, g[tag + "_v"][iv:iv + m]) < 1e-12 and rel(lm, g[tag + "_lmbda"][sl]) < 1e-12
            assert abs(beta - g[tag + "_beta"][bidx]) < 1e-12 * beta
            for inv in "NI":
                assert rel(R.scale_q(g[tag + "_X"][sl], v, beta, inv == "I"), g["%s_scale_N%s" % (tag, inv)][sl]) < 1e-12   # both columns
            x1, y1, lmk = g[tag + "_x1"][sl], g[tag + "_y1"][sl], g[tag + "_lmbda"][sl]
            assert rel(R.sprod_q(x1, y1), g[tag + "_sprod"][sl]) < 1e-12
            assert rel(R.scale2_q(lmk, x1), g[tag + "_scale2_N"][sl]) < 1e-12
            assert rel(R.scale2_q(lmk, x1, True), g[tag + "_scale2_I"][sl]) < 1e-12
            assert rel(R.sinv_q(x1, y1), g[tag + "_sinv"][sl]) < 1e-12
            us = R.update_scaling_q(g[tag + "_v"][iv:iv + m], g[tag + "_beta"][bidx], g[tag + "_us_s_in"][sl], g[tag + "_us_z_in"][sl])
            for got, name, lo in zip(us, ("us_s", "us_z", "us_v", "us_beta", "us_lmbda"), (ind, ind, iv, None, ind)):
                want = g[tag + "_" + name][bidx] if lo is None else g[tag + "_" + name][lo:lo + m]
                assert rel(got, want) < 1e-12, name
            ind += m
            iv += m
        x1 = g[tag + "_x1"]
        t = max([float(np.max(-x1[:k + 4]))] + [float(R.max_step_q(x1[o:o + m])) for o, m in ((k + 4, 5), (k + 9, 1), (k + 10, 9))])
        assert abs(t - float(g[tag + "_max_step"])) < 1e-12


@pytest.mark.parametrize("precision", ["float64", "longdouble"])
def test_without_cones_the_restatement_is_the_one_of_lp_batch(precision):
    M = R.batch("orthant")
    dt = getattr(np, precision)
    for k in range(M.B):
        c, G, h, dims, A, b = R.member(M, k)
        r, q = R.solve_member(c, G, h, dims, A, b, None, dt), LPN.solve_member(c, G, h, A, b, None, dt)
        assert (r.status, r.iterations, r.exit) == (q.status, q.iterations, q.exit)
        for v in VECTORS:
            assert np.array_equal(getattr(r, v), getattr(q, v)), v
        assert r.stats == q.stats


def agree(a, b):
    """Statuses, counts and exits of two runs agree; the largest distance of their vectors in units of the GPU's bound."""
    assert [(r.status, r.iterations, r.exit) for r in a] == [(r.status, r.iterations, r.exit) for r in b]
    worst = 0.0
    for u, w in zip(a, b):
        for v in VECTORS:
            x, y = np.asarray(getattr(u, v), float), np.asarray(getattr(w, v), float)
            assert np.array_equal(np.isnan(x), np.isnan(y))
            if y.size and not np.isnan(y).any():
                worst = max(worst, vec_err(x, y))
    return worst


@pytest.mark.parametrize("name", R.SMALL_BATCHES)
def test_float64_and_longdouble_agree_on_every_member(name):
    a, b = R.restated(name, "float64"), R.restated(name)
    worst = agree(a, b)
    M = R.batch(name)
    print("%s: (exit, iterations) %s, float64 within %.2e of the GPU's bound of longdouble" % (name, [(r.exit, r.iterations) for r in b], worst))
    assert worst <= 1e-2
    want = {R.FEASIBLE: "optimal", R.PRIMAL_INFEASIBLE: "primal infeasible", R.DUAL_INFEASIBLE: "dual infeasible"}
    assert [r.status for r in b] == [want[k] for k in M.kind]
    free = R.BATCHES[name][4]
    assert all(r.singular == bool(free) for r in a) and all(r.singular == bool(free) for r in b)


def test_the_mixed_batch_ends_in_every_way_at_its_median_count():
    M = R.batch("mixed")
    m = int(np.median([r.iterations for r in R.restated("mixed")]))
    a, b = R.restate(M, {"maxiters": m}, np.float64), R.restate(M, {"maxiters": m}, np.longdouble)
    assert agree(a, b) <= 1e-2
    kept = [r.exit for k, r in enumerate(b) if k not in R.MIXED_CHANGED]
    assert set(kept) == {0, 1, 4, 5}, kept
    assert all(M.kind[k] == R.FEASIBLE for k in R.MIXED_CHANGED)


@pytest.mark.parametrize("part", range(4))
def test_float64_and_longdouble_agree_on_the_independence_batch(part):
    M, B = R.batch("independence"), R.BATCHES["independence"][1]
    which = range(part * B // 4, (part + 1) * B // 4)
    a, b = R.restate(M, None, np.float64, which), R.restate(M, None, np.longdouble, which)
    assert agree(a, b) <= 1e-2
    assert len(set(r.iterations for r in b)) >= 2 and set(r.status for r in b) == {"optimal"}


# ---- argument checks: all of them before a device is asked for
def data(n=4, ml=2, q=(3, 2), p=2, B=3, seed=0):
    M = R.members(n, ml, q, p, B, seed)
    return M.c, M.G, M.h, M.dims, M.A, M.b


@pytest.mark.parametrize("n,ml,q,p,text", [
    (65, 70, (3,), 0, r"n = 65 is outside its limit 1 <= n <= 64.*solvers\.socp"),
    (4, 510, (3,), 0, r"N = 513 is outside its limit 1 <= N <= 512.*solvers\.socp"),
    (4, 0, (1,) * 129, 0, r"nq = 129 is outside its limit 0 <= nq <= 128.*solvers\.socp"),
    (4, 2, (3, 2), 5, r"p = 5 is outside its limit 0 <= p <= n.*solvers\.socp"),
    (8, 2, (3,), 2, r"p \+ N = 7 is outside its limit p \+ N >= n = 8.*solvers\.socp")])
def test_limits(n, ml, q, p, text):
    c, G, h, dims, A, b = data(n, ml, q, p)
    with pytest.raises(ValueError, match=text):
        solvers.socp_batch(c, G, h, dims, A, b)
    with pytest.raises(ValueError, match=text):                       # shared matrices run into the same limits
        solvers.socp_batch(c, G[0], h, dims, None if A is None else A[0], b)


def test_dims():
    c, G, h, dims, A, b = data()
    with pytest.raises(ValueError, match=r"dims\['s'\] = \[2\] is outside its limit, absent or empty"):
        solvers.socp_batch(c, G, h, {"l": 2, "q": [3, 2], "s": [2]}, A, b)
    with pytest.raises(TypeError, match=r"'dims\['q'\]' must be a list of positive integers"):
        solvers.socp_batch(c, G, h, {"l": 2, "q": [3, 0]}, A, b)
    with pytest.raises(TypeError, match=r"'dims\['l'\]' must be a nonnegative integer"):
        solvers.socp_batch(c, G, h, {"l": -1, "q": [3, 2]}, A, b)
    with pytest.raises(TypeError, match="'dims' must be a dictionary"):
        solvers.socp_batch(c, G, h, None, A, b)
    with pytest.raises(ValueError, match="N = 0 is outside its limit 1 <= N <= 512"):
        solvers.socp_batch(c, np.zeros((0, 4)), np.zeros(0), {"l": 0, "q": []})
    with pytest.raises(TypeError, match=r"'G' must be a 'd' matrix of size \(8, 4\)"):
        solvers.socp_batch(c, G, h, {"l": 3, "q": [3, 2]}, A, b)
    opt, sizes, parts = socpbatch._prepare(c, G, h, {"l": 2, "q": [3, 2], "s": []}, A, b, None)       # 's' empty: accepted
    assert sizes == (3, 4, 2, [3, 2], 7, 2) and [s for _, s in parts] == [4, 28, 7, 8, 2]


def test_sizes_and_types():
    c, G, h, dims, A, b = data()
    bad = [
        ((c, G[:2], h, dims, A, b), "'G' has 2 members, 'c' has 3 columns"),
        ((c, G, h[:, :2], dims, A, b), "'h' must have one column or B = 3 columns"),
        ((c, G, h[:5], dims, A, b), r"'h' must be a 'd' matrix of size \(7,1\)"),
        ((c, G, h, dims, A[:, :, :3], b), "'A' must be a 'd' matrix with 4 columns"),
        ((c, G, h, dims, A, None), "'b' must have length 2"),
        ((c, G, h, dims, None, b), "'b' must have length 0"),
        ((c, G.astype(np.float32), h, dims, A, b), r"'G' must be one matrix or a float64 array of shape \(B, rows, 4\)"),
    ]
    for args, text in bad:
        with pytest.raises(TypeError, match=text):
            solvers.socp_batch(*args)


def test_options():
    args = data()
    with pytest.raises(NotImplementedError, match=r"options\['refinement'\] = 1 is not carried.*solvers\.socp refines"):
        solvers.socp_batch(*args, options={"refinement": 1})
    opt, _, _ = socpbatch._prepare(*args, None)
    assert opt.refinement == 0                                         # absent: 0 here, whereas solvers.socp defaults to 1
    assert socpbatch._prepare(*args, {"refinement": 0, "show_progress": True})[0].refinement == 0
    for o, text in (({"maxiters": 0}, r"options\['maxiters'\] must be a positive integer"),
                    ({"abstol": "a"}, r"options\['abstol'\] must be a scalar"),
                    ({"reltol": -1.0, "abstol": 0.0}, r"at least one of options\['reltol'\] and options\['abstol'\] must be positive"),
                    ({"feastol": 0.0}, r"options\['feastol'\] must be a positive scalar"),
                    ({"refinement": -1}, r"options\['refinement'\] must be a nonnegative integer")):
        with pytest.raises(ValueError, match=text):
            solvers.socp_batch(*args, options=o)
    for kw in ({"primalstart": {}}, {"dualstart": {}}, {"kktsolver": "chol"}, {"solver": "mosek"}):
        with pytest.raises(TypeError):
            solvers.socp_batch(*args, **kw)
    solvers.options["refinement"] = 2                                  # the module-level dict is not read
    try:
        assert socpbatch._prepare(*args, None)[0].refinement == 0
    finally:
        del solvers.options["refinement"]


def test_the_entry_is_public():
    assert hasattr(solvers, "socp_batch") and solvers.socp_batch is socpbatch.socp_batch and "socp_batch" in solvers.__doc__
    for text in ("certificate", "solvers.socp defaults to 1", "_ipm.conelp_start", "max_step"):
        assert text in socpbatch.__doc__


def test_good_arguments_reach_the_device_or_fail_loudly():
    """No fallback loop: without a device a call that passes every check raises, it does not compute."""
    args = data()
    if _lib.lib().kvx_device_count() > 0:
        assert solvers.socp_batch(*args)["status"] == ["optimal"] * 3
    else:
        with pytest.raises(RuntimeError, match="no HIP device"):
            solvers.socp_batch(*args)


@pytest.mark.parametrize("entry", ["kvx_socp_batch_solve", "kvx_socp_batch_solve_dev"])
def test_c_entries_answer_einval_without_a_device(entry):
    fn = getattr(_lib.lib(), entry)
    n, ml, p, B = 4, 2, 2, 3
    buf = np.zeros(4096)
    ints = np.zeros(8, dtype=np.int64)
    dev = entry.endswith("_dev")
    D = (lambda a: a.ctypes.data) if dev else _lib.pd
    Di = (lambda a: a.ctypes.data) if dev else _lib.pi

    def call(B=B, n=n, ml=ml, q=(3, 2), nq=None, p=p, strides=(4, 28, 7, 8, 2), null=(), maxiters=10, abstol=1e-7, reltol=1e-6,
             feastol=1e-7):
        data = []
        for k, s in enumerate(strides):
            data += [None if k in null else D(buf), s]
        outs = [None if 5 + k in null else D(buf) for k in range(5)] + [None if 10 + k in null else Di(ints) for k in range(2)]
        qv = np.asarray(q, dtype=np.int64)
        return fn(B, n, ml, len(q) if nq is None else nq, None if 12 in null or not len(q) else _lib.pi(qv), p, *data, maxiters, abstol,
                  reltol, feastol, *outs)

    for kw, text in (({"B": 0}, "1 <= B"), ({"n": 0}, "1 <= n <= 64"), ({"n": 65}, "1 <= n <= 64"), ({"ml": -1}, "0 <= ml <= 512"),
                     ({"ml": 513}, "0 <= ml <= 512"), ({"nq": -1}, "0 <= nq <= 128"), ({"q": (1,) * 129}, "0 <= nq <= 128"),
                     ({"null": (12,)}, "cone orders q are NULL"), ({"q": (3, 0)}, "every cone order"), ({"q": (3, 513)}, "every cone order"),
                     ({"ml": 508}, "1 <= N = ml + sum(q) <= 512"), ({"ml": 0, "q": ()}, "1 <= N = ml + sum(q) <= 512"),
                     ({"p": -1}, "0 <= p <= n"), ({"p": 5}, "0 <= p <= n"), ({"n": 10, "p": 2}, "p + N >= n"),
                     ({"strides": (3, 28, 7, 8, 2)}, "stride of c"), ({"strides": (4, 27, 7, 8, 2)}, "stride of G"),
                     ({"strides": (4, 28, 6, 8, 2)}, "stride of h"), ({"strides": (4, 28, 7, 8, 1)}, "stride of b"),
                     ({"strides": (4, 28, 7, -8, 2)}, "stride of A"),
                     ({"null": (0,)}, "data pointer"), ({"null": (2,)}, "data pointer"), ({"null": (3,)}, "data pointer"),
                     ({"null": (5,)}, "result pointer"), ({"null": (6,)}, "result pointer"), ({"null": (9,)}, "result pointer"),
                     ({"null": (11,)}, "result pointer"), ({"maxiters": 0}, "maxiters"), ({"feastol": 0.0}, "feastol"),
                     ({"abstol": 0.0, "reltol": -1.0}, "reltol and abstol"), ({"feastol": float("nan")}, "feastol")):
        assert call(**kw) == _lib.KVX_EINVAL, kw
        assert entry in _lib.last_error() and text in _lib.last_error(), (kw, _lib.last_error())
    if _lib.lib().kvx_device_count() == 0:
        assert call() == _lib.KVX_EDEVICE and "no CPU fallback" in _lib.last_error()
        assert call(p=0, null=(3, 4, 6), strides=(0, 0, 0, 0, 0)) == _lib.KVX_EDEVICE        # A, b, y may be NULL when p = 0
        assert call(ml=7, q=(), strides=(4, 28, 7, 8, 2)) == _lib.KVX_EDEVICE                # no cones: q may be NULL
