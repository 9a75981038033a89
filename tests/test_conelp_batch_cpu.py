"""The host side of solvers.conelp_batch, without a device: the restatement of tests/conelp_batch_numpy.py against
the reference's own runs at refinement 0 (G28) in status, iterations and x, y, s, z to 1e-8 relative; with dims['s'] = [] against
tests/socp_batch_numpy.py, with dims['q'] = [] against tests/sdp_batch_numpy.py and with both empty against tests/lp_batch_numpy.py
on the same members, bit for bit; that float64 and numpy.longdouble agree in status, count and exit for every member of every batch
of tests/test_conelp_batch_gpu.py and differ by at most 1e-2 of the bound the GPU results are held to; the argument checks of
conelp_batch with their texts; and the KVX_EINVAL of both C entries.

Measured (this file's prints), largest relative distance of x, y, s, z to G28 in float64 / longdouble: doc_conelp 8.3e-13 / 1.1e-11,
doc_conelp_lower the same, mixed_eq 4.3e-11 / 3.9e-11, conelp_pinf 2.1e-14 / 2.2e-14, conelp_dinf 3.3e-15 / 5.1e-15.  The reference
eliminates the equality rows by a QR factorisation (misc.kkt_chol) and takes its singular and eigenvalues from LAPACK, the
restatement eliminates through X and K (misc.kkt_chol2) and iterates by Jacobi: the same solution, other roundings.

The LDS refusal of the C entries is a backstop that no member of the limits reaches: the largest one needs 152640 bytes.
What is tested is that the largest members found pass it, in test_the_largest_members_pass_the_lds_check."""
import json
import os

import numpy as np
import pytest

import conelp_batch_numpy as R
import lp_batch_numpy as LPN
import sdp_batch_numpy as SDN
import socp_batch_numpy as SON
from kvxopt_amd import _lib, conelpbatch, solvers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VECTORS = ("x", "y", "s", "z")
G28_CASES = ("doc_conelp", "doc_conelp_lower", "mixed_eq", "conelp_pinf", "conelp_dinf")


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def vec_err(got, ref):
    """|got - ref| in units of the bound 1e-6 max(|ref|, 1) the GPU results are held to."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - ref) / (1e-6 * max(np.linalg.norm(ref), 1.0)))


def g28_case(name):
    meta = json.load(open(os.path.join(GOLDEN, "g28_conelp_batch.json")))["cases"][name]
    g = np.load(os.path.join(GOLDEN, "g28_conelp_batch.npz"))
    get = lambda k: g["%s__%s" % (name, k)] if "%s__%s" % (name, k) in g else None         # noqa: E731
    return meta, (get("c"), get("G"), get("h"), meta["dims"], get("A"), get("b")), {k: get("sol_" + k) for k in VECTORS}


@pytest.mark.parametrize("precision", ["float64", "longdouble"])
@pytest.mark.parametrize("name", G28_CASES)
def test_restatement_reproduces_the_reference_at_refinement_0(name, precision):
    meta, data, sol = g28_case(name)
    r = R.solve_member(*data, dtype=getattr(np, precision))
    assert r.status == meta["status"] and r.iterations == meta["iterations"] and r.exit == R.EXITS[meta["status"]]
    errs = {k: rel(getattr(r, k), sol[k]) for k in VECTORS if sol[k] is not None and sol[k].size}
    print("%s in %s: relative distance to G28: %s" % (name, precision, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) < 1e-8
    if meta["status"] == "optimal":
        assert abs(r.stats[2] - meta["primal objective"]) < 1e-8 * max(abs(meta["primal objective"]), 1.0)
        assert r.stats[6] > 0 and r.stats[7] > 0
    elif meta["status"] == "primal infeasible":
        assert np.isnan(r.x).all() and np.isnan(r.s).all() and r.stats[3] == 1.0 and r.stats[7] > 0
    else:
        assert np.isnan(r.z).all() and r.stats[2] == -1.0 and r.stats[6] > 0


def test_g28_holds_the_doc_example_twice_and_every_status_on_all_three_kinds():
    (ma, a, sa), (_, b, sb) = g28_case("doc_conelp"), g28_case("doc_conelp_lower")
    assert ma["dims"] == {"l": 2, "q": [4, 4], "s": [3]}
    assert not np.array_equal(a[1], b[1]) and not np.array_equal(a[2], b[2])
    assert np.array_equal(SDN.symmetrise(b[1].copy(), 10, [3]), a[1]) and np.array_equal(SDN.symmetrise(b[2].copy(), 10, [3]), a[2])
    assert np.abs(b[1]).max() > 900 and all(np.array_equal(sa[k], sb[k]) for k in VECTORS if sa[k] is not None)
    metas = {name: g28_case(name)[0] for name in G28_CASES}
    assert metas["mixed_eq"]["dims"] == {"l": 4, "q": [3, 4], "s": [3, 2]} and g28_case("mixed_eq")[1][4].shape[0] == 2
    assert metas["conelp_pinf"]["status"] == "primal infeasible" and metas["conelp_dinf"]["status"] == "dual infeasible"
    assert all(m["dims"]["l"] and m["dims"]["q"] and m["dims"]["s"] for m in metas.values())


def same_to_the_bit(r, q):
    assert (r.status, r.iterations, r.exit, r.singular) == (q.status, q.iterations, q.exit, q.singular)
    for v in VECTORS:
        assert np.array_equal(getattr(r, v), getattr(q, v), equal_nan=True), v
    assert np.array_equal(np.array(r.stats), np.array(q.stats), equal_nan=True)


@pytest.mark.parametrize("precision", ["float64", "longdouble"])
@pytest.mark.parametrize("name", ["shape-8-5-q1_2_7-3", "certificates-8", "free"])
def test_without_blocks_the_restatement_is_the_one_of_socp_batch(name, precision):
    M, dt = SON.batch(name), getattr(np, precision)
    assert M.dims["q"] and not M.dims["s"]
    for k in range(M.B):
        same_to_the_bit(R.solve_member(*SON.member(M, k), None, dt), SON.solve_member(*SON.member(M, k), None, dt))


@pytest.mark.parametrize("precision", ["float64", "longdouble"])
@pytest.mark.parametrize("name", ["shape-6-2-s1_2_3-2", "certificates-6", "free"])
def test_without_cones_the_restatement_is_the_one_of_sdp_batch(name, precision):
    M, dt = SDN.batch(name), getattr(np, precision)
    assert M.dims["s"] and not M.dims["q"]
    for k in range(M.B):
        same_to_the_bit(R.solve_member(*SDN.member(M, k), None, dt), SDN.solve_member(*SDN.member(M, k), None, dt))


@pytest.mark.parametrize("precision", ["float64", "longdouble"])
@pytest.mark.parametrize("name", ["shape-8-17-3", "certificates-8-17-3", "free-8-17-3"])
def test_without_cones_and_blocks_the_restatement_is_the_one_of_lp_batch(name, precision):
    M, dt = LPN.batch(name), getattr(np, precision)
    dims = {"l": M.ml, "q": [], "s": []}
    for k in range(M.B):
        c, G, h, A, b = LPN.member(M, k)
        same_to_the_bit(R.solve_member(c, G, h, dims, A, b, None, dt), LPN.solve_member(c, G, h, A, b, None, dt))


def test_the_generator_draws_what_its_siblings_draw_when_a_kind_is_absent():
    a, b = SON.members(8, 5, (1, 2, 7), 3, 6, 99, SON.THIRDS, 0), R.members(8, 5, (1, 2, 7), (), 3, 6, 99, R.THIRDS, 0)
    assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("c", "G", "h", "A", "b"))
    a, b = SDN.members(6, 2, (1, 2, 3), 2, 6, 98, SDN.THIRDS, 0), R.members(6, 2, (), (1, 2, 3), 2, 6, 98, R.THIRDS, 0)
    assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("c", "G", "h", "A", "b"))


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


def test_the_batches_have_the_shapes_they_are_to_show():
    n, ml, q, s, p = R.CORNER
    assert (n, p, max(s), ml + sum(q) + sum(m * m for m in s)) == (64, 64, 16, 384) and max(q) > 64
    for name in R.SMALL_BATCHES:
        if not name.startswith("absent"):
            M = R.batch(name)
            assert M.q and M.s, name                      # every batch but the three on purpose has both kinds
    assert R.batch("certificates").dims == R.batch("free").dims == R.batch("mixed").dims == {"l": 3, "q": [4], "s": [3]}


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
def data(n=4, ml=2, q=(3,), s=(2, 1), p=2, B=3, seed=0):
    M = R.members(n, ml, q, s, p, B, seed)
    return M.c, M.G, M.h, M.dims, M.A, M.b


@pytest.mark.parametrize("n,ml,q,s,p,text", [
    (65, 70, (3,), (3,), 0, r"n = 65 is outside its limit 1 <= n <= 64.*solvers\.conelp"),
    (4, 373, (3,), (3,), 0, r"N = 385 is outside its limit 1 <= N <= 384.*solvers\.conelp solves one problem"),
    (4, 382, (3,), (), 0, r"N = 385 is outside its limit 1 <= N <= 384; solvers\.socp_batch solves batches without 's' blocks.*solvers\.conelp"),
    (4, 0, (1,) * 129, (2,), 0, r"nq = 129 is outside its limit 0 <= nq <= 128.*solvers\.conelp"),
    (4, 0, (2,), (1,) * 33, 0, r"ns = 33 is outside its limit 0 <= ns <= 32.*solvers\.conelp"),
    (4, 2, (2,), (17,), 0, r"m_k = 17 is outside its limit 1 <= m_k <= 16.*solvers\.conelp"),
    (4, 2, (3,), (2, 1), 5, r"p = 5 is outside its limit 0 <= p <= n.*solvers\.conelp"),
    # the packed dimension counts, not N: N = 1 + 2 + 9 = 12 >= 10, but 1 + 2 + 6 + p = 9 < 10 (coneprog.py:512, 572)
    (10, 1, (2,), (3,), 0, r"p \+ ml \+ sum\(q_k\) \+ sum\(m_k \(m_k \+ 1\) / 2\) = 9 is outside its limit, at least n = 10.*solvers\.conelp")])
def test_limits(n, ml, q, s, p, text):
    c, G, h, dims, A, b = data(n, ml, q, s, p)
    with pytest.raises(ValueError, match=text):
        solvers.conelp_batch(c, G, h, dims, A, b)
    with pytest.raises(ValueError, match=text):                       # shared matrices run into the same limits
        solvers.conelp_batch(c, G[0], h, dims, None if A is None else A[0], b)


def test_dims():
    c, G, h, dims, A, b = data()
    with pytest.raises(TypeError, match=r"'dims\['s'\]' must be a list of nonnegative integers"):
        solvers.conelp_batch(c, G, h, {"l": 2, "q": [3], "s": [2, -1]}, A, b)
    with pytest.raises(TypeError, match=r"'dims\['q'\]' must be a list of positive integers"):
        solvers.conelp_batch(c, G, h, {"l": 2, "q": [3, 0], "s": [2, 1]}, A, b)
    with pytest.raises(ValueError, match=r"m_k = 0 is outside its limit 1 <= m_k <= 16"):
        solvers.conelp_batch(c, G, h, {"l": 2, "q": [3], "s": [2, 1, 0]}, A, b)
    with pytest.raises(TypeError, match=r"'dims\['l'\]' must be a nonnegative integer"):
        solvers.conelp_batch(c, G, h, {"l": -1, "q": [3], "s": [2, 1]}, A, b)
    with pytest.raises(TypeError, match="'dims' must be a dictionary"):
        solvers.conelp_batch(c, G, h, None, A, b)
    with pytest.raises(ValueError, match="N = 0 is outside its limit 1 <= N <= 384"):
        solvers.conelp_batch(c, np.zeros((0, 4)), np.zeros(0), {"l": 0, "q": [], "s": []})
    with pytest.raises(TypeError, match=r"'G' must be a 'd' matrix of size \(11, 4\)"):
        solvers.conelp_batch(c, G, h, {"l": 3, "q": [3], "s": [2, 1]}, A, b)
    opt, sizes, parts = conelpbatch._prepare(c, G, h, dims, A, b, None)
    assert sizes == (3, 4, 2, [3], [2, 1], 10, 2) and [s for _, s in parts] == [4, 40, 10, 8, 2]
    for d in ({"l": 10}, {"l": 5, "q": [5]}, {"l": 1, "s": [3]}):         # absent kinds are empty: the same kernel takes them
        assert conelpbatch._prepare(c, G, h, d, A, b, None)[1][5] == 10


def test_sizes_and_types():
    c, G, h, dims, A, b = data()
    bad = [
        ((c, G[:2], h, dims, A, b), "'G' has 2 members, 'c' has 3 columns"),
        ((c, G, h[:, :2], dims, A, b), "'h' must have one column or B = 3 columns"),
        ((c, G, h[:5], dims, A, b), r"'h' must be a 'd' matrix of size \(10,1\)"),
        ((c, G, h, dims, A[:, :, :3], b), "'A' must be a 'd' matrix with 4 columns"),
        ((c, G, h, dims, A, None), "'b' must have length 2"),
        ((c, G, h, dims, None, b), "'b' must have length 0"),
        ((c, G.astype(np.float32), h, dims, A, b), r"'G' must be one matrix or a float64 array of shape \(B, rows, 4\)"),
    ]
    for args, text in bad:
        with pytest.raises(TypeError, match=text):
            solvers.conelp_batch(*args)


def test_options():
    args = data()
    with pytest.raises(NotImplementedError, match=r"options\['refinement'\] = 1 is not carried, only 0 \(the default here\); "
                                                  r"solvers\.conelp refines, once by default"):
        solvers.conelp_batch(*args, options={"refinement": 1})
    opt, _, _ = conelpbatch._prepare(*args, None)
    assert opt.refinement == 0                                         # absent: 0 here, whereas solvers.conelp defaults to 1
    assert conelpbatch._prepare(*args, {"refinement": 0, "show_progress": True})[0].refinement == 0
    for o, text in (({"maxiters": 0}, r"options\['maxiters'\] must be a positive integer"),
                    ({"abstol": "a"}, r"options\['abstol'\] must be a scalar"),
                    ({"reltol": -1.0, "abstol": 0.0}, r"at least one of options\['reltol'\] and options\['abstol'\] must be positive"),
                    ({"feastol": 0.0}, r"options\['feastol'\] must be a positive scalar"),
                    ({"refinement": -1}, r"options\['refinement'\] must be a nonnegative integer")):
        with pytest.raises(ValueError, match=text):
            solvers.conelp_batch(*args, options=o)
    for kw in ({"primalstart": {}}, {"dualstart": {}}, {"kktsolver": "chol"}, {"solver": "mosek"}):
        with pytest.raises(TypeError):
            solvers.conelp_batch(*args, **kw)
    solvers.options["refinement"] = 2                                  # the module-level dict is not read
    try:
        assert conelpbatch._prepare(*args, None)[0].refinement == 0
    finally:
        del solvers.options["refinement"]


def test_the_entry_is_public():
    assert hasattr(solvers, "conelp_batch") and solvers.conelp_batch is conelpbatch.conelp_batch and "conelp_batch" in solvers.__doc__
    for text in ("certificate", "solvers.conelp defaults to 1", "_ipm.conelp_start", "max_step", "lower triangle",
                 "lp_batch, socp_batch and sdp_batch are the faster entries"):
        assert text in conelpbatch.__doc__


def test_good_arguments_reach_the_device_or_fail_loudly():
    """No fallback loop: without a device a call that passes every check raises, it does not compute."""
    args = data()
    if _lib.lib().kvx_device_count() > 0:
        assert solvers.conelp_batch(*args)["status"] == ["optimal"] * 3
    else:
        with pytest.raises(RuntimeError, match="no HIP device"):
            solvers.conelp_batch(*args)


def c_call(entry, B=3, n=4, ml=2, q=(3,), nq=None, m=(2, 1), ns=None, p=2, strides=(4, 40, 10, 8, 2), null=(), maxiters=10, abstol=1e-7,
           reltol=1e-6, feastol=1e-7):
    fn = getattr(_lib.lib(), entry)
    buf = np.zeros(65536)
    ints = np.zeros(8, dtype=np.int64)
    dev = entry.endswith("_dev")
    D = (lambda a: a.ctypes.data) if dev else _lib.pd
    Di = (lambda a: a.ctypes.data) if dev else _lib.pi
    data = []
    for k, s in enumerate(strides):
        data += [None if k in null else D(buf), s]
    outs = [None if 5 + k in null else D(buf) for k in range(5)] + [None if 10 + k in null else Di(ints) for k in range(2)]
    qv, mv = np.asarray(q, dtype=np.int64), np.asarray(m, dtype=np.int64)
    return fn(B, n, ml, len(q) if nq is None else nq, None if 12 in null or not len(q) else _lib.pi(qv), len(m) if ns is None else ns,
              None if 13 in null or not len(m) else _lib.pi(mv), p, *data, maxiters, abstol, reltol, feastol, *outs)


ENTRIES = ["kvx_conelp_batch_solve", "kvx_conelp_batch_solve_dev"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_c_entries_answer_einval_without_a_device(entry):
    for kw, text in (({"B": 0}, "1 <= B"), ({"n": 0}, "1 <= n <= 64"), ({"n": 65}, "1 <= n <= 64"), ({"ml": -1}, "0 <= ml <= 384"),
                     ({"ml": 385}, "0 <= ml <= 384"), ({"nq": -1}, "0 <= nq <= 128"), ({"q": (1,) * 129}, "0 <= nq <= 128"),
                     ({"null": (12,)}, "cone orders q are NULL"), ({"q": (3, 0)}, "every cone order"), ({"q": (385,)}, "every cone order"),
                     ({"ns": -1}, "0 <= ns <= 32"), ({"m": (1,) * 33}, "0 <= ns <= 32"),
                     ({"null": (13,)}, "block orders m are NULL"), ({"m": (2, 0)}, "every block order"), ({"m": (2, 17)}, "every block order"),
                     ({"ml": 377}, "1 <= N = ml + sum(q) + sum(m^2) <= 384"), ({"ml": 0, "q": (), "m": ()}, "1 <= N = ml + sum(q) + sum(m^2) <= 384"),
                     ({"p": -1}, "0 <= p <= n"), ({"p": 5}, "0 <= p <= n"),
                     ({"n": 10, "ml": 1, "q": (2,), "m": (3,), "p": 0, "strides": (10, 120, 12, 0, 0)},
                      "p + ml + sum(q) + sum(m (m + 1) / 2) >= n"),
                     ({"strides": (3, 40, 10, 8, 2)}, "stride of c"), ({"strides": (4, 39, 10, 8, 2)}, "stride of G"),
                     ({"strides": (4, 40, 9, 8, 2)}, "stride of h"), ({"strides": (4, 40, 10, 8, 1)}, "stride of b"),
                     ({"strides": (4, 40, 10, -8, 2)}, "stride of A"),
                     ({"null": (0,)}, "data pointer"), ({"null": (2,)}, "data pointer"), ({"null": (3,)}, "data pointer"),
                     ({"null": (5,)}, "result pointer"), ({"null": (6,)}, "result pointer"), ({"null": (9,)}, "result pointer"),
                     ({"null": (11,)}, "result pointer"), ({"maxiters": 0}, "maxiters"), ({"feastol": 0.0}, "feastol"),
                     ({"abstol": 0.0, "reltol": -1.0}, "reltol and abstol"), ({"feastol": float("nan")}, "feastol")):
        assert c_call(entry, **kw) == _lib.KVX_EINVAL, kw
        assert entry in _lib.last_error() and text in _lib.last_error(), (kw, _lib.last_error())
    if _lib.lib().kvx_device_count() == 0:
        assert c_call(entry) == _lib.KVX_EDEVICE and "no CPU fallback" in _lib.last_error()
        assert c_call(entry, p=0, null=(3, 4, 6), strides=(0, 0, 0, 0, 0)) == _lib.KVX_EDEVICE     # A, b, y may be NULL when p = 0
        assert c_call(entry, ml=10, q=(), m=()) == _lib.KVX_EDEVICE                                # no cones, no blocks: q, m may be NULL
        assert c_call(entry, ml=7, m=()) == _lib.KVX_EDEVICE and c_call(entry, ml=5, q=()) == _lib.KVX_EDEVICE


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_largest_members_pass_the_lds_check(entry):
    """The members of the box with the most LDS ('l' rows, cones of order 1 and blocks of order 1 cost the most per row)
    and the corner of the GPU tests pass every check, the 160 KiB backstop among them: without a device they are refused for the
    missing device alone; with one the host entry runs them (all-zero data: the documented exit 3), and the _dev entry, which would
    take this test's host buffers for device memory, is not called."""
    device = _lib.lib().kvx_device_count() > 0
    if device and entry.endswith("_dev"):
        return
    for ml, q, m in ((225, (1,) * 128, (1,) * 31), (224, (1,) * 128, (1,) * 32), (225, (1,) * 127, (1,) * 32), (28, (100,), (16,)), (0, (128,), (16,))):
        assert ml + sum(q) + sum(k * k for k in m) == 384
        rc = c_call(entry, B=1, n=64, ml=ml, q=q, m=m, p=64, strides=(0, 0, 0, 0, 0))
        assert rc == (_lib.KVX_OK if device else _lib.KVX_EDEVICE), (ml, q, m, _lib.last_error())
