"""The host side of solvers.coneqp_batch, without a device: the restatement of tests/coneqp_batch_numpy.py against
the reference's own runs at refinement 0 (G29) in status, iterations and x, y, s, z to 1e-8 relative; with dims['q'] = dims['s'] = []
against tests/qp_batch_numpy.py on the same members, bit for bit; that float64 and numpy.longdouble agree in status, count and exit
for every member of every batch of tests/test_coneqp_batch_gpu.py and differ by at most 1e-2 of the bound the GPU results are held
to; the argument checks of coneqp_batch with their texts; and the KVX_EINVAL of both C entries.

Measured (this file's prints), largest relative distance of x, y, s, z to G29 in float64 / longdouble: doc_coneqp 3.8e-13 / 7.5e-13,
mixed_eq 1.4e-11 / 7.3e-12, p_rank_deficient 2.1e-11 / 1.1e-11, mixed_eq_cut 5.9e-15 / 9.4e-15; the garbage variants the same as
their clean cases.  The reference eliminates the equality rows by a QR factorisation (misc.kkt_chol) and takes its singular and
eigenvalues from LAPACK, the restatement eliminates through X and K and iterates by Jacobi: the same solution, other roundings.

The LDS refusal of the C entries is a backstop that no member of the limits reaches: the largest one needs 145472 bytes.
What is tested is that the largest members found pass it, in test_the_largest_members_pass_the_lds_check."""
import json
import os

import numpy as np
import pytest

import coneqp_batch_numpy as R
import qp_batch_numpy as QBN
import sdp_batch_numpy as SDN
from kvxopt_amd import _lib, coneqpbatch, solvers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VECTORS = ("x", "y", "s", "z")
G29_CASES = ("doc_coneqp", "doc_coneqp_garbage", "mixed_eq", "mixed_eq_garbage", "p_rank_deficient", "mixed_eq_cut")


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def vec_err(got, ref):
    """|got - ref| in units of the bound 1e-6 max(|ref|, 1) the GPU results are held to."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - ref) / (1e-6 * max(np.linalg.norm(ref), 1.0)))


def g29_case(name):
    meta = json.load(open(os.path.join(GOLDEN, "g29_coneqp_batch.json")))["cases"][name]
    g = np.load(os.path.join(GOLDEN, "g29_coneqp_batch.npz"))
    get = lambda k: g["%s__%s" % (name, k)] if "%s__%s" % (name, k) in g else None         # noqa: E731
    return meta, (get("P"), get("q"), get("G"), get("h"), meta["dims"], get("A"), get("b")), {k: get("sol_" + k) for k in VECTORS}


@pytest.mark.parametrize("precision", ["float64", "longdouble"])
@pytest.mark.parametrize("name", G29_CASES)
def test_restatement_reproduces_the_reference_at_refinement_0(name, precision):
    meta, data, sol = g29_case(name)
    r = R.solve_member(*data, meta["options"], getattr(np, precision))
    assert r.status == meta["status"] and r.iterations == meta["iterations"]
    assert r.exit == (0 if meta["status"] == "optimal" else 1)
    errs = {k: rel(getattr(r, k), sol[k]) for k in VECTORS if sol[k].size}
    print("%s in %s: relative distance to G29: %s" % (name, precision, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) < 1e-8
    assert abs(r.stats[2] - meta["primal objective"]) < 1e-8 * max(abs(meta["primal objective"]), 1.0)
    assert r.stats[6] > 0 and r.stats[7] > 0


def test_g29_holds_the_cases_it_is_to_hold():
    (ma, a, sa), (_, b, sb) = g29_case("doc_coneqp"), g29_case("doc_coneqp_garbage")
    assert ma["dims"] == {"l": 3, "q": [4], "s": []} and ma["status"] == "optimal"
    assert np.array_equal(np.tril(a[0]), np.tril(b[0])) and np.abs(np.triu(b[0], 1)).max() > 100
    assert all(np.array_equal(sa[k], sb[k]) for k in VECTORS)
    (mc, c, sc), (_, d, sd) = g29_case("mixed_eq"), g29_case("mixed_eq_garbage")
    assert mc["dims"] == {"l": 4, "q": [3, 4], "s": [3, 2]} and c[5].shape[0] == 2
    assert np.array_equal(np.tril(c[0]), np.tril(d[0])) and np.abs(np.triu(d[0], 1)).max() > 100
    assert not np.array_equal(c[2], d[2]) and not np.array_equal(c[3], d[3]) and np.abs(d[2]).max() > 900
    assert np.array_equal(SDN.symmetrise(d[2].copy(), 11, [3, 2]), c[2]) and np.array_equal(SDN.symmetrise(d[3].copy(), 11, [3, 2]), c[3])
    assert all(np.array_equal(sc[k], sd[k]) for k in VECTORS)
    mr, r, _ = g29_case("p_rank_deficient")
    assert np.linalg.matrix_rank(r[0]) == 2 < r[0].shape[0] == np.linalg.matrix_rank(r[2]) and mr["status"] == "optimal"
    mk, _, _ = g29_case("mixed_eq_cut")
    assert (mk["status"], mk["iterations"], mk["options"]) == ("unknown", 3, {"maxiters": 3}) and mc["iterations"] > 3


@pytest.mark.parametrize("precision", ["float64", "longdouble"])
@pytest.mark.parametrize("shape", [(1, 1, 0), (8, 17, 3), (33, 65, 5)])
@pytest.mark.parametrize("correction", [True, False])
def test_without_cones_and_blocks_the_restatement_is_the_one_of_qp_batch(shape, precision, correction):
    M, dt = QBN.batch(shape), getattr(np, precision)
    dims, opts = {"l": M.ml, "q": [], "s": []}, {"use_correction": correction}
    for k in range(M.B):
        A, b = (None, None) if M.A is None else (M.A[k], M.b[:, k])
        r = R.solve_member(M.P[k], M.q[:, k], M.G[k], M.h[:, k], dims, A, b, opts, dt)
        q = QBN.solve_member(M.P[k], M.q[:, k], M.G[k], M.h[:, k], A, b, opts, dt)
        assert (r.status, r.iterations, r.exit) == (q.status, q.iterations, q.exit)
        for v in VECTORS:
            assert np.array_equal(getattr(r, v), getattr(q, v)), v
        assert np.array_equal(np.array(r.stats[:6]), np.array(q.stats), equal_nan=True)
        assert r.stats[6] == float(min(q.s)) and r.stats[7] == float(min(q.z))


def agree(a, b):
    """Statuses, counts and exits of two runs agree; the largest distance of their vectors in units of the GPU's bound."""
    assert [(r.status, r.iterations, r.exit) for r in a] == [(r.status, r.iterations, r.exit) for r in b]
    worst = 0.0
    for u, w in zip(a, b):
        for v in VECTORS:
            y = np.asarray(getattr(w, v), float)
            if y.size:
                worst = max(worst, vec_err(getattr(u, v), y))
    return worst


@pytest.mark.parametrize("name", R.SMALL_BATCHES)
def test_float64_and_longdouble_agree_on_every_member(name):
    a, b = R.restated(name, "float64"), R.restated(name)
    worst = agree(a, b)
    print("%s: (exit, iterations) %s, float64 within %.2e of the GPU's bound of longdouble" % (name, [(r.exit, r.iterations) for r in b], worst))
    assert worst <= 1e-2
    if name == "mixed":
        assert {r.exit for r in b} == {0, 1, 3} and all((r.exit == 3) == (k in R.MIXED_RANK) for k, r in enumerate(b))
        assert b[R.MIXED_NAN].exit in (0, 1)                               # the member the GPU test spoils is a healthy one
    elif name == "maxiters-3":
        assert [(r.exit, r.iterations) for r in b] == [(1, 3)] * R.SHAPE_B
    else:
        assert [r.status for r in b] == ["optimal"] * R.SHAPE_B


def test_the_batches_have_the_shapes_they_are_to_show():
    n, ml, q, s, p = R.CORNER
    assert (n, p, max(s), ml + sum(q) + sum(m * m for m in s)) == (64, 64, 16, 384) and max(q) > 64
    for name in R.SMALL_BATCHES:
        M = R.batch(name)
        assert M.qd and M.s, name                                          # every batch has both kinds beside the orthant or without it
    M = R.batch("p-rank")
    assert all(np.linalg.matrix_rank(M.P[k]) == M.n - 2 and np.linalg.matrix_rank(np.vstack([M.P[k], M.G[k]])) == M.n for k in range(M.B))
    a, b = R.restated("correction"), R.restated("no-correction")
    assert any(u.iterations != w.iterations for u, w in zip(a, b))
    M = R.batch("mixed")
    for k in R.MIXED_RANK:
        assert np.linalg.matrix_rank(np.vstack([M.P[k], M.G[k], M.A[k]])) == M.n - 1


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
    return M.P, M.q, M.G, M.h, M.dims, M.A, M.b


@pytest.mark.parametrize("n,ml,q,s,p,text", [
    (65, 70, (3,), (3,), 0, r"n = 65 is outside its limit 1 <= n <= 64.*solvers\.coneqp solves one problem"),
    (4, 373, (3,), (3,), 0, r"N = 385 is outside its limit 1 <= N <= 384.*solvers\.coneqp"),
    (4, 382, (3,), (), 0, r"N = 385 is outside its limit 1 <= N <= 384.*solvers\.coneqp"),
    (4, 0, (1,) * 129, (2,), 0, r"nq = 129 is outside its limit 0 <= nq <= 128.*solvers\.coneqp"),
    (4, 0, (2,), (1,) * 33, 0, r"ns = 33 is outside its limit 0 <= ns <= 32.*solvers\.coneqp"),
    (4, 2, (2,), (17,), 0, r"m_k = 17 is outside its limit 1 <= m_k <= 16.*solvers\.coneqp"),
    (4, 2, (3,), (2, 1), 5, r"p = 5 is outside its limit 0 <= p <= n.*solvers\.coneqp")])
def test_limits(n, ml, q, s, p, text):
    P, qv, G, h, dims, A, b = data(n, ml, q, s, p)
    with pytest.raises(ValueError, match=text):
        solvers.coneqp_batch(P, qv, G, h, dims, A, b)
    with pytest.raises(ValueError, match=text):                       # shared matrices run into the same limits
        solvers.coneqp_batch(P[0], qv, G[0], h, dims, None if A is None else A[0], b)


def test_there_is_no_rank_condition_on_the_packed_dimension():
    """1 + 2 + 6 + p = 9 < n = 10, which conelp_batch refuses: P may supply the rank, so every check passes."""
    args = data(10, 1, (2,), (3,), 0)
    _, sizes, _ = coneqpbatch._prepare(*args, None)
    assert sizes == (3, 10, 1, [2], [3], 12, 0)


def test_dims():
    P, q, G, h, dims, A, b = data()
    with pytest.raises(TypeError, match=r"'dims\['s'\]' must be a list of nonnegative integers"):
        solvers.coneqp_batch(P, q, G, h, {"l": 2, "q": [3], "s": [2, -1]}, A, b)
    with pytest.raises(TypeError, match=r"'dims\['q'\]' must be a list of positive integers"):
        solvers.coneqp_batch(P, q, G, h, {"l": 2, "q": [3, 0], "s": [2, 1]}, A, b)
    with pytest.raises(ValueError, match=r"m_k = 0 is outside its limit 1 <= m_k <= 16"):
        solvers.coneqp_batch(P, q, G, h, {"l": 2, "q": [3], "s": [2, 1, 0]}, A, b)
    with pytest.raises(TypeError, match=r"'dims\['l'\]' must be a nonnegative integer"):
        solvers.coneqp_batch(P, q, G, h, {"l": -1, "q": [3], "s": [2, 1]}, A, b)
    with pytest.raises(TypeError, match="'dims' must be a dictionary"):
        solvers.coneqp_batch(P, q, G, h, None, A, b)
    with pytest.raises(ValueError, match="N = 0 is outside its limit 1 <= N <= 384"):
        solvers.coneqp_batch(P, q, np.zeros((0, 4)), np.zeros(0), {"l": 0, "q": [], "s": []})
    with pytest.raises(TypeError, match=r"'G' must be a 'd' matrix of size \(11, 4\)"):
        solvers.coneqp_batch(P, q, G, h, {"l": 3, "q": [3], "s": [2, 1]}, A, b)
    opt, sizes, parts = coneqpbatch._prepare(P, q, G, h, dims, A, b, None)
    assert sizes == (3, 4, 2, [3], [2, 1], 10, 2) and [s for _, s in parts] == [16, 4, 40, 10, 8, 2]
    for d in ({"l": 10}, {"l": 5, "q": [5]}, {"l": 1, "s": [3]}):         # absent kinds are empty: the same kernel takes them
        assert coneqpbatch._prepare(P, q, G, h, d, A, b, None)[1][5] == 10


def test_sizes_and_types():
    P, q, G, h, dims, A, b = data()
    bad = [
        ((P[:2], q, G, h, dims, A, b), "'P' has 2 members, 'q' has 3 columns"),
        ((P[:, :3], q, G, h, dims, A, b), r"'P' must be a 'd' matrix of size \(4, 4\)"),
        ((P[0][:3], q, G, h, dims, A, b), r"'P' must be a 'd' matrix of size \(4, 4\)"),
        ((P, q, G[:2], h, dims, A, b), "'G' has 2 members, 'q' has 3 columns"),
        ((P, q, G, h[:, :2], dims, A, b), "'h' must have one column or B = 3 columns"),
        ((P, q, G, h[:5], dims, A, b), r"'h' must be a 'd' matrix of size \(10,1\)"),
        ((P, q, G, h, dims, A[:, :, :3], b), "'A' must be a 'd' matrix with 4 columns"),
        ((P, q, G, h, dims, A, None), "'b' must have length 2"),
        ((P, q, G, h, dims, None, b), "'b' must have length 0"),
        ((P, q, G.astype(np.float32), h, dims, A, b), r"'G' must be one matrix or a float64 array of shape \(B, rows, 4\)"),
    ]
    for args, text in bad:
        with pytest.raises(TypeError, match=text):
            solvers.coneqp_batch(*args)


def test_options():
    args = data()
    with pytest.raises(NotImplementedError, match=r"options\['refinement'\] = 1 is not carried, only 0 \(the default here\); "
                                                  r"solvers\.coneqp refines, once by default"):
        solvers.coneqp_batch(*args, options={"refinement": 1})
    opt, _, _ = coneqpbatch._prepare(*args, None)
    assert opt.refinement == 0 and opt.correction is True              # absent: 0 here, whereas solvers.coneqp defaults to 1
    o = coneqpbatch._prepare(*args, {"refinement": 0, "show_progress": True, "use_correction": False})[0]
    assert o.refinement == 0 and o.correction is False
    for o, text in (({"maxiters": 0}, r"options\['maxiters'\] must be a positive integer"),
                    ({"abstol": "a"}, r"options\['abstol'\] must be a scalar"),
                    ({"reltol": -1.0, "abstol": 0.0}, r"at least one of options\['reltol'\] and options\['abstol'\] must be positive"),
                    ({"feastol": 0.0}, r"options\['feastol'\] must be a positive scalar"),
                    ({"refinement": -1}, r"options\['refinement'\] must be a nonnegative integer")):
        with pytest.raises(ValueError, match=text):
            solvers.coneqp_batch(*args, options=o)
    for kw in ({"initvals": {}}, {"kktsolver": "chol"}, {"solver": "mosek"}):
        with pytest.raises(TypeError):
            solvers.coneqp_batch(*args, **kw)
    solvers.options["refinement"] = 2                                  # the module-level dict is not read
    try:
        assert coneqpbatch._prepare(*args, None)[0].refinement == 0
    finally:
        del solvers.options["refinement"]


def test_the_entry_is_public():
    assert hasattr(solvers, "coneqp_batch") and solvers.coneqp_batch is coneqpbatch.coneqp_batch and "coneqp_batch" in solvers.__doc__
    for text in ("solvers.coneqp defaults to 1", "_ipm.coneqp_start", "max_step", "lower triangle", "there is no A'A", "exit 3",
                 "qp_batch is the faster entry"):
        assert text in coneqpbatch.__doc__, text


def test_good_arguments_reach_the_device_or_fail_loudly():
    """No fallback loop: without a device a call that passes every check raises, it does not compute."""
    args = data()
    if _lib.lib().kvx_device_count() > 0:
        assert solvers.coneqp_batch(*args)["status"] == ["optimal"] * 3
    else:
        with pytest.raises(RuntimeError, match="no HIP device"):
            solvers.coneqp_batch(*args)


def c_call(entry, B=3, n=4, ml=2, q=(3,), nq=None, m=(2, 1), ns=None, p=2, strides=(16, 4, 40, 10, 8, 2), null=(), maxiters=10,
           abstol=1e-7, reltol=1e-6, feastol=1e-7, correction=1):
    """null: 0..5 the data P, q, G, h, A, b; 6..10 the results x, y, s, z, stats; 11, 12 iterations and exit; 13, 14 the orders."""
    fn = getattr(_lib.lib(), entry)
    buf = np.zeros(65536)
    ints = np.zeros(8, dtype=np.int64)
    dev = entry.endswith("_dev")
    D = (lambda a: a.ctypes.data) if dev else _lib.pd
    Di = (lambda a: a.ctypes.data) if dev else _lib.pi
    data = []
    for k, s in enumerate(strides):
        data += [None if k in null else D(buf), s]
    outs = [None if 6 + k in null else D(buf) for k in range(5)] + [None if 11 + k in null else Di(ints) for k in range(2)]
    qv, mv = np.asarray(q, dtype=np.int64), np.asarray(m, dtype=np.int64)
    return fn(B, n, ml, len(q) if nq is None else nq, None if 13 in null or not len(q) else _lib.pi(qv), len(m) if ns is None else ns,
              None if 14 in null or not len(m) else _lib.pi(mv), p, *data, maxiters, abstol, reltol, feastol, correction, *outs)


ENTRIES = ["kvx_coneqp_batch_solve", "kvx_coneqp_batch_solve_dev"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_c_entries_answer_einval_without_a_device(entry):
    for kw, text in (({"B": 0}, "1 <= B"), ({"n": 0}, "1 <= n <= 64"), ({"n": 65}, "1 <= n <= 64"), ({"ml": -1}, "0 <= ml <= 384"),
                     ({"ml": 385}, "0 <= ml <= 384"), ({"nq": -1}, "0 <= nq <= 128"), ({"q": (1,) * 129}, "0 <= nq <= 128"),
                     ({"null": (13,)}, "cone orders q are NULL"), ({"q": (3, 0)}, "every cone order"), ({"q": (385,)}, "every cone order"),
                     ({"ns": -1}, "0 <= ns <= 32"), ({"m": (1,) * 33}, "0 <= ns <= 32"),
                     ({"null": (14,)}, "block orders m are NULL"), ({"m": (2, 0)}, "every block order"), ({"m": (2, 17)}, "every block order"),
                     ({"ml": 377}, "1 <= N = ml + sum(q) + sum(m^2) <= 384"), ({"ml": 0, "q": (), "m": ()}, "1 <= N = ml + sum(q) + sum(m^2) <= 384"),
                     ({"p": -1}, "0 <= p <= n"), ({"p": 5}, "0 <= p <= n"),
                     ({"strides": (15, 4, 40, 10, 8, 2)}, "stride of P"), ({"strides": (16, 3, 40, 10, 8, 2)}, "stride of q"),
                     ({"strides": (16, 4, 39, 10, 8, 2)}, "stride of G"), ({"strides": (16, 4, 40, 9, 8, 2)}, "stride of h"),
                     ({"strides": (16, 4, 40, 10, 8, 1)}, "stride of b"), ({"strides": (16, 4, 40, 10, -8, 2)}, "stride of A"),
                     ({"null": (0,)}, "data pointer"), ({"null": (1,)}, "data pointer"), ({"null": (3,)}, "data pointer"),
                     ({"null": (4,)}, "data pointer"),
                     ({"null": (6,)}, "result pointer"), ({"null": (7,)}, "result pointer"), ({"null": (10,)}, "result pointer"),
                     ({"null": (12,)}, "result pointer"), ({"maxiters": 0}, "maxiters"), ({"feastol": 0.0}, "feastol"),
                     ({"abstol": 0.0, "reltol": -1.0}, "reltol and abstol"), ({"feastol": float("nan")}, "feastol")):
        assert c_call(entry, **kw) == _lib.KVX_EINVAL, kw
        assert entry in _lib.last_error() and text in _lib.last_error(), (kw, _lib.last_error())
    if _lib.lib().kvx_device_count() == 0:
        assert c_call(entry) == _lib.KVX_EDEVICE and "no CPU fallback" in _lib.last_error()
        assert c_call(entry, p=0, null=(4, 5, 7), strides=(0, 0, 0, 0, 0, 0)) == _lib.KVX_EDEVICE   # A, b, y may be NULL when p = 0
        assert c_call(entry, ml=10, q=(), m=()) == _lib.KVX_EDEVICE                                # no cones, no blocks: q, m may be NULL
        assert c_call(entry, ml=7, m=()) == _lib.KVX_EDEVICE and c_call(entry, ml=5, q=()) == _lib.KVX_EDEVICE
        # no rank condition on the packed dimension: 1 + 2 + 6 + 0 < 10 is a good call
        assert c_call(entry, n=10, ml=1, q=(2,), m=(3,), p=0, strides=(100, 10, 120, 12, 0, 0)) == _lib.KVX_EDEVICE
        assert c_call(entry, correction=0) == _lib.KVX_EDEVICE


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
        rc = c_call(entry, B=1, n=64, ml=ml, q=q, m=m, p=64, strides=(0, 0, 0, 0, 0, 0))
        assert rc == (_lib.KVX_OK if device else _lib.KVX_EDEVICE), (ml, q, m, _lib.last_error())
