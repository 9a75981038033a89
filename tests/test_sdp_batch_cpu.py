"""The host side of solvers.sdp_batch, without a device: the restatement of tests/sdp_batch_numpy.py against the
reference's own runs at refinement 0 (G27) in status, iterations and x, y, s, z to 1e-8 relative; its 's' operations against G16 to
the tolerances tests/test_oracle.py holds the oracle to on G16 (1e-12, and 1e-11 for r r' and rti rti'); with dims['s'] = [] against
tests/lp_batch_numpy.py on the same member, bit for bit; that float64 and numpy.longdouble agree in status, count and exit for every
member of every batch of tests/test_sdp_batch_gpu.py and differ by at most 1e-2 of the bound the GPU results are held to; the
argument checks of sdp_batch with their texts; and the KVX_EINVAL of both C entries.

Measured (this file's prints), largest relative distance of x, y, s, z to G27 in float64 / longdouble: doc_sdp 1.1e-13 / 6.8e-14,
doc_sdp_lower the same, mixed_eq 3.3e-11 / 2.9e-11, sdp_pinf 5.6e-16 / 4.4e-16, sdp_dinf 4.9e-15 / 4.4e-15.  The reference eliminates the
equality rows by a QR factorisation (misc.kkt_chol) and takes its singular and eigenvalues from LAPACK, the restatement eliminates
through X and K (misc.kkt_chol2) and iterates by Jacobi: the same solution, other roundings."""
import json
import os

import numpy as np
import pytest

import lp_batch_numpy as LPN
import sdp_batch_numpy as R
from kvxopt_amd import _lib, sdpbatch, solvers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VECTORS = ("x", "y", "s", "z")
G27_CASES = ("doc_sdp", "doc_sdp_lower", "mixed_eq", "sdp_pinf", "sdp_dinf")


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def vec_err(got, ref):
    """|got - ref| in units of the bound 1e-6 max(|ref|, 1) the GPU results are held to."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - ref) / (1e-6 * max(np.linalg.norm(ref), 1.0)))


def g27_case(name):
    meta = json.load(open(os.path.join(GOLDEN, "g27_sdp_batch.json")))["cases"][name]
    g = np.load(os.path.join(GOLDEN, "g27_sdp_batch.npz"))
    get = lambda k: g["%s__%s" % (name, k)] if "%s__%s" % (name, k) in g else None         # noqa: E731
    return meta, (get("c"), get("G"), get("h"), meta["dims"], get("A"), get("b")), {k: get("sol_" + k) for k in VECTORS}


@pytest.mark.parametrize("precision", ["float64", "longdouble"])
@pytest.mark.parametrize("name", G27_CASES)
def test_restatement_reproduces_the_reference_at_refinement_0(name, precision):
    meta, data, sol = g27_case(name)
    r = R.solve_member(*data, dtype=getattr(np, precision))
    assert r.status == meta["status"] and r.iterations == meta["iterations"] and r.exit == R.EXITS[meta["status"]]
    errs = {k: rel(getattr(r, k), sol[k]) for k in VECTORS if sol[k] is not None and sol[k].size}
    print("%s in %s: relative distance to G27: %s" % (name, precision, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) < 1e-8
    if meta["status"] == "optimal":
        assert abs(r.stats[2] - meta["primal objective"]) < 1e-8 * max(abs(meta["primal objective"]), 1.0)
        assert r.stats[6] > 0 and r.stats[7] > 0
    elif meta["status"] == "primal infeasible":
        assert np.isnan(r.x).all() and np.isnan(r.s).all() and r.stats[3] == 1.0 and r.stats[7] > 0
    else:
        assert np.isnan(r.z).all() and r.stats[2] == -1.0 and r.stats[6] > 0


def test_g27_holds_the_doc_example_twice_and_garbage_above_the_diagonals():
    (_, a, sa), (_, b, sb) = g27_case("doc_sdp")[:3], g27_case("doc_sdp_lower")[:3]
    assert not np.array_equal(a[1], b[1]) and not np.array_equal(a[2], b[2])
    assert np.array_equal(R.symmetrise(b[1].copy(), 0, [2, 3]), a[1]) and np.array_equal(R.symmetrise(b[2].copy(), 0, [2, 3]), a[2])
    assert np.abs(b[1]).max() > 900 and all(np.array_equal(sa[k], sb[k]) for k in VECTORS if sa[k] is not None)


def test_s_operations_reproduce_g16():
    """dims = {'l': 3, 'q': [4], 's': [3, 1, 6]} without (a) and with (b, 2 more rows) an offset, as tests/test_oracle.py reads G16:
    the 's' blocks alone, in an engine on {'l': 0, 's': [3, 1, 6]}."""
    g = np.load(os.path.join(GOLDEN, "g16_s_cone_scaling.npz"))
    sd = [3, 1, 6]
    N, Nd = sum(m * m for m in sd), sum(sd)
    low = lambda v: R.symmetrise(np.array(v, dtype=float), 0, sd)                          # noqa: E731
    for tag, k in (("a", 0), ("b", 2)):
        nlq = k + 7
        e = R.SdpEngine(np.zeros(1), np.zeros((N, 1)), np.zeros(N), {"l": 0, "q": [], "s": sd})
        e.s.a, e.z.a = low(g[tag + "_s"][nlq:]), low(g[tag + "_z"][nlq:])
        e.scaling()
        assert rel(e.lmbda.a, g[tag + "_lmbda"][nlq:]) < 1e-12
        o = 0
        for i, m in enumerate(sd):
            Rg, Tg = (R.mat(g[tag + name], o, m) for name in ("_r", "_rti"))
            assert rel(e.r[i] @ e.r[i].T, Rg @ Rg.T) < 1e-11 and rel(e.rti[i] @ e.rti[i].T, Tg @ Tg.T) < 1e-11
            e.r[i], e.rti[i] = Rg.copy(), Tg.copy()            # the signs of singular vectors are arbitrary: scale with the golden's
            o += m * m
        e.lmbda.a = g[tag + "_lmbda"][nlq:].copy()
        for tr in "NT":
            for inv in "NI":
                for c in range(2):
                    got = e.W(low(g[tag + "_X"][nlq:, c]), inv == "I", tr == "T")
                    assert rel(got, low(g["%s_scale_%s%s" % (tag, tr, inv)][nlq:, c])) < 1e-12, (tr, inv)
        x1, y1 = low(g[tag + "_x1"][nlq:]), low(g[tag + "_y1"][nlq:])
        assert rel(e.scale2(x1), low(g[tag + "_scale2_N"][nlq:])) < 1e-12
        assert rel(e.scale2(x1, True), low(g[tag + "_scale2_I"][nlq:])) < 1e-12
        assert rel(e.sprod(x1, y1), low(g[tag + "_sprod"][nlq:])) < 1e-12
        e.lmbda.a = g[tag + "_yd"][nlq:].copy()
        assert rel(e.sinv_diag(x1), low(g[tag + "_sinv"][nlq:])) < 1e-12
        assert abs(x1 @ y1 - (float(g[tag + "_sdot"]) - g[tag + "_x1"][:nlq] @ g[tag + "_y1"][:nlq])) < 1e-12 * abs(x1 @ y1)
        eig = e.eig(x1)
        assert rel(np.concatenate([sig for sig, _ in eig]), g[tag + "_max_step_sigma"]) < 1e-12
        for (sig, Qm), (_, ob, _, m) in zip(eig, e.blk):
            assert rel((Qm * sig) @ Qm.T, R.mat(x1, ob, m)) < 1e-12 and rel(Qm.T @ Qm, np.eye(m)) < 1e-12
        # update_scaling: lmbda and the new scaling point through r r', rti rti'
        o, il = 0, 0
        for i, m in enumerate(sd):
            Ls, Lz = (R.mat(g[tag + name][nlq:], o, m) for name in ("_us_s_in", "_us_z_in"))
            r2, t2, lm2 = R.update_scaling_s(R.mat(g[tag + "_r"], o, m), R.mat(g[tag + "_rti"], o, m), Ls, Lz)
            Rn, Tn = (R.mat(g[tag + name], o, m) for name in ("_us_r", "_us_rti"))
            assert rel(lm2, g[tag + "_us_lmbda"][nlq + il:nlq + il + m]) < 1e-12
            assert rel(r2 @ r2.T, Rn @ Rn.T) < 1e-11 and rel(t2 @ t2.T, Tn @ Tn.T) < 1e-11
            o += m * m
            il += m
        assert Nd == il


@pytest.mark.parametrize("precision", ["float64", "longdouble"])
def test_without_blocks_the_restatement_is_the_one_of_lp_batch(precision):
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
def data(n=4, ml=2, s=(2, 1), p=2, B=3, seed=0):
    M = R.members(n, ml, s, p, B, seed)
    return M.c, M.G, M.h, M.dims, M.A, M.b


@pytest.mark.parametrize("n,ml,s,p,text", [
    (65, 70, (3,), 0, r"n = 65 is outside its limit 1 <= n <= 64.*solvers\.sdp"),
    (4, 376, (3,), 0, r"N = 385 is outside its limit 1 <= N <= 384.*solvers\.sdp"),
    (4, 0, (1,) * 33, 0, r"ns = 33 is outside its limit 0 <= ns <= 32.*solvers\.sdp"),
    (4, 2, (17,), 0, r"m_k = 17 is outside its limit 1 <= m_k <= 16.*solvers\.sdp"),
    (4, 2, (2, 1), 5, r"p = 5 is outside its limit 0 <= p <= n.*solvers\.sdp"),
    # the packed dimension counts, not N: N = 2 + 9 = 11 >= 10, but 2 + 6 + p = 9 < 10 (coneprog.py:512, 572)
    (10, 2, (3,), 1, r"p \+ ml \+ sum\(m_k \(m_k \+ 1\) / 2\) = 9 is outside its limit, at least n = 10.*solvers\.sdp")])
def test_limits(n, ml, s, p, text):
    c, G, h, dims, A, b = data(n, ml, s, p)
    with pytest.raises(ValueError, match=text):
        solvers.sdp_batch(c, G, h, dims, A, b)
    with pytest.raises(ValueError, match=text):                       # shared matrices run into the same limits
        solvers.sdp_batch(c, G[0], h, dims, None if A is None else A[0], b)


def test_dims():
    c, G, h, dims, A, b = data()
    with pytest.raises(ValueError, match=r"dims\['q'\] = \[3\] is outside its limit, absent or empty; solvers\.socp_batch.*solvers\.conelp"):
        solvers.sdp_batch(c, G, h, {"l": 2, "q": [3], "s": [2, 1]}, A, b)
    with pytest.raises(TypeError, match=r"'dims\['s'\]' must be a list of nonnegative integers"):
        solvers.sdp_batch(c, G, h, {"l": 2, "s": [2, -1]}, A, b)
    with pytest.raises(ValueError, match=r"m_k = 0 is outside its limit 1 <= m_k <= 16"):
        solvers.sdp_batch(c, G, h, {"l": 2, "s": [2, 1, 0]}, A, b)
    with pytest.raises(TypeError, match=r"'dims\['l'\]' must be a nonnegative integer"):
        solvers.sdp_batch(c, G, h, {"l": -1, "s": [2, 1]}, A, b)
    with pytest.raises(TypeError, match="'dims' must be a dictionary"):
        solvers.sdp_batch(c, G, h, None, A, b)
    with pytest.raises(ValueError, match="N = 0 is outside its limit 1 <= N <= 384"):
        solvers.sdp_batch(c, np.zeros((0, 4)), np.zeros(0), {"l": 0, "s": []})
    with pytest.raises(TypeError, match=r"'G' must be a 'd' matrix of size \(8, 4\)"):
        solvers.sdp_batch(c, G, h, {"l": 3, "s": [2, 1]}, A, b)
    opt, sizes, parts = sdpbatch._prepare(c, G, h, {"l": 2, "q": [], "s": [2, 1]}, A, b, None)       # 'q' empty: accepted
    assert sizes == (3, 4, 2, [2, 1], 7, 2) and [s for _, s in parts] == [4, 28, 7, 8, 2]


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
            solvers.sdp_batch(*args)


def test_options():
    args = data()
    with pytest.raises(NotImplementedError, match=r"options\['refinement'\] = 1 is not carried.*solvers\.sdp refines"):
        solvers.sdp_batch(*args, options={"refinement": 1})
    opt, _, _ = sdpbatch._prepare(*args, None)
    assert opt.refinement == 0                                         # absent: 0 here, whereas solvers.sdp defaults to 1
    assert sdpbatch._prepare(*args, {"refinement": 0, "show_progress": True})[0].refinement == 0
    for o, text in (({"maxiters": 0}, r"options\['maxiters'\] must be a positive integer"),
                    ({"abstol": "a"}, r"options\['abstol'\] must be a scalar"),
                    ({"reltol": -1.0, "abstol": 0.0}, r"at least one of options\['reltol'\] and options\['abstol'\] must be positive"),
                    ({"feastol": 0.0}, r"options\['feastol'\] must be a positive scalar"),
                    ({"refinement": -1}, r"options\['refinement'\] must be a nonnegative integer")):
        with pytest.raises(ValueError, match=text):
            solvers.sdp_batch(*args, options=o)
    for kw in ({"primalstart": {}}, {"dualstart": {}}, {"kktsolver": "chol"}, {"solver": "mosek"}):
        with pytest.raises(TypeError):
            solvers.sdp_batch(*args, **kw)
    solvers.options["refinement"] = 2                                  # the module-level dict is not read
    try:
        assert sdpbatch._prepare(*args, None)[0].refinement == 0
    finally:
        del solvers.options["refinement"]


def test_the_entry_is_public():
    assert hasattr(solvers, "sdp_batch") and solvers.sdp_batch is sdpbatch.sdp_batch and "sdp_batch" in solvers.__doc__
    for text in ("certificate", "solvers.sdp defaults to 1", "_ipm.conelp_start", "max_step", "lower triangle"):
        assert text in sdpbatch.__doc__


def test_good_arguments_reach_the_device_or_fail_loudly():
    """No fallback loop: without a device a call that passes every check raises, it does not compute."""
    args = data()
    if _lib.lib().kvx_device_count() > 0:
        assert solvers.sdp_batch(*args)["status"] == ["optimal"] * 3
    else:
        with pytest.raises(RuntimeError, match="no HIP device"):
            solvers.sdp_batch(*args)


@pytest.mark.parametrize("entry", ["kvx_sdp_batch_solve", "kvx_sdp_batch_solve_dev"])
def test_c_entries_answer_einval_without_a_device(entry):
    fn = getattr(_lib.lib(), entry)
    n, ml, p, B = 4, 2, 2, 3
    buf = np.zeros(4096)
    ints = np.zeros(8, dtype=np.int64)
    dev = entry.endswith("_dev")
    D = (lambda a: a.ctypes.data) if dev else _lib.pd
    Di = (lambda a: a.ctypes.data) if dev else _lib.pi

    def call(B=B, n=n, ml=ml, m=(2, 1), ns=None, p=p, strides=(4, 28, 7, 8, 2), null=(), maxiters=10, abstol=1e-7, reltol=1e-6,
             feastol=1e-7):
        data = []
        for k, s in enumerate(strides):
            data += [None if k in null else D(buf), s]
        outs = [None if 5 + k in null else D(buf) for k in range(5)] + [None if 10 + k in null else Di(ints) for k in range(2)]
        mv = np.asarray(m, dtype=np.int64)
        return fn(B, n, ml, len(m) if ns is None else ns, None if 12 in null or not len(m) else _lib.pi(mv), p, *data, maxiters, abstol,
                  reltol, feastol, *outs)

    for kw, text in (({"B": 0}, "1 <= B"), ({"n": 0}, "1 <= n <= 64"), ({"n": 65}, "1 <= n <= 64"), ({"ml": -1}, "0 <= ml <= 384"),
                     ({"ml": 385}, "0 <= ml <= 384"), ({"ns": -1}, "0 <= ns <= 32"), ({"m": (1,) * 33}, "0 <= ns <= 32"),
                     ({"null": (12,)}, "block orders m are NULL"), ({"m": (2, 0)}, "every block order"), ({"m": (2, 17)}, "every block order"),
                     ({"ml": 380}, "1 <= N = ml + sum(m^2) <= 384"), ({"ml": 0, "m": ()}, "1 <= N = ml + sum(m^2) <= 384"),
                     ({"p": -1}, "0 <= p <= n"), ({"p": 5}, "0 <= p <= n"),
                     ({"n": 10, "ml": 2, "m": (3,), "p": 1, "strides": (10, 110, 11, 10, 1)}, "p + ml + sum(m (m + 1) / 2) >= n"),
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
        assert call(ml=7, m=(), strides=(4, 28, 7, 8, 2)) == _lib.KVX_EDEVICE                # no blocks: m may be NULL
