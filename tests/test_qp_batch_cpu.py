"""The host side of solvers.qp_batch, without a device: the restatement of tests/qp_batch_numpy.py against the
reference's own runs (G5 qp6x5, G9 qpeq6x5p4) to the 1e-10 of tests/test_qp_loop_cpu.py; that no expected iteration count of a batch
of tests/test_qp_batch_gpu.py sits on a rounding edge (float64, numpy.longdouble and float64 with numpy.linalg.solve in place of
the Cholesky factors agree in status and count for every member); the argument checks of qp_batch with their texts; and the
KVX_EINVAL of both C entries."""
import json
import os

import numpy as np
import pytest

import qp_batch_numpy as R
from kvxopt_amd import _lib, base, qpbatch, solvers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("name,gfile,p", [("qp6x5", "g5_coneqp", 0), ("qpeq6x5p4", "g9_coneqp_eq", 4)])
@pytest.mark.parametrize("precision", ["float64", "longdouble"])
def test_restatement_reproduces_the_reference(name, gfile, p, precision):
    meta = json.load(open(os.path.join(GOLDEN, gfile + ".json")))["cases"][name]
    g = np.load(os.path.join(GOLDEN, gfile + ".npz"))
    r = R.solve_member(*R.grid_dense(p), dtype=getattr(np, precision))
    assert r.status == meta["status"] == "optimal" and r.exit == 0 and r.iterations == meta["iterations"]
    errs = {k: rel(getattr(r, k), g[name + "_" + k]) for k in ("x", "y", "s", "z") if name + "_" + k in g.files}
    print("%s in %s: relative distance to the golden: %s" % (name, precision, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert set(errs) == ({"x", "y", "s", "z"} if p else {"x", "s", "z"}) and max(errs.values()) < 1e-10
    assert abs(r.stats[2] - meta["primal objective"]) < 1e-10 * abs(meta["primal objective"])


def test_restatement_reports_a_failed_factorisation_and_maxiters():
    P, q, G, h, A, b = R.grid_dense(4)
    P0, G0 = P.copy(), G.copy()
    P0[:, 7] = 0.0; P0[7, :] = 0.0; G0[:, 7] = 0.0
    r = R.solve_member(P0, q, G0, h, A, b)
    assert (r.status, r.exit, r.iterations) == ("unknown", 3, 0) and not r.x.any() and not r.s.any()
    r = R.solve_member(P, q, G, h, A, b, {"maxiters": 7})             # the reference needs 7: at maxiters it is "unknown"
    assert (r.status, r.exit, r.iterations) == ("unknown", 1, 7)
    with pytest.raises(ArithmeticError):
        R.cholesky(np.array([[1.0, 2.0], [2.0, 1.0]]))


def same_counts(shape, B, seed, which=None, correction=True):
    M = R.batch(shape, B, seed)
    opts = {"use_correction": correction}
    runs = [R.restate(M, opts, np.longdouble, which=which) if which is not None else R.restated(shape, B, seed, correction=correction),
            R.restate(M, opts, np.float64, which=which), R.restate(M, opts, np.float64, True, which=which)]
    outcomes = [[(r.status, r.iterations) for r in run] for run in runs]
    assert outcomes[0] == outcomes[1] == outcomes[2], outcomes
    xdiff = max(rel(a.x, b.x) for a, b in zip(runs[1], runs[0]))
    return [it for _, it in outcomes[0]], xdiff


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "n%d-ml%d-p%d" % s)
def test_no_count_of_a_shape_batch_sits_on_a_rounding_edge(shape):
    counts, xdiff = same_counts(shape, R.SHAPE_B, None)
    print("%s: iterations %s, float64 x within %.2e of longdouble" % (shape, counts, xdiff))
    assert all(3 <= c <= 12 for c in counts) and xdiff < 1e-9


def test_no_count_without_correction_sits_on_a_rounding_edge():
    counts, _ = same_counts((8, 17, 3), R.SHAPE_B, None, correction=False)
    assert counts != [r.iterations for r in R.restated((8, 17, 3))]


def test_no_count_of_the_mixed_batch_sits_on_a_rounding_edge():
    shape, B, seed = R.MIXED
    counts, _ = same_counts(shape, B, seed)
    m = int(np.median(counts))
    assert min(counts) < m <= max(counts)


@pytest.mark.parametrize("part", range(4))
def test_no_count_of_the_independence_batch_sits_on_a_rounding_edge(part):
    shape, B, seed = R.INDEPENDENCE
    counts, _ = same_counts(shape, B, seed, which=range(part * B // 4, (part + 1) * B // 4))
    assert len(counts) == B // 4 and len(set(counts)) >= 2


# ---- argument checks: all of them before a device is asked for (this box has none, or the call would go on to the device)
def data(n=4, ml=6, p=2, B=3, seed=0):
    M = R.members(n, ml, p, B, seed)
    return M.P, M.q, M.G, M.h, M.A, M.b


@pytest.mark.parametrize("n,ml,p,text", [(65, 6, 0, r"n = 65 is outside its limit 1 <= n <= 64.*solvers\.qp"),
                                         (4, 513, 0, r"ml = 513 is outside its limit 1 <= ml <= 512.*solvers\.qp"),
                                         (4, 6, 5, r"p = 5 is outside its limit 0 <= p <= n.*solvers\.qp")])
def test_limits(n, ml, p, text):
    P, q, G, h, A, b = data(n, ml, p)
    with pytest.raises(ValueError, match=text):
        solvers.qp_batch(P, q, G, h, A, b)
    with pytest.raises(ValueError, match=text):                       # shared matrices run into the same limits
        solvers.qp_batch(P[0], q, G[0], h, None if A is None else A[0], b)


def test_limits_at_zero():
    P, q, G, h, A, b = data()
    with pytest.raises(ValueError, match="ml = 0 is outside its limit 1 <= ml <= 512"):
        solvers.qp_batch(P[0], q, np.zeros((0, 4)), np.zeros(0))
    with pytest.raises(ValueError, match="n = 0 is outside its limit 1 <= n <= 64"):
        solvers.qp_batch(np.zeros((0, 0)), np.zeros((0, 3)), np.zeros((6, 0)), h)


def test_sizes_and_types():
    P, q, G, h, A, b = data()
    bad = [
        ((P[:2], q, G, h, A, b), "'P' has 2 members, 'q' has 3 columns"),
        ((P, q, G[:2], h, A, b), "'G' has 2 members, 'q' has 3 columns"),
        ((P, q, G, h, A[:1], b), "'A' has 1 members, 'q' has 3 columns"),
        ((P, q, G, h[:, :2], A, b), "'h' must have one column or B = 3 columns"),
        ((P, q, G, h, A, b[:, :2]), "'b' must have one column or B = 3 columns"),
        ((P[:, :3, :], q, G, h, A, b), r"'P' must be a 'd' matrix of size \(4, 4\)"),
        ((P[0][:3], q, G, h, A, b), r"'P' must be a 'd' matrix of size \(4, 4\)"),
        ((P, q, G[:, :, :3], h, A, b), r"'G' must be a 'd' matrix of size \(ml, 4\)"),
        ((P, q, G, h[:5], A, b), r"'h' must be a 'd' matrix of size \(6,1\)"),
        ((P, q, G, h, A[:, :, :3], b), "'A' must be a 'd' matrix with 4 columns"),
        ((P, q, G, h, A, b[:1]), "'b' must have length 2"),
        ((P, q, G, h, A, None), "'b' must have length 2"),
        ((P, q, G, h, None, b), "'b' must have length 0"),
        ((P.astype(np.float32), q, G, h, A, b), r"'P' must be one matrix or a float64 array of shape \(B, rows, 4\)"),
        ((P, q, G[None], h, A, b), r"'G' must be one matrix or a float64 array of shape \(B, rows, 4\)"),
        ((P, q[:, :, None], G, h, A, b), "'q' must be a 'd' matrix with one column per member"),
    ]
    for args, text in bad:
        with pytest.raises(TypeError, match=text):
            solvers.qp_batch(*args)


def test_shared_inputs_of_every_kind_pass_the_checks():
    P, q, G, h, A, b = data()
    sp = base.spmatrix([1.0, 2.0, 3.0, 4.0], [0, 1, 2, 3], [0, 1, 2, 3], (4, 4))
    for Pm in (P[0], base.matrix(np.asfortranarray(P[0])), sp):
        opt, dims, parts = qpbatch._prepare(Pm, base.matrix(np.asfortranarray(q)), G[0], h[:, 0], base.matrix(np.asfortranarray(A[0])), b[:, :1], None)
        assert dims == (3, 4, 6, 2) and [s for _, s in parts] == [0, 4, 0, 0, 0, 0]
    assert np.array_equal(parts[0][0].reshape(4, 4), np.diag([1.0, 2.0, 3.0, 4.0]))
    opt, dims, parts = qpbatch._prepare(P, q, G, h, A, b, {"maxiters": 7, "use_correction": False})
    assert (opt.maxiters, opt.correction) == (7, False) and [s for _, s in parts] == [16, 4, 24, 6, 8, 2]
    assert np.array_equal(parts[2][0][24:48].reshape(4, 6).T, G[1]) and np.array_equal(parts[3][0][6:12], h[:, 1])       # column-major members
    opt, dims, parts = qpbatch._prepare(P[0], q[:, 0], G[0], h[:, 0], None, None, None)                                     # B = 1, p = 0
    assert dims == (1, 4, 6, 0) and parts[4] == (None, 0) and parts[5] == (None, 0)


def test_options():
    args = data()
    with pytest.raises(NotImplementedError, match=r"options\['refinement'\] = 1 is not carried"):
        solvers.qp_batch(*args, options={"refinement": 1})
    for o, text in (({"maxiters": 0}, r"options\['maxiters'\] must be a positive integer"),
                    ({"maxiters": 2.5}, r"options\['maxiters'\] must be a positive integer"),
                    ({"abstol": "a"}, r"options\['abstol'\] must be a scalar"),
                    ({"reltol": -1.0, "abstol": 0.0}, r"at least one of options\['reltol'\] and options\['abstol'\] must be positive"),
                    ({"feastol": 0.0}, r"options\['feastol'\] must be a positive scalar"),
                    ({"refinement": -1}, r"options\['refinement'\] must be a nonnegative integer")):
        with pytest.raises(ValueError, match=text):
            solvers.qp_batch(*args, options=o)
    assert solvers.qp_batch is qpbatch.qp_batch and "qp_batch" in solvers.__doc__


def test_good_arguments_reach_the_device_or_fail_loudly():
    """No fallback loop: without a device a call that passes every check raises, it does not compute."""
    args, opts = data(), {"refinement": 0, "show_progress": True}
    if _lib.lib().kvx_device_count() > 0:
        assert solvers.qp_batch(*args, options=opts)["status"] == ["optimal"] * 3
    else:
        with pytest.raises(RuntimeError, match="no HIP device"):
            solvers.qp_batch(*args, options=opts)


@pytest.mark.parametrize("entry", ["kvx_qp_batch_solve", "kvx_qp_batch_solve_dev"])
def test_c_entries_answer_einval_without_a_device(entry):
    fn = getattr(_lib.lib(), entry)
    n, ml, p, B = 4, 6, 2, 3
    buf = np.zeros(4096)
    ints = np.zeros(8, dtype=np.int64)
    dev = entry.endswith("_dev")
    D = (lambda a: a.ctypes.data) if dev else _lib.pd
    Di = (lambda a: a.ctypes.data) if dev else _lib.pi

    def call(B=B, n=n, ml=ml, p=p, strides=(16, 4, 24, 6, 8, 2), null=(), maxiters=10, abstol=1e-7, reltol=1e-6, feastol=1e-7):
        data = []
        for k, s in enumerate(strides):
            data += [None if k in null else D(buf), s]
        outs = [None if 6 + k in null else D(buf) for k in range(5)] + [None if 11 + k in null else Di(ints) for k in range(2)]
        return fn(B, n, ml, p, *data, maxiters, abstol, reltol, feastol, 1, *outs)

    for kw, text in (({"B": 0}, "1 <= B"), ({"n": 0}, "1 <= n <= 64"), ({"n": 65}, "1 <= n <= 64"), ({"ml": 0}, "1 <= ml <= 512"),
                     ({"ml": 513}, "1 <= ml <= 512"), ({"p": -1}, "0 <= p <= n"), ({"p": 5}, "0 <= p <= n"),
                     ({"strides": (15, 4, 24, 6, 8, 2)}, "stride of P"), ({"strides": (16, 4, 23, 6, 8, 2)}, "stride of G"),
                     ({"strides": (16, 4, 24, 6, 8, 1)}, "stride of b"), ({"strides": (16, 4, 24, 6, -8, 2)}, "stride of A"),
                     ({"null": (0,)}, "data pointer"), ({"null": (3,)}, "data pointer"), ({"null": (4,)}, "data pointer"),
                     ({"null": (6,)}, "result pointer"), ({"null": (7,)}, "result pointer"), ({"null": (10,)}, "result pointer"),
                     ({"null": (12,)}, "result pointer"), ({"maxiters": 0}, "maxiters"), ({"feastol": 0.0}, "feastol"),
                     ({"abstol": 0.0, "reltol": -1.0}, "reltol and abstol"), ({"feastol": float("nan")}, "feastol")):
        assert call(**kw) == _lib.KVX_EINVAL, kw
        assert entry in _lib.last_error() and text in _lib.last_error(), (kw, _lib.last_error())
    if _lib.lib().kvx_device_count() == 0:
        assert call() == _lib.KVX_EDEVICE and "no CPU fallback" in _lib.last_error()
        assert call(p=0, null=(4, 5, 7), strides=(0, 0, 0, 0, 0, 0)) == _lib.KVX_EDEVICE        # A, b, y may be NULL when p = 0
