"""The host side of solvers.qp_batch_vjp / qp_batch_jvp, without a device: the restatement of
tests/qp_batch_diff_numpy.py against itself (the identity between the two modes), against central differences of
qp_batch_numpy.solve_member in numpy.longdouble, the float64 reduced solve with 0 / 1 / 2 refinement steps against the longdouble
elimination on the batches of tests/test_qp_batch_diff_gpu.py, the admissibility of the end-to-end comparison of the GPU file,
the argument checks with their texts, the exits 1 and 2 of the restatement, KVX_EINVAL / KVX_EDEVICE of the four C entries and
the LDS layout at the corners of the box of admissible shapes."""
import functools
import types

import numpy as np
import pytest

import qp_batch_diff_numpy as D
import qp_batch_numpy as R
from kvxopt_amd import _lib, qpbatchdiff, solvers

# 10 x the largest distance between the longdouble restatement and central differences of longdouble solves at tolerances 1e-12
# measured over the two batches of D.FD_BATCHES: 1.07e-5 (member 11 of (8, 17, 3), in y; the others 1e-10 .. 2e-7).
FD_BOUND = 10 * 1.07e-5

def float_solution(shape, B=R.SHAPE_B, seed=None):
    seed = D.SEEDS[shape] if seed is None else seed
    return R.batch(shape, B, seed), D.solution(R.restated(shape, B, seed, precision="float64"))


@pytest.mark.parametrize("shape", [(8, 17, 3), (16, 33, 2), (33, 65, 5)], ids=lambda s: "n%d-ml%d-p%d" % s)
def test_both_modes_of_the_restatement_agree(shape):
    """<gx, dx> = <grads, d theta> with dP, dG, dA among the perturbations, per member."""
    M, sol = float_solution(shape, seed=D.SEEDS.get(shape, R.INDEPENDENCE[2]))
    gx = np.random.default_rng(3).standard_normal((M.n, M.B))
    d = D.direction(M, 4)
    V, J = D.derivatives(M, sol, gx, d, "longdouble")
    worst = 0.0
    for k in range(M.B):
        lhs = gx[:, k] @ J["x"][:, k]
        rhs = D.inner({name: (V[name][k] if name in "PGA" else V[name][:, k]) for name in D.NAMES if V[name] is not None},
                      D.member_perturbation(d, k))
        worst = max(worst, abs(lhs - rhs) / abs(lhs))
    print("%s: the identity holds to %.2e relative" % (shape, worst))
    assert list(V["exit"]) == [0] * M.B and worst <= 1e-12


@functools.lru_cache(maxsize=None)
def central(shape, B, seed, precision, tol):
    """(M, d, solution, solution at +eps, solution at -eps) of the batch along one random direction in all six data."""
    M = R.batch(shape, B, seed)
    d = D.direction(M, 1000 + shape[0])
    opts, dtype = dict(tol), getattr(np, precision)
    return M, d, *(D.solution(R.restate(m, opts, dtype)) for m in (M, D.moved(M, d, D.EPS), D.moved(M, d, -D.EPS)))


@pytest.mark.parametrize("shape,B,seed", D.FD_BATCHES, ids=lambda v: str(v))
def test_restatement_against_central_differences(shape, B, seed):
    M, d, sol, plus, minus = central(shape, B, seed, "longdouble", tuple(D.TIGHT_LONGDOUBLE.items()))
    J = D.jvp_batch(M, sol, d, "longdouble")
    errs = D.fd_errors(J, plus, minus)
    left = int(np.isnan(errs).sum())
    print("%s: distance to central differences %s, %d left out" % (shape, ["%.1e" % e for e in errs], left))
    assert left <= B // 4
    assert np.nanmax(errs) <= FD_BOUND


def test_end_to_end_comparison_is_admissible():
    """What tests/test_qp_batch_diff_gpu.py does on the device, in float64 here: at most one member in four is left out, no
    count sits on a rounding edge, and the distance to central differences is within D.E2E_ERROR."""
    shape, tol = D.E2E_SHAPE, tuple(D.E2E_TOL.items())
    M, d, sol, plus, minus = central(shape, R.SHAPE_B, D.SEEDS[shape], "float64", tol)
    J = D.jvp_batch(M, sol, d, "reduced", 1)
    errs = D.fd_errors(J, plus, minus)
    left = int(np.isnan(errs).sum())
    print("%s at %s: distance to central differences %s, %d left out" % (shape, D.E2E_TOL, ["%.1e" % e for e in errs], left))
    assert left <= R.SHAPE_B // 4 and np.nanmax(errs) <= D.E2E_ERROR
    for m in (M, D.moved(M, d, D.EPS), D.moved(M, d, -D.EPS)):
        runs = [R.restate(m, D.E2E_TOL, np.longdouble), R.restate(m, D.E2E_TOL, np.float64), R.restate(m, D.E2E_TOL, np.float64, True)]
        outcomes = [[(r.exit, r.iterations) for r in run] for run in runs]
        assert outcomes[0] == outcomes[1] == outcomes[2], outcomes


def table_batches():
    return [(shape, R.SHAPE_B, D.SEEDS[shape]) for shape in D.SHAPES] + [(R.INDEPENDENCE[0], R.INDEPENDENCE[1], R.INDEPENDENCE[2]), R.MIXED]


@pytest.mark.parametrize("shape,B,seed", table_batches(), ids=lambda v: str(v))
def test_refinement_table(shape, B, seed):
    """The float64 reduced solve with 0, 1, 2 refinement steps against the longdouble elimination on the same inputs, both
    modes, every output, in units of the project's rule 1e-6 max(|ref|, 1); one step is within the rule on every member."""
    M, sol = float_solution(shape, B, seed)
    gx = np.random.default_rng(5).standard_normal((M.n, B))
    d = D.direction(M, 6)
    Vr, Jr = D.derivatives(M, sol, gx, d, "longdouble")
    worst = []
    for steps in (0, 1, 2):
        V, J = D.derivatives(M, sol, gx, d, "reduced", steps)
        assert list(V["exit"]) == list(Vr["exit"]) == [0] * B
        per_member = []
        for k in range(B):
            e = [D.rule(V[v][:, k], Vr[v][:, k]) for v in ("ux", "uy", "uz")] + [D.rule(J[v][:, k], Jr[v][:, k]) for v in ("x", "y", "z", "s")]
            e += [D.rule(V[v][k], Vr[v][k]) for v in "PGA" if V[v] is not None]
            per_member.append(max(e))
        worst.append(max(per_member))
    print("%s B = %d: largest error in units of the rule at 0 / 1 / 2 steps: %.2e / %.2e / %.2e" % (shape, B, *worst))
    assert worst[1] <= 1.0


# ---- the exits of the restatement
def test_restatement_skips_and_fails_members():
    shape, B, seed = R.MIXED
    M, sol = float_solution(shape, B, seed)
    M = types.SimpleNamespace(**dict(vars(M), P=M.P.copy()))         # the cached batch stays as it is
    sol = {k: v.copy() for k, v in sol.items()}
    sol["exit"][1] = 1
    sol["s"][2, 3] = 0.0
    sol["z"][4, 5] = np.nan
    M.P[8][:] = -1e6 * np.eye(M.n)                                   # a failed pivot of S
    gx = np.ones((M.n, B))
    V, J = D.derivatives(M, sol, gx, D.direction(M, 1), "reduced", 1, shared=("G", "h"))
    assert list(V["exit"]) == list(J["exit"]) == [0, 1, 0, 2, 0, 2, 0, 0, 2, 0, 0, 0]
    for k in (1, 3, 5, 8):
        assert not V["ux"][:, k].any() and not V["uz"][:, k].any() and not V["P"][k].any() and not J["x"][:, k].any() and not J["s"][:, k].any()
    assert V["G"].shape == (M.ml, M.n) and np.all(np.isfinite(V["G"])) and V["h"].shape == (M.ml,)
    good = [k for k in range(B) if V["exit"][k] == 0]
    assert np.allclose(V["h"], -V["uz"][:, good].sum(axis=1), rtol=1e-13, atol=0)


# ---- argument checks: all of them before a device is asked for
def data(n=4, ml=6, p=2, B=3, seed=0):
    M = R.members(n, ml, p, B, seed)
    sol = {"x": np.zeros((n, B)), "y": np.zeros((p, B)), "s": np.ones((ml, B)), "z": np.ones((ml, B)), "exit": np.zeros(B, dtype=np.int64)}
    return (M.P, M.q, M.G, M.h, M.A, M.b), sol


def both(args, sol, **kw):
    """The two entries as callables that take what is common to them."""
    n, B = args[1].shape
    return [("qp_batch_vjp", lambda a=args, s=sol, **k: solvers.qp_batch_vjp(*a, sol=s, **dict({"gx": np.ones((n, B))}, **kw, **k))),
            ("qp_batch_jvp", lambda a=args, s=sol, **k: solvers.qp_batch_jvp(*a, sol=s, **dict(kw, **k)))]


@pytest.mark.parametrize("n,ml,p,text", [(65, 6, 0, r"%s: n = 65 is outside its limit 1 <= n <= 64.*solvers\.qp"),
                                         (4, 513, 0, r"%s: ml = 513 is outside its limit 1 <= ml <= 512.*solvers\.qp"),
                                         (4, 6, 5, r"%s: p = 5 is outside its limit 0 <= p <= n.*solvers\.qp")])
def test_limits(n, ml, p, text):
    args, sol = data(n, ml, p)
    for name, fn in both(args, sol):
        with pytest.raises(ValueError, match=text % name):
            fn()


def test_problem_arguments_are_checked_as_qp_batch_checks_them():
    (P, q, G, h, A, b), sol = data()
    bad = [((P[:2], q, G, h, A, b), "'P' has 2 members, 'q' has 3 columns"),
           ((P, q, G, h[:, :2], A, b), "'h' must have one column or B = 3 columns"),
           ((P, q, G[:, :, :3], h, A, b), r"'G' must be a 'd' matrix of size \(ml, 4\)"),
           ((P, q, G, h, A, None), "'b' must have length 2"),
           ((P.astype(np.float32), q, G, h, A, b), r"'P' must be one matrix or a float64 array of shape \(B, rows, 4\)")]
    for args, text in bad:
        for _, fn in both(args, sol):
            with pytest.raises(TypeError, match=text):
                fn()


def test_solution_cotangent_perturbations_and_wrt():
    args, sol = data()
    n, ml, p, B = 4, 6, 2, 3
    for name, fn in both(args, sol):
        with pytest.raises(TypeError, match="'sol' must be the dictionary qp_batch returned"):
            fn(s={k: v for k, v in sol.items() if k != "z"})
        with pytest.raises(TypeError, match="'sol' must be the dictionary qp_batch returned"):
            fn(s=None)
        for key, shape, text in (("x", (n, B + 1), r"sol\['x'\] must be a 'd' matrix of size \(4, 3\)"),
                                 ("y", (p + 1, B), r"sol\['y'\] must be a 'd' matrix of size \(2, 3\)"),
                                 ("s", (ml, 1), r"sol\['s'\] must be a 'd' matrix of size \(6, 3\)"),
                                 ("z", (ml - 1, B), r"sol\['z'\] must be a 'd' matrix of size \(6, 3\)")):
            with pytest.raises(TypeError, match=text):
                fn(s=dict(sol, **{key: np.ones(shape)}))
        with pytest.raises(TypeError, match=r"sol\['exit'\] must be an integer array of length 3"):
            fn(s=dict(sol, exit=np.zeros(B)))
        with pytest.raises(TypeError, match=r"sol\['exit'\] must be an integer array of length 3"):
            fn(s=dict(sol, exit=np.zeros(B + 1, dtype=np.int64)))
    vjp, jvp = both(args, sol)[0][1], both(args, sol)[1][1]
    with pytest.raises(TypeError, match=r"'gx' must be a 'd' matrix of size \(4, 3\)"):
        vjp(gx=np.ones((n, B - 1)))
    with pytest.raises(TypeError, match=r"'gx' must be a 'd' matrix of size \(4, 3\)"):
        vjp(gx=np.ones((n + 1, B)))
    with pytest.raises(ValueError, match=r"qp_batch_vjp: wrt names 'x'; it takes 'P', 'q', 'G', 'h', 'A', 'b'"):
        vjp(wrt=("q", "x"))
    P, q, G, h, A, b = args
    for kw, text in (({"dP": P[:2]}, "'dP' has 2 members, 'q' has 3 columns"),
                     ({"dP": P[0][:3]}, r"'dP' must be a 'd' matrix of size \(4, 4\)"),
                     ({"dG": G[:, :5, :]}, r"'dG' must be a 'd' matrix of size \(6, 4\)"),
                     ({"dG": G.astype(np.float32)}, r"'dG' must be one matrix or a float64 array of shape \(B, rows, 4\)"),
                     ({"dA": A[:, :1, :]}, r"'dA' must be a 'd' matrix of size \(2, 4\)"),
                     ({"dq": q[:3]}, r"'dq' must be a 'd' matrix of size \(4,1\)"),
                     ({"dq": q[:, :2]}, "'dq' must have one column or B = 3 columns"),
                     ({"dh": h[:5]}, r"'dh' must be a 'd' matrix of size \(6,1\)"),
                     ({"db": b[:, :2]}, "'db' must have one column or B = 3 columns")):
        with pytest.raises(TypeError, match=text):
            jvp(**kw)


def test_options():
    args, sol = data()
    for name, fn in both(args, sol):
        for o, text in (({"refinement": -1}, r"options\['refinement'\] must be a nonnegative integer"),
                        ({"refinement": 1.5}, r"options\['refinement'\] must be a nonnegative integer"),
                        ({"refinement": 4}, r"%s: options\['refinement'\] = 4 is outside its limit 0 <= refinement <= 3" % name),
                        ({"maxiters": 10}, "%s: options accepts only 'refinement', not 'maxiters'" % name),
                        ({"refinement": 1, "abstol": 1e-9}, "%s: options accepts only 'refinement', not 'abstol'" % name)):
            with pytest.raises(ValueError, match=text):
                fn(options=o)
    assert solvers.qp_batch_vjp is qpbatchdiff.qp_batch_vjp and solvers.qp_batch_jvp is qpbatchdiff.qp_batch_jvp
    assert "qp_batch_vjp" in solvers.__doc__ and "qp_batch_jvp" in solvers.__doc__


def test_good_arguments_reach_the_device_or_fail_loudly():
    """No fallback: without a device a call that passes every check raises, it does not compute."""
    args, sol = data()
    P, q, G, h, A, b = args
    calls = [fn for _, fn in both(args, sol, options={"refinement": 2})]
    calls += [lambda: solvers.qp_batch_jvp(P[0], q, G[0], h[:, 0], A[0], b[:, :1], sol=sol, dP=P[0], dq=q[:, 0], dG=G, dh=h[:, 0], dA=A[0], db=b),
              lambda: solvers.qp_batch_vjp(P[0], q, G, h, sol=dict(sol, y=np.zeros((0, 3))), gx=q, wrt="q")]
    for fn in calls:
        if _lib.lib().kvx_device_count() > 0:
            assert list(fn()["exit"]) == [0, 0, 0]
        else:
            with pytest.raises(RuntimeError, match="no HIP device"):
                fn()


@pytest.mark.parametrize("entry", ["kvx_qp_batch_vjp", "kvx_qp_batch_vjp_dev", "kvx_qp_batch_jvp", "kvx_qp_batch_jvp_dev"])
def test_c_entries_answer_einval_without_a_device(entry):
    fn = getattr(_lib.lib(), entry)
    n, ml, p, B = 4, 6, 2, 3
    buf = np.zeros(4096)
    ints = np.zeros(8, dtype=np.int64)
    dev, jvp = entry.endswith("_dev"), "jvp" in entry
    D_ = (lambda a: a.ctypes.data) if dev else _lib.pd
    Di = (lambda a: a.ctypes.data) if dev else _lib.pi

    def call(B=B, n=n, ml=ml, p=p, strides=(16, 24, 8), null=(), refinement=1, dstrides=(16, 4, 24, 6, 8, 2)):
        """null: positions among P G A | x y s z exitcode | mode inputs | outputs that are passed as NULL"""
        pos = iter(range(64))
        ptr = lambda ints_=False: None if next(pos) in null else (Di(ints) if ints_ else D_(buf))          # noqa: E731
        a = [B, n, ml, p]
        for s in strides:
            a += [ptr(), s]
        a += [ptr(), ptr(), ptr(), ptr(), ptr(True), refinement]
        if jvp:
            for s in dstrides:
                a += [ptr(), s]
            a += [ptr(), ptr(), ptr(), ptr(), ptr(True)]                     # dx dy dz ds gexit: positions 14 .. 18
        else:
            a += [ptr()] + [ptr() for _ in range(6)] + [ptr(True)]          # gx: 8; ux uy uz gP gG gA gexit: 9 .. 15
        return fn(*a)

    cases = [({"B": 0}, "1 <= B"), ({"n": 0}, "1 <= n <= 64"), ({"n": 65}, "1 <= n <= 64"), ({"ml": 0}, "1 <= ml <= 512"),
             ({"ml": 513}, "1 <= ml <= 512"), ({"p": -1}, "0 <= p <= n"), ({"p": 5}, "0 <= p <= n"),
             ({"strides": (15, 24, 8)}, "stride of P"), ({"strides": (16, 23, 8)}, "stride of G"), ({"strides": (16, 24, -8)}, "stride of A"),
             ({"refinement": -1}, "0 <= refinement <= 3"), ({"refinement": 4}, "0 <= refinement <= 3"),
             ({"null": (0,)}, "data pointer"), ({"null": (1,)}, "data pointer"), ({"null": (2,)}, "data pointer"),
             ({"null": (3,)}, "solution pointer"), ({"null": (4,)}, "solution pointer"), ({"null": (5,)}, "solution pointer"),
             ({"null": (6,)}, "solution pointer"), ({"null": (7,)}, "solution pointer")]
    if jvp:
        cases += [({"dstrides": (15, 4, 24, 6, 8, 2)}, "stride of dP"), ({"dstrides": (16, 3, 24, 6, 8, 2)}, "stride of dq"),
                  ({"dstrides": (16, 4, 23, 6, 8, 2)}, "stride of dG"), ({"dstrides": (16, 4, 24, 5, 8, 2)}, "stride of dh"),
                  ({"dstrides": (16, 4, 24, 6, 7, 2)}, "stride of dA"), ({"dstrides": (16, 4, 24, 6, 8, 1)}, "stride of db"),
                  ({"null": (14,)}, "result pointer"), ({"null": (15,)}, "result pointer"), ({"null": (16,)}, "result pointer"),
                  ({"null": (17,)}, "result pointer"), ({"null": (18,)}, "result pointer")]
    else:
        cases += [({"null": (8,)}, "cotangent pointer"), ({"null": (9,)}, "result pointer"), ({"null": (10,)}, "result pointer"),
                  ({"null": (11,)}, "result pointer"), ({"null": (15,)}, "result pointer")]
    for kw, text in cases:
        assert call(**kw) == _lib.KVX_EINVAL, kw
        assert entry in _lib.last_error() and text in _lib.last_error(), (kw, _lib.last_error())
    if _lib.lib().kvx_device_count() == 0:
        assert call() == _lib.KVX_EDEVICE and "no CPU fallback" in _lib.last_error()
        if jvp:                                                   # every perturbation may be NULL; A, y, dy, dA, db when p = 0
            assert call(null=(8, 9, 10, 11, 12, 13), dstrides=(1, 1, 1, 1, 1, 1)) == _lib.KVX_EDEVICE
            assert call(p=0, null=(2, 4, 12, 13, 15), strides=(0, 0, 0), dstrides=(0, 0, 0, 0, 0, 0)) == _lib.KVX_EDEVICE
        else:                                                     # the matrix gradients may be NULL; A, y, uy when p = 0
            assert call(null=(12, 13, 14)) == _lib.KVX_EDEVICE
            assert call(p=0, null=(2, 4, 10, 14), strides=(0, 0, 0)) == _lib.KVX_EDEVICE


@pytest.mark.parametrize("shape", [(1, 1, 0), (64, 512, 64), (64, 512, 0), (64, 1, 64), (32, 64, 8)], ids=lambda s: "n%d-ml%d-p%d" % s)
def test_lds_layout_fits_where_the_forward_kernel_fits(shape):
    fwd = np.zeros(1, dtype=np.int64)
    mine = _lib.lib().kvx_qp_batch_diff_lds_bytes(*shape, _lib.pi(fwd))
    n, ml, p = shape
    even = lambda v: (v + 1) & ~1                                                       # noqa: E731
    expect = 8 * (even(n * (n | 1)) + max(even(p * (n | 1)) + even(p * (p | 1)), even(32 * (n | 1))) + 3 * even(n) + 3 * even(p) + 5 * even(ml) + 32)
    print("%s: %d bytes of LDS, the forward kernel %d" % (shape, mine, fwd[0]))
    assert mine == expect and 0 < mine <= fwd[0] <= 160 * 1024
    assert fwd[0] - mine == 8 * 4 * even(ml)
    L = _lib.lib()
    assert L.kvx_qp_batch_diff_lds_bytes(65, 1, 0, None) == -1 and L.kvx_qp_batch_diff_lds_bytes(4, 6, 5, None) == -1
    assert L.kvx_qp_batch_diff_lds_bytes(4, 0, 0, None) == -1 and L.kvx_qp_batch_diff_lds_bytes(4, 6, 2, None) > 0
