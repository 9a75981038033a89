"""The host side of solvers.coneqp_batch_vjp / coneqp_batch_jvp, without a device: the table the defaults of
'centering' and 'centol' are chosen from (the float64 restatement of tests/coneqp_batch_diff_numpy.py against its longdouble form on
every batch of tests/test_coneqp_batch_diff_gpu.py), the identity between the two modes in longdouble, the restatement against
central differences of coneqp_batch_numpy.solve_member in longdouble with and without centring, the exits of the restatement, the
argument checks with their texts, KVX_EINVAL / KVX_EDEVICE of the four C entries and the LDS layout at the corners of the limits."""
import functools
import types

import numpy as np
import pytest

import coneqp_batch_diff_numpy as D
import coneqp_batch_numpy as CQN
from kvxopt_amd import _lib, coneqpbatchdiff, solvers

CENTERING, CENTOL = coneqpbatchdiff.DEFAULT_CENTERING, coneqpbatchdiff.DEFAULT_CENTOL

# The largest distance between the longdouble restatement at the defaults (on float64 solutions at 1e-8) and central differences of
# longdouble solves at 1e-10 with eps = 1e-4, relative in the 2-norm over x, y, s, z, measured over D.FD_BATCHES: 8.3e-3 (member 0 of
# (12, 3, (2,) * 6, (1, 2, 3), 2); the others 2e-8 .. 2.4e-3); the test allows 10 x that.  It is the truncation of the derivative
# (mu > 0) and the error of the difference quotient.  Without centring the same distance is 1e-2 .. 2.6 (the members that are at 1e-7
# there have no active 'q' or 's' row); it is largest on "absent-q", 2.6 on member 8.
FD_FOUND = 8.3e-3
FD_BOUND = 10 * FD_FOUND


@pytest.mark.parametrize("name", sorted(D.BATCHES))
def test_table_of_defaults(name):
    """At the defaults every member of every batch is within the rule 1e-6 max(|ref|, 1) of the longdouble restatement, is centred
    within the cap, and the threshold leaves less than the rule between the point it stops at and the central path; at most one
    member in twelve is skipped."""
    t = D.table(name, CENTOL)
    B = D.BATCHES[name][1]
    for cap in D.CAPS:
        print("%s centering %d: refinement 0 / 1 / 2: %s in units of the rule; exits %s"
              % (name, cap, " / ".join("%.2e" % t["rounding"][cap, r] for r in D.REFINEMENTS),
                 {c: t["exits"][cap].count(c) for c in sorted(set(t["exits"][cap]))}))
    for tol, (worst, steps) in t["truncation"].items():
        print("%s threshold %s: %.2e from the central path in units of the rule, at most %d steps" % (name, tol, worst, steps))
    assert CENTERING in D.CAPS and CENTOL in D.THRESHOLDS
    assert t["rounding"][CENTERING, 1] <= 1.0
    assert t["rounding"][CENTERING, 1] <= 1.05 * D.ROUNDING[name] + 1e-9                 # what the GPU test takes its bound from
    assert len(t["skipped"]) <= B // 12 and t["exits"][CENTERING].count(0) >= B - B // 12
    assert t["exits"][CENTERING].count(D.EXIT_NOT_CENTRED) == 0
    worst, steps = t["truncation"][CENTOL]
    assert worst <= 1.0 and steps <= CENTERING
    # why the default of centering is not 0; at (2, 0, (1,), (1,), 0) every cone has order 1, an orthant row, where W'W is exact
    assert t["truncation"][None][0] > 1.0 or name == D.shape_name(D.SHAPES[0])


def members_of(name):
    return range(min(D.BATCHES[name][1], D.FD_MEMBERS))


@pytest.mark.parametrize("name", ["mixed", D.shape_name(D.MANY)])
def test_both_modes_of_the_restatement_agree(name):
    """<gx, dx> = <grads, d theta> with all six perturbations, dG and dh symmetric in their 's' blocks, per member in longdouble."""
    M, sol = D.batch(name), D.solved(name)
    gx, d = D.cotangent(M, 3), D.direction(M, 4)
    V, J = D.derivatives(M, sol, gx, d, "longdouble", 0, CENTERING, CENTOL)
    worst = 0.0
    for k in range(M.B):
        lhs = gx[:, k] @ J["x"][:, k]
        rhs = D.inner(M, {v: (V[v][k] if v in "PGA" else V[v][:, k]) for v in D.NAMES if V[v] is not None}, D.QDN.member_perturbation(d, k))
        worst = max(worst, abs(lhs - rhs) / abs(lhs))
    print("%s: the identity holds to %.2e relative" % (name, worst))
    assert list(V["exit"]) == [0] * M.B and worst <= 1e-12


@functools.lru_cache(maxsize=None)
def central(name):
    """(M, d, which, solution at +eps, solution at -eps) in longdouble at 1e-10 along one random direction in all six data."""
    M = D.batch(name)
    which = list(members_of(name))
    M = CQN.take(M, which)
    d = D.direction(M, 1000 + M.n)
    return M, d, which, *(D.solution(CQN.restate(m, D.TIGHT_LONGDOUBLE, np.longdouble)) for m in (D.moved(M, d, D.EPS), D.moved(M, d, -D.EPS)))


def fd_distances(name, centering):
    M, d, which, plus, minus = central(name)
    sol = {k: (v[which] if k == "exit" else v[:, which]) for k, v in D.solved(name).items()}
    J = D.derivatives(M, sol, None, d, "longdouble", 0, centering, CENTOL)[1]
    return D.QDN.fd_errors(J, plus, minus, D.EPS)


@pytest.mark.parametrize("name", D.FD_BATCHES)
def test_restatement_against_central_differences(name):
    errs, raw = fd_distances(name, CENTERING), fd_distances(name, 0)
    left = int(np.isnan(errs).sum())
    print("%s: distance to central differences %s, %d left out; without centring %s"
          % (name, ["%.1e" % e for e in errs], left, ["%.1e" % e for e in raw]))
    assert left <= len(errs) // 4
    assert np.nanmax(errs) <= FD_BOUND
    if name == "absent-q":                                  # where the uncentred system is furthest off
        assert np.nanmax(raw) > FD_BOUND


# ---- the exits of the restatement
def test_restatement_exits():
    M, sol = D.batch("mixed"), D.solved("mixed")
    M = types.SimpleNamespace(**dict(vars(M), P=M.P.copy()))         # the cached batch stays as it is
    sol = {k: v.copy() for k, v in sol.items()}
    sol["exit"][1] = 1
    sol["s"][0, 3] = 0.0                                             # an 'l' row
    sol["z"][4, 5] = np.nan                                          # a 'q' row
    sol["s"][M.Ms, 7] = -1.0                                         # the (0, 0) entry of the block
    M.P[8][:] = -1e6 * np.eye(M.n)                                   # a failed pivot of S
    gx = np.ones((M.n, M.B))
    V, J = D.derivatives(M, sol, gx, D.direction(M, 1), "reduced", 1, CENTERING, CENTOL, shared=("G", "h"))
    assert list(V["exit"]) == list(J["exit"]) == [0, 1, 0, 2, 0, 2, 0, 2, 2, 0, 0, 0]
    for k in (1, 3, 5, 7, 8):
        assert not V["ux"][:, k].any() and not V["uz"][:, k].any() and not V["P"][k].any() and not J["x"][:, k].any() and not J["s"][:, k].any()
        assert np.isnan(V["centrality"][k])
    assert V["G"].shape == (M.N, M.n) and np.all(np.isfinite(V["G"])) and V["h"].shape == (M.N,)
    good = [k for k in range(M.B) if V["exit"][k] == 0]
    assert np.allclose(V["h"], -V["uz"][:, good].sum(axis=1), rtol=1e-13, atol=0)
    assert np.all(V["centrality"][good] <= CENTOL) and np.all(V["centering steps"][good] >= 1)
    # one step is not enough for the members that need more: exit 3 with the centrality reached, zeros; the others as before
    V1 = D.derivatives(M, sol, gx, None, "reduced", 1, 1, CENTOL)[0]
    assert set(V1["exit"][good]) == {D.EXIT_NOT_CENTRED} or set(V1["exit"][good]) == {0, D.EXIT_NOT_CENTRED}
    late = [k for k in good if V1["exit"][k] == D.EXIT_NOT_CENTRED]
    assert late and all(V1["centrality"][k] > CENTOL and V1["centering steps"][k] == 1 and not V1["ux"][:, k].any() for k in late)
    # centering = 0: the uncentred system, whatever the centrality
    V0 = D.derivatives(M, sol, gx, None, "reduced", 1, 0, CENTOL)[0]
    assert list(V0["exit"]) == list(V["exit"]) and np.all(V0["centering steps"] == 0) and np.all(V0["centrality"][good] > 0.1)


# ---- argument checks: all of them before a device is asked for
DIMS = {"l": 2, "q": [3], "s": [2]}


def data(n=4, dims=DIMS, p=2, B=3, seed=0):
    M = CQN.members(n, dims["l"], dims["q"], dims["s"], p, B, seed)
    sol = {"x": np.zeros((n, B)), "y": np.zeros((p, B)), "s": np.ones((M.N, B)), "z": np.ones((M.N, B)), "exit": np.zeros(B, dtype=np.int64)}
    return (M.P, M.q, M.G, M.h, M.dims, M.A, M.b), sol


def both(args, sol, **kw):
    """The two entries as callables that take what is common to them."""
    n, B = args[1].shape
    return [("coneqp_batch_vjp", lambda a=args, s=sol, **k: solvers.coneqp_batch_vjp(*a, sol=s, **dict({"gx": np.ones((n, B))}, **kw, **k))),
            ("coneqp_batch_jvp", lambda a=args, s=sol, **k: solvers.coneqp_batch_jvp(*a, sol=s, **dict(kw, **k)))]


@pytest.mark.parametrize("n,dims,p,text", [(65, DIMS, 0, r"%s: n = 65 is outside its limit 1 <= n <= 64.*solvers\.coneqp"),
                                           (4, {"l": 381, "q": [3], "s": [1]}, 0, r"%s: N = 385 is outside its limit 1 <= N <= 384"),
                                           (4, {"l": 1, "q": [], "s": [17]}, 0, r"%s: m_k = 17 is outside its limit 1 <= m_k <= 16"),
                                           (4, DIMS, 5, r"%s: p = 5 is outside its limit 0 <= p <= n.*solvers\.coneqp")])
def test_limits(n, dims, p, text):
    args, sol = data(n, dims, p)
    for name, fn in both(args, sol):
        with pytest.raises(ValueError, match=text % name):
            fn()


def test_problem_arguments_are_checked_as_coneqp_batch_checks_them():
    (P, q, G, h, dims, A, b), sol = data()
    bad = [((P[:2], q, G, h, dims, A, b), "'P' has 2 members, 'q' has 3 columns"),
           ((P, q, G, h[:, :2], dims, A, b), "'h' must have one column or B = 3 columns"),
           ((P, q, G[:, :8, :], h, dims, A, b), r"'G' must be a 'd' matrix of size \(9, 4\)"),
           ((P, q, G, h, dims, A, None), "'b' must have length 2"),
           ((P, q, G, h, [2, 3], A, b), "'dims' must be a dictionary"),
           ((P.astype(np.float32), q, G, h, dims, A, b), r"'P' must be one matrix or a float64 array of shape \(B, rows, 4\)")]
    for args, text in bad:
        for _, fn in both(args, sol):
            with pytest.raises(TypeError, match=text):
                fn()


def test_solution_cotangent_perturbations_and_wrt():
    args, sol = data()
    n, N, p, B = 4, 9, 2, 3
    for name, fn in both(args, sol):
        with pytest.raises(TypeError, match="'sol' must be the dictionary coneqp_batch returned"):
            fn(s={k: v for k, v in sol.items() if k != "z"})
        with pytest.raises(TypeError, match="'sol' must be the dictionary coneqp_batch returned"):
            fn(s=None)
        for key, shape, text in (("x", (n, B + 1), r"sol\['x'\] must be a 'd' matrix of size \(4, 3\)"),
                                 ("y", (p + 1, B), r"sol\['y'\] must be a 'd' matrix of size \(2, 3\)"),
                                 ("s", (N, 1), r"sol\['s'\] must be a 'd' matrix of size \(9, 3\)"),
                                 ("z", (N - 1, B), r"sol\['z'\] must be a 'd' matrix of size \(9, 3\)")):
            with pytest.raises(TypeError, match=text):
                fn(s=dict(sol, **{key: np.ones(shape)}))
        with pytest.raises(TypeError, match=r"sol\['exit'\] must be an integer array of length 3"):
            fn(s=dict(sol, exit=np.zeros(B)))
    vjp, jvp = both(args, sol)[0][1], both(args, sol)[1][1]
    with pytest.raises(TypeError, match=r"'gx' must be a 'd' matrix of size \(4, 3\)"):
        vjp(gx=np.ones((n, B - 1)))
    with pytest.raises(ValueError, match=r"coneqp_batch_vjp: wrt names 'x'; it takes 'P', 'q', 'G', 'h', 'A', 'b'"):
        vjp(wrt=("q", "x"))
    P, q, G, h, dims, A, b = args
    for kw, text in (({"dP": P[:2]}, "'dP' has 2 members, 'q' has 3 columns"),
                     ({"dG": G[:, :5, :]}, r"'dG' must be a 'd' matrix of size \(9, 4\)"),
                     ({"dA": A[:, :1, :]}, r"'dA' must be a 'd' matrix of size \(2, 4\)"),
                     ({"dq": q[:3]}, r"'dq' must be a 'd' matrix of size \(4,1\)"),
                     ({"dh": h[:5]}, r"'dh' must be a 'd' matrix of size \(9,1\)"),
                     ({"db": b[:, :2]}, "'db' must have one column or B = 3 columns")):
        with pytest.raises(TypeError, match=text):
            jvp(**kw)


def test_options():
    args, sol = data()
    for name, fn in both(args, sol):
        for o, text in (({"refinement": -1}, r"options\['refinement'\] must be a nonnegative integer"),
                        ({"refinement": 4}, r"%s: options\['refinement'\] = 4 is outside its limit 0 <= refinement <= 3" % name),
                        ({"centering": 1.5}, r"options\['centering'\] must be a nonnegative integer"),
                        ({"centering": 17}, r"%s: options\['centering'\] = 17 is outside its limit 0 <= centering <= 16" % name),
                        ({"centol": 0.0}, r"options\['centol'\] must be a positive scalar"),
                        ({"centol": "tight"}, r"options\['centol'\] must be a positive scalar"),
                        ({"maxiters": 10}, "%s: options accepts only 'refinement', 'centering' and 'centol', not 'maxiters'" % name)):
            with pytest.raises(ValueError, match=text):
                fn(options=o)
    assert solvers.coneqp_batch_vjp is coneqpbatchdiff.coneqp_batch_vjp and solvers.coneqp_batch_jvp is coneqpbatchdiff.coneqp_batch_jvp
    assert "coneqp_batch_vjp" in solvers.__doc__ and "coneqp_batch_jvp" in solvers.__doc__
    assert (CENTERING, CENTOL) == (8, 1e-6)


def test_good_arguments_reach_the_device_or_fail_loudly():
    """No fallback: without a device a call that passes every check raises, it does not compute."""
    args, sol = data()
    P, q, G, h, dims, A, b = args
    calls = [fn for _, fn in both(args, sol, options={"refinement": 2, "centering": 0, "centol": 1e-6})]
    calls += [lambda: solvers.coneqp_batch_jvp(P[0], q, G[0], h[:, 0], dims, A[0], b[:, :1], sol=sol, dP=P[0], dq=q[:, 0], dG=G, dh=h[:, 0],
                                               dA=A[0], db=b),
              lambda: solvers.coneqp_batch_vjp(P[0], q, G, h, dims, sol=dict(sol, y=np.zeros((0, 3))), gx=q, wrt="q")]
    for fn in calls:
        if _lib.lib().kvx_device_count() > 0:
            assert len(fn()["exit"]) == 3
        else:
            with pytest.raises(RuntimeError, match="no HIP device"):
                fn()


@pytest.mark.parametrize("entry", ["kvx_coneqp_batch_vjp", "kvx_coneqp_batch_vjp_dev", "kvx_coneqp_batch_jvp", "kvx_coneqp_batch_jvp_dev"])
def test_c_entries_answer_einval_without_a_device(entry):
    fn = getattr(_lib.lib(), entry)
    n, ml, p, B = 4, 2, 2, 3                                 # the cone of DIMS: N = 9
    buf = np.zeros(4096)
    ints = np.zeros(8, dtype=np.int64)
    dev, jvp = entry.endswith("_dev"), "jvp" in entry
    D_ = (lambda a: a.ctypes.data) if dev else _lib.pd
    Di = (lambda a: a.ctypes.data) if dev else _lib.pi

    def call(B=B, n=n, ml=ml, p=p, q=(3,), m=(2,), nullq=False, nullm=False, strides=(16, 4, 36, 9, 8, 2), null=(), refinement=1, centering=8,
             centol=1e-8, dstrides=(16, 4, 36, 9, 8, 2)):
        """null: positions among P q G h A b | x y s z exitcode | mode inputs | outputs that are passed as NULL"""
        pos = iter(range(64))
        ptr = lambda ints_=False: None if next(pos) in null else (Di(ints) if ints_ else D_(buf))          # noqa: E731
        qv, mv = np.asarray(q, dtype=np.int64), np.asarray(m, dtype=np.int64)
        a = [B, n, ml, len(q), None if nullq else _lib.pi(qv), len(m), None if nullm else _lib.pi(mv), p]
        for s in strides:
            a += [ptr(), s]
        a += [ptr(), ptr(), ptr(), ptr(), ptr(True), refinement, centering, centol]         # x y s z exitcode: 6 .. 10
        if jvp:
            for s in dstrides:
                a += [ptr(), s]                                      # dP .. db: 11 .. 16
            a += [ptr(), ptr(), ptr(), ptr(), ptr(), ptr(True), ptr(True)]           # dx dy dz ds centrality steps gexit: 17 .. 23
        else:
            a += [ptr()] + [ptr() for _ in range(7)] + [ptr(True), ptr(True)]        # gx: 11; ux uy uz gP gG gA centrality steps gexit: 12 .. 20
        return fn(*a)

    cases = [({"B": 0}, "1 <= B"), ({"n": 0}, "1 <= n <= 64"), ({"n": 65}, "1 <= n <= 64"), ({"ml": -1}, "0 <= ml <= 384"),
             ({"ml": 385}, "0 <= ml <= 384"), ({"q": (3,) * 129}, "0 <= nq <= 128"), ({"nullq": True}, "cone orders q are NULL"),
             ({"m": (1,) * 33}, "0 <= ns <= 32"), ({"nullm": True}, "block orders m are NULL"), ({"q": (0,)}, "every cone order"),
             ({"m": (17,)}, "every block order"), ({"ml": 380}, "1 <= N"), ({"ml": 0, "q": (), "m": ()}, "1 <= N"),
             ({"p": -1}, "0 <= p <= n"), ({"p": 5}, "0 <= p <= n"),
             ({"refinement": -1}, "0 <= refinement <= 3"), ({"refinement": 4}, "0 <= refinement <= 3"),
             ({"centering": -1}, "0 <= centering <= 16"), ({"centering": 17}, "0 <= centering <= 16"),
             ({"centol": 0.0}, "centol must be a positive scalar"), ({"centol": float("nan")}, "centol must be a positive scalar"),
             ({"strides": (15, 4, 36, 9, 8, 2)}, "stride of P"), ({"strides": (16, 3, 36, 9, 8, 2)}, "stride of q"),
             ({"strides": (16, 4, 35, 9, 8, 2)}, "stride of G"), ({"strides": (16, 4, 36, 8, 8, 2)}, "stride of h"),
             ({"strides": (16, 4, 36, 9, -8, 2)}, "stride of A"), ({"strides": (16, 4, 36, 9, 8, 1)}, "stride of b")]
    cases += [({"null": (k,)}, "data pointer") for k in range(6)] + [({"null": (k,)}, "solution pointer") for k in range(6, 11)]
    if jvp:
        cases += [({"dstrides": (15, 4, 36, 9, 8, 2)}, "stride of dP"), ({"dstrides": (16, 3, 36, 9, 8, 2)}, "stride of dq"),
                  ({"dstrides": (16, 4, 35, 9, 8, 2)}, "stride of dG"), ({"dstrides": (16, 4, 36, 8, 8, 2)}, "stride of dh"),
                  ({"dstrides": (16, 4, 36, 9, 7, 2)}, "stride of dA"), ({"dstrides": (16, 4, 36, 9, 8, 1)}, "stride of db")]
        cases += [({"null": (k,)}, "result pointer") for k in range(17, 24)]
    else:
        cases += [({"null": (11,)}, "cotangent pointer")] + [({"null": (k,)}, "result pointer") for k in (12, 13, 14, 18, 19, 20)]
    for kw, text in cases:
        assert call(**kw) == _lib.KVX_EINVAL, kw
        assert entry in _lib.last_error() and text in _lib.last_error(), (kw, _lib.last_error())
    if _lib.lib().kvx_device_count() == 0:
        assert call() == _lib.KVX_EDEVICE and "no CPU fallback" in _lib.last_error()
        if jvp:                                                   # every perturbation may be NULL; A, b, y, dy, dA, db when p = 0
            assert call(null=(11, 12, 13, 14, 15, 16), dstrides=(1, 1, 1, 1, 1, 1)) == _lib.KVX_EDEVICE
            assert call(p=0, null=(4, 5, 7, 15, 16, 18), strides=(0,) * 6, dstrides=(0,) * 6) == _lib.KVX_EDEVICE
        else:                                                     # the matrix gradients may be NULL; A, b, y, uy when p = 0
            assert call(null=(15, 16, 17)) == _lib.KVX_EDEVICE
            assert call(p=0, null=(4, 5, 7, 13, 17), strides=(0,) * 6) == _lib.KVX_EDEVICE


CORNERS = [(1, 1, (), (), 0), (64, 0, (), (16,), 64), (64, 384, (), (), 64), (64, 0, (384,), (), 64), (64, 0, (1,) * 128, (16,), 64),
           (64, 0, (), (3,) * 32, 64), D.CORNER, (64, 28, (100,), (16,), 0), (16, 30, (5,), (3,), 2)]


@pytest.mark.parametrize("shape", CORNERS, ids=D.shape_name)
def test_lds_layout_fits_at_the_corners_of_the_limits(shape):
    n, ml, q, s, p = shape
    fwd = np.zeros(1, dtype=np.int64)
    qv, mv = np.asarray(q, dtype=np.int64), np.asarray(s, dtype=np.int64)
    L = _lib.lib()
    mine = L.kvx_coneqp_batch_diff_lds_bytes(n, ml, len(q), _lib.pi(qv) if q else None, len(s), _lib.pi(mv) if s else None, p, _lib.pi(fwd))
    even = lambda v: (v + 1) & ~1                                                       # noqa: E731
    print("%s: %d bytes of LDS, the forward kernel %d" % (shape, mine, fwd[0]))
    assert mine == fwd[0] + 8 * (even(n) + even(p)) and 0 < mine <= 160 * 1024
    assert L.kvx_coneqp_batch_diff_lds_bytes(65, 1, 0, None, 0, None, 0, None) == -1
    assert L.kvx_coneqp_batch_diff_lds_bytes(4, 385, 0, None, 0, None, 0, None) == -1
    assert L.kvx_coneqp_batch_diff_lds_bytes(4, 0, 0, None, 0, None, 0, None) == -1
    assert L.kvx_coneqp_batch_diff_lds_bytes(4, 6, 0, None, 0, None, 5, None) == -1
