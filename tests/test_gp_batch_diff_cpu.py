"""The host side of solvers.gp_batch_vjp / gp_batch_jvp, without a device: the restatement of
tests/gp_batch_diff_numpy.py against itself (the identity between the two modes), against central differences of
gp_batch_numpy.solve_member in numpy.longdouble, the float64 reduced solve with 0 / 1 / 2 refinement steps against the longdouble
elimination on the batches of tests/test_gp_batch_diff_gpu.py (the table that decides the default of `refinement`), one-term
constraint rows against the same rows in G, a one-term objective, the argument checks with their texts, the exits 1 and 2 of the
restatement, KVX_EINVAL / KVX_EDEVICE of the four C entries and the LDS layout at the corners of the box of admissible shapes."""
import functools
import types

import numpy as np
import pytest

import gp_batch_diff_numpy as D
import gp_batch_numpy as R
from kvxopt_amd import _lib, gpbatchdiff, solvers

# 10 x the largest distance (gp_batch_diff_numpy.fd_errors: |J - fd| / max(|fd|, 1) in the 2-norm, over x, y, znl, snl, zl, sl)
# between the longdouble restatement and central differences of longdouble solves at tolerances 1e-13 with eps = 1e-6, measured
# over the three batches of D.FD_BATCHES: 2.10e-8 (member 4 of (6, [5, 3, 2], 12, 1); the others 2e-11 .. 2e-9).  No member is left
# out.  The truncation remark of DESIGN section 20 holds here: the derivative is that of the point handed in, a point of the
# central path, so the distance at looser tolerances is that of the path to the optimum; for derivatives solve near 1e-8 to 1e-9.
FD_BOUND = 10 * 2.10e-8


def float_solution(name):
    M = D.named(name)
    return M, D.solution(D.restated(name), len(M.K))


def fd_batch(shape, B, seed):
    return R.shaped((shape[0], tuple(shape[1])) + tuple(shape[2:]), B, seed)


@pytest.mark.parametrize("name", ["mixed_one_term", "k63_64_65", "N192_linear"])
def test_both_modes_of_the_restatement_agree(name):
    """<gx, dx> = <grads, d theta> with all six perturbations, per member."""
    M, sol = float_solution(name)
    gx = np.random.default_rng(3).standard_normal((M.n, M.B))
    d = D.direction(M, 4)
    V, J = D.derivatives(M, sol, gx, d, "longdouble")
    worst = 0.0
    for k in range(M.B):
        lhs = gx[:, k] @ J["x"][:, k]
        rhs = D.inner(D.member_gradients(V, k), D.member_perturbation(d, k))
        worst = max(worst, float(abs(lhs - rhs) / abs(lhs)))
    print("%s: the identity holds to %.2e relative" % (name, worst))
    assert list(V["exit"]) == [0] * M.B and worst <= 1e-12


@functools.lru_cache(maxsize=None)
def central(shape, B, seed):
    """(M, d, the longdouble runs at the point, at +eps and at -eps) along one random direction in all six data."""
    M = fd_batch(shape, B, seed)
    d = D.direction(M, 1000 + shape[0])
    return M, d, [R.restate(m, D.TIGHT_LONGDOUBLE, np.longdouble) for m in (M, D.moved(M, d, D.EPS), D.moved(M, d, -D.EPS))]


@pytest.mark.parametrize("shape,B,seed", D.FD_BATCHES, ids=lambda v: str(v))
def test_restatement_against_central_differences(shape, B, seed):
    M, d, runs = central((shape[0], tuple(shape[1])) + tuple(shape[2:]), B, seed)
    J = D.derivatives(M, D.solution(runs[0], len(M.K)), None, d, "longdouble")[1]
    errs = D.fd_errors(J, runs)
    left = int(np.isnan(errs).sum())
    print("%s: distance to central differences %s, %d left out" % (shape, ["%.1e" % e for e in errs], left))
    assert left <= B // 4
    assert np.nanmax(errs) <= FD_BOUND


def test_refinement_table_decides_the_default():
    """The float64 reduced solve with 0, 1, 2 refinement steps against the longdouble elimination on the same inputs, both modes,
    every output, every batch of the GPU file, in units of the project's rule 1e-6 max(|ref|, 1): the default is the smallest
    count at which every member is within the rule.  ds = -(s / z) dz and ds from the third block row are both inside it."""
    table = D.refinement_table()
    for name, row in table.items():
        print("%-18s ds = -(s/z) dz: %.2e / %.2e / %.2e   third block row: %.2e / %.2e / %.2e" % ((name,) + row))
    worst = [max(row[c] for row in table.values()) for c in range(6)]
    smallest = min(c for c in range(3) if worst[c] <= 1.0)
    assert smallest == gpbatchdiff.DEFAULT_REFINEMENT == 1
    assert worst[1] <= 1.0 and worst[4] <= 1.0 and worst[0] > 1.0


def test_one_term_rows_are_rows_of_G():
    """A block of one term is the linear row F_k x + g_k <= 0: the same rows placed in G with h = -g give dl/dF_k = dl/dG_k and
    dl/dg_k = -dl/dh_k, to the rule, at longdouble solutions of both programs."""
    n, K, B = 3, [5, 1, 1, 1], 6
    M = R.members(n, K, 6, 0, B, 5201)
    M2 = types.SimpleNamespace(n=n, K=K[:1], ml=9, p=0, B=B, F=M.F[:, :5], g=np.asfortranarray(M.g[:5]),
                               G=np.concatenate([M.F[:, 5:], M.G], axis=1), h=np.asfortranarray(np.vstack([-M.g[5:], M.h])), A=None, b=None)
    gx = np.random.default_rng(7).standard_normal((n, B))
    V = [D.derivatives(m, D.solution(R.restate(m, D.TIGHT_LONGDOUBLE, np.longdouble), len(m.K)), gx, None, "longdouble")[0] for m in (M, M2)]
    assert list(V[0]["exit"]) == list(V[1]["exit"]) == [0] * B
    worst = 0.0
    for k in range(B):
        worst = max(worst, D.rule(V[0]["F"][k][5:], V[1]["G"][k][:3]), D.rule(V[0]["g"][5:, k], -V[1]["h"][:3, k]),
                    D.rule(V[0]["ux"][:, k], V[1]["ux"][:, k]), D.rule(V[0]["uznl"][:, k], V[1]["uzl"][:3, k]))
    print("one-term rows against rows of G: %.2e in units of the rule" % worst)
    assert worst <= 1.0


def test_one_term_objective():
    """With one term in the objective y_0 = 1: dl/dg_0 = 0 exactly and dl/dF_0 = ux'."""
    M, sol = float_solution("one_term_blocks")
    gx = np.random.default_rng(8).standard_normal((M.n, M.B))
    for precision in ("float64", "longdouble"):
        V = D.derivatives(M, sol, gx, None, precision)[0]
        assert list(V["exit"]) == [0] * M.B
        for k in range(M.B):
            assert V["g"][0, k] == 0.0 and np.array_equal(V["F"][k][0], V["ux"][:, k]) and V["ux"][:, k].any()


# ---- the exits of the restatement
def test_restatement_skips_and_fails_members():
    M = R.named("mixed")
    sol = {k: v.copy() for k, v in D.solution(R.restated("mixed", "float64"), len(M.K)).items()}
    M = types.SimpleNamespace(**dict(vars(M), F=M.F.copy()))         # the cached batch stays as it is
    B = M.B
    assert list(sol["exit"]) == [0] * B
    sol["exit"][1] = 1
    sol["sl"][2, 3] = 0.0
    sol["znl"][0, 5] = np.nan
    M.F[8][:] = np.nan                                               # a failed pivot of S
    gx = np.ones((M.n, B))
    V, J = D.derivatives(M, sol, gx, D.direction(M, 1), "float64", 1, shared=("F", "G", "h"))
    assert list(V["exit"]) == list(J["exit"]) == [0, 1, 0, 2, 0, 2, 0, 0, 2]
    for k in (1, 3, 5, 8):
        assert not V["ux"][:, k].any() and not V["uzl"][:, k].any() and not V["g"][:, k].any() and not V["A"][k].any()
        assert not J["x"][:, k].any() and not J["sl"][:, k].any() and not J["znl"][:, k].any()
    assert V["F"].shape == (sum(M.K), M.n) and np.all(np.isfinite(V["F"])) and V["G"].shape == (M.ml, M.n) and V["h"].shape == (M.ml,)
    good = [k for k in range(B) if V["exit"][k] == 0]
    assert np.allclose(V["h"], -V["uzl"][:, good].sum(axis=1), rtol=1e-13, atol=0)


# ---- argument checks: all of them before a device is asked for
def data(n=4, K=(3, 2), ml=6, p=2, B=3, seed=0):
    M = R.members(n, list(K), ml, min(p, n), B, seed, free=True)
    if p > n:                                                        # members() has orthonormal rows in A, so at most n
        M.A, M.b = np.ones((B, p, n)), np.ones((p, B))
    mnl = len(K) - 1
    sol = {"x": np.zeros((n, B)), "y": np.zeros((p, B)), "znl": np.ones((mnl, B)), "snl": np.ones((mnl, B)), "zl": np.ones((ml, B)),
           "sl": np.ones((ml, B)), "exit": np.zeros(B, dtype=np.int64)}
    return R.batch_args(M), sol


def both(args, sol, **kw):
    """The two entries as callables that take what is common to them."""
    n, B = args[1].shape[-1], args[2].shape[1]
    return [("gp_batch_vjp", lambda a=args, s=sol, **k: solvers.gp_batch_vjp(*a, sol=s, **dict({"gx": np.ones((n, B))}, **kw, **k))),
            ("gp_batch_jvp", lambda a=args, s=sol, **k: solvers.gp_batch_jvp(*a, sol=s, **dict(kw, **k)))]


@pytest.mark.parametrize("n,K,ml,p,text", [(64, (3, 2), 6, 0, r"%s: n = 64 is outside its limit 1 <= n <= 63.*solvers\.gp"),
                                           (4, (3, 2), 191, 0, r"%s: N = 193 is outside its limit 1 <= N <= 192.*solvers\.gp"),
                                           (4, (700, 69), 6, 0, r"%s: l = 769 is outside its limit 1 <= l <= 768.*solvers\.gp"),
                                           (4, (3, 2), 6, 5, r"%s: p = 5 is outside its limit 0 <= p <= n.*solvers\.gp")])
def test_limits(n, K, ml, p, text):
    args, sol = data(n, K, ml, p)
    for name, fn in both(args, sol):
        with pytest.raises(ValueError, match=text % name):
            fn()


def test_problem_arguments_are_checked_as_gp_batch_checks_them():
    (K, F, g, G, h, A, b), sol = data()
    bad = [(([3, 0], F, g, G, h, A, b), "'K' must be a list of positive integers"),
           ((K, F[:2], g, G, h, A, b), "'F' has 2 members, 'g' has 3 columns"),
           ((K, F[:, :4], g, G, h, A, b), "'F' must be a dense or sparse 'd' matrix with 5 rows"),
           ((K, F, g, G, h[:, :2], A, b), "'h' must have one column or B = 3 columns"),
           ((K, F, g, G[:, :, :3], h, A, b), "'G' must be a dense or sparse 'd' matrix with 4 columns"),
           ((K, F, g, G, h, A, None), r"'b' must be a dense 'd' matrix of size \(2,1\)"),
           ((K, F.astype(np.float32), g, G, h, A, b), "'F' must be a dense or sparse 'd' matrix with 5 rows")]
    for args, text in bad:
        for _, fn in both(args, sol):
            with pytest.raises(TypeError, match=text):
                fn(a=args)


def test_solution_cotangent_perturbations_and_wrt():
    args, sol = data()
    n, mnl, ml, p, B, l = 4, 1, 6, 2, 3, 5
    for name, fn in both(args, sol):
        with pytest.raises(TypeError, match="'sol' must be the dictionary gp_batch returned, with 'x', 'y', 'znl', 'snl', 'zl', 'sl' and 'exit'"):
            fn(s={k: v for k, v in sol.items() if k != "zl"})
        with pytest.raises(TypeError, match="'sol' must be the dictionary gp_batch returned"):
            fn(s=None)
        for key, shape, text in (("x", (n, B + 1), r"sol\['x'\] must be a 'd' matrix of size \(4, 3\)"),
                                 ("y", (p + 1, B), r"sol\['y'\] must be a 'd' matrix of size \(2, 3\)"),
                                 ("znl", (mnl + 1, B), r"sol\['znl'\] must be a 'd' matrix of size \(1, 3\)"),
                                 ("snl", (mnl, 1), r"sol\['snl'\] must be a 'd' matrix of size \(1, 3\)"),
                                 ("zl", (ml - 1, B), r"sol\['zl'\] must be a 'd' matrix of size \(6, 3\)"),
                                 ("sl", (ml, B - 1), r"sol\['sl'\] must be a 'd' matrix of size \(6, 3\)")):
            with pytest.raises(TypeError, match=text):
                fn(s=dict(sol, **{key: np.ones(shape)}))
        with pytest.raises(TypeError, match=r"sol\['exit'\] must be an integer array of length 3"):
            fn(s=dict(sol, exit=np.zeros(B)))
    vjp, jvp = both(args, sol)[0][1], both(args, sol)[1][1]
    with pytest.raises(TypeError, match=r"'gx' must be a 'd' matrix of size \(4, 3\)"):
        vjp(gx=np.ones((n, B - 1)))
    with pytest.raises(ValueError, match=r"gp_batch_vjp: wrt names 'P', 'K'; it takes 'F', 'g', 'G', 'h', 'A', 'b'"):
        vjp(wrt=("g", "P", "K"))
    K, F, g, G, h, A, b = args
    for kw, text in (({"dF": F[:2]}, "'dF' has 2 members, 'g' has 3 columns"),
                     ({"dF": F[0][:4]}, r"'dF' must be a 'd' matrix of size \(5, 4\)"),
                     ({"dG": G[:, :5, :]}, r"'dG' must be a 'd' matrix of size \(6, 4\)"),
                     ({"dG": G.astype(np.float32)}, r"'dG' must be one matrix or a float64 array of shape \(B, rows, 4\)"),
                     ({"dA": A[:, :1, :]}, r"'dA' must be a 'd' matrix of size \(2, 4\)"),
                     ({"dg": g[:4]}, r"'dg' must be a 'd' matrix of size \(5,1\)"),
                     ({"dg": g[:, :2]}, "'dg' must have one column or B = 3 columns"),
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
    assert solvers.gp_batch_vjp is gpbatchdiff.gp_batch_vjp and solvers.gp_batch_jvp is gpbatchdiff.gp_batch_jvp
    assert "gp_batch_vjp" in solvers.__doc__ and "gp_batch_jvp" in solvers.__doc__


def test_good_arguments_reach_the_device_or_fail_loudly():
    """No fallback: without a device a call that passes every check raises, it does not compute."""
    args, sol = data()
    K, F, g, G, h, A, b = args
    calls = [fn for _, fn in both(args, sol, options={"refinement": 2})]
    calls += [lambda: solvers.gp_batch_jvp(K, F[0], g, G[0], h[:, 0], A[0], b[:, :1], sol=sol, dF=F[0], dg=g[:, 0], dG=G, dh=h[:, 0], dA=A[0], db=b),
              lambda: solvers.gp_batch_vjp(K, F[0], g, sol=dict(sol, y=np.zeros((0, 3)), zl=np.zeros((0, 3)), sl=np.zeros((0, 3))), gx=np.ones((4, 3)), wrt="g")]
    for fn in calls:
        if _lib.lib().kvx_device_count() > 0:
            assert len(fn()["exit"]) == 3
        else:
            with pytest.raises(RuntimeError, match="no HIP device"):
                fn()


@pytest.mark.parametrize("entry", ["kvx_gp_batch_vjp", "kvx_gp_batch_vjp_dev", "kvx_gp_batch_jvp", "kvx_gp_batch_jvp_dev"])
def test_c_entries_answer_einval_without_a_device(entry):
    fn = getattr(_lib.lib(), entry)
    n, ml, p, B = 4, 6, 2, 3
    buf = np.zeros(4096)
    ints = np.zeros(8, dtype=np.int64)
    dev, jvp = entry.endswith("_dev"), "jvp" in entry
    D_ = (lambda a: a.ctypes.data) if dev else _lib.pd
    Di = (lambda a: a.ctypes.data) if dev else _lib.pi

    def call(B=B, n=n, K=(3, 2), ml=ml, p=p, strides=(20, 5, 24, 8), null=(), refinement=1, dstrides=(20, 5, 24, 6, 8, 2), no_K=False):
        """null: positions among F g G A | x y s z exitcode | mode inputs | outputs that are passed as NULL"""
        pos = iter(range(64))
        ptr = lambda ints_=False: None if next(pos) in null else (Di(ints) if ints_ else D_(buf))          # noqa: E731
        a = [B, n, len(K) - 1, None if no_K else _lib.pi(np.asarray(K, dtype=np.int64)), ml, p]
        for s in strides:
            a += [ptr(), s]
        a += [ptr(), ptr(), ptr(), ptr(), ptr(True), refinement]
        if jvp:
            for s in dstrides:
                a += [ptr(), s]
            a += [ptr(), ptr(), ptr(), ptr(), ptr(True)]                     # dx dy dz ds gexit: positions 15 .. 19
        else:                                                               # gx: 9; ux uy uz gg gF gG gA [work] gexit: 10 ..
            a += [ptr()] + [ptr() for _ in range(8 if dev else 7)] + [ptr(True)]
        return fn(*a)

    cases = [({"B": 0}, "1 <= B"), ({"n": 0}, "1 <= n <= 63"), ({"n": 64}, "1 <= n <= 63"), ({"ml": -1}, "ml >= 0"),
             ({"ml": 191}, "N = mnl + 1 + ml <= 192"), ({"K": (3, 0)}, "every block size K[i] is a positive integer"),
             ({"K": (700, 69)}, "l = sum(K) <= 768"), ({"no_K": True}, "the block sizes K are NULL"),
             ({"p": -1}, "0 <= p <= n"), ({"p": 5}, "0 <= p <= n"),
             ({"strides": (19, 5, 24, 8)}, "stride of F"), ({"strides": (20, 4, 24, 8)}, "stride of g"),
             ({"strides": (20, 5, 23, 8)}, "stride of G"), ({"strides": (20, 5, 24, -8)}, "stride of A"),
             ({"refinement": -1}, "0 <= refinement <= 3"), ({"refinement": 4}, "0 <= refinement <= 3"),
             ({"null": (0,)}, "data pointer"), ({"null": (1,)}, "data pointer"), ({"null": (2,)}, "data pointer"), ({"null": (3,)}, "data pointer"),
             ({"null": (4,)}, "solution pointer"), ({"null": (5,)}, "solution pointer"), ({"null": (6,)}, "solution pointer"),
             ({"null": (7,)}, "solution pointer"), ({"null": (8,)}, "solution pointer")]
    if jvp:
        cases += [({"dstrides": (19, 5, 24, 6, 8, 2)}, "stride of dF"), ({"dstrides": (20, 4, 24, 6, 8, 2)}, "stride of dg"),
                  ({"dstrides": (20, 5, 23, 6, 8, 2)}, "stride of dG"), ({"dstrides": (20, 5, 24, 5, 8, 2)}, "stride of dh"),
                  ({"dstrides": (20, 5, 24, 6, 7, 2)}, "stride of dA"), ({"dstrides": (20, 5, 24, 6, 8, 1)}, "stride of db"),
                  ({"null": (15,)}, "result pointer"), ({"null": (16,)}, "result pointer"), ({"null": (17,)}, "result pointer"),
                  ({"null": (18,)}, "result pointer"), ({"null": (19,)}, "result pointer")]
    else:
        last = 18 if dev else 17
        cases += [({"null": (9,)}, "cotangent pointer"), ({"null": (10,)}, "result pointer"), ({"null": (11,)}, "result pointer"),
                  ({"null": (12,)}, "result pointer"), ({"null": (13,)}, "result pointer"), ({"null": (last,)}, "result pointer")]
        if dev:                                                   # a shared F whose gradient is asked for needs the workspace
            cases += [({"null": (17,), "strides": (0, 5, 24, 8)}, "workspace pointer")]
    for kw, text in cases:
        assert call(**kw) == _lib.KVX_EINVAL, kw
        assert entry in _lib.last_error() and text in _lib.last_error(), (kw, _lib.last_error())
    if _lib.lib().kvx_device_count() == 0:
        assert call() == _lib.KVX_EDEVICE and "no CPU fallback" in _lib.last_error()
        if jvp:                                                   # every perturbation may be NULL; G with ml = 0; A, y, dy with p = 0
            assert call(null=(9, 10, 11, 12, 13, 14), dstrides=(1, 1, 1, 1, 1, 1)) == _lib.KVX_EDEVICE
            assert call(ml=0, p=0, null=(2, 3, 5, 11, 12, 13, 14, 16), strides=(0, 0, 0, 0), dstrides=(0, 0, 0, 0, 0, 0)) == _lib.KVX_EDEVICE
        else:                                                     # the matrix gradients and then the workspace may be NULL
            assert call(null=(14, 15, 16, 17) if dev else (14, 15, 16)) == _lib.KVX_EDEVICE
            if dev:                                               # F has a member stride, so no workspace is needed
                assert call(null=(17,)) == _lib.KVX_EDEVICE
            assert call(ml=0, p=0, null=(2, 3, 5, 11, 15, 16), strides=(0, 5, 0, 0)) == _lib.KVX_EDEVICE


CORNERS = [(1, (1,), 0, 0), (63, (768,), 191, 63), (63, tuple(R.CORNER_K), 192 - len(R.CORNER_K), 63), (63, (1,) * 192, 0, 0),
           (63, (4,) * 192, 0, 63), (63, (577,) + (1,) * 191, 0, 63), (1, (768,), 191, 1), R.TIMING]


@pytest.mark.parametrize("n,K,ml,p", CORNERS, ids=lambda v: str(v)[:24])
def test_lds_layout_fits_at_the_corners(n, K, ml, p):
    """Every shape gp_batch admits fits in 160 KiB, with room to spare against the solver's own layout."""
    fwd = np.zeros(1, dtype=np.int64)
    Kp = _lib.pi(np.asarray(K, dtype=np.int64))
    mine = _lib.lib().kvx_gp_batch_diff_lds_bytes(n, len(K) - 1, Kp, ml, p, _lib.pi(fwd))
    m, l = len(K), sum(K)
    N, ldn, ldp = m + ml, n | 1, p | 1
    even = lambda v: (v + 1) & ~1                                                       # noqa: E731
    expect = 8 * (even(n * ldn) + max(even(p * ldn) + even(p * ldp), 2 * even(32 * ldn)) + 4 * even(n) + 3 * even(p) + 6 * even(N) + even(m)
                  + 3 * even(l) + even(even(m + 1) // 2 + even(l) // 2) + 32)
    print("n = %d, m = %d, l = %d, ml = %d, p = %d: %d bytes of LDS, the solver %d" % (n, m, l, ml, p, mine, fwd[0]))
    assert mine == expect and 0 < mine < fwd[0] <= 160 * 1024
    L = _lib.lib()
    assert L.kvx_gp_batch_diff_lds_bytes(64, len(K) - 1, Kp, ml, p, None) == -1 and L.kvx_gp_batch_diff_lds_bytes(n, len(K) - 1, None, ml, p, None) == -1
    assert L.kvx_gp_batch_diff_lds_bytes(n, len(K) - 1, Kp, 193, p, None) == -1 and L.kvx_gp_batch_diff_lds_bytes(n, len(K) - 1, Kp, ml, n + 1, None) == -1
