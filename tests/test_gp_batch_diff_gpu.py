"""solvers.gp_batch_vjp / gp_batch_jvp on the device against the numpy.longdouble restatement of
tests/gp_batch_diff_numpy.py.  The device's own solution `sol` of gp_batch is fed both to the kernel and to the restatement, so
only the derivative is under test.  The rule of tests/test_gp_batch_gpu.py, vectors and matrices to 1e-6 max(|ref|, 1) in the
2-norm, holds at the default refinement count (1) and at the next (2), in both modes and for every output.
tests/test_gp_batch_diff_cpu.py shows what the restatement itself is worth.

Measured on the MI355X, in units of the bound: the figures each test prints, recorded in DESIGN section 22."""
import functools
import types

import numpy as np
import pytest

import gp_batch_diff_numpy as D
import gp_batch_numpy as R
from kvxopt_amd import _lib, gpbatchdiff, solvers

pytestmark = pytest.mark.gpu
VJP_VECTORS, JVP_VECTORS = ("ux", "uy", "uznl", "uzl"), D.SOL_KEYS
COUNTS = (gpbatchdiff.DEFAULT_REFINEMENT, gpbatchdiff.DEFAULT_REFINEMENT + 1)


def members_of(sol, which):
    w = list(which)
    return dict({k: sol[k][:, w] for k in D.SOL_KEYS}, exit=sol["exit"][w])


def perturbations(d, which=None):
    w = slice(None) if which is None else list(which)
    return {"d" + k: (None if v is None else (v[w] if k in D.MATRICES else v[:, w])) for k, v in d.items()}


def make_case(M, options=None, reference=True, seed=1):
    sol = solvers.gp_batch(*R.batch_args(M), options=options)
    gx = np.asfortranarray(np.random.default_rng(seed).standard_normal((M.n, M.B)))
    d = D.direction(M, seed + 1)
    Vr, Jr = D.derivatives(M, sol, gx, d, "longdouble") if reference else (None, None)
    return types.SimpleNamespace(M=M, sol=sol, gx=gx, d=d, Vr=Vr, Jr=Jr)


@functools.lru_cache(maxsize=None)
def case(name, reference=True):
    """The batch, the device's solution of it, a cotangent, a direction in all six data and the longdouble restatement of both
    modes at that solution: computed once per process and left unchanged."""
    return make_case(D.named(name), R.EDGE_OPTIONS.get(name), reference)


def both_modes(C, refinement, which=None):
    opts = {"refinement": refinement}
    sol = C.sol if which is None else members_of(C.sol, which)
    gx = C.gx if which is None else C.gx[:, list(which)]
    V = solvers.gp_batch_vjp(*R.batch_args(C.M, which), sol=sol, gx=gx, options=opts)
    J = solvers.gp_batch_jvp(*R.batch_args(C.M, which), sol=sol, options=opts, **perturbations(C.d, which))
    return V, J


def errors(V, J, Vr, Jr, k):
    """The errors of member k in units of the rule: every vector of both modes and every gradient."""
    e = {v: D.rule(V[v][:, k], Vr[v][:, k]) for v in VJP_VECTORS}
    e.update({"d" + v: D.rule(J[v][:, k], Jr[v][:, k]) for v in JVP_VECTORS})
    for name in D.NAMES:
        if Vr[name] is not None:
            mat = name in D.MATRICES
            e["g" + name] = D.rule(V[name][k] if mat else V[name][:, k], Vr[name][k] if mat else Vr[name][:, k])
    return e


def vjp_bytes(V, k, names=D.NAMES):
    parts = [np.ascontiguousarray(V[v][:, k]).tobytes() for v in VJP_VECTORS] + [np.int64(V["exit"][k]).tobytes()]
    for name in names:
        if V.get(name) is not None:
            parts.append(np.ascontiguousarray(V[name][k] if name in D.MATRICES else V[name][:, k]).tobytes())
    return b"".join(parts)


def jvp_bytes(J, k):
    return b"".join([np.ascontiguousarray(J[v][:, k]).tobytes() for v in JVP_VECTORS] + [np.int64(J["exit"][k]).tobytes()])


def all_zero(V, J, k):
    return not any(V[v][:, k].any() for v in VJP_VECTORS + ("g", "h", "b") if V[v] is not None) \
        and not any(V[v][k].any() for v in D.MATRICES if V[v] is not None) and not any(J[v][:, k].any() for v in JVP_VECTORS)


@pytest.mark.parametrize("name", D.EDGE_NAMES)
def test_edges(name):
    """Both modes, all six gradients, per-member matrices, at the default refinement count and the next.  At n63_p63 A x = b
    pins x, the ux are about 0 and the rule compares absolutely below |ref| = 1; spread700 has g of +-700 and stays finite."""
    C = case(name)
    M, B = C.M, C.M.B
    n, m, ml, p, l = M.n, len(M.K), M.ml, M.p, sum(M.K)
    assert list(C.sol["exit"]) == [0] * B
    for refinement in COUNTS:
        V, J = both_modes(C, refinement)
        assert list(V["exit"]) == list(J["exit"]) == [0] * B
        assert V["ux"].shape == J["x"].shape == (n, B) and V["uy"].shape == J["y"].shape == (p, B)
        assert V["uznl"].shape == J["znl"].shape == J["snl"].shape == (m - 1, B) and V["uzl"].shape == J["zl"].shape == J["sl"].shape == (ml, B)
        assert V["F"].shape == (B, l, n) and V["g"].shape == (l, B)
        assert (V["G"].shape == (B, ml, n) and V["h"].shape == (ml, B)) if ml else (V["G"] is None and V["h"] is None)
        assert (V["A"].shape == (B, p, n) and V["b"].shape == (p, B)) if p else (V["A"] is None and V["b"] is None)
        assert all(np.all(np.isfinite(v)) for v in list(V.values()) + list(J.values()) if v is not None)
        worst = {}
        for k in range(B):
            for key, e in errors(V, J, C.Vr, C.Jr, k).items():
                worst[key] = max(worst.get(key, 0.0), e)
        print("%s refinement %d: largest errors in units of the bound: %s" % (name, refinement, ", ".join("%s %.1e" % kv for kv in worst.items())))
        assert max(worst.values()) <= 1.0, (name, refinement, worst)


def test_members_the_solver_gave_up_are_skipped():
    """n1_k1: every member ends gp_batch with exit 3, so every member is exit 1 here and every output is zero."""
    C = case("n1_k1", reference=False)
    B = C.M.B
    assert list(C.sol["exit"]) == [R.EXIT_RANK] * B
    V, J = both_modes(C, 1)
    assert list(V["exit"]) == list(J["exit"]) == [1] * B
    assert all(all_zero(V, J, k) for k in range(B))


@pytest.mark.parametrize("name", ["mixed_one_term", "k63_64_65", "N192_linear"])
def test_both_modes_agree_on_the_device(name):
    """<gx, dx> = <grads, d theta> per member at the higher refinement count, to 1e-9 relative."""
    C = case(name)
    V, J = both_modes(C, COUNTS[1])
    worst = 0.0
    for k in range(C.M.B):
        lhs = C.gx[:, k] @ J["x"][:, k]
        rhs = D.inner(D.member_gradients(V, k), D.member_perturbation(C.d, k))
        worst = max(worst, abs(lhs - rhs) / abs(lhs))
    print("%s: the identity holds on the device to %.2e relative" % (name, worst))
    assert worst <= 1e-9


@functools.lru_cache(maxsize=None)
def shared_case(B=9):
    """B members that share F, G, A, h, b of member 0 of the mixed batch and differ in the g of their objective block, which
    keeps every member feasible; the same data as B copies; the device solution."""
    M0 = R.named("mixed")
    K, F, G, A, h, b = M0.K, M0.F[0], M0.G[0], M0.A[0], M0.h[:, 0], M0.b[:, 0]
    g = np.tile(M0.g[:, :1], (1, B))
    g[:K[0]] += 0.3 * np.random.default_rng(31).standard_normal((K[0], B))
    g = np.asfortranarray(g)
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))         # noqa: E731
    col = lambda v: np.asfortranarray(np.tile(v.reshape(-1, 1), (1, B)))              # noqa: E731
    copies = types.SimpleNamespace(n=M0.n, K=K, ml=M0.ml, p=M0.p, B=B, F=rep(F), g=g, G=rep(G), h=col(h), A=rep(A), b=col(b))
    shared = (K, F, g, G, h, A, b)
    sol = solvers.gp_batch(*shared)
    gx = np.asfortranarray(np.random.default_rng(32).standard_normal((M0.n, B)))
    return copies, shared, sol, gx


def test_shared_and_per_member_data():
    """The same data given once for all members and as B copies: the shared form returns the sums over the members, the copies
    return per-member gradients, ux, uy, uz and the gradient of g are the same bytes in both, two identical calls give
    identical bytes, and wrt = ("g",) forms no matrix gradient."""
    copies, shared_args, sol, gx = shared_case()
    B = copies.B
    n, l, ml, p = copies.n, sum(copies.K), copies.ml, copies.p
    assert list(sol["exit"]) == [0] * B
    shared = solvers.gp_batch_vjp(*shared_args, sol=sol, gx=gx)
    per = solvers.gp_batch_vjp(*R.batch_args(copies), sol=sol, gx=gx)
    ref = D.derivatives(copies, sol, gx, None, "longdouble", shared=("F", "G", "A", "h", "b"))[0]
    assert shared["F"].shape == (l, n) and shared["G"].shape == (ml, n) and shared["A"].shape == (p, n)
    assert shared["h"].shape == (ml,) and shared["b"].shape == (p,) and shared["g"].shape == (l, B)
    errs = {name: D.rule(shared[name], ref[name]) for name in ("F", "G", "A", "h", "b")}
    errs.update({"sum of per-member " + name: D.rule(per[name].sum(axis=0), shared[name]) for name in D.MATRICES})
    print("shared F, G, A: errors of the sums in units of the bound: %s" % ", ".join("%s %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) <= 1.0
    for k in range(B):
        assert vjp_bytes(shared, k, ("g",)) == vjp_bytes(per, k, ("g",)), k
    again = solvers.gp_batch_vjp(*shared_args, sol=sol, gx=gx)
    assert all(again[name].tobytes() == shared[name].tobytes() for name in D.NAMES + VJP_VECTORS)
    only_g = solvers.gp_batch_vjp(*shared_args, sol=sol, gx=gx, wrt=("g",))
    assert sorted(only_g) == ["exit", "g", "ux", "uy", "uzl", "uznl"] and only_g["g"].tobytes() == shared["g"].tobytes()
    K, F, g, G, h, A, b = shared_args
    mixed = solvers.gp_batch_vjp(K, F, g, copies.G, copies.h, A, b, sol=sol, gx=gx)    # any mixture of the two
    assert mixed["G"].tobytes() == per["G"].tobytes() and mixed["h"].tobytes() == per["h"].tobytes()
    assert mixed["F"].tobytes() == shared["F"].tobytes() and mixed["A"].tobytes() == shared["A"].tobytes()


def test_a_member_does_not_depend_on_its_batch():
    C = make_case(R.named("independence"), reference=False)
    B = C.M.B
    assert B == 300 and list(C.sol["exit"]) == [0] * B
    V, J = both_modes(C, 1)
    assert list(V["exit"]) == list(J["exit"]) == [0] * B
    for k in D.INDEPENDENT:
        Vk, Jk = both_modes(C, 1, which=[k])
        assert vjp_bytes(Vk, 0) == vjp_bytes(V, k) and jvp_bytes(Jk, 0) == jvp_bytes(J, k), k
    V2, J2 = both_modes(C, 1)
    assert all(vjp_bytes(V2, k) == vjp_bytes(V, k) and jvp_bytes(J2, k) == jvp_bytes(J, k) for k in range(B))


def test_mixed_outcomes_in_one_batch():
    """maxiters = 9 on the mixed batch: a member gp_batch did not bring to its optimum is skipped with exit 1 and zeros."""
    C = make_case(R.named("mixed"), {"maxiters": 9}, seed=21)
    M, B = C.M, C.M.B
    V, J = both_modes(C, 1)
    done = C.sol["exit"] == 0
    print("maxiters = 9: exits of gp_batch %s, of the derivative %s" % (C.sol["exit"].tolist(), V["exit"].tolist()))
    assert done.any() and not done.all()
    assert list(V["exit"]) == list(J["exit"]) == [0 if t else 1 for t in done]
    for k in range(B):
        if done[k]:
            assert max(errors(V, J, C.Vr, C.Jr, k).values()) <= 1.0, k
        else:
            assert all_zero(V, J, k), k
        Vk, Jk = both_modes(C, 1, which=[k])
        assert vjp_bytes(Vk, 0) == vjp_bytes(V, k) and jvp_bytes(Jk, 0) == jvp_bytes(J, k), k


def test_a_bad_slack_ends_one_member_alone():
    """A NaN written into sol['sl'] of one member gives it exit 2 and zeros; it adds nothing to the sums for the shared F, G, A,
    and every other member returns the bytes it had before."""
    copies, shared_args, sol, gx = shared_case()
    B, bad = copies.B, 4
    before = solvers.gp_batch_vjp(*shared_args, sol=sol, gx=gx)
    d = D.direction(copies, 33)
    pert = dict(perturbations(d), dF=d["F"][0], dG=d["G"][0], dA=d["A"][0])
    Jbefore = solvers.gp_batch_jvp(*shared_args, sol=sol, **pert)
    poisoned = dict(sol, sl=sol["sl"].copy())
    poisoned["sl"][3, bad] = np.nan
    V = solvers.gp_batch_vjp(*shared_args, sol=poisoned, gx=gx)
    J = solvers.gp_batch_jvp(*shared_args, sol=poisoned, **pert)
    expect = [2 if k == bad else 0 for k in range(B)]
    assert list(V["exit"]) == list(J["exit"]) == expect
    ref = D.derivatives(copies, poisoned, gx, None, "longdouble", shared=D.MATRICES)[0]
    assert list(ref["exit"]) == expect
    errs = {name: D.rule(V[name], ref[name]) for name in D.MATRICES}
    print("sl[3, %d] = nan: errors of the sums without that member in units of the bound: %s" % (bad, ", ".join("%s %.1e" % kv for kv in errs.items())))
    assert all(np.all(np.isfinite(V[name])) for name in D.MATRICES) and max(errs.values()) <= 1.0
    for k in range(B):
        if k == bad:
            assert not any(V[v][:, k].any() for v in VJP_VECTORS + ("g",)) and not any(J[v][:, k].any() for v in JVP_VECTORS)
        else:
            assert vjp_bytes(V, k, ("g",)) == vjp_bytes(before, k, ("g",)) and jvp_bytes(J, k) == jvp_bytes(Jbefore, k), k


def test_dev_entries_return_the_bytes_of_the_host_entries():
    """The _dev entries on resident buffers, fed by kvx_gp_batch_solve_dev's own s and z (whose row 0 holds the objective row of
    the epigraph form, which the derivative does not read), return the host entries' bytes."""
    C = case("mixed_one_term")
    M, B = C.M, C.M.B
    n, m, ml, p, l = M.n, len(M.K), M.ml, M.p, sum(M.K)
    N = m + ml
    V, J = both_modes(C, 1)
    shared = solvers.gp_batch_vjp(M.K, M.F[0], M.g, M.G, M.h, M.A[0], M.b, sol=C.sol, gx=C.gx, wrt=("F", "A"))
    L = _lib.lib()
    cm = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(-1)             # noqa: E731  members column-major
    cols = lambda a: np.ascontiguousarray(a.T).reshape(-1)                            # noqa: E731
    up = lambda a: _lib.DeviceBuffer.from_array(a)                                    # noqa: E731
    new = lambda count: _lib.DeviceBuffer(8 * max(count, 1))                          # noqa: E731
    Fd, gd, Gd, hd, Ad, bd = up(cm(M.F)), up(cols(M.g)), up(cm(M.G)), up(cols(M.h)), up(cm(M.A)), up(cols(M.b))
    x, y, s, z, stats, iters, code = new(n * B), new(p * B), new(N * B), new(N * B), new(8 * B), new(B), new(B)
    scratch = new(L.kvx_gp_batch_scratch_doubles(n, m - 1, ml, p) * B)
    Kp = _lib.pi(np.asarray(M.K, dtype=np.int64))
    rc = L.kvx_gp_batch_solve_dev(B, n, m - 1, Kp, ml, p, Fd.ptr, l * n, gd.ptr, l, Gd.ptr, ml * n, hd.ptr, ml, Ad.ptr, p * n, bd.ptr, p,
                                  100, 1e-7, 1e-6, 1e-7, x.ptr, y.ptr, s.ptr, z.ptr, stats.ptr, iters.ptr, code.ptr, scratch.ptr)
    _lib.raise_for(rc, "kvx_gp_batch_solve_dev")
    assert x.download(np.float64, n * B).tobytes() == cols(C.sol["x"]).tobytes() and s.download(np.float64, N * B).reshape(B, N)[:, 0].all()
    gxd = up(cols(C.gx))
    head = lambda sF, sA: [B, n, m - 1, Kp, ml, p, Fd.ptr, sF, gd.ptr, l, Gd.ptr, ml * n, Ad.ptr, sA, x.ptr, y.ptr, s.ptr, z.ptr, code.ptr, 1]   # noqa: E731
    ux, uy, uz, us, gg, work = new(n * B), new(p * B), new(N * B), new(N * B), new(l * B), new(l * B)
    gF, gG, gA, gexit = new(B * l * n), new(B * ml * n), new(B * p * n), new(B)
    split = lambda buf: buf.download(np.float64, N * B).reshape(B, N)                 # noqa: E731
    # reverse mode, per-member matrices, no workspace
    rc = L.kvx_gp_batch_vjp_dev(*head(l * n, p * n), gxd.ptr, ux.ptr, uy.ptr, uz.ptr, gg.ptr, gF.ptr, gG.ptr, gA.ptr, None, gexit.ptr)
    _lib.raise_for(rc, "kvx_gp_batch_vjp_dev")
    assert ux.download(np.float64, n * B).tobytes() == cols(V["ux"]).tobytes() and uy.download(np.float64, p * B).tobytes() == cols(V["uy"]).tobytes()
    t = split(uz)
    assert not t[:, 0].any() and np.ascontiguousarray(t[:, 1:m]).tobytes() == cols(V["uznl"]).tobytes()
    assert np.ascontiguousarray(t[:, m:]).tobytes() == cols(V["uzl"]).tobytes() and not gexit.download(np.int64, B).any()
    assert gg.download(np.float64, l * B).tobytes() == cols(V["g"]).tobytes()
    assert gF.download(np.float64, B * l * n).tobytes() == cm(V["F"]).tobytes() and gG.download(np.float64, B * ml * n).tobytes() == cm(V["G"]).tobytes()
    assert gA.download(np.float64, B * p * n).tobytes() == cm(V["A"]).tobytes()
    # reverse mode, F and A of member 0 for all: the sums, G not formed
    rc = L.kvx_gp_batch_vjp_dev(*head(0, 0), gxd.ptr, ux.ptr, uy.ptr, uz.ptr, gg.ptr, gF.ptr, None, gA.ptr, work.ptr, gexit.ptr)
    _lib.raise_for(rc, "kvx_gp_batch_vjp_dev")
    assert gF.download(np.float64, l * n).tobytes() == np.ascontiguousarray(shared["F"].T).tobytes()
    assert gA.download(np.float64, p * n).tobytes() == np.ascontiguousarray(shared["A"].T).tobytes()
    # forward mode
    d = C.d
    dF, dg, dG, dh, dA, db = up(cm(d["F"])), up(cols(d["g"])), up(cm(d["G"])), up(cols(d["h"])), up(cm(d["A"])), up(cols(d["b"]))
    rc = L.kvx_gp_batch_jvp_dev(*head(l * n, p * n), dF.ptr, l * n, dg.ptr, l, dG.ptr, ml * n, dh.ptr, ml, dA.ptr, p * n, db.ptr, p,
                                ux.ptr, uy.ptr, uz.ptr, us.ptr, gexit.ptr)
    _lib.raise_for(rc, "kvx_gp_batch_jvp_dev")
    tz, ts = split(uz), split(us)
    assert ux.download(np.float64, n * B).tobytes() == cols(J["x"]).tobytes() and uy.download(np.float64, p * B).tobytes() == cols(J["y"]).tobytes()
    assert not tz[:, 0].any() and not ts[:, 0].any() and not gexit.download(np.int64, B).any()
    for key, part in (("znl", tz[:, 1:m]), ("zl", tz[:, m:]), ("snl", ts[:, 1:m]), ("sl", ts[:, m:])):
        assert np.ascontiguousarray(part).tobytes() == cols(J[key]).tobytes(), key
