"""solvers.coneqp_batch_vjp / coneqp_batch_jvp on the device against the numpy.longdouble restatement of
tests/coneqp_batch_diff_numpy.py.  The device's own solution `sol` of coneqp_batch at abstol = reltol = feastol = 1e-8 is fed both to
the kernel and to the restatement, so only the derivative is under test.  The bound is the larger of the project's rule, vectors and
matrices to 1e-6 max(|ref|, 1) in the 2-norm, and 10 x the distance the float64 restatement shows for that batch on the CPU
(D.ROUNDING, measured by tests/test_coneqp_batch_diff_cpu.py); that is the rule on every batch but (20, 3, (65,), (16,), 3): 1.3.

Measured on the MI355X, in units of the bound: the figures each test prints, recorded in DESIGN section 21."""
import functools
import types

import numpy as np
import pytest

import coneqp_batch_diff_numpy as D
from kvxopt_amd import _lib, coneqpbatchdiff, solvers

pytestmark = pytest.mark.gpu
VJP_VECTORS, JVP_VECTORS = ("ux", "uy", "uz"), ("x", "y", "z", "s")
CENTERING, CENTOL = coneqpbatchdiff.DEFAULT_CENTERING, coneqpbatchdiff.DEFAULT_CENTOL


def arguments(M, which=None):
    w = slice(None) if which is None else list(which)
    return (M.P[w], M.q[:, w], M.G[w], M.h[:, w], M.dims, None if M.A is None else M.A[w], None if M.b is None else M.b[:, w])


def members_of(sol, which):
    w = list(which)
    return dict({k: sol[k][:, w] for k in ("x", "y", "s", "z")}, exit=sol["exit"][w])


def perturbations(d, which=None):
    w = slice(None) if which is None else list(which)
    return {"d" + k: (None if v is None else (v[w] if k in "PGA" else v[:, w])) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def case(name, reference=True):
    """The batch, the device's solution of it, a cotangent, a direction in all six data and the restatements of both modes at that
    solution (longdouble, and float64 as the kernel for the exits): computed once per process and left unchanged."""
    M = D.batch(name)
    sol = solvers.coneqp_batch(*arguments(M), options=D.SOLVE_TOL)
    gx, d = D.cotangent(M, 5), D.direction(M, 6)
    Vr, Jr = D.derivatives(M, sol, gx, d, "longdouble", 0, CENTERING, CENTOL) if reference else (None, None)
    Vf, Jf = D.derivatives(M, sol, gx, d, "reduced", 1, CENTERING, CENTOL) if reference else (None, None)
    return types.SimpleNamespace(M=M, sol=sol, gx=gx, d=d, Vr=Vr, Jr=Jr, Vf=Vf, Jf=Jf)


def errors(V, J, Vr, Jr, k):
    """The errors of member k in units of the rule: every vector of both modes and every gradient."""
    e = {v: D.rule(V[v][:, k], Vr[v][:, k]) for v in VJP_VECTORS if Vr[v].shape[0]}
    e.update({"d" + v: D.rule(J[v][:, k], Jr[v][:, k]) for v in JVP_VECTORS if Jr[v].shape[0]})
    for name in D.NAMES:
        if Vr[name] is not None:
            e["g" + name] = D.rule(V[name][k] if name in "PGA" else V[name][:, k], Vr[name][k] if name in "PGA" else Vr[name][:, k])
    return e


def both_modes(C, which=None, options=None):
    sol = C.sol if which is None else members_of(C.sol, which)
    gx = C.gx if which is None else C.gx[:, list(which)]
    V = solvers.coneqp_batch_vjp(*arguments(C.M, which), sol=sol, gx=gx, options=options)
    J = solvers.coneqp_batch_jvp(*arguments(C.M, which), sol=sol, options=options, **perturbations(C.d, which))
    return V, J


def vjp_bytes(V, k, names=D.NAMES):
    parts = [np.ascontiguousarray(V[v][:, k]).tobytes() for v in VJP_VECTORS]
    parts += [np.int64(V["exit"][k]).tobytes(), np.int64(V["centering steps"][k]).tobytes(), np.float64(V["centrality"][k]).tobytes()]
    for name in names:
        if V.get(name) is not None:
            parts.append(np.ascontiguousarray(V[name][k] if name in "PGA" else V[name][:, k]).tobytes())
    return b"".join(parts)


def jvp_bytes(J, k):
    return b"".join([np.ascontiguousarray(J[v][:, k]).tobytes() for v in JVP_VECTORS]
                    + [np.int64(J["exit"][k]).tobytes(), np.int64(J["centering steps"][k]).tobytes(), np.float64(J["centrality"][k]).tobytes()])


def all_zero(V, J, k):
    return not any(V[v][:, k].any() for v in VJP_VECTORS + ("q", "h") + (("b",) if V["b"] is not None else ())) \
        and not any(V[v][k].any() for v in "PGA" if V[v] is not None) and not any(J[v][:, k].any() for v in JVP_VECTORS)


@pytest.mark.parametrize("name", D.SMALL_BATCHES)
def test_batches(name):
    """Both modes, all six gradients, per-member matrices, at the defaults.  The exits are those of the float64 restatement: where
    float64 loses a pivot that longdouble keeps (one member of "p-zero") the kernel loses it too, and returns zeros."""
    C = case(name)
    M, B = C.M, C.M.B
    n, N, p = M.n, M.N, M.p
    bound = max(1.0, 10.0 * D.ROUNDING[name])
    V, J = both_modes(C)
    print("%s: exits of coneqp_batch %s, of the derivative %s, steps %s, largest centrality %.1e"
          % (name, C.sol["exit"].tolist(), V["exit"].tolist(), V["centering steps"].tolist(), np.nanmax(V["centrality"])))
    assert list(V["exit"]) == list(J["exit"]) == list(C.Vf["exit"]) and list(V["centering steps"]) == list(J["centering steps"])
    assert int((C.sol["exit"] != 0).sum() + (V["exit"] > 1).sum()) <= B // 12
    assert V["ux"].shape == J["x"].shape == (n, B) and V["uy"].shape == J["y"].shape == (p, B)
    assert V["uz"].shape == J["z"].shape == J["s"].shape == (N, B)
    assert V["P"].shape == (B, n, n) and V["q"].shape == (n, B) and V["G"].shape == (B, N, n) and V["h"].shape == (N, B)
    assert (V["A"].shape == (B, p, n) and V["b"].shape == (p, B)) if p else (V["A"] is None and V["b"] is None)
    assert np.array_equal(V["P"], V["P"].transpose(0, 2, 1))                  # symmetric to the last bit
    for _, o, _, m in D.SDN.blocks(M.Ms, M.s):                                # and so are the 's' blocks of uz, dz, ds and of the rows of G
        for u in (V["uz"], J["z"], J["s"], V["h"]):
            blk = u[o:o + m * m].reshape(m, m, B)
            assert np.array_equal(blk, blk.transpose(1, 0, 2))
        blk = V["G"][:, o:o + m * m, :].reshape(B, m, m, n)
        assert np.array_equal(blk, blk.transpose(0, 2, 1, 3))
    worst = {}
    for k in range(B):
        if C.Vf["exit"][k] == 0:
            assert V["exit"][k] == 0 and V["centrality"][k] <= CENTOL and C.Vr["exit"][k] == 0, k
            for key, e in errors(V, J, C.Vr, C.Jr, k).items():
                worst[key] = max(worst.get(key, 0.0), e)
        else:
            assert V["exit"][k] and all_zero(V, J, k), k
    print("%s: largest errors in units of the bound: %s" % (name, ", ".join("%s %.1e" % (a, b / bound) for a, b in worst.items())))
    assert max(worst.values()) <= bound, (name, worst)


@pytest.mark.parametrize("name", ["mixed", D.shape_name(D.MANY)])
def test_both_modes_agree_on_the_device(name):
    """<gx, dx> = <grads, d theta> per member at 2 refinement steps, to 1e-9 relative."""
    C = case(name)
    V, J = both_modes(C, options={"refinement": 2})
    worst = 0.0
    for k in range(C.M.B):
        lhs = C.gx[:, k] @ J["x"][:, k]
        rhs = D.inner(C.M, {v: (V[v][k] if v in "PGA" else V[v][:, k]) for v in D.NAMES}, D.QDN.member_perturbation(C.d, k))
        worst = max(worst, abs(lhs - rhs) / abs(lhs))
    print("%s: the identity holds on the device to %.2e relative" % (name, worst))
    assert list(V["exit"]) == [0] * C.M.B and worst <= 1e-9


def test_shared_and_per_member_data():
    """The same data given once for all members and as B copies: the shared form returns the sums over the members, the copies
    return per-member gradients, and ux, uy, uz, the gradient of q and every per-member gradient are the same bytes in both."""
    M = D.batch("mixed")
    B = M.B
    gx = D.cotangent(M, 5)
    P, G, A, h, b = M.P[0], M.G[0], M.A[0], M.h[:, 0], M.b[:, 0]
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))         # noqa: E731
    col = lambda v: np.asfortranarray(np.tile(v.reshape(-1, 1), (1, B)))              # noqa: E731
    copies = types.SimpleNamespace(**dict(vars(M), P=rep(P), G=rep(G), h=col(h), A=rep(A), b=col(b)))
    sol = solvers.coneqp_batch(P, M.q, G, h, M.dims, A, b, options=D.SOLVE_TOL)
    assert list(sol["exit"]) == [0] * B
    call = lambda: solvers.coneqp_batch_vjp(P, M.q, G, h, M.dims, A, b, sol=sol, gx=gx)          # noqa: E731
    shared = call()
    per = solvers.coneqp_batch_vjp(*arguments(copies), sol=sol, gx=gx)
    ref = D.derivatives(copies, sol, gx, None, "longdouble", 0, CENTERING, CENTOL, shared=("P", "G", "A", "h", "b"))[0]
    assert list(shared["exit"]) == list(ref["exit"]) == [0] * B
    assert shared["P"].shape == (M.n, M.n) and shared["G"].shape == (M.N, M.n) and shared["A"].shape == (M.p, M.n)
    assert shared["h"].shape == (M.N,) and shared["b"].shape == (M.p,) and shared["q"].shape == (M.n, B)
    errs = {name: D.rule(shared[name], ref[name]) for name in ("P", "G", "A", "h", "b")}
    errs.update({"sum of per-member " + name: D.rule(per[name].sum(axis=0), ref[name]) for name in "PGA"})
    print("mixed, shared: errors of the sums in units of the bound: %s" % ", ".join("%s %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) <= 1.0
    assert np.array_equal(shared["P"], shared["P"].T)
    for k in range(B):
        assert vjp_bytes(shared, k, ("q",)) == vjp_bytes(per, k, ("q",)), k
    mixed = solvers.coneqp_batch_vjp(P, M.q, rep(G), col(h), M.dims, A, b, sol=sol, gx=gx)       # any mixture of the two
    assert mixed["G"].tobytes() == per["G"].tobytes() and mixed["h"].tobytes() == per["h"].tobytes()
    assert mixed["P"].tobytes() == shared["P"].tobytes() and mixed["A"].tobytes() == shared["A"].tobytes()
    only_q = solvers.coneqp_batch_vjp(P, M.q, G, h, M.dims, A, b, sol=sol, gx=gx, wrt=("q",))
    assert sorted(only_q) == ["centering steps", "centrality", "exit", "q", "ux", "uy", "uz"] and only_q["q"].tobytes() == shared["q"].tobytes()
    again = call()
    assert all(np.asarray(shared[k]).tobytes() == np.asarray(again[k]).tobytes() for k in shared)


def test_a_member_does_not_depend_on_its_batch():
    C = case("independence", reference=False)
    B = C.M.B
    V, J = both_modes(C)
    assert list(V["exit"]) == list(J["exit"]) and int((V["exit"] != 0).sum()) <= B // 12
    for k in (0, 63, 64, 299):
        Vk, Jk = both_modes(C, which=[k])
        assert vjp_bytes(Vk, 0) == vjp_bytes(V, k) and jvp_bytes(Jk, 0) == jvp_bytes(J, k), k
    V2, J2 = both_modes(C)
    assert all(vjp_bytes(V2, k) == vjp_bytes(V, k) and jvp_bytes(J2, k) == jvp_bytes(J, k) for k in range(B))


@pytest.mark.parametrize("poison", [0.0, np.nan])
def test_mixed_outcomes_in_one_batch(poison):
    """D.mixed_outcomes(), the P of member 0 for all, solved with maxiters = 6: members end with exit 0 and 1 and the latter are
    skipped with zeros.  A 0 or a NaN written into an 'l' row of sol['s'] of a done member gives it exit 2 and zeros; centering = 1
    gives exit 3 and zeros to the members that need more.  The sum for the shared P stays finite and is the sum over the done members,
    and every member returns the bytes of its solo run."""
    M = D.mixed_outcomes()
    B, P = M.B, M.P[0]
    d, gx = D.direction(M, 23), D.cotangent(M, 24)
    args = lambda w=None: (P,) + arguments(M, w)[1:]                                  # noqa: E731
    sol = solvers.coneqp_batch(*args(), options={"maxiters": 6})
    done = np.flatnonzero(sol["exit"] == 0)
    assert 2 <= len(done) < B, sol["exit"]
    bad = int(done[0])
    sol = dict(sol, s=sol["s"].copy())
    sol["s"][1, bad] = poison
    before = {k: np.array(sol[k], copy=True) for k in ("x", "y", "s", "z", "exit")}
    for options, cap, code in ((None, CENTERING, 0), ({"centering": 1}, 1, 3)):
        V = solvers.coneqp_batch_vjp(*args(), sol=sol, gx=gx, options=options)
        J = solvers.coneqp_batch_jvp(*args(), sol=sol, options=options, **dict(perturbations(d), dP=d["P"][0]))
        ref = D.derivatives(M, sol, gx, None, "longdouble", 0, cap, CENTOL, shared=("P",))[0]
        assert list(V["exit"]) == list(D.derivatives(M, sol, gx, None, "reduced", 1, cap, CENTOL)[0]["exit"])
        print("s[1, %d] = %s, %s: exits of coneqp_batch %s, of the derivative %s" % (bad, poison, options, sol["exit"].tolist(), V["exit"].tolist()))
        assert list(V["exit"]) == list(J["exit"]) == list(ref["exit"])
        assert all((V["exit"][k] == 1) == (sol["exit"][k] != 0) for k in range(B)) and V["exit"][bad] == 2 and code in V["exit"]
        assert all(np.array_equal(sol[k], before[k], equal_nan=True) for k in before)              # sol is never modified
        assert V["P"].shape == (M.n, M.n) and np.all(np.isfinite(V["P"])) and D.rule(V["P"], ref["P"]) <= 1.0
        names = ("q", "G", "h", "A", "b")
        for k in range(B):
            if V["exit"][k]:
                assert not any(V[v][:, k].any() for v in VJP_VECTORS + ("q", "h", "b")) and not V["G"][k].any() and not V["A"][k].any(), k
                assert not any(J[v][:, k].any() for v in JVP_VECTORS), k
            Vk = solvers.coneqp_batch_vjp(*args([k]), sol=members_of(sol, [k]), gx=gx[:, [k]], wrt=names, options=options)
            Jk = solvers.coneqp_batch_jvp(*args([k]), sol=members_of(sol, [k]), options=options, **dict(perturbations(d, [k]), dP=d["P"][0]))
            assert vjp_bytes(Vk, 0, names) == vjp_bytes(V, k, names) and jvp_bytes(Jk, 0) == jvp_bytes(J, k), k


def test_dev_entries_return_the_bytes_of_the_host_entries():
    C = case("mixed")
    M, B = C.M, C.M.B
    n, N, p = M.n, M.N, M.p
    V, J = both_modes(C)
    shared = solvers.coneqp_batch_vjp(M.P[0], M.q, M.G[0], M.h, M.dims, M.A[0], M.b, sol=C.sol, gx=C.gx, wrt=("P", "G", "A"))
    L = _lib.lib()
    cm = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(-1)             # noqa: E731  members column-major
    cols = lambda a: np.ascontiguousarray(a.T).reshape(-1)                            # noqa: E731
    up = lambda a: _lib.DeviceBuffer.from_array(a)                                    # noqa: E731
    new = lambda count: _lib.DeviceBuffer(8 * max(count, 1))                          # noqa: E731
    Pd, qd, Gd, hd, Ad, bd = up(cm(M.P)), up(cols(M.q)), up(cm(M.G)), up(cols(M.h)), up(cm(M.A)), up(cols(M.b))
    x, y, s, z = (up(cols(C.sol[v])) for v in ("x", "y", "s", "z"))
    code, gxd = up(C.sol["exit"].astype(np.int64)), up(cols(C.gx))
    qv, mv = np.asarray(M.qd, dtype=np.int64), np.asarray(M.s, dtype=np.int64)
    head = lambda sP, sG, sA: [B, n, M.ml, len(qv), _lib.pi(qv), len(mv), _lib.pi(mv), p, Pd.ptr, sP, qd.ptr, n, Gd.ptr, sG, hd.ptr, N,      # noqa: E731
                               Ad.ptr, sA, bd.ptr, p, x.ptr, y.ptr, s.ptr, z.ptr, code.ptr, 1, CENTERING, CENTOL]
    ux, uy, uz, us, gP, gG, gA = new(n * B), new(p * B), new(N * B), new(N * B), new(B * n * n), new(B * N * n), new(B * p * n)
    cen, steps, gexit = new(B), new(B), new(B)
    # reverse mode, per-member matrices
    rc = L.kvx_coneqp_batch_vjp_dev(*head(n * n, N * n, p * n), gxd.ptr, ux.ptr, uy.ptr, uz.ptr, gP.ptr, gG.ptr, gA.ptr, cen.ptr, steps.ptr, gexit.ptr)
    _lib.raise_for(rc, "kvx_coneqp_batch_vjp_dev")
    assert ux.download(np.float64, n * B).tobytes() == cols(V["ux"]).tobytes() and uy.download(np.float64, p * B).tobytes() == cols(V["uy"]).tobytes()
    assert uz.download(np.float64, N * B).tobytes() == cols(V["uz"]).tobytes() and not gexit.download(np.int64, B).any()
    assert gP.download(np.float64, B * n * n).tobytes() == cm(V["P"]).tobytes() and gG.download(np.float64, B * N * n).tobytes() == cm(V["G"]).tobytes()
    assert gA.download(np.float64, B * p * n).tobytes() == cm(V["A"]).tobytes()
    assert cen.download(np.float64, B).tobytes() == V["centrality"].tobytes() and steps.download(np.int64, B).tobytes() == V["centering steps"].tobytes()
    # reverse mode, P, G and A of member 0 for all: the sums
    rc = L.kvx_coneqp_batch_vjp_dev(*head(0, 0, 0), gxd.ptr, ux.ptr, uy.ptr, uz.ptr, gP.ptr, gG.ptr, gA.ptr, cen.ptr, steps.ptr, gexit.ptr)
    _lib.raise_for(rc, "kvx_coneqp_batch_vjp_dev")
    assert gexit.download(np.int64, B).tobytes() == shared["exit"].tobytes()
    assert gP.download(np.float64, n * n).tobytes() == np.ascontiguousarray(shared["P"].T).tobytes()
    assert gG.download(np.float64, N * n).tobytes() == np.ascontiguousarray(shared["G"].T).tobytes()
    assert gA.download(np.float64, p * n).tobytes() == np.ascontiguousarray(shared["A"].T).tobytes()
    # forward mode
    dP, dq, dG, dh, dA, db = up(cm(C.d["P"])), up(cols(C.d["q"])), up(cm(C.d["G"])), up(cols(C.d["h"])), up(cm(C.d["A"])), up(cols(C.d["b"]))
    rc = L.kvx_coneqp_batch_jvp_dev(*head(n * n, N * n, p * n), dP.ptr, n * n, dq.ptr, n, dG.ptr, N * n, dh.ptr, N, dA.ptr, p * n, db.ptr, p,
                                    ux.ptr, uy.ptr, uz.ptr, us.ptr, cen.ptr, steps.ptr, gexit.ptr)
    _lib.raise_for(rc, "kvx_coneqp_batch_jvp_dev")
    got = {"x": ux.download(np.float64, n * B), "y": uy.download(np.float64, p * B), "z": uz.download(np.float64, N * B),
           "s": us.download(np.float64, N * B)}
    assert all(got[v].tobytes() == cols(J[v]).tobytes() for v in JVP_VECTORS) and not gexit.download(np.int64, B).any()
