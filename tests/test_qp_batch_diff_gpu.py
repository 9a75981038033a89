"""solvers.qp_batch_vjp / qp_batch_jvp on the device against the numpy.longdouble restatement of
tests/qp_batch_diff_numpy.py.  The device's own solution `sol` of qp_batch is fed both to the kernel and to the restatement, so
only the derivative is under test.  The rule of tests/test_qp_batch_gpu.py, vectors and matrices to 1e-6 max(|ref|, 1) in the
2-norm, holds at 1 and 2 refinement steps; without refinement the bound is the larger of the rule and 10 x the error the float64
restatement of the same reduced solve shows against longdouble on the same inputs.  tests/test_qp_batch_diff_cpu.py shows what
the restatement itself is worth and that the end-to-end comparison with central differences of qp_batch is admissible.

Measured on the MI355X, in units of the bound: the figures each test prints, recorded in DESIGN section 20."""
import functools
import types

import numpy as np
import pytest

import qp_batch_diff_numpy as D
import qp_batch_numpy as R
from kvxopt_amd import _lib, solvers

pytestmark = pytest.mark.gpu
VJP_VECTORS, JVP_VECTORS = ("ux", "uy", "uz"), ("x", "y", "z", "s")


def arguments(M, which=None):
    w = slice(None) if which is None else list(which)
    return (M.P[w], M.q[:, w], M.G[w], M.h[:, w], None if M.A is None else M.A[w], None if M.b is None else M.b[:, w])


def members_of(sol, which):
    w = list(which)
    return dict({k: sol[k][:, w] for k in ("x", "y", "s", "z")}, exit=sol["exit"][w])


def perturbations(d, which=None):
    w = slice(None) if which is None else list(which)
    return {"d" + k: (None if v is None else (v[w] if k in "PGA" else v[:, w])) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def case(shape, B=R.SHAPE_B, seed=None, reference=True):
    """The batch, the device's solution of it, a cotangent, a direction in all six data and the longdouble restatement of both
    modes at that solution: computed once per process and left unchanged."""
    seed = D.SEEDS[shape] if seed is None else seed
    M = R.batch(shape, B, seed)
    sol = solvers.qp_batch(*arguments(M))
    gx = np.asfortranarray(np.random.default_rng(seed + 1).standard_normal((M.n, B)))
    d = D.direction(M, seed + 2)
    Vr, Jr = D.derivatives(M, sol, gx, d, "longdouble") if reference else (None, None)
    return types.SimpleNamespace(M=M, sol=sol, gx=gx, d=d, Vr=Vr, Jr=Jr)


def errors(V, J, Vr, Jr, k):
    """The errors of member k in units of the rule: every vector of both modes and every gradient."""
    e = {v: D.rule(V[v][:, k], Vr[v][:, k]) for v in VJP_VECTORS}
    e.update({"d" + v: D.rule(J[v][:, k], Jr[v][:, k]) for v in JVP_VECTORS})
    for name in D.NAMES:
        if Vr[name] is not None:
            e["g" + name] = D.rule(V[name][k] if name in "PGA" else V[name][:, k], Vr[name][k] if name in "PGA" else Vr[name][:, k])
    return e


def both_modes(C, refinement, which=None):
    opts = {"refinement": refinement}
    sol = C.sol if which is None else members_of(C.sol, which)
    gx = C.gx if which is None else C.gx[:, list(which)]
    V = solvers.qp_batch_vjp(*arguments(C.M, which), sol=sol, gx=gx, options=opts)
    J = solvers.qp_batch_jvp(*arguments(C.M, which), sol=sol, options=opts, **perturbations(C.d, which))
    return V, J


def vjp_bytes(V, k, names=D.NAMES):
    parts = [np.ascontiguousarray(V[v][:, k]).tobytes() for v in VJP_VECTORS] + [np.int64(V["exit"][k]).tobytes()]
    for name in names:
        if V.get(name) is not None:
            parts.append(np.ascontiguousarray(V[name][k] if name in "PGA" else V[name][:, k]).tobytes())
    return b"".join(parts)


def jvp_bytes(J, k):
    return b"".join([np.ascontiguousarray(J[v][:, k]).tobytes() for v in JVP_VECTORS] + [np.int64(J["exit"][k]).tobytes()])


@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda s: "n%d-ml%d-p%d" % s)
def test_shape_edges(shape):
    """Both modes, all six gradients, per-member matrices, at 1 and 2 refinement steps.  At p = n the ux are about 0: the rule
    compares absolutely below |ref| = 1."""
    C = case(shape)
    n, ml, p = shape
    B = C.M.B
    assert list(C.sol["exit"]) == [0] * B
    for refinement in (1, 2):
        V, J = both_modes(C, refinement)
        assert list(V["exit"]) == list(J["exit"]) == [0] * B
        assert V["ux"].shape == J["x"].shape == (n, B) and V["uy"].shape == J["y"].shape == (p, B)
        assert V["uz"].shape == J["z"].shape == J["s"].shape == (ml, B)
        assert V["P"].shape == (B, n, n) and V["q"].shape == (n, B) and V["G"].shape == (B, ml, n) and V["h"].shape == (ml, B)
        assert (V["A"].shape == (B, p, n) and V["b"].shape == (p, B)) if p else (V["A"] is None and V["b"] is None)
        assert np.array_equal(V["P"], V["P"].transpose(0, 2, 1))                  # symmetric to the last bit
        worst = {}
        for k in range(B):
            for name, e in errors(V, J, C.Vr, C.Jr, k).items():
                worst[name] = max(worst.get(name, 0.0), e)
        print("%s refinement %d: largest errors in units of the bound: %s" % (shape, refinement, ", ".join("%s %.1e" % kv for kv in worst.items())))
        assert max(worst.values()) <= 1.0, (shape, refinement, worst)


@pytest.mark.parametrize("shape", [(8, 17, 3), (33, 65, 5)], ids=lambda s: "n%d-ml%d-p%d" % s)
def test_both_modes_agree_on_the_device(shape):
    """<gx, dx> = <grads, d theta> per member at 2 refinement steps, to 1e-9 relative."""
    C = case(shape)
    V, J = both_modes(C, 2)
    worst = 0.0
    for k in range(C.M.B):
        lhs = C.gx[:, k] @ J["x"][:, k]
        rhs = D.inner({name: (V[name][k] if name in "PGA" else V[name][:, k]) for name in D.NAMES}, D.member_perturbation(C.d, k))
        worst = max(worst, abs(lhs - rhs) / abs(lhs))
    print("%s: the identity holds on the device to %.2e relative" % (shape, worst))
    assert worst <= 1e-9


def test_refinement_steps():
    """0, 1, 2, 3 steps at (33, 65, 5).  Without refinement the bound is the larger of the rule and 10 x the error of the float64
    restatement of the reduced solve against longdouble on the same inputs; the error must not grow from 0 to 1 steps."""
    C = case((33, 65, 5))
    B = C.M.B
    V0, J0 = D.derivatives(C.M, C.sol, C.gx, C.d, "reduced", 0)
    own = max(max(errors(V0, J0, C.Vr, C.Jr, k).values()) for k in range(B))
    bounds = {0: max(1.0, 10.0 * own), 1: 1.0, 2: 1.0, 3: 1.0}
    worst = {}
    for refinement in (0, 1, 2, 3):
        V, J = both_modes(C, refinement)
        assert list(V["exit"]) == list(J["exit"]) == [0] * B
        worst[refinement] = max(max(errors(V, J, C.Vr, C.Jr, k).values()) for k in range(B))
    print("(33, 65, 5): largest error in units of the rule at 0 / 1 / 2 / 3 steps: %s; the float64 restatement at 0 steps: %.2e"
          % (" / ".join("%.2e" % worst[r] for r in range(4)), own))
    for refinement, bound in bounds.items():
        assert worst[refinement] <= bound, (refinement, worst, bound)
    assert worst[1] <= worst[0] + bounds[1]


def test_shared_and_per_member_data():
    """The same data given once for all members and as B copies: the shared form returns the sums over the members, the copies
    return per-member gradients, and ux, uy, uz, the gradient of q and every per-member gradient are the same bytes in both."""
    C = case((33, 65, 5))
    M, B = C.M, C.M.B
    P, G, A, h, b = M.P[0], M.G[0], M.A[0], M.h[:, 0], M.b[:, 0]
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))         # noqa: E731
    col = lambda v: np.asfortranarray(np.tile(v.reshape(-1, 1), (1, B)))              # noqa: E731
    copies = types.SimpleNamespace(n=M.n, ml=M.ml, p=M.p, B=B, P=rep(P), q=M.q, G=rep(G), h=col(h), A=rep(A), b=col(b))
    sol = solvers.qp_batch(P, M.q, G, h, A, b)
    assert list(sol["exit"]) == [0] * B
    shared = solvers.qp_batch_vjp(P, M.q, G, h, A, b, sol=sol, gx=C.gx)
    per = solvers.qp_batch_vjp(*arguments(copies), sol=sol, gx=C.gx)
    ref = D.vjp_batch(copies, sol, C.gx, "longdouble", shared=("P", "G", "A", "h", "b"))
    assert shared["P"].shape == (M.n, M.n) and shared["G"].shape == (M.ml, M.n) and shared["A"].shape == (M.p, M.n)
    assert shared["h"].shape == (M.ml,) and shared["b"].shape == (M.p,) and shared["q"].shape == (M.n, B)
    errs = {name: D.rule(shared[name], ref[name]) for name in ("P", "G", "A", "h", "b")}
    errs.update({"sum of per-member " + name: D.rule(per[name].sum(axis=0), ref[name]) for name in "PGA"})
    print("(33, 65, 5) shared: errors of the sums in units of the bound: %s" % ", ".join("%s %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) <= 1.0
    assert np.array_equal(shared["P"], shared["P"].T)
    for k in range(B):
        assert vjp_bytes(shared, k, ("q",)) == vjp_bytes(per, k, ("q",)), k
    mixed = solvers.qp_batch_vjp(P, M.q, rep(G), col(h), A, b, sol=sol, gx=C.gx)       # any mixture of the two
    assert mixed["G"].tobytes() == per["G"].tobytes() and mixed["h"].tobytes() == per["h"].tobytes()
    assert mixed["P"].tobytes() == shared["P"].tobytes() and mixed["A"].tobytes() == shared["A"].tobytes()
    only_q = solvers.qp_batch_vjp(P, M.q, G, h, A, b, sol=sol, gx=C.gx, wrt=("q",))
    assert sorted(only_q) == ["exit", "q", "ux", "uy", "uz"] and only_q["q"].tobytes() == shared["q"].tobytes()
    col_h = solvers.qp_batch_vjp(P, M.q, G, h.reshape(-1, 1), A, b, sol=sol, gx=C.gx, wrt=("h",))
    assert col_h["h"].shape == (M.ml, 1) and col_h["h"].tobytes() == shared["h"].tobytes()


@functools.lru_cache(maxsize=None)
def shared_matrices_case():
    """B = 300 members at (16, 33, 2) that share everything of member 0 but q, their device solution and the longdouble
    gradients per member."""
    shape, B, seed = R.INDEPENDENCE
    M = R.batch(shape, B, seed)
    data = (M.P[0], M.q, M.G[0], M.h[:, 0], M.A[0], M.b[:, 0])
    sol = solvers.qp_batch(*data)
    gx = np.asfortranarray(np.random.default_rng(11).standard_normal((M.n, B)))
    rep = lambda a: np.broadcast_to(a, (B,) + a.shape)                                # noqa: E731
    col = lambda v: np.tile(v.reshape(-1, 1), (1, B))                                 # noqa: E731
    same = types.SimpleNamespace(n=M.n, ml=M.ml, p=M.p, B=B, P=rep(data[0]), q=M.q, G=rep(data[2]), h=col(data[3]), A=rep(data[4]), b=col(data[5]))
    return data, sol, gx, D.vjp_batch(same, sol, gx, "longdouble")


@pytest.mark.parametrize("B", [1, 63, 64, 65, 300])
def test_sum_over_the_members(B):
    """k_batch_outer_sum at batch sizes around its split of the members."""
    (P, q, G, h, A, b), sol, gx, ref = shared_matrices_case()
    assert list(sol["exit"][:B]) == [0] * B
    call = lambda: solvers.qp_batch_vjp(P, q[:, :B], G, h, A, b, sol=members_of(sol, range(B)), gx=gx[:, :B], wrt=("P", "G", "A"))   # noqa: E731
    V = call()
    errs = {name: D.rule(V[name], ref[name][:B].sum(axis=0)) for name in "PGA"}
    print("B = %d: errors of the sums in units of the bound: %s" % (B, ", ".join("%s %.1e" % kv for kv in errs.items())))
    assert list(V["exit"]) == [0] * B and max(errs.values()) <= 1.0
    again = call()
    assert all(V[name].tobytes() == again[name].tobytes() for name in "PGA")


def test_a_member_does_not_depend_on_its_batch():
    shape, B, seed = R.INDEPENDENCE
    C = case(shape, B, seed, reference=False)
    assert list(C.sol["exit"]) == [0] * B
    V, J = both_modes(C, 1)
    assert list(V["exit"]) == list(J["exit"]) == [0] * B
    for k in (0, 63, 64, 299):
        Vk, Jk = both_modes(C, 1, which=[k])
        assert vjp_bytes(Vk, 0) == vjp_bytes(V, k) and jvp_bytes(Jk, 0) == jvp_bytes(J, k), k
    V2, J2 = both_modes(C, 1)
    assert all(vjp_bytes(V2, k) == vjp_bytes(V, k) and jvp_bytes(J2, k) == jvp_bytes(J, k) for k in range(B))


def all_zero(V, J, k):
    return not any(V[v][:, k].any() for v in VJP_VECTORS + ("q", "h", "b")) and not any(V[v][k].any() for v in "PGA") \
        and not any(J[v][:, k].any() for v in JVP_VECTORS)


def test_mixed_outcomes_in_one_batch():
    """maxiters = 6 on the mixed batch: a member qp_batch did not bring to its optimum is skipped with exit 1 and zeros."""
    shape, B, seed = R.MIXED
    M = R.batch(shape, B, seed)
    d = D.direction(M, 21)
    gx = np.asfortranarray(np.random.default_rng(22).standard_normal((M.n, B)))
    C = types.SimpleNamespace(M=M, sol=solvers.qp_batch(*arguments(M), options={"maxiters": 6}), gx=gx, d=d)
    V, J = both_modes(C, 1)
    done = C.sol["exit"] == 0
    print("maxiters = 6: exits of qp_batch %s, of the derivative %s" % (C.sol["exit"].tolist(), V["exit"].tolist()))
    assert done.any() and not done.all()
    assert list(V["exit"]) == list(J["exit"]) == [0 if t else 1 for t in done]
    Vr, Jr = D.derivatives(M, C.sol, gx, d, "longdouble")
    for k in range(B):
        if done[k]:
            assert max(errors(V, J, Vr, Jr, k).values()) <= 1.0, k
        else:
            assert all_zero(V, J, k), k
        Vk, Jk = both_modes(C, 1, which=[k])
        assert vjp_bytes(Vk, 0) == vjp_bytes(V, k) and jvp_bytes(Jk, 0) == jvp_bytes(J, k), k


@pytest.mark.parametrize("poison", [0.0, np.nan])
def test_a_bad_slack_ends_one_member_alone(poison):
    """The mixed batch with the P of member 0 for all, maxiters = 6: members end with exit 0 and 1.  A 0 or a NaN written into
    sol['s'] of a member that was done gives it exit 2 and zeros; it adds nothing to the sum for the shared P, and every other
    member returns the bytes of its solo run."""
    shape, B, seed = R.MIXED
    M0 = R.batch(shape, B, seed)
    P = M0.P[0]
    M = types.SimpleNamespace(**dict(vars(M0), P=np.ascontiguousarray(np.broadcast_to(P, M0.P.shape))))
    d = D.direction(M, 23)
    gx = np.asfortranarray(np.random.default_rng(24).standard_normal((M.n, B)))
    args = (P,) + arguments(M)[1:]
    sol = solvers.qp_batch(*args, options={"maxiters": 6})
    done = np.flatnonzero(sol["exit"] == 0)
    assert 2 <= len(done) < B, sol["exit"]
    bad = int(done[0])
    sol = dict(sol, s=sol["s"].copy())
    sol["s"][3, bad] = poison
    pert = perturbations(d)
    pert["dP"] = d["P"][0]
    V = solvers.qp_batch_vjp(*args, sol=sol, gx=gx)
    J = solvers.qp_batch_jvp(*args, sol=sol, **pert)
    expect = [(2 if k == bad else 0) if sol["exit"][k] == 0 else 1 for k in range(B)]
    print("s[3, %d] = %s: exits of qp_batch %s, of the derivative %s" % (bad, poison, sol["exit"].tolist(), V["exit"].tolist()))
    assert list(V["exit"]) == list(J["exit"]) == expect
    ref = D.vjp_batch(M, sol, gx, "longdouble", shared=("P",))
    assert list(ref["exit"]) == expect and np.all(np.isfinite(V["P"])) and D.rule(V["P"], ref["P"]) <= 1.0
    for k in range(B):
        if expect[k]:
            assert not any(V[v][:, k].any() for v in VJP_VECTORS + ("q", "h", "b")) and not V["G"][k].any() and not V["A"][k].any(), k
            assert not any(J[v][:, k].any() for v in JVP_VECTORS), k
        one = tuple(a[[k]] if a.ndim == 3 else a[:, [k]] for a in arguments(M)[1:])
        solo = members_of(sol, [k])
        Vk = solvers.qp_batch_vjp(P, *one, sol=solo, gx=gx[:, [k]], wrt=("q", "G", "h", "A", "b"))
        Jk = solvers.qp_batch_jvp(P, *one, sol=solo, **dict(perturbations(d, [k]), dP=d["P"][0]))
        names = ("q", "G", "h", "A", "b")
        assert vjp_bytes(Vk, 0, names) == vjp_bytes(V, k, names) and jvp_bytes(Jk, 0) == jvp_bytes(J, k), k


def test_dev_entries_return_the_bytes_of_the_host_entries():
    C = case((8, 17, 3))
    M, B = C.M, C.M.B
    n, ml, p = M.n, M.ml, M.p
    V, J = both_modes(C, 1)
    shared = solvers.qp_batch_vjp(M.P[0], M.q, M.G, M.h, M.A[0], M.b, sol=C.sol, gx=C.gx, wrt=("P", "A"))
    L = _lib.lib()
    cm = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(-1)             # noqa: E731  members column-major
    cols = lambda a: np.ascontiguousarray(a.T).reshape(-1)                            # noqa: E731
    up = lambda a: _lib.DeviceBuffer.from_array(a)                                    # noqa: E731
    new = lambda count: _lib.DeviceBuffer(8 * max(count, 1))                          # noqa: E731
    Pd, Gd, Ad = up(cm(M.P)), up(cm(M.G)), up(cm(M.A))
    x, y, s, z = (up(cols(C.sol[v])) for v in ("x", "y", "s", "z"))
    code, gxd = up(C.sol["exit"].astype(np.int64)), up(cols(C.gx))
    head = lambda sP, sA: [B, n, ml, p, Pd.ptr, sP, Gd.ptr, ml * n, Ad.ptr, sA, x.ptr, y.ptr, s.ptr, z.ptr, code.ptr, 1]       # noqa: E731
    ux, uy, uz, us, gP, gG, gA, gexit = new(n * B), new(p * B), new(ml * B), new(ml * B), new(B * n * n), new(B * ml * n), new(B * p * n), new(B)
    # reverse mode, per-member matrices
    rc = L.kvx_qp_batch_vjp_dev(*head(n * n, p * n), gxd.ptr, ux.ptr, uy.ptr, uz.ptr, gP.ptr, gG.ptr, gA.ptr, gexit.ptr)
    _lib.raise_for(rc, "kvx_qp_batch_vjp_dev")
    assert ux.download(np.float64, n * B).tobytes() == cols(V["ux"]).tobytes() and uy.download(np.float64, p * B).tobytes() == cols(V["uy"]).tobytes()
    assert uz.download(np.float64, ml * B).tobytes() == cols(V["uz"]).tobytes() and not gexit.download(np.int64, B).any()
    assert gP.download(np.float64, B * n * n).tobytes() == cm(V["P"]).tobytes() and gG.download(np.float64, B * ml * n).tobytes() == cm(V["G"]).tobytes()
    assert gA.download(np.float64, B * p * n).tobytes() == cm(V["A"]).tobytes()
    # reverse mode, P and A of member 0 for all: the sums, G not formed
    rc = L.kvx_qp_batch_vjp_dev(*head(0, 0), gxd.ptr, ux.ptr, uy.ptr, uz.ptr, gP.ptr, None, gA.ptr, gexit.ptr)
    _lib.raise_for(rc, "kvx_qp_batch_vjp_dev")
    assert gP.download(np.float64, n * n).tobytes() == np.ascontiguousarray(shared["P"].T).tobytes()
    assert gA.download(np.float64, p * n).tobytes() == np.ascontiguousarray(shared["A"].T).tobytes()
    # forward mode
    dP, dq, dG, dh, dA, db = up(cm(C.d["P"])), up(cols(C.d["q"])), up(cm(C.d["G"])), up(cols(C.d["h"])), up(cm(C.d["A"])), up(cols(C.d["b"]))
    rc = L.kvx_qp_batch_jvp_dev(*head(n * n, p * n), dP.ptr, n * n, dq.ptr, n, dG.ptr, ml * n, dh.ptr, ml, dA.ptr, p * n, db.ptr, p,
                                ux.ptr, uy.ptr, uz.ptr, us.ptr, gexit.ptr)
    _lib.raise_for(rc, "kvx_qp_batch_jvp_dev")
    got = {"x": ux.download(np.float64, n * B), "y": uy.download(np.float64, p * B), "z": uz.download(np.float64, ml * B),
           "s": us.download(np.float64, ml * B)}
    assert all(got[v].tobytes() == cols(J[v]).tobytes() for v in JVP_VECTORS) and not gexit.download(np.int64, B).any()


def test_end_to_end_against_central_differences_of_qp_batch():
    """qp_batch at the tolerances tests/test_qp_batch_diff_cpu.py found admissible, its directional derivative from
    qp_batch_jvp, and central differences of qp_batch itself along the same direction; the bound is 10 x what the float64
    restatement shows for this batch on the CPU (D.E2E_ERROR)."""
    shape = D.E2E_SHAPE
    M = R.batch(shape, R.SHAPE_B, D.SEEDS[shape])
    d = D.direction(M, 1000 + shape[0])
    sol, plus, minus = (solvers.qp_batch(*arguments(m), options=D.E2E_TOL) for m in (M, D.moved(M, d, D.EPS), D.moved(M, d, -D.EPS)))
    J = solvers.qp_batch_jvp(*arguments(M), sol=sol, **perturbations(d))
    errs = D.fd_errors(J, plus, minus)
    left = int(np.isnan(errs).sum())
    print("%s at %s: distance to central differences of qp_batch %s, %d left out; the bound %.2e"
          % (shape, D.E2E_TOL, ["%.1e" % e for e in errs], left, 10 * D.E2E_ERROR))
    assert left <= M.B // 4 and np.nanmax(errs) <= 10 * D.E2E_ERROR
