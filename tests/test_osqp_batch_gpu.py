"""osqp.Problem.solve_batch and the kvx_admm_batch_* entry points on the device against tests/osqp_session_numpy.py (DESIGN
section 11, "A batch on the kept factor").  Member b of a batch is, in the restatement, a copy of the kept Session after
update(q_b, l_b, u_b), solved from zero with adaptive_rho = 0 at the kept rho; statuses and iteration counts are taken from it
at test time, and it takes no decision within 1e-6 of a threshold (asserted from its margins).

Bounds.  Parity (tests 1, 3, 6): a vector's distance to the longdouble restatement is at most 4 x the largest of: the distance
of the single-problem path (kvx_admm_iterate / Problem.solve on the same member: the solve with many right-hand sides sums in
another order than the solve with one, and the margin is taken over that path), the float64 restatement's distance, 1e-13 of
the vector's infinity norm -- factor and floor of test_osqp_gpu.compare.  The 24 residual numbers (test 1): that rule itself, both
restatements evaluated at the state the device holds.  Decisions, frozen members, the kept problem, repeated runs: exact.
Termination (tests 2, 7): the two inequalities of section 11 recomputed in numpy from the returned x_b, y_b.  Every measured
figure is printed before its assertion.
"""
import copy
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import osqp_numpy as R  # noqa: E402
import osqp_session_numpy as N  # noqa: E402
import test_osqp_gpu as G0  # noqa: E402  (device, sp, vec, residuals_at: the helpers of the iteration's own tests)

from kvxopt_amd import _lib, osqp  # noqa: E402

pytestmark = pytest.mark.gpu

QUIET = {"verbose": 0}
TIGHT = {"verbose": 0, "eps_abs": 1e-6, "eps_rel": 1e-6}
MEMBER = {"adaptive_rho": 0, "warm_start": 0, "polish": 0}
PROBE = [0, 63, 64, 69]                                  # first and last member of the first block of 64, and of the partial one


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


def mixed_problem():
    """n = 8, A = [I; I; 1'] (m = 17): the base member and five members, one primal and one dual infeasible."""
    n = 8
    A = np.vstack([np.eye(n), np.eye(n), np.ones((1, n))])
    P = np.diag([2.0, 1.0, 3.0, 1.5, 0.5, 1.0, 2.5, 0.0])
    P[0, 1] = P[1, 0] = 0.3
    rng = np.random.default_rng(77)

    def draw():
        q = rng.standard_normal(n)
        q[7] = -1.0
        l1 = -1.0 + 0.1 * rng.standard_normal(n)
        u1 = l1 + 3.0
        l2 = -0.5 + 0.1 * rng.standard_normal(n)
        u2 = l2 + 3.0
        l1[7] = l2[7] = -R.INFTY
        return q, np.concatenate([l1, l2, [-R.INFTY]]), np.concatenate([u1, u2, [R.INFTY]])

    q, l, u = draw()
    p = {"P": P, "q": q, "A": A, "l": l, "u": u}
    Q, L, U = np.empty((n, 5), order="F"), np.empty((17, 5), order="F"), np.empty((17, 5), order="F")
    for b in range(5):
        Q[:, b], L[:, b], U[:, b] = draw()
    L[n + 2, 1], U[n + 2, 1] = U[2, 1] + 1.0, U[2, 1] + 4.0             # member 1: the same row of A with disjoint bounds
    Q[7, 3] = 1.0                                                       # member 3: unbounded below along x_7
    return p, Q, L, U


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "mixed":
        return mixed_problem()[0]
    return {"generated_P": lambda: R.case_generated(True), "generated_noP": lambda: R.case_generated(False),
            "qp_grid_6_5": lambda: R.case_qp_grid(6, 5)}[name]()


def variants(p, B, seed):
    """B members in order: q = p.q + 0.1 max(1, |p.q|_inf) N(0, 1); one shift 0.05 N(0, 1) per row on both finite bounds."""
    rng = np.random.default_rng(seed)
    n, m = p["q"].size, p["l"].size
    Q, L, U = np.empty((n, B), order="F"), np.empty((m, B), order="F"), np.empty((m, B), order="F")
    for b in range(B):
        Q[:, b] = p["q"] + 0.1 * max(1.0, np.abs(p["q"]).max()) * rng.standard_normal(n)
        shift = 0.05 * rng.standard_normal(m)
        L[:, b] = np.where(p["l"] > -R.INF_FROM, p["l"] + shift, p["l"])
        U[:, b] = np.where(p["u"] < R.INF_FROM, p["u"] + shift, p["u"])
    return Q, L, U


@functools.lru_cache(maxsize=None)
def members(name):
    """The batch of a case: 70 variants (a batch of B < 70 is its first B members), or the five members of the mixed batch."""
    return mixed_problem()[1:] if name == "mixed" else variants(case(name), 70, 31)


def problem(p, opts):
    P = None if p["P"] is None else G0.sp(np.tril(p["P"]))
    return osqp.Problem(G0.vec(p["q"]), G0.sp(p["A"]), G0.vec(p["l"]), G0.vec(p["u"]), P, options=opts)


def options(tight, polish=0, **more):
    return dict(TIGHT if tight else QUIET, polish=polish, **more)


@functools.lru_cache(maxsize=None)
def restated(name, tight=False, polish=0, dtype=np.float64, only=None):
    """The restatement of a batch on the kept problem after one base solve: {"base": info of the base solve, "rho", "members":
    [(status, x, y, info)] (None for members outside `only`), "margin": the closest decision}."""
    p, (Q, L, U) = case(name), members(name)
    opts = options(tight, polish)
    base = N.new_session(p, opts, dtype)
    bstatus, _, _, binfo = N.session_solve(base, opts)
    lb, ub = base.lb64, base.ub64
    out, margins = [], []
    for b in range(Q.shape[1]):
        if only is not None and b not in only:
            out.append(None)
            continue
        M = copy.deepcopy(base)
        assert M.update(Q[:, b], L[:, b], U[:, b]) is False             # no row changes its class
        assert np.array_equal(N.rho_classes(M.lb64, M.ub64), N.rho_classes(lb, ub))
        out.append(N.session_solve(M, dict(opts, **MEMBER), margins))
        assert out[-1][3]["factorisations"] == binfo["factorisations"] + (1 if base.stale else 0)
    return {"base": dict(binfo, status=bstatus), "rho": base.rho, "members": out, "margin": min(margins) if margins else float("inf")}


def expect(rs, B):
    return [t[0] for t in rs["members"][:B]], [t[3]["iterations"] for t in rs["members"][:B]]


def dist(a, ref):
    ref = np.asarray(ref, dtype=np.longdouble)
    return float(np.abs(np.asarray(a, dtype=np.longdouble) - ref).max()) if ref.size else 0.0


def rule(tag, name, batch, single, f64, ref, worst):
    """d_batch <= 4 max(d_single, d_f64, 1e-13 |v|_inf), v the longdouble vector; `worst` collects the ratios d_batch / bound."""
    scale = float(np.abs(np.asarray(ref, dtype=np.float64)).max()) if np.size(ref) else 0.0
    d_batch, d_single, d_f64 = dist(batch, ref), dist(single, ref), dist(f64, ref)
    bound = 4.0 * max(d_single, d_f64, 1e-13 * scale)
    ratio = d_batch / bound if bound else 0.0
    print("%s %-3s batch %.3e  single %.3e  float64 %.3e  bound %.3e  ratio %.3f" % (tag, name, d_batch, d_single, d_f64, bound, ratio))
    worst.append((ratio, tag, name))
    assert d_batch <= bound, (tag, name, d_batch, d_single, d_f64, bound)


def termination_holds(p, q, l, u, x, y, eps, tag):
    P = np.zeros((x.size, x.size)) if p["P"] is None else p["P"]
    ax = p["A"] @ x
    z = np.clip(ax, l, u)
    rp, rd = np.abs(ax - z).max(), np.abs(P @ x + q + p["A"].T @ y).max()
    tp = eps + eps * max(np.abs(ax).max(), np.abs(z).max())
    td = eps + eps * max(np.abs(P @ x).max(), np.abs(p["A"].T @ y).max(), np.abs(q).max())
    assert rp <= tp and rd <= td, (tag, rp, tp, rd, td)
    return rp / tp, rd / td


# ---- 1. iterate parity ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restated_iterates(dtype):
    """{(b, k): state} of the members PROBE of generated_P after k = 25 and 50 iterations from zero at rho = 0.1."""
    p, (Q, L, U) = case("generated_P"), members("generated_P")
    out = {}
    for b in PROBE:
        T = N.new_session(p, QUIET, dtype)
        T.update(Q[:, b], L[:, b], U[:, b])
        for k in (25, 50):
            T.iterate(25)
            out[b, k] = copy.deepcopy(T)
    return out


@pytest.mark.parametrize("k", [25, 50])
def test_iterate_parity(k):
    p, (Q, L, U) = case("generated_P"), members("generated_P")
    r64, rld = restated_iterates(np.float64), restated_iterates(np.longdouble)
    S = G0.device(p, 10)
    worst = []
    try:
        S.batch_begin(Q, L, U)
        res = S.batch_iterate(k, np.ones(70, dtype=np.int64))
        state = S.batch_state()
        assert res.shape == (70, 24)
        for b in PROBE:
            T = G0.device(p, 10)
            try:
                T.update(Q[:, b], L[:, b], U[:, b])
                T.iterate(k)
                single = T.state()
            finally:
                T.close()
            mine = tuple(v[:, b] for v in state)
            for key, g, s, a, ref in zip(("x", "z", "y", "dx", "dy"), mine, single, r64[b, k].state(), rld[b, k].state()):
                rule("k=%d member %d" % (k, b), key, g, s, a, ref, worst)
            # the residual kernels: both restatements evaluate the 24 numbers at the state the device holds for the member
            (res64, _), (resld, sums) = G0.residuals_at(r64[b, k], mine), G0.residuals_at(rld[b, k], mine)
            sentinel = np.asarray(resld == R.NEG_MAX)
            assert np.array_equal(res[b] == R.NEG_MAX, sentinel)
            top = max(abs(float(resld[i])) for i in range(24) if not sentinel[i] and i not in sums)
            for i in range(24):
                if sentinel[i]:
                    continue
                err, own = dist(res[b, i:i + 1], resld[i:i + 1]), dist(res64[i:i + 1], resld[i:i + 1])
                bound = max(4.0 * own, 1e-13 * (float(sums[i]) if i in sums else top))
                assert err <= bound, ("res", b, i, err, own, bound)
    finally:
        S.close()
    print("k=%d tightest: %s" % (k, ", ".join("%s %s %.3f" % (t, n, r) for r, t, n in sorted(worst, reverse=True)[:3])))


# ---- 2. decisions and answers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tight,B", [("generated_P", False, 1), ("generated_P", False, 5), ("generated_P", False, 48),
                                          ("generated_P", False, 64), ("generated_P", False, 70), ("qp_grid_6_5", False, 70),
                                          ("qp_grid_6_5", True, 70), ("generated_noP", False, 70)])
def test_decisions_and_answers(name, tight, B):
    """B = 48 and 64 put the triangular solve at and above its switch to blocks of 64 right-hand sides, 1 and 5 below it, 70
    gives a partial last block."""
    p, (Q, L, U) = case(name), members(name)
    rs = restated(name, tight)
    with problem(p, options(tight)) as K:
        status, _, _ = K.solve()
        base = dict(K.info)
        statuses, X, Y = K.solve_batch(Q[:, :B], L[:, :B], U[:, :B])
        info = K.batch_info
    rstat, rits = expect(rs, B)
    carried = int((info["iterations"].max() - info["iterations"]).sum())
    print("%s eps %.0e B=%d: base %s %d iterations rho %.3g; statuses %s; iterations %d-%d (%d distinct); closest margin %.2e; "
          "frozen member-iterations carried %d of %d" % (name, 1e-6 if tight else 1e-3, B, status, base["iterations"], base["rho"],
                                                         sorted(set(statuses)), info["iterations"].min(), info["iterations"].max(),
                                                         len(set(info["iterations"])), rs["margin"], carried, B * int(info["iterations"].max())))
    assert rs["margin"] >= 1e-6
    assert (status, base["iterations"], base["factorisations"], base["rho"]) == \
        (rs["base"]["status"], rs["base"]["iterations"], rs["base"]["factorisations"], rs["rho"])
    assert statuses == rstat and list(info["iterations"]) == rits
    assert X.shape == (p["q"].size, B) and Y.shape == (p["l"].size, B)
    for key in ("iterations", "pri_res", "dua_res", "obj_val"):
        assert len(info[key]) == B
    assert info["rho"] == base["rho"] and info["factorisations"] == base["factorisations"]
    worst = (0.0, 0.0)
    for b in range(B):
        if statuses[b] == "solved":
            got = termination_holds(p, Q[:, b], L[:, b], U[:, b], X[:, b], Y[:, b], 1e-6 if tight else 1e-3, (name, b))
            worst = max(worst, got)
            xb, Pd = X[:, b], np.zeros((X.shape[0], X.shape[0])) if p["P"] is None else p["P"]
            terms = 0.5 * np.abs(xb) @ np.abs(Pd) @ np.abs(xb) + np.abs(Q[:, b]) @ np.abs(xb)
            assert abs(info["obj_val"][b] - (0.5 * xb @ Pd @ xb + Q[:, b] @ xb)) <= 1e-9 * (1.0 + terms)
    print("   largest residual / tolerance among the solved members: primal %.3f dual %.3f" % worst)
    if name == "generated_noP":
        assert set(statuses) == {"dual infeasible"} and not Y.any()
    else:
        assert set(statuses) == {"solved"}


# ---- 3. mixed statuses -------------------------------------------------------------------------------------------------------------
def single_member(p, opts, rho, q, l, u):
    """The single-problem path on one member: a kept problem at rho, update, solve from zero without adaptive rho."""
    with problem(p, dict(opts, rho=rho, **MEMBER)) as K:
        K.update(G0.vec(q), G0.vec(l), G0.vec(u))
        return K.solve() + (dict(K.info),)


def test_mixed_statuses():
    p, (Q, L, U) = case("mixed"), members("mixed")
    rs, rld = restated("mixed"), restated("mixed", dtype=np.longdouble)
    with problem(p, QUIET) as K:
        K.solve()
        statuses, X, Y = K.solve_batch(Q, L, U)
        info = K.batch_info
    rstat, rits = expect(rs, 5)
    print("mixed: %s, iterations %s, closest margin %.2e" % (statuses, list(info["iterations"]), rs["margin"]))
    assert rs["margin"] >= 1e-6 and expect(rld, 5) == (rstat, rits)
    assert rstat[1] == "primal infeasible" and rstat[3] == "dual infeasible" and [rstat[b] for b in (0, 2, 4)] == ["solved"] * 3
    assert statuses == rstat and list(info["iterations"]) == rits
    worst = []
    for b in range(5):
        sstatus, sx, sy, _ = single_member(p, QUIET, rs["rho"], Q[:, b], L[:, b], U[:, b])
        assert sstatus == statuses[b]
        _, x64, y64, _ = rs["members"][b]
        _, xld, yld, _ = rld["members"][b]
        rule("mixed member %d (%s)" % (b, statuses[b]), "x", X[:, b], sx, x64, xld, worst)
        rule("mixed member %d (%s)" % (b, statuses[b]), "y", Y[:, b], sy, y64, yld, worst)
    assert not X[:, 1].any() and Y[:, 1].any()                          # the certificate of primal infeasibility is a y
    assert X[:, 3].any() and not Y[:, 3].any()                          # that of dual infeasibility an x
    # zero columns for every other status: the same batch stopped at its first check
    with problem(p, dict(QUIET, max_iter=25)) as K:
        s25, X25, Y25 = K.solve_batch(Q, L, U)
    r25 = []
    for b in range(5):
        M = N.new_session(p, QUIET)
        M.update(Q[:, b], L[:, b], U[:, b])
        r25.append(N.session_solve(M, dict(MEMBER, max_iter=25))[0])
    print("mixed at max_iter = 25: %s" % s25)
    assert s25 == r25 and s25[2] == "solved"
    for b in range(5):
        named = s25[b].startswith(("solved", "primal infeasible", "dual infeasible"))
        assert named or (not X25[:, b].any() and not Y25[:, b].any())
    assert "maximum iterations reached" in s25


# ---- 4. frozen means frozen --------------------------------------------------------------------------------------------------------
def test_frozen_means_frozen():
    """State level: members frozen after 25 iterations keep every byte of x, z, y, dx, dy and of their 24 numbers while the
    batch runs on to 200.  Problem level: the member of the mixed batch that is solved at its first check returns the bytes it
    returns when the whole batch stops at max_iter = 25."""
    p, (Q, L, U) = case("generated_P"), members("generated_P")
    frozen = [0, 7, 63, 64, 69]
    S = G0.device(p, 10)
    try:
        S.batch_begin(Q, L, U)
        run = np.ones(70, dtype=np.int64)
        res25 = S.batch_iterate(25, run)
        at25 = S.batch_state()
        run[frozen] = 0
        for _ in range(7):
            res = S.batch_iterate(25, run)
        at200 = S.batch_state()
        for a, b in zip(at25, at200):
            assert a[:, frozen].tobytes() == b[:, frozen].tobytes()
        assert all(at25[0][:, j].tobytes() != at200[0][:, j].tobytes() for j in range(70) if j not in frozen)
        assert res[frozen].tobytes() == res25[frozen].tobytes()
        assert all(np.isfinite(v).all() for v in at200)
        # the members that ran are what they are without frozen neighbours
        T = G0.device(p, 10)
        try:
            T.batch_begin(Q, L, U)
            T.batch_iterate(200, np.ones(70, dtype=np.int64))
            full = T.batch_state()
        finally:
            T.close()
        live = [j for j in range(70) if j not in frozen]
        assert all(a[:, live].tobytes() == b[:, live].tobytes() for a, b in zip(at200, full))
    finally:
        S.close()
    p, (Q, L, U) = case("mixed"), members("mixed")
    with problem(p, QUIET) as K:
        s, X, Y = K.solve_batch(Q, L, U)
        its = list(K.batch_info["iterations"])
    with problem(p, dict(QUIET, max_iter=25)) as K:
        s25, X25, Y25 = K.solve_batch(Q, L, U)
    print("mixed: %s %s; at max_iter = 25: %s" % (s, its, s25))
    assert its[2] == 25 and max(its) > 25 and s[2] == s25[2] == "solved"
    assert X[:, 2].tobytes() == X25[:, 2].tobytes() and Y[:, 2].tobytes() == Y25[:, 2].tobytes()


# ---- 5. the kept problem is untouched --------------------------------------------------------------------------------------------------
def test_kept_problem_is_untouched():
    p, (Q, L, U) = case("generated_P"), members("generated_P")
    with problem(p, QUIET) as K:
        K.solve()
        K.solve_batch(Q, L, U)
        with_batch = K.solve()
        info_a = dict(K.info)
    with problem(p, QUIET) as K:
        K.solve()
        without = K.solve()
        info_b = dict(K.info)
    print(with_batch[0], info_a)
    assert with_batch[0] == without[0] and with_batch[1].tobytes() == without[1].tobytes() and with_batch[2].tobytes() == without[2].tobytes()
    assert info_a == info_b
    assert info_a["iterations"] > 0                                     # the second solve did iterate: from the kept state, on the kept data


# ---- 6. repeatability and chunks -----------------------------------------------------------------------------------------------------
def test_repeatability_and_chunks():
    p, (Q, L, U) = case("generated_P"), members("generated_P")
    probe = (0, 31, 32, 63, 64, 69)                                     # first and last member of the passes of chunk = 32
    rs, rld = restated("generated_P"), restated("generated_P", dtype=np.longdouble, only=probe)
    with problem(p, QUIET) as K:
        K.solve()
        first = K.solve_batch(Q, L, U)
        its = K.batch_info["iterations"].copy()
        second = K.solve_batch(Q, L, U)
        assert first[0] == second[0] and first[1].tobytes() == second[1].tobytes() and first[2].tobytes() == second[2].tobytes()
        assert np.array_equal(its, K.batch_info["iterations"])
        s32, X32, Y32 = K.solve_batch(Q, L, U, chunk=32)
        assert s32 == first[0] and np.array_equal(its, K.batch_info["iterations"])
    worst = []
    for b in probe:
        sstatus, sx, sy, sinfo = single_member(p, QUIET, rs["rho"], Q[:, b], L[:, b], U[:, b])
        assert (sstatus, sinfo["iterations"]) == (s32[b], its[b]) == (rld["members"][b][0], rld["members"][b][3]["iterations"])
        for tag, X, Y in (("chunk 1024", first[1], first[2]), ("chunk 32", X32, Y32)):
            rule("%s member %d" % (tag, b), "x", X[:, b], sx, rs["members"][b][1], rld["members"][b][1], worst)
            rule("%s member %d" % (tag, b), "y", Y[:, b], sy, rs["members"][b][2], rld["members"][b][2], worst)
    print("tightest: %s" % ", ".join("%s %s %.3f" % (t, n, r) for r, t, n in sorted(worst, reverse=True)[:3]))


# ---- 7. after a polish -------------------------------------------------------------------------------------------------------------------
def test_after_a_polish():
    """A solve() with polish = 1 leaves the factor of S_pol: the batch rebuilds S once, counted, and its members are those of
    test 2."""
    p, (Q, L, U) = case("generated_P"), members("generated_P")
    B = 5
    rs = restated("generated_P", polish=1)
    with problem(p, options(False, 1)) as K:
        status, _, _ = K.solve()
        base = dict(K.info)
        assert status == "solved" and base["status_polish"] != 0
        statuses, X, Y = K.solve_batch(Q[:, :B], L[:, :B], U[:, :B])
        info = K.batch_info
        assert info["factorisations"] == base["factorisations"] + 1
        K.solve_batch(Q[:, :B], L[:, :B], U[:, :B])
        assert K.batch_info["factorisations"] == base["factorisations"] + 1        # the factor is S's again
    print("after a polish: %s, iterations %s, factorisations %d -> %d" % (statuses, list(info["iterations"]), base["factorisations"], info["factorisations"]))
    assert rs["margin"] >= 1e-6 and (base["factorisations"], base["rho"]) == (rs["base"]["factorisations"], rs["rho"])
    assert (statuses, list(info["iterations"])) == expect(rs, B)
    for b in range(B):
        assert statuses[b] == "solved"
        termination_holds(p, Q[:, b], L[:, b], U[:, b], X[:, b], Y[:, b], 1e-3, b)
