"""The small-front Cholesky kernels (m <= 128, k <= 64) at their order and pivot-count edges, on the designed systems of
chol_class_cases.py (test_chol_classes_cpu.py pins the designs).  Per case and routing: the factor to the componentwise backward
error bound of Cholesky, the triangular solves to the substitution bound -- both evaluated in numpy.longdouble --, identical bytes
across eager / capturing / replayed factorisations, across the two factor schedules and for a column solved alone or in a block,
the failing column of an indefinite matrix, and the launch counters (kvx_dbg_chol_small_counts) against the launches the realised
fronts, levels and subtrees map to.

Routings (the knobs are read once per factor at its device set-up, so setting them before the first factorize is enough):
  default                                     level schedule;            subtree walks, rhs-major from 48 right-hand sides
  KVX_FACTOR_SUBTREES=1 KVX_WIDE_FROM=0       subtrees by one wave each; subtree walks (blocks of four from 16 right-hand sides)
  KVX_NO_SUBTREES=1                           level schedule;            k_fwd_wave / k_bwd_wave and the LDS kernels per level
"""
import numpy as np
import pytest
import scipy.linalg as sla

import chol_class_cases as cc
from chol_class_cases import LD, U, dense_factor, rho_of, tree_ranges
from kvxopt_amd import _lib
from kvxopt_amd.chol import Factor
from oracle.kvx_oracle import OracleChol

pytestmark = pytest.mark.gpu

NRHS = (1, 3, 16, 18, 64, 70)
ROUTINGS = {"default": {}, "subtrees": {"KVX_FACTOR_SUBTREES": "1", "KVX_WIDE_FROM": "0"}, "levels": {"KVX_NO_SUBTREES": "1"}}
KNOBS = ("KVX_SUB_MAXF", "KVX_NO_SUBTREES", "KVX_FACTOR_SUBTREES", "KVX_WIDE_FROM")

COUNTERS = (["front_wave%d_k%d" % (i, k) for i in (32, 48, 64) for k in (16, 32)] +
            ["front_lds%d_k%d" % (i, k) for i in (96, 128) for k in (32, 64)] + ["factor_subtree%d" % i for i in (32, 48, 64)] +
            ["fwd_wave16", "fwd_wave32", "bwd_wave32", "bwd_wave48", "bwd_wave64", "fwd_lds32", "fwd_lds64", "bwd_lds", "fwd_subtree",
             "bwd_subtree32", "bwd_subtree48", "bwd_subtree64", "fwd_subtree_mr", "bwd_subtree_mr32", "bwd_subtree_mr64",
             "wide_fwd32", "wide_fwd64", "wide_bwd32", "wide_bwd64"])

HITS = {r: {c: 0 for c in COUNTERS} for r in ROUTINGS}      # launches seen per routing over the whole module
HITS_1RHS = {c: 0 for c in COUNTERS}                        # ... of the default routing with one right-hand side
RAN = set()
WORST = {}                                                  # per kernel class of the case's designs: largest rho seen


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


def counters(reset=True):
    out = np.zeros(len(COUNTERS), dtype=np.int64)
    assert _lib.lib().kvx_dbg_chol_small_counts(_lib.pi(out), 1 if reset else 0) == len(COUNTERS)
    return {c: int(v) for c, v in zip(COUNTERS, out)}


def img(m):
    return cc.wave_image(m)


# ---- the launches a factor must enqueue, from its realised fronts ---------------------------------------------------------------
def expect_factor(fronts, level, subs, by_subtree):
    """chol_factor.cpp small_fronts: per level one launch per LDS class and per wave image, each with the template size of the
    largest pivot count in it; KVX_FACTOR_SUBTREES=1: the subtree fronts leave the levels, one launch per image group of subtrees"""
    want = {c: 0 for c in COUNTERS}
    inside = set()
    if by_subtree:
        for lo, hi in subs:
            inside |= set(range(lo, hi + 1))
            want["factor_subtree%d" % img(max(fronts[q][0] for q in range(lo, hi + 1)))] = 1
    for l in set(level):
        groups = {}
        for s, (m, k, _) in enumerate(fronts):
            if level[s] != l or s in inside:
                continue
            c = cc.front_class(m, k)
            if c == cc.CLS_BIG:
                continue
            key = "front_lds%d" % (128 if c == cc.CLS_LDS128 else 96) if c < cc.CLS_WAVE0 else "front_wave%d" % img(m)
            groups[key] = max(groups.get(key, 0), k)
        for key, kmax in groups.items():
            want[key + "_k%d" % ((32 if kmax <= 32 else 64) if "lds" in key else (16 if kmax <= 16 else 32))] += 1
    return want


def expect_solve(fronts, level, subs, sys, nrhs, wide, merged):
    """chol_solve.cpp: enqueue_fwd / enqueue_bwd (merged: every small front outside the subtrees in the LDS kernels' launch of its
    level; otherwise wave and LDS fronts in their own kernels) and the rhs-major sweeps"""
    want = {c: 0 for c in COUNTERS}
    fwd, bwd = sys in (0, 4), sys in (0, 5)
    inside = set()
    for lo, hi in subs:
        inside |= set(range(lo, hi + 1))
    for l in set(level):
        here = [(m, k) for s, (m, k, _) in enumerate(fronts) if level[s] == l and cc.front_class(m, k) != cc.CLS_BIG and
                not (merged and not wide and s in inside)]
        lds = [(m, k) for m, k in here if cc.front_class(m, k) < cc.CLS_WAVE0]
        wav = [(m, k) for m, k in here if cc.front_class(m, k) >= cc.CLS_WAVE0]
        if wide:
            for lst in (lds, wav):
                if lst:
                    sz = 32 if max(k for _, k in lst) <= 32 else 64
                    want["wide_fwd%d" % sz] += fwd
                    want["wide_bwd%d" % sz] += bwd
        elif merged:
            if here:
                want["fwd_lds%d" % (32 if max(k for _, k in here) <= 32 else 64)] += fwd
                want["bwd_lds"] += bwd
        else:
            if wav:
                want["fwd_wave%d" % (16 if max(k for _, k in wav) <= 16 else 32)] += fwd
                want["bwd_wave%d" % img(max(m for m, _ in wav))] += bwd
            if lds:
                want["fwd_lds%d" % (32 if max(k for _, k in lds) <= 32 else 64)] += fwd
                want["bwd_lds"] += bwd
    if merged and not wide and subs:
        sizes = {img(max(fronts[q][0] for q in range(lo, hi + 1))) for lo, hi in subs}
        if nrhs >= 16:
            want["fwd_subtree_mr"] += fwd
            want["bwd_subtree_mr32"] += bwd * (32 in sizes)
            want["bwd_subtree_mr64"] += bwd * bool(sizes - {32})
        else:
            want["fwd_subtree"] += fwd
            if nrhs == 1:
                for z in sizes:
                    want["bwd_subtree%d" % z] += bwd
            else:
                want["bwd_subtree32"] += bwd * (32 in sizes)
                want["bwd_subtree64"] += bwd * bool(sizes - {32})
    return want


# ---- references in longdouble, tree by tree (the systems are block diagonal over their designs) ---------------------------------
def subst(Lb, B, trans):
    """L^-1 B (trans = False) or L^-T B in the precision of the arguments, column-oriented substitution"""
    X = B.copy()
    nb = Lb.shape[0]
    if not trans:
        for j in range(nb):
            X[j] /= Lb[j, j]
            X[j + 1:] -= np.outer(Lb[j + 1:, j], X[j])
    else:
        for j in range(nb - 1, -1, -1):
            X[j] /= Lb[j, j]
            X[:j] -= np.outer(Lb[j, :j], X[j])
    return X


def exact_solve(L, ranges, B, sys, perm):
    """longdouble reference of sys 4 (L X = B), 5 (L' X = B) or 0 (A X = B through P, L) from the factor L"""
    Bp = B[perm] if sys == 0 else B
    X = np.zeros(B.shape, dtype=LD)
    for a, b in ranges:
        Lb, Y = L[a:b, a:b].astype(LD), Bp[a:b].astype(LD)
        if sys in (0, 4):
            Y = subst(Lb, Y, False)
        if sys in (0, 5):
            Y = subst(Lb, Y, True)
        X[a:b] = Y
    if sys == 0:
        out = np.zeros_like(X)
        out[perm] = X
        return out
    return X


def float64_solve(L, ranges, B, sys, perm):
    """the same substitutions in float64 (LAPACK dtrtrs through scipy)"""
    Bp = B[perm] if sys == 0 else B
    X = np.zeros(B.shape)
    for a, b in ranges:
        Y = Bp[a:b]
        if sys in (0, 4):
            Y = sla.solve_triangular(L[a:b, a:b], Y, lower=True, trans=0)
        if sys in (0, 5):
            Y = sla.solve_triangular(L[a:b, a:b], Y, lower=True, trans=1)
        X[a:b] = Y
    if sys == 0:
        out = np.zeros_like(X)
        out[perm] = X
        return out
    return X


def check_substitution(L, ranges, B, X, trans, n, what):
    """|B - L X| <= (n + 1) 2^-53 |L| |X| componentwise (Higham, Thm 8.5: any order of evaluation)"""
    for a, b in ranges:
        Lb = L[a:b, a:b].astype(LD)
        Lb = Lb.T if trans else Lb
        R = np.abs(B[a:b].astype(LD) - Lb @ X[a:b].astype(LD))
        bound = (n + 1) * U * (np.abs(Lb) @ np.abs(X[a:b].astype(LD)))
        assert np.all(R <= bound), (what, float((R / np.maximum(bound, LD(1e-300))).max()))


def set_env(monkeypatch, case, routing):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("KVX_GRAPH_SYNC_INSTANTIATE", "1")      # the third factorisation is then a replay for certain
    for k, v in list(case.env.items()) + list(ROUTINGS[routing].items()):
        monkeypatch.setenv(k, v)


def factor_bytes(F):
    Lp, Li, Lx = F.get_factor()
    return Lp, Li, Lx.copy()


def run_case(case, routing, monkeypatch, level_bytes=None):
    set_env(monkeypatch, case, routing)
    n, cp, ri, vx = case.system()
    _, _, _, vx2 = case.system(seed=case.seed + 1)
    F = Factor(n, cp, ri, "L", opts=cc.OPTS)
    fronts, level, parent, sup = cc.realised(F)
    assert sorted(fronts) == case.fronts
    perm = F.perm()
    ip = np.empty(n, dtype=np.int64)
    ip[perm] = np.arange(n)
    ranges = tree_ranges(case, ip)
    merged = routing != "levels"
    subs = cc.pick_subtrees(fronts, parent, sup, cc.default_maxf(n, case.env)) if merged else []
    A = cc.dense_lower(n, cp, ri, vx)
    A2 = cc.dense_lower(n, cp, ri, vx2)
    O = None
    if not case.all_small:
        O = OracleChol(n, cp, ri, "L", perm)

    def bound_for(values):
        if O is None:
            return float(n + 3), None
        O.factorize(values)
        ro = rho_of(cc.dense_lower(n, cp, ri, values)[np.ix_(perm, perm)], dense_factor(n, *O.L()), ranges)
        return max(float(n + 3), 4.0 * ro), ro

    # ---- the factor: eager, capturing, replayed with new values, and the first values again
    counters()
    F.factorize(vx)
    got = counters()
    inf = F.info()
    assert (inf["solve_subtrees"], inf["subtree_fronts"]) == (len(subs), sum(hi - lo + 1 for lo, hi in subs)), (case.name, routing, inf)
    want = expect_factor(fronts, level, subs, routing == "subtrees")
    assert got == want, (case.name, routing, "factor launches", {k: (got[k], want[k]) for k in got if got[k] != want[k]})
    for k, v in got.items():
        HITS[routing][k] += v
    Lp, Li, L1 = factor_bytes(F)
    F.factorize(vx)
    counters()
    assert np.array_equal(L1, factor_bytes(F)[2]), (case.name, routing, "capturing factorisation: other bytes")
    F.factorize(vx2)
    replay = counters()
    assert not any(replay.values()), (case.name, routing, "the third factorisation enqueued launches: not a replay", replay)
    L3 = factor_bytes(F)[2]
    F.factorize(vx)
    assert np.array_equal(L1, factor_bytes(F)[2]), (case.name, routing, "replayed factorisation: other bytes")
    if level_bytes is not None:
        assert np.array_equal(L1, level_bytes[0]) and np.array_equal(L3, level_bytes[1]), (case.name, routing, "not the bytes of the level schedule")
    for values, Am, Lx, which in ((vx, A, L1, "first"), (vx2, A2, L3, "replayed")):
        rho = rho_of(Am[np.ix_(perm, perm)], dense_factor(n, Lp, Li, Lx), ranges)
        bound, ro = bound_for(values)
        print("rho %-24s %-9s %-8s n=%4d rho=%6.3f bound=%8.1f%s" % (case.name, routing, which, n, rho, bound, "" if ro is None else " rho_oracle=%.3f" % ro))
        key = (case.name.split("_bigroot")[0], O is not None)
        WORST[key] = max(WORST.get(key, (0.0, 0.0)), (rho, ro or 0.0))
        assert rho <= bound, (case.name, routing, which, rho, bound, ro)

    # ---- the solves, with the factor as the device holds it
    L = dense_factor(n, Lp, Li, L1)
    if O is not None:
        O.factorize(vx)
        LO = dense_factor(n, *O.L())
    rng = np.random.default_rng(case.seed + 7)
    for nrhs in NRHS:
        B = np.asfortranarray(rng.uniform(-1.0, 1.0, (n, nrhs)))
        wide = routing != "subtrees" and nrhs >= 48
        for sys in (4, 5, 0):
            counters()
            X = F.solve(np.asfortranarray(B.copy()), sys=sys)
            got = counters()
            want = expect_solve(fronts, level, subs, sys, nrhs, wide, merged)
            assert got == want, (case.name, routing, "solve launches", sys, nrhs, {k: (got[k], want[k]) for k in got if got[k] != want[k]})
            for k, v in got.items():
                HITS[routing][k] += v
                if routing == "default" and nrhs == 1:
                    HITS_1RHS[k] += v
            what = (case.name, routing, "sys", sys, "nrhs", nrhs)
            ref = exact_solve(L, ranges, B, sys, perm)
            err = float(np.abs(X.astype(LD) - ref).max())
            floor = 1e-13 * float(np.abs(ref).max())
            if O is None:
                if sys == 4:
                    check_substitution(L, ranges, B, X, False, n, what)
                elif sys == 5:
                    check_substitution(L, ranges, B, X, True, n, what)
                else:
                    e64 = float(np.abs(float64_solve(L, ranges, B, 0, perm).astype(LD) - ref).max())
                    assert err <= max(4.0 * e64, floor), (what, err, e64)
            else:
                XO = O.solve(np.asfortranarray(B.copy()), sys=sys)
                eo = float(np.abs(XO.astype(LD) - exact_solve(LO, ranges, B, sys, perm)).max())
                assert err <= max(4.0 * eo, floor), (what, err, eo)
            if 1 < nrhs < 64:        # a column solved alone: the same bits as inside the block
                for j in range(nrhs):
                    xj = F.solve(B[:, j].copy(), sys=sys)
                    assert np.array_equal(xj, X[:, j]), (what, "column", j)
    return L1, L3


NAMES = [c.name for c in cc.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_case(name, monkeypatch):
    case = cc.BY_NAME[name]
    lv = run_case(case, "default", monkeypatch)
    run_case(case, "subtrees", monkeypatch, level_bytes=lv)
    run_case(case, "levels", monkeypatch, level_bytes=lv)
    RAN.add(name)


# ---- the failing column -----------------------------------------------------------------------------------------------------------
FAILING = (("leaves_wave32_k16", 32, 16), ("leaves_wave32_k32", 32, 17), ("leaves_wave48_k16", 48, 16), ("leaves_wave48_k32", 48, 32),
           ("leaves_wave64_k16", 64, 16), ("leaves_wave64_k32", 64, 32), ("leaves_lds96_k64", 96, 64), ("leaves_lds128_k64", 128, 64))


def spoil_and_check(F, O, cp, vx, perm, cols, good, what):
    """a negative diagonal at the permuted columns cols: the failing column is the oracle's, and the handle recovers"""
    bad = vx.copy()
    for c in cols:
        bad[cp[perm[c]]] = -1.0 - 0.01 * c               # (the diagonal is the first entry of its column)
    with pytest.raises(ArithmeticError) as eo:
        O.factorize(bad)
    with pytest.raises(ArithmeticError) as eg:
        F.factorize(bad)
    assert eg.value.args[0] == eo.value.args[0] == min(cols), (what, cols, eg.value.args, eo.value.args)
    F.factorize(vx)
    assert np.array_equal(good, factor_bytes(F)[2]), (what, cols, "other bytes after a failed factorisation")


FACTOR_ROUTINGS = ("default", "subtrees")


def walked_fronts(case, n, fronts, parent, sup, routing):
    """the fronts a subtree walk factors under this routing (KVX_FACTOR_SUBTREES=1: k_factor_subtree instead of the level kernels)"""
    if routing != "subtrees":
        return set()
    return {q for lo, hi in cc.pick_subtrees(fronts, parent, sup, cc.default_maxf(n, case.env)) for q in range(lo, hi + 1)}


@pytest.mark.parametrize("routing", FACTOR_ROUTINGS)
@pytest.mark.parametrize("name,m,k", FAILING)
def test_failing_column(name, m, k, routing, monkeypatch):
    case = cc.BY_NAME[name]
    set_env(monkeypatch, case, routing)
    n, cp, ri, vx = case.system()
    F = Factor(n, cp, ri, "L", opts=cc.OPTS)
    fronts, level, parent, sup = cc.realised(F)
    perm = F.perm()
    O = OracleChol(n, cp, ri, "L", perm)
    counters()
    F.factorize(vx)
    got = counters()
    good = factor_bytes(F)[2]
    s = fronts.index((m, k, 0))
    # the wave designs are inside a subtree: with KVX_FACTOR_SUBTREES=1 the failing pivot is met by the walk, which then goes on to
    # the parents of the same subtree
    assert (s in walked_fronts(case, n, fronts, parent, sup, routing)) == (routing == "subtrees" and m <= 64), (name, routing)
    assert (sum(got["factor_subtree%d" % i] for i in (32, 48, 64)) > 0) == (routing == "subtrees"), (name, routing, got)
    js = [0, k - 1] + ([k // 2 - (k // 2) % 2 + 1, k // 2 - (k // 2) % 2] if m > 64 else [])        # LDS classes: an odd and an even interior pivot
    for j in js:
        assert 0 <= j < k
        spoil_and_check(F, O, cp, vx, perm, [sup[s] + j], good, (name, routing, m, k))


@pytest.mark.parametrize("routing", FACTOR_ROUTINGS)
def test_failing_columns_of_one_launch(routing, monkeypatch):
    """two fronts of the same launch fail at once: the smaller column is reported"""
    case = cc.BY_NAME["forest3"]
    set_env(monkeypatch, case, routing)
    n, cp, ri, vx = case.system()
    F = Factor(n, cp, ri, "L", opts=cc.OPTS)
    fronts, level, parent, sup = cc.realised(F)
    perm = F.perm()
    O = OracleChol(n, cp, ri, "L", perm)
    F.factorize(vx)
    good = factor_bytes(F)[2]
    for m, k in ((20, 5), (30, 20), (40, 5), (40, 20), (60, 5), (60, 20), (70, 40), (110, 50)):
        copies = [s for s, f in enumerate(fronts) if f == (m, k, 0)]
        assert len(copies) == 3 and len({level[s] for s in copies}) == 1
        spoil_and_check(F, O, cp, vx, perm, [sup[copies[2]] + 1, sup[copies[0]] + k - 1], good, ("forest3", routing, m, k))
        spoil_and_check(F, O, cp, vx, perm, [sup[copies[1]], sup[copies[2]] + k - 1], good, ("forest3", routing, m, k))


# the leaf systems of the ten factor kernels: between them they launch every instantiation counted below (30 factors)
ENOUGH = tuple("leaves_" + c for c in cc.CLASS_NAMES[3:]) + ("leaves_lds96_k32", "leaves_lds96_k64", "leaves_lds128_k32", "leaves_lds128_k64")


@pytest.fixture(scope="module")
def hits():
    """the launches seen over the module; selected alone, the test below gets the cases of ENOUGH run here"""
    with pytest.MonkeyPatch.context() as mp:
        for name in ENOUGH:
            if name not in RAN:
                test_case(name, mp)
    return HITS


def test_every_kernel_ran(hits):
    """across the cases every instantiation of the small-front family was launched"""
    print("largest rho per system (rho, rho_oracle):", sorted(WORST.items()))
    d, s, l = hits["default"], hits["subtrees"], hits["levels"]
    zero = [c for c in COUNTERS if c.startswith("front_") and d[c] == 0]
    assert not zero, ("factor kernels never launched by the level schedule", zero)
    assert all(s["factor_subtree%d" % i] > 0 for i in (32, 48, 64)), s
    assert all(l[c] > 0 for c in ("fwd_wave16", "fwd_wave32", "bwd_wave32", "bwd_wave48", "bwd_wave64", "fwd_lds32", "fwd_lds64", "bwd_lds")), l
    assert all(l[c] == 0 for c in COUNTERS if "subtree" in c), l
    assert all(HITS_1RHS["bwd_subtree%d" % i] > 0 for i in (32, 48, 64)) and HITS_1RHS["fwd_subtree"] > 0, HITS_1RHS
    assert all(d[c] > 0 for c in ("fwd_lds32", "fwd_lds64", "bwd_lds", "fwd_subtree_mr", "bwd_subtree_mr32", "bwd_subtree_mr64")), d
    assert all(d[c] > 0 for c in ("wide_fwd32", "wide_fwd64", "wide_bwd32", "wide_bwd64")), d
    assert all(s[c] == 0 for c in COUNTERS if c.startswith("wide_")) and s["fwd_subtree_mr"] > 0, s
