"""Every kernel class of the sparse LU path at its size-class and panel-width edges (lu_class_child.py: the knobs are read once per
process, so every setting is a process of its own).  The child holds the factor, the solves and the pivots of every case, after a
factorisation, a refactorisation and a replayed refactorisation, to bounds that follow from the arithmetic; here the launch counters
(kvx_dbg_lu_counts) prove that the kernel the case names did the work:

  k_lu_front_wp<T>         LDS classes, orders 1 .. 112 (test_lds_classes)
  k_lu_front_tiled<T>      more than 512 fronts in a launch (test_multi_front[many20]), KVX_LU_WP=0, KVX_LU_WP_MAXCNT=0
  k_lu_front<true>         KVX_LU_LDS_LEGACY=1            k_lu_front<false>   KVX_LU_UNBLOCKED=1
  k_lub_panel_reg<32,1>, <16,2>, <8,4> and their REUSE twins, the width switches inside one factorisation (test_width_edges,
                           test_first_blocked_fronts, test_multi_front[mixed]: a 300-row front under <16,2>)
  k_lub_trsm left out on a refactorisation without interchanges (pattern c)
  k_lu_fwd / k_lu_bwd and k_lu_*_big_* on both sides of m = 384, unit and non-unit, N and T, 1 and 3 right-hand sides (test_solve_edges)
  k_lub_panel              not pinned: the smallest case (order 4100) takes 18 s per value pattern, see docs/lab.md"""
import pytest

from kvxopt_amd import _lib

import lu_class_child as child

pytestmark = pytest.mark.gpu

PANELS = ("panel_reg32", "panel_reg16", "panel_reg8", "panel_lds")
LDS_KERNELS = ["wp%d" % t for t in range(8)] + ["tiled%d" % t for t in range(8)] + ["lds_legacy"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


def names(orders, patterns="abc"):
    """pattern e (one interchange in a known pivot block) goes with every blocked order"""
    return ["d%d%s" % (n, p) for n in orders for p in patterns + ("e" if n > child.LDS_M else "")
            if not (n == 1 and p == "b")]                                                          # (the zero matrix of order 1 is singular)


def enqueued(st):
    """numeric passes of a step whose launches went through the launchers (a replayed graph enqueues nothing)"""
    return st["passes"] - st["pass_replays"]


def expect_single_front(name, res):
    """default routing of one dense block: exactly the kernels its order maps to, at every step"""
    (n,), pattern = child.case_blocks(name)
    for s, st in enumerate(res["steps"]):
        c, e = st["factor"], enqueued(st)
        assert st["passes"] >= st["calls"] and (s > 0 or st["passes"] == 1), (name, s, st)
        if pattern in "ce" or (s > 0 and st["same_pivots"]):
            assert st["passes"] == st["calls"], (name, s, "a refactorisation that keeps its pivots took another attempt", st)
        if n <= child.LDS_M:
            want = {k: 0 for k in LDS_KERNELS + list(PANELS) + ["unblocked", "gemm", "trsm", "trsm_skipped"]}
            want["wp%d" % child.lds_T(n)] = e
        else:
            steps = child.panel_steps(n, n)
            want = {k: 0 for k in LDS_KERNELS + ["unblocked"]}
            want.update({k: v * e for k, v in steps.items()})
            want["gemm"] = sum(steps[k] for k in PANELS[:3]) * e
            assert c["trsm"] + c["trsm_skipped"] == want["gemm"], (name, s, c)
            if s == 0:
                assert c["trsm_skipped"] == 0, (name, s, c)
            if pattern == "c" and s > 0:                              # no block interchanges: the refactorisation leaves every launch out
                assert c["trsm"] == 0 and c["trsm_skipped"] > 0, (name, s, c)
            if pattern == "e" and s > 0:
                # one interchange, at pivot 20: the host's flags (refresh_swap_steps) name one block.  With the widths of the launch
                # loop it is the block the loop runs at that step; with any other widths the loop would leave out the interchange
                # launch of the block that has the interchange and the factor would miss its bound in the child
                assert c["trsm"] == e and c["trsm_skipped"] == want["gemm"] - e, (name, s, c)
        assert {k: c[k] for k in want} == want, (name, s, c, want)
        big = n > child.SOLVE_BIG_M
        v = st["solve"]
        assert (v["fwd_big"] > 0) == big and (v["bwd_big"] > 0) == big, (name, s, v)
        assert (v["fwd_small"] > 0) == (not big) and (v["bwd_small"] > 0) == (not big), (name, s, v)


def run_default(cases, timeout=300):
    res = child.run_setting({}, cases, timeout=timeout)
    for name in cases:
        expect_single_front(name, res[name])
    return res


def test_lds_classes():
    run_default(names([1, 2, 15, 16, 17, 32, 33, 48, 49, 64, 65, 88, 89, 111, 112]))


def test_first_blocked_fronts():
    run_default(names([113, 128, 129]))


@pytest.mark.parametrize("n", [1024, 1025, 1056, 2048, 2049, 2080])
def test_width_edges(n):
    res = run_default(names([n]))
    steps = child.panel_steps(n, n)
    assert steps["panel_reg32"] == 32 and (steps["panel_reg16"] > 0) == (n > 1024) and (steps["panel_reg8"] > 0) == (n > 2048)
    assert all(res[c]["steps"][1]["factor"]["panel_reg32"] > 0 for c in res)      # (the REUSE twins ran too)


def test_solve_edges():
    run_default(names([384, 385, 416, 513]))


@pytest.mark.parametrize("case", ["mixed", "many20", "two_classes"])
def test_multi_front(case):
    cases = [case + p for p in "abc"]
    res = child.run_setting({}, cases)
    for name in cases:
        orders = child.MULTI[case]
        assert res[name]["info"]["nfront"] == len(orders) and res[name]["info"]["max_front"] == max(orders), res[name]["info"]
        for s, st in enumerate(res[name]["steps"]):
            c, e = st["factor"], enqueued(st)
            if case == "mixed":                                       # the width follows the tallest front: the 300-row front runs under <16,2>
                steps = child.panel_steps(1500, 1500)
                assert steps["panel_reg16"] > 300 // 16
                assert {k: c[k] for k in PANELS} == {k: v * e for k, v in steps.items()}, (name, s, c)
                assert c["wp3"] == e and c["unblocked"] == 0, (name, s, c)           # the block of order 40
                if name[-1] == "c" and s > 0:
                    assert c["trsm"] == 0 and c["trsm_skipped"] > 0, (name, s, c)
            elif case == "many20":                                    # more than 512 fronts in one launch
                assert c["tiled2"] == e and all(c["wp%d" % t] == 0 for t in range(8)), (name, s, c)
            else:                                                     # more than 256 LDS fronts: one launch per class
                assert c["wp1"] == e and c["wp3"] == e and all(c["tiled%d" % t] == 0 for t in range(8)), (name, s, c)


SETTING_CASES = names([16, 48, 64, 88, 112, 129, 1056]) + ["mixeda", "mixedb", "mixedc"]
SETTINGS = {"wp_off": {"KVX_LU_WP": 0}, "wp_maxcnt0": {"KVX_LU_WP_MAXCNT": 0}, "lds_legacy": {"KVX_LU_LDS_LEGACY": 1},
            "unblocked": {"KVX_LU_UNBLOCKED": 1}}


def total(res, part, key):
    return sum(st[part][key] for r in res.values() for st in r["steps"])


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_settings(setting):
    res = child.run_setting(SETTINGS[setting], SETTING_CASES, timeout=420)
    t = {k: total(res, "factor", k) for k in child.COUNTERS}
    if setting in ("wp_off", "wp_maxcnt0"):
        assert all(t["wp%d" % k] == 0 for k in range(8)) and t["lds_legacy"] == 0, t
        for n in (16, 48, 64, 88, 112):
            for p in "abc":
                assert all(st["factor"]["tiled%d" % child.lds_T(n)] == enqueued(st) for st in res["d%d%s" % (n, p)]["steps"]), (n, p)
        assert t["panel_reg32"] > 0 and t["panel_reg16"] > 0, t
    elif setting == "lds_legacy":
        assert t["lds_legacy"] > 0 and all(t[k] == 0 for k in LDS_KERNELS[:-1]), t
        assert t["panel_reg32"] > 0 and t["panel_reg16"] > 0, t
    else:
        assert t["unblocked"] > 0 and all(t[k] == 0 for k in PANELS + ("gemm", "trsm", "trsm_skipped")), t
        assert t["wp1"] > 0 and t["wp7"] > 0, t


def test_graphs_off_gives_the_same_bits():
    base = child.run_setting({}, SETTING_CASES, timeout=420)
    off = child.run_setting({"KVX_LU_GRAPH": 0}, SETTING_CASES, timeout=420)
    for name in SETTING_CASES:
        assert all(st["replays"] == 0 for st in off[name]["steps"]), (name, off[name]["steps"])
        assert off[name]["digest"] == base[name]["digest"], name
        assert any(st["replays"] > 0 for st in base[name]["steps"]), name


def test_no_btf():
    res = child.run_setting({"KVX_LU_NO_BTF": 1}, ["bp_800", "mixeda", "mixedb", "mixedc"])
    assert res["bp_800"]["info"]["factored"] == 1


def test_knobs_are_read_per_factor(monkeypatch):
    """LuKnobs is filled when a numeric object is created: a knob changed inside a process holds for the factors made after it and
    leaves the ones that exist alone"""
    from kvxopt_amd import klu
    from kvxopt_amd.base import spmatrix
    for k in child.KNOBS:
        monkeypatch.delenv(k, raising=False)
    n, cp, ri, v = child.case_matrix("d48a")
    A, As = spmatrix.from_ccs(n, n, cp, ri, v), child.to_csc(n, cp, ri, v)
    Fs = klu.symbolic(A)
    child.counts(reset=True)
    F1 = klu.numeric(A, Fs)
    c1 = child.counts(reset=True)
    monkeypatch.setenv("KVX_LU_WP", "0")
    F2 = klu.numeric(A, Fs)
    c2 = child.counts(reset=True)
    assert klu.numeric(A, Fs, F1) is F1
    c3 = child.counts(reset=True)
    wp = lambda c: sum(c["wp%d" % t] for t in range(8))
    tiled = lambda c: sum(c["tiled%d" % t] for t in range(8))
    assert c1["wp3"] == 1 and wp(c1) == 1 and tiled(c1) == 0 and c1["lds_legacy"] == 0, c1
    assert c2["tiled3"] == 1 and tiled(c2) == 1 and wp(c2) == 0 and c2["lds_legacy"] == 0, c2
    assert c3["tiled3"] == 0 and tiled(c3) == 0 and wp(c3) == c3["wp3"] <= 1, c3          # still wp (or a replay: nothing counted)
    for F in (F1, F2):
        fa, _ = child.factors_from_get_numeric(n, klu.get_numeric(A, Fs, F))
        r = child.factor_ratio(As, fa)
        print("factor ratio %.3e" % r)
        assert r <= 1.0, r
