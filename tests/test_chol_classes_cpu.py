"""The designed systems of chol_class_cases.py, on the host: the analysis must cut every one of them into exactly the fronts the
design declares, and together they must cover the order, pivot-count, Schur-complement, child and subtree edges of the small-front
Cholesky kernels (k_front_wave, k_front_lds and the sweeps that go with them).  No device is touched."""
import numpy as np
import pytest

import chol_class_cases as cc
from kvxopt_amd.chol import Factor

ENV_KNOBS = ("KVX_SUB_MAXF", "KVX_NO_SUBTREES", "KVX_FACTOR_SUBTREES", "KVX_WIDE_FROM")


def analysed(case, monkeypatch):
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    n, cp, ri, vx = case.system()
    return Factor(n, cp, ri, "L", opts=cc.OPTS), (n, cp, ri, vx)


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_design_is_exact(name, monkeypatch):
    case = cc.BY_NAME[name]
    F, (n, cp, ri, vx) = analysed(case, monkeypatch)
    assert n == case.n < 1500
    fronts, level, parent, sup = cc.realised(F)
    assert sorted(fronts) == case.fronts, (name, sorted(set(fronts) - set(case.fronts)), sorted(set(case.fronts) - set(fronts)))
    # the permutation keeps every tree of the forest together: the GPU tests evaluate their bounds tree by tree
    ip = np.empty(n, dtype=np.int64)
    ip[F.perm()] = np.arange(n)
    for first, cols in case.trees():
        pos = np.sort(ip[first:first + cols])
        assert pos[-1] - pos[0] == cols - 1, (name, first)
    # the subtrees of the sweeps: the restatement the GPU tests route by agrees with the library, and with the design where it pins them
    inf = F.info()
    subs = cc.pick_subtrees(fronts, parent, sup, cc.default_maxf(n, case.env))
    assert (inf["solve_subtrees"], inf["subtree_fronts"]) == (len(subs), sum(hi - lo + 1 for lo, hi in subs)), (name, inf, subs)
    if case.subtrees is not None:
        assert (inf["solve_subtrees"], inf["subtree_fronts"]) == case.subtrees, (name, inf)
    monkeypatch.setenv("KVX_NO_SUBTREES", "1")       # (the handle keeps the numbers of its first query: a new one)
    G = Factor(n, cp, ri, "L", opts=cc.OPTS)
    assert (G.info()["solve_subtrees"], G.info()["subtree_fronts"]) == (0, 0)
    assert (F.info()["solve_subtrees"], F.info()["subtree_fronts"]) == (inf["solve_subtrees"], inf["subtree_fronts"])
    # the values: off-diagonals in [-1, -0.25] u [0.25, 1], all different, strictly diagonally dominant
    A = cc.dense_lower(n, cp, ri, vx)
    col = np.repeat(np.arange(n), np.diff(cp))
    off = vx[ri != col]
    assert np.all((np.abs(off) >= 0.25) & (np.abs(off) <= 1.0)) and np.unique(off).size == off.size
    d = np.diag(A)
    slack = d - (np.abs(A).sum(axis=1) - np.abs(d))
    assert np.all(slack >= 0.5 - 1e-12) and np.all(slack <= 1.5 + 1e-12)


def test_designs_land_in_their_class():
    """every leaf design of a system named after a kernel class is of that class (front_class of symbolic.hpp, restated)"""
    for case in cc.CASES:
        for cls, cname in enumerate(cc.CLASS_NAMES):
            if case.name in ("leaves_" + cname, "leaves_" + cname + "_bigroot"):
                assert {cc.front_class(t[1], t[2]) for t in case.tags if t[0] == "leaf"} == {cls}, case.name
    for name, cls in (("leaves_lds96_k32", cc.CLS_LDS96), ("leaves_lds96_k64", cc.CLS_LDS96), ("leaves_lds128_k32", cc.CLS_LDS128),
                      ("leaves_lds128_k64", cc.CLS_LDS128), ("leaves_lds128_bigroot", cc.CLS_LDS128), ("leaves_big", cc.CLS_BIG)):
        assert {cc.front_class(t[1], t[2]) for t in cc.BY_NAME[name].tags if t[0] == "leaf"} == {cls}, name
    assert [cc.front_class(m, k) for m, k in ((32, 16), (32, 17), (33, 16), (48, 32), (49, 1), (64, 32), (64, 33), (65, 1), (96, 64), (97, 1), (128, 64),
                                               (129, 1), (65, 65))] == [8, 7, 6, 5, 4, 3, 2, 2, 2, 1, 1, 0, 0]


def test_coverage(monkeypatch):
    """the union of the cases meets every condition of the list; checked on the REALISED fronts"""
    leaves, us, levels_of = set(), set(), {}
    u0_root_with_children = u0_childless_in_forest = False
    for case in cc.CASES:
        F, _ = analysed(case, monkeypatch)
        fronts, level, parent, sup = cc.realised(F)
        levels_of[case.name] = (fronts, level)
        for m, k, nch in fronts:
            us.add(m - k)
            if nch == 0:
                leaves.add((m, k))
            u0_root_with_children |= m == k and nch > 0
            u0_childless_in_forest |= m == k and nch == 0 and len(case.designs) > 1
    tags = {t for c in cc.CASES for t in c.tags}
    missing = []
    # leaf fronts
    want = [(m, k) for m in cc.WAVE_M for k in cc.WAVE_K if k <= m] + list(cc.LDS96_LEAVES) + list(cc.LDS128_LEAVES) + [(129, 1), (65, 65)]
    missing += [("leaf", mk) for mk in want if mk not in leaves or ("leaf",) + mk not in tags]
    assert cc.front_class(129, 1) == cc.CLS_BIG and cc.front_class(65, 65) == cc.CLS_BIG
    # Schur complements
    missing += [("u", u) for u in (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 127) if u not in us]
    missing += [x for x, ok in (("u0 root with children", u0_root_with_children), ("u0 childless in a forest", u0_childless_in_forest)) if not ok]
    # fronts with children
    groups = {"wave": set(range(cc.CLS_WAVE0, 9)), "lds96": {cc.CLS_LDS96}, "lds128": {cc.CLS_LDS128}}
    counts = {t[2] for t in tags if t[0] == "parent"}
    missing += [("children", c) for c in (1, 2) if c not in counts]
    for g, cls in groups.items():
        missing += [("four or more children", g)] if not any(t[0] == "parent" and t[1] in cls and t[2] >= 4 for t in tags) else []
    lds = groups["lds96"] | groups["lds128"]
    missing += [("uc into wave", uc) for uc in (1, 16, 17, 33, 64) if not any(t[0] == "child_u" and t[1] in groups["wave"] and t[2] == uc for t in tags)]
    missing += [("uc into lds", uc) for uc in (1, 32, 33, 64, 65, 128) if not any(t[0] == "child_u" and t[1] in lds and t[2] == uc for t in tags)]
    for what in ("scattered", "first_row", "last_row"):
        missing += [(what, g) for g, cls in (("wave", groups["wave"]), ("lds", lds)) if not any(t[0] == what and t[1] in cls for t in tags)]
    # mixed levels, on the realised levels
    def level_has(pred_a, pred_b):
        for fronts, level in levels_of.values():
            for l in set(level):
                here = [f for f, fl in zip(fronts, level) if fl == l]
                for a in here:
                    for b in here:
                        if pred_a(a) and pred_b(b) and (a[0] <= 32) == (b[0] <= 32) and (a[0] <= 48) == (b[0] <= 48):
                            return True
        return False
    is96 = lambda f: cc.front_class(f[0], f[1]) == cc.CLS_LDS96
    missing += [] if level_has(lambda f: is96(f) and f[1] <= 32, lambda f: is96(f) and f[1] > 32) else ["mixed lds96 level"]
    wave = lambda f: cc.front_class(f[0], f[1]) >= cc.CLS_WAVE0
    missing += [] if level_has(lambda f: wave(f) and f[1] <= 16, lambda f: wave(f) and f[1] > 16) else ["mixed wave level"]
    # the forest of three copies: every launch of it numbers at least three fronts, and every small class is in it
    fronts, level = levels_of["forest3"]
    launches = {}
    for (m, k, _), l in zip(fronts, level):
        c = cc.front_class(m, k)
        key = (l, c if c < cc.CLS_WAVE0 else 100 + cc.wave_image(m))
        launches[key] = launches.get(key, 0) + 1
    assert min(launches.values()) >= 3, launches
    missing += [("forest3 class", c) for c in range(1, 9) if sum(1 for m, k, n in fronts if n == 0 and cc.front_class(m, k) == c) < 3]
    # subtree limits
    missing += [t for t in (("sub_fronts", 4), ("sub_fronts", 5), ("sub_fronts", 12), ("sub_fronts", 13), ("sub_cols", 256), ("sub_cols", 257))
                if t not in tags]
    assert not missing, missing


def test_bound_notices_a_transposition():
    """What the designed values are for.  Exchange the entries of two update rows of one child -- what a swap of two relative
    indices in the extend-add, or of two rows of a Schur tile, does to the assembled matrix -- and factor that: against the
    true matrix the factor misses rho <= n + 3 by many orders of magnitude, while the float64 oracle's own factor is far inside
    it.  With the constant off-diagonals of a Laplacian the exchanged matrix IS the matrix and nothing could be seen."""
    from oracle.kvx_oracle import OracleChol
    case = cc.BY_NAME["kids_wave5"]
    n, cp, ri, vx = case.system()
    F = Factor(n, cp, ri, "L", opts=cc.OPTS)
    perm = F.perm()
    ip = np.empty(n, dtype=np.int64)
    ip[perm] = np.arange(n)
    ranges = cc.tree_ranges(case, ip)
    O = OracleChol(n, cp, ri, "L", perm)
    C = cc.dense_lower(n, cp, ri, vx)[np.ix_(perm, perm)]

    def rho(values):
        O.factorize(values)
        return cc.rho_of(C, cc.dense_factor(n, *O.L()), ranges)

    assert rho(vx) <= 0.25 * (n + 3)
    j = 0                                        # first column of the first child: its last two update rows
    a, b = cp[j + 1] - 2, cp[j + 1] - 1
    swapped = vx.copy()
    swapped[[a, b]] = vx[[b, a]]
    assert rho(swapped) > 1e9 * (n + 3)
