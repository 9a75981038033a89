"""The designed systems of chol_big_solve_cases.py, on the host: the analysis must cut every one of them into exactly the fronts
its design declares, the launchers of the big-front sweeps (restated: expect_big) must take the kernel forms the cases are for,
together the cases must meet every block, row and child edge of those kernels, and the scheme the kernels use -- explicit inverses
of the 64 x 64 diagonal blocks -- must stay far inside the substitution bound on these values in plain float64.  No device."""
import numpy as np
import pytest

import chol_big_solve_cases as bc
from chol_class_cases import LD, dense_lower
from kvxopt_amd.chol import Factor

NAMES = [c.name for c in bc.CASES]
_ANALYSED = {}


def analysed(name):
    """(case, system, factor handle, realised fronts, inverse permutation, tree ranges), analysed once per module"""
    if name not in _ANALYSED:
        case = bc.BY_NAME[name]
        n, cp, ri, vx = case.system()
        F = Factor(n, cp, ri, "L", opts=bc.OPTS)
        ip = np.empty(n, dtype=np.int64)
        ip[F.perm()] = np.arange(n)
        _ANALYSED[name] = (case, (n, cp, ri, vx), F, bc.realised(F), ip)
    return _ANALYSED[name]


@pytest.mark.parametrize("name", NAMES)
def test_design_is_exact(name):
    case, (n, cp, ri, vx), F, (fronts, level, parent, sup), ip = analysed(name)
    assert n == case.n and (n < 1100 or name in bc.CROWDS)
    assert sorted(fronts) == case.fronts, (name, sorted(set(fronts) - set(case.fronts)), sorted(set(case.fronts) - set(fronts)))
    for first, cols in case.trees():        # the permutation keeps every tree together: the bounds are evaluated tree by tree
        pos = np.sort(ip[first:first + cols])
        assert pos[-1] - pos[0] == cols - 1, (name, first)
    # the values: off-diagonals in [-1, -0.25] u [0.25, 1], all different, strictly diagonally dominant (Case.system)
    col = np.repeat(np.arange(n), np.diff(cp))
    off = ri != col
    assert np.all((np.abs(vx[off]) >= 0.25) & (np.abs(vx[off]) <= 1.0)) and np.unique(vx[off]).size == off.sum()
    rowsum = np.zeros(n)
    np.add.at(rowsum, ri[off], np.abs(vx[off]))
    np.add.at(rowsum, col[off], np.abs(vx[off]))
    slack = vx[cp[:-1]] - rowsum
    assert np.all(ri[cp[:-1]] == np.arange(n)) and np.all(slack >= 0.5 - 1e-12) and np.all(slack <= 1.5 + 1e-12)


def counts(name, sys, nrhs, form, narrow_wgs=bc.NARROW_WGS):
    fronts, level = analysed(name)[3][:2]
    return {k: v for k, v in bc.expect_big(fronts, level, sys, nrhs, form, narrow_wgs).items() if v}


def test_launch_counts():
    """the kernel forms the cases promise, from the launchers' own rules"""
    # super3: levels (258, 258, 2) and {(770, 513, 0), (259, 1, 1)}: one first and two next steps for the leaf, the root adds one each
    assert counts("super3", 4, 1, "rhs") == {"fwd_first64": 2, "fwd_next64": 3}
    assert counts("super3", 5, 1, "rhs") == {"bwd_init": 2, "bwd_step": 5}
    assert counts("super3", 5, 64, "rhs") == {"bwd_mr_init": 2, "bwd_mr_step_diag": 5, "bwd_mr_step_cols": 3}
    assert counts("super3", 4, 3, "rhs", 0) == {"fwd_first256": 2, "fwd_next256": 3}
    assert counts("super3", 4, 67, "rhs", 0) == {"fwd_mr_first_diag": 2, "fwd_mr_first_rows": 2, "fwd_mr_next_diag": 3, "fwd_mr_next_rows": 3}
    assert counts("super3", 0, 48, "wide") == {"wide_fwd_asm": 2, "wide_fwd_step": 14, "wide_bwd_head": 2, "wide_bwd_step": 12}
    # roots: one level, max_m = max_k = 321; the rhs-major loop ends where no row is left below a block (jb = 320)
    assert counts("roots", 0, 65, "wide") == {"wide_fwd_asm": 1, "wide_fwd_step": 5, "wide_bwd_head": 1, "wide_bwd_step": 5}
    assert counts("roots", 0, 1, "rhs") == {"fwd_first64": 1, "fwd_next64": 1, "bwd_init": 1, "bwd_step": 2}
    # without a knob every case but crowd257 stays within 512 workgroups of 64 rows on every level: the 64-row form only, also
    # from 64 right-hand sides on (the layered single-rhs kernel); with KVX_FWD_NARROW_WGS=0 never
    for name in NAMES:
        for nrhs in (1, 3, 64, 67):
            c = counts(name, 0, nrhs, "rhs")
            if name != "crowd257":
                assert not any(k.startswith("fwd_mr") or k.endswith("256") for k in c), (name, nrhs, c)
            c0 = counts(name, 0, nrhs, "rhs", 0)
            assert not any(k.endswith("64") for k in c0), (name, nrhs, c0)
            assert any(k.startswith("fwd_mr") for k in c0) == (nrhs >= 64) and ("bwd_mr_init" in c) == ("bwd_mr_init" in c0) == (nrhs >= 64)
    # many fronts per launch: roots (130, 130, 2) of three workgroups of 64 rows each, leaves (129, 1, 0) of two; 86 of them do not
    # reach the threshold
    for name in ("crowd85", "crowd86"):
        cnt = len(bc.BY_NAME[name].designs)
        assert 3 * cnt <= 512 and counts(name, 4, 1, "rhs") == counts(name, 4, 64, "rhs") == {"fwd_first64": 2}, name
    # the threshold: childless roots (66, 66), two workgroups of 64 rows each
    assert counts("crowd256", 4, 1, "rhs") == counts("crowd256", 4, 64, "rhs") == {"fwd_first64": 1}
    assert counts("crowd257", 4, 1, "rhs") == {"fwd_first256": 1}
    assert counts("crowd257", 4, 64, "rhs") == {"fwd_mr_first_diag": 1, "fwd_mr_first_rows": 1}
    assert counts("crowd257", 4, 64, "rhs", 514) == {"fwd_first64": 1} and 2 * 256 == 512 < 2 * 257


def child_rows(F, fronts, parent, s):
    """per child of front s: the rows of s (0 .. m - 1, front order) its update vector is added to"""
    rp, ri = F.front_rows()
    mine = list(ri[rp[s]:rp[s + 1]])
    pos = {int(r): i for i, r in enumerate(mine)}
    out = []
    for c, p in enumerate(parent):
        if p == s:
            kc = fronts[c][1]
            out.append([pos[int(r)] for r in ri[rp[c] + kc:rp[c + 1]]])
    return out


def test_coverage():
    """the union of the cases meets every edge of the list; checked on the REALISED fronts"""
    nbs, below, kmod64, kmod256, wide_last = set(), set(), set(), set(), set()
    pull = set()
    split_level = early_k = early_m = chain3 = root_with_kids = lds_child = False
    bwd_grid = set()
    for name in NAMES:
        case, _, F, (fronts, level, parent, sup), _ = analysed(name)
        for s, (m, k, nch) in enumerate(fronts):
            if not bc.is_big(m, k):
                continue
            kmod64.add(k % 64)
            kmod256.add(k % 256)
            wide_last.add((k - 1) % 64 + 1)
            root_with_kids |= m == k and nch >= 2
            for jb, nb, rows in bc.super_steps(m, k):
                nbs.add(nb)
                below.add(rows)
            for b in range((k + bc.SB - 1) // bc.SB):
                bwd_grid.add((b, max(1, b * bc.SB // bc.NB)))
            p = parent[s]
            if p >= 0 and bc.is_big(*fronts[p][:2]) and parent[p] >= 0 and bc.is_big(*fronts[parent[p]][:2]):
                chain3 = True
            if nch > 0:
                nb0 = min(bc.SB, k)
                kids = [c for c, q in enumerate(parent) if q == s]
                lds_child |= any(bc.front_class(*fronts[c][:2]) in (1, 2) for c in kids)
                for rows in child_rows(F, fronts, parent, s):
                    for rows_wg in (64, 256):
                        for what, sel in (("t < nb", [t for t in rows if t < nb0]), ("nb <= t < k", [t for t in rows if nb0 <= t < k]),
                                          ("t >= k", [t for t in rows if t >= k])):
                            if sel:
                                pull.add((what, rows_wg))
                            if what == "t >= k" and len({(t - nb0) // rows_wg for t in sel}) > 1:
                                pull.add(("t >= k in two workgroups", rows_wg))
                            if what == "nb <= t < k" and sel and any(t >= k and (t - nb0) // rows_wg == (sel[0] - nb0) // rows_wg for t in rows):
                                pull.add(("pivot and update rows in one workgroup", rows_wg))
                    if len(kids) >= 3 and {255, 256} <= set(rows) and {k - 1, k} <= set(rows):
                        pull.add("three children, rows on both sides of 256 and of k")
        for l, here in bc.big_levels(fronts, level):
            max_m, max_k = max(f[0] for f in here), max(f[1] for f in here)
            split_level |= not any(f[0] == max_m and f[1] == max_k for f in here)
            early_k |= any(f[1] <= bc.SB < max_k for f in here)                                    # jb0 >= k in the second super-step
            early_m |= any((f[0] - min(bc.SB, f[1]) + 63) // 64 < (max_m - 1 + 63) // 64 for f in here)      # a workgroup past the front's rows
    missing = []
    missing += [("nb", v) for v in (1, 17, 64, 65, 128, 129, 256) if v not in nbs]
    missing += [("k mod 64", v) for v in (0, 1) if v not in kmod64] + [("k mod 256", v) for v in (0, 1) if v not in kmod256]
    missing += [("rows below a super-block", v) for v in (0, 1, 64, 65, 256, 257) if v not in below]
    missing += [("last block of the rhs-major form", v) for v in (1, 64) if v not in wide_last]
    missing += [("backward step (b, grid x)", v) for v in ((2, 8), (1, 4), (0, 1)) if v not in bwd_grid]
    for rows_wg in (64, 256):
        missing += [(what, rows_wg) for what in ("t < nb", "nb <= t < k", "t >= k", "t >= k in two workgroups", "pivot and update rows in one workgroup")
                    if (what, rows_wg) not in pull]
    missing += [x for x in ("three children, rows on both sides of 256 and of k",) if x not in pull]
    missing += [x for x, ok in (("max_m and max_k of a level from different fronts", split_level), ("jb0 >= k", early_k), ("rbase >= m", early_m),
                                ("big front under big front under big front", chain3), ("root m == k with two children", root_with_kids),
                                ("child of an LDS class under a big front", lds_child)) if not ok]
    assert not missing, missing


def tree_matrices(case, system, ip):
    """the permuted matrix of every tree, dense, and its rows in the permuted system"""
    n, cp, ri, vx = system
    out = []
    for first, cols in case.trees():
        p0, p1 = int(cp[first]), int(cp[first + cols])
        A = dense_lower(cols, cp[first:first + cols + 1] - p0, ri[p0:p1] - first, vx[p0:p1])
        a = int(ip[first:first + cols].min())
        loc = ip[first:first + cols] - a                    # position of every column of the tree inside its permuted range
        P = np.empty(cols, dtype=np.int64)
        P[loc] = np.arange(cols)
        out.append(((a, a + cols), A[np.ix_(P, P)]))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_reference_scheme_meets_the_bound(name):
    """Explicit inverses of the diagonal blocks do not satisfy the substitution bound in general; on these diagonally dominant
    values the float64 restatement of the scheme (blocked_stack) stays within a quarter of it, for L and for L'.  The GPU tests
    hold the kernels to the whole bound."""
    case, system, F, _, ip = analysed(name)
    trees = tree_matrices(case, system, ip)
    ranges = [r for r, _ in trees]
    stk = bc.stacks([np.linalg.cholesky(A) for _, A in trees], ranges)
    B = np.random.default_rng(case.seed + 11).uniform(-1.0, 1.0, (case.n, 3))
    for sys, trans in ((4, False), (5, True)):
        X = bc.solve_trees(stk, B, sys, None, bc.blocked_stack, np.float64)
        ratio = bc.substitution_ratio(stk, B, X, trans)
        print("%-9s sys %d: blocked float64 scheme at %.3f of the bound" % (name, sys, ratio))
        assert ratio <= 0.25, (name, sys, ratio)
        # and the reference the GPU tests measure against solves the same systems
        ref = bc.solve_trees(stk, B, sys, None, bc.subst_stack, LD)
        assert float(np.abs(X - ref).max()) <= 1e-12 * float(np.abs(ref).max())


def test_bound_notices_a_swapped_row():
    """What the criterion is worth: the right-hand side of `kids` with two neighbouring rows of its big parent exchanged -- what a
    swap of two relative indices in the parent-pull does -- misses the substitution bound by many orders of magnitude."""
    case, system, F, (fronts, level, parent, sup), ip = analysed("kids")
    trees = tree_matrices(case, system, ip)
    stk = bc.stacks([np.linalg.cholesky(A) for _, A in trees], [r for r, _ in trees])
    B = np.random.default_rng(5).uniform(-1.0, 1.0, (case.n, 1))
    s = fronts.index((600, 300, 3))
    for r in (sup[s] + 255, sup[s] + 298):          # across the first super-block's edge; inside the pivot rows past it
        Bs = B.copy()
        Bs[[r, r + 1]] = B[[r + 1, r]]
        X = bc.solve_trees(stk, Bs, 4, None, bc.blocked_stack, np.float64)
        assert bc.substitution_ratio(stk, Bs, X, False) <= 0.25
        assert bc.substitution_ratio(stk, B, X, False) > 1e9
