"""Designed SPD systems for the triangular sweeps over the big fronts (m > 128 or k > 64): kernels_big.hip k_fwd_big_step,
k_bwd_big_init, k_bwd_big_step and their blocks-of-eight forms, kernels_wide.hip k_wide_fwd_big_* / k_wide_bwd_big_*.
test_chol_big_solve_cpu.py pins the designs, the launch counts and the reference on the host; chol_big_solve_child.py runs them on
the device for test_chol_big_solve_gpu.py.  Not a conftest: plain helpers.  The designs are those of chol_class_cases.py.

What each case is for (NB = 64 columns per sub-block, SB = 256 per super-step, 64 or 256 rows per workgroup below a super-block):
  k_edges   nb = 1, 65, 64, 128, 129 in one launch: max_m and max_k from different fronts; roots of k = 1 with one child above
  super2    one full super-step with 256 rows below; a second super-step of one column with 257 rows below; roots m == k = 257, 258
  super3    three super-steps, the last of one column: the backward step at b = 2, 1, 0
  roots     childless, nothing below: the last block of the rhs-major form holds 1, 64, 1, 1 columns
  kids      a FIRST step with three children (classes big -- 130 rows --, wave, big) whose rows land in [0, 256), in [256, 300)
            -- pivot rows past the first super-block -- and in the update rows, on both sides of rows 256, 300, 364 and 556
  chain     a big child under a big parent under a big root
  mixed     max_m from one front, max_k from the other: both early exits (jb0 >= k, rbase >= m) in every step after the first
  crowd85, crowd86      85 / 86 trees of leaf(129, 1): many fronts per launch (grid y).  Their levels hold 85 / 86 big fronts each -- roots
            (130, 130, 2) of three 64-row workgroups, leaves (129, 1, 0) of two -- so both stay within the 512-workgroup threshold
  crowd256, crowd257    256 / 257 childless roots (66, 66): two 64-row workgroups each, 512 <= 512 < 514 -- the threshold
            KVX_FWD_NARROW_WGS between the 64-row and the 256-row form without any knob, at the smallest order that reaches it
  extra     root(320): exactly 64 rows below the first super-block (one full 64-row workgroup, no second one);
            leaf(146, 17): nb = 17, the 64-row form's column groups of two columns with a ragged last group;
            family(200, 70, one child (128, 40)): a big front that pulls the update vector an LDS-class kernel wrote
"""
import numpy as np

from chol_class_cases import (LD, OPTS, U, Case, Design, _spread, dense_factor, family, front_class, leaf, realised, root,      # noqa: F401
                              tree_ranges, CLS_BIG)

NB, SB, RB, MR_FROM, NARROW_WGS = 64, 256, 8, 64, 512

COUNTERS = ("fwd_first64", "fwd_next64", "fwd_first256", "fwd_next256",
            "fwd_mr_first_diag", "fwd_mr_first_rows", "fwd_mr_next_diag", "fwd_mr_next_rows",
            "bwd_init", "bwd_step", "bwd_mr_init", "bwd_mr_step_diag", "bwd_mr_step_cols",
            "wide_fwd_asm", "wide_fwd_step", "wide_bwd_head", "wide_bwd_step")


def _cases():
    C = []
    C.append(Case("k_edges", [leaf(129, 1), leaf(130, 65), leaf(192, 64), leaf(193, 128), leaf(200, 129)]))
    C.append(Case("super2", [leaf(512, 256), leaf(514, 257)]))
    C.append(Case("super3", [leaf(770, 513)]))
    C.append(Case("roots", [root(129), root(256), root(257), root(321)]))
    C.append(Case("kids", [family(600, 300, [(40, _spread(600, 90, True, True)),
                                             (5, [255, 256, 257, 299, 300, 301, 363, 364, 555, 556, 599]),
                                             (70, _spread(600, 200, True, False))])]))
    C.append(Case("chain", [family(400, 130, [(100, _spread(400, 300, True, True))])]))
    C.append(Case("mixed", [leaf(700, 65), leaf(300, 290)]))
    for count in (85, 86):
        C.append(Case("crowd%d" % count, [leaf(129, 1) for _ in range(count)]))
    for count in (256, 257):
        C.append(Case("crowd%d" % count, [root(66) for _ in range(count)]))
    C.append(Case("extra", [root(320), leaf(146, 17), family(200, 70, [(40, _spread(200, 88, True, True))])]))
    return C


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
CROWDS = tuple(c.name for c in CASES if c.name.startswith("crowd"))


def is_big(m, k):
    return front_class(m, k) == CLS_BIG


def big_levels(fronts, level):
    """per level that holds big fronts, root level first: (level, [(m, k, children)] of its big fronts)"""
    out = []
    for l in sorted(set(level)):
        here = [f for f, fl in zip(fronts, level) if fl == l and is_big(f[0], f[1])]
        if here:
            out.append((l, here))
    return out


def expect_big(fronts, level, sys, nrhs, form, narrow_wgs=NARROW_WGS):
    """The launches of launch_fwd_big / launch_bwd_big (form "rhs": one grid layer per right-hand side, blocks of eight from 64
    on) or launch_wide_fwd_big / launch_wide_bwd_big (form "wide") for one solve, restated: per level with big fronts from their
    count, the largest order and the largest pivot count."""
    want = {c: 0 for c in COUNTERS}
    fwd, bwd = sys in (0, 4), sys in (0, 5)
    for _, here in big_levels(fronts, level):
        count, max_m, max_k = len(here), max(f[0] for f in here), max(f[1] for f in here)
        nsb = (max_k + SB - 1) // SB
        if form == "wide":
            if fwd:
                want["wide_fwd_asm"] += 1
                for jb in range(0, max_k, NB):
                    if max_m - jb - 1 <= 0:
                        break
                    want["wide_fwd_step"] += 1
            if bwd:
                want["wide_bwd_head"] += 1
                want["wide_bwd_step"] += (max_k + NB - 1) // NB - 1
            continue
        assert form == "rhs"
        if fwd:
            for jb in range(0, max_k, SB):
                rows = max_m - jb - 1
                narrow = max(1, (rows + 63) // 64) * count <= narrow_wgs
                step = "first" if jb == 0 else "next"
                if nrhs >= MR_FROM and not narrow:
                    want["fwd_mr_%s_diag" % step] += 1
                    want["fwd_mr_%s_rows" % step] += 1
                else:
                    want["fwd_%s%d" % (step, 64 if narrow else 256)] += 1
        if bwd:
            if nrhs >= MR_FROM:
                want["bwd_mr_init"] += 1
                want["bwd_mr_step_diag"] += nsb
                want["bwd_mr_step_cols"] += nsb - 1
            else:
                want["bwd_init"] += 1
                want["bwd_step"] += nsb
    return want


def super_steps(m, k):
    """(jb0, nb, rows below the super-block) of every forward super-step of a front"""
    return [(jb, min(SB, k - jb), m - jb - min(SB, k - jb)) for jb in range(0, k, SB)]


# ---- per tree: the factor as dense blocks, references on stacks of trees of equal order -------------------------------------------
def tree_blocks(Lp, Li, Lx, ranges):
    """the diagonal block of the factor of every tree [a, b), dense (the systems are block diagonal over their designs; the whole
    factor of a crowd would not fit as a dense matrix)"""
    out = []
    for a, b in ranges:
        p0, p1 = int(Lp[a]), int(Lp[b])
        assert Li[p0:p1].min() >= a and Li[p0:p1].max() < b
        out.append(dense_factor(b - a, Lp[a:b + 1] - p0, Li[p0:p1] - a, Lx[p0:p1]))
    return out


def stacks(blocks, ranges):
    """trees of equal order as one array: [(rows (T, nb) of the permuted system, L (T, nb, nb))]"""
    by = {}
    for (a, b), Lb in zip(ranges, blocks):
        by.setdefault(b - a, []).append((a, Lb))
    return [(np.array([np.arange(a, a + nb) for a, _ in lst]), np.array([Lb for _, Lb in lst])) for nb, lst in sorted(by.items())]


def subst_stack(L, B, trans):
    """L^-1 B or L^-T B for a stack L (T, nb, nb), B (T, nb, r), in the precision of the arguments: column-oriented substitution"""
    X = B.copy()
    nb = L.shape[1]
    d = L[:, np.arange(nb), np.arange(nb)]
    if not trans:
        for j in range(nb):
            X[:, j] /= d[:, j, None]
            X[:, j + 1:] -= L[:, j + 1:, j, None] * X[:, None, j]
    else:
        for j in range(nb - 1, -1, -1):
            X[:, j] /= d[:, j, None]
            X[:, :j] -= L[:, j, :j, None] * X[:, None, j]
    return X


def blocked_stack(L, B, trans):
    """The scheme of the big-front sweeps in float64: the inverse of each 64 x 64 diagonal block applied as a product, the
    blocks below (above, for L') taken off by products."""
    X = B.copy()
    nb = L.shape[1]
    edges = list(range(0, nb, NB))
    inv = {j: np.linalg.inv(L[:, j:j + NB, j:j + NB]) for j in edges}
    for j in (edges if not trans else edges[::-1]):
        e = min(j + NB, nb)
        if not trans:
            X[:, j:e] = inv[j] @ X[:, j:e]
            X[:, e:] -= L[:, e:, j:e] @ X[:, j:e]
        else:
            X[:, j:e] = inv[j].transpose(0, 2, 1) @ X[:, j:e]
            X[:, :j] -= L[:, j:e, :j].transpose(0, 2, 1) @ X[:, j:e]
    return X


def solve_trees(stk, B, sys, perm, how, dtype):
    """sys 4 (L X = B), 5 (L' X = B) or 0 (A X = B through P and L) tree by tree with how(L, B, trans), computed in dtype"""
    Bp = B[perm] if sys == 0 else B
    X = np.zeros(B.shape, dtype=dtype)
    for rows, L in stk:
        Y, Ld = Bp[rows].astype(dtype), L.astype(dtype)
        if sys in (0, 4):
            Y = how(Ld, Y, False)
        if sys in (0, 5):
            Y = how(Ld, Y, True)
        X[rows] = Y
    if sys == 0:
        out = np.zeros_like(X)
        out[perm] = X
        return out
    return X


def lapack_stack(L, B, trans):
    import scipy.linalg as sla
    return np.array([sla.solve_triangular(Lt, Bt, lower=True, trans=1 if trans else 0) for Lt, Bt in zip(L, B)])


def substitution_ratio(stk, B, X, trans):
    """max of |B - L X| / ((nb + 1) 2^-53 |L| |X|) over the components of every tree, nb the order of the tree, in longdouble
    (the criterion of check_substitution of test_chol_classes_gpu.py: Higham, Thm 8.5)"""
    worst = 0.0
    for rows, L in stk:
        Ld = L.astype(LD)
        Ld = Ld.transpose(0, 2, 1) if trans else Ld
        Xd = X[rows].astype(LD)
        R = np.abs(B[rows].astype(LD) - Ld @ Xd)
        bound = (L.shape[1] + 1) * U * (np.abs(Ld) @ np.abs(Xd))
        assert np.all(bound > 0)
        worst = max(worst, float((R / bound).max()))
    return worst
